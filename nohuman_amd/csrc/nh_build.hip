// nh_build.hip -- nh_build_db: FASTA in, a kraken2 database directory out, built on the GPU (include/nohuman_engine.h).
//
// What it replaces: kraken2-build's build_db.cc for one taxon, or the taxa of a manifest, at the default geometry (k = 35, l = 31, default spaced seed and
// toggle mask, revcom_version 1, minimum_acceptable_hash_value 0, linear probing).  That is the limit, on purpose: it is what the
// HPRC databases are and what the classifier's fast path (is_std) is built for.
//
// The sequence text goes to HBM in batches of bounded size (BATCH_BYTES; a 3 Gbase genome is never resident as a whole).  Every
// sequence is cut into PIECES of P k-mers: piece p covers k-mers [p P, min((p + 1) P, n - 34)), i.e. bases [p P, p P + P + 34), so
// consecutive pieces overlap by k - 1 bases and every k-mer belongs to exactly one piece.  A k-mer's minimizer and its ambiguity
// depend only on that k-mer's own 35 bases, so the union over the pieces is the set of the whole sequence; a sequence that does not
// fit what is left of a batch is cut the same way at the batch's end.  One wave scans one piece with the classifier's own scanner
// (nh_scan.h: scan_tile) -- the builder skips a k-mer exactly when the classifier would not look it up.  The walk over the pieces
// is written once (walk_pieces); the kernel of a pass gives it what to do with a tile's minimizers and when to stop.
//
// Two passes over the text:
//   COUNT   every run-start minimizer goes into a device open-addressing set of 64-bit keys (key = minimizer + 1, 0 = empty; the
//           minimizer is below 2^62).  A slot is claimed by compare-and-swap exactly once per distinct key, so the claims counted
//           are the distinct minimizers.  Before a batch is counted the set is grown (doubling, re-inserting the keys on the
//           device) until slots >= 2 x (distinct so far + k-mers of the batch): it is never more than half full, a probe always
//           ends, and no batch can overflow it.  HBM: 8 bytes a slot, 16 to 32 bytes per distinct minimizer when idle and old + new
//           = up to 48 while it grows -- about 1.5 G minimizers of a human genome: 32 GiB resident, 48 GiB at the last doubling.
//   INSERT  into a zeroed table of `capacity` cells: kraken2's CompareAndSet with a constant value, linear probing, 64-bit cell
//           indices.  The probe loop is bounded by the capacity; a lane that has seen every cell raises `full`, which every other
//           lane polls, and the call ends with NH_ECAPACITY.
// Both kernels add their totals with one atomic per wave behind a wave-level reduction; cells and slots are written by
// compare-and-swap only.
//
// Low-complexity masking (mask_low_complexity; nh_dust.hip): in both passes every batch is masked on the device
// between its upload and k_build_pieces, so the scanner reads a masked base as an N.  Whether a base is masked depends on the 63
// bases on either side of it, so a sequence cut at a batch's end carries up to 63 bases of context before its first and behind its
// last base of the batch (beside the batch's size: at most one chunk of a batch starts, and one ends, inside a sequence); the
// pieces still cover every k-mer once.  The chunks are the segments of the mask: no triplet spans two records.  Every input base is
// counted as masked in one chunk only, sequences too short for a k-mer included.
//
// Several taxa (taxa_file; nh_taxa.h): every piece carries the internal id of its taxon (piece_value), INSERT runs as
// k_build_pieces<false, true> and merges a key that two taxa share into their lowest common ancestor with compare-and-swap -- the
// node table (parent) is read from global memory: it is at most 16 KB, shared by every wave and looked at only on that path -- and
// k_value_cells counts the cells per node of the finished table.  COUNT knows no taxon.  A build of one taxon launches the kernels
// it always did (MULTI = false).
//
// Extension (nh_extend_db; nh_extend.hip): the table is not zeroed but loaded from the base database's hash.k2d and
// re-keyed in place for the merged taxonomy; INSERT then runs as for several taxa (MULTI even for one added taxon: it merges with
// values of the base), there is no COUNT, and the capacity is the base's.
//
// Exclusion (nh_build_db_exclude): the host's minimizers that a set of other sequences also carries are left out.
// The set of COUNT stays on the device (COUNT runs even where `capacity` is given), then a third pass, EXCLUDE, streams the
// exclusion sequences through the same batches, pieces and scanner (never masked) and looks every run-start minimizer up in the
// set, find-only: a key that is there gets bit 63 of its slot set (keys are below 2^62 + 1) by atomicOr, and the lane that saw
// the bit clear counts it, so the count is |H and X| whatever the order, the batches or the repeats of the exclusion input; a miss
// writes nothing.  INSERT then runs as k_build_pieces<false, MULTI, true>: it finds each minimizer's slot again and skips a
// flagged one.  The capacity comes from what is kept.  Nothing of the exclusion input is stored and the set is not larger
// for it.  A build without an exclusion list launches the kernels it always did (FILTER = false) and frees the set before INSERT.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "nh_device.h"
#include "nh_dust.h"
#include "nh_extend.h"
#include "nh_fastx.h"
#include "nh_internal.h"
#include "nh_scan.h"
#include "nh_taxa.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

// second kernel argument of k_build_pieces (the first is the classifier's KArgs: scan_tile reads the geometry from it)
struct BuildDev {
    unsigned long long *set;       // COUNT, EXCLUDE, INSERT with FILTER: slots of the key set
    uint64_t set_cap, set_magic;   // slots, floor((2^64 - 1) / slots)
    unsigned long long *counters;  // [0] slots / cells claimed (EXCLUDE: look-ups), [1] k-mers that are not ambiguous, [7] EXCLUDE: slots flagged
    int *full;                     // raised by a lane whose probe saw every slot / cell
    uint32_t value, pad;           // INSERT: the value field of every cell (one taxon)
    // INSERT of several taxa (MULTI)
    const uint32_t *piece_value;   // the internal id of each piece's taxon
    const uint32_t *parent;        // the node table: parent[id] < id, 2^value_bits entries (zero behind the last node)
};

constexpr uint32_t FULL_POLL = 1023;  // a probing lane looks at `full` every 1024 cells
constexpr unsigned long long SET_EXCLUDED = 1ull << 63;  // a slot of the set whose minimizer the exclusion input carries too (a key is below 2^63)

// The slot of minimizer mz in the set, find-only: plain loads from its home on, the index wrapping at the set's end, until an empty
// slot or the key (whatever its flag); at most `cap` slots are looked at.  -> the slot's index and its word in `word`, or `cap`.
// Only for a set that no longer grows: slots change by their flag alone.
__device__ __forceinline__ uint64_t set_find(const unsigned long long *set, const uint64_t cap, const uint64_t magic, const uint64_t mz,
                                             unsigned long long &word) {
    const unsigned long long key = mz + 1;
    uint64_t idx = mod_capacity(fmix64(mz), cap, magic);
    for (uint64_t tries = 0; tries < cap; tries++) {
        const unsigned long long cur = set[idx];
        if (cur == 0) break;
        if ((cur & ~SET_EXCLUDED) == key) {
            word = cur;
            return idx;
        }
        idx++;
        if (idx >= cap) idx = 0;
    }
    word = 0;
    return cap;
}

// The walk over the pieces that every pass makes: one wave per piece, sequence text[seq_off[p], +seq_len[p]) (starts and lengths, so
// that pieces may overlap), a piece a tile at a time through walk_tiles (nh_scan.h) with no minimizer carried into it.  The text
// is readable for 8 bytes behind its end, which is the tail the walk's loads are clamped to, and a piece that leaves the text is
// skipped by the whole wave (the host makes no such piece).  enter(p) is called once for a piece that is walked, before its text
// is read, and what it returns goes to every per_tile(it, nruns) of the piece; that is called between two wave_sync() with the
// tile's run-start minimizers in S.q[0][0 .. nruns): the caller's lanes take them r = lane, lane + 64, ...; stop() is asked behind
// every piece and is wave-uniform.  -> CLEAN: the k-mers walked that are not ambiguous (wave-uniform); else 0.
template <bool CLEAN, class WL, class Enter, class PerTile, class Stop>
__device__ __forceinline__ unsigned long long walk_pieces(KArgsP ap, WL &S, const int lane, const int wib, Enter &&enter,
                                                          PerTile &&per_tile, Stop &&stop) {
    unsigned long long clean = 0;
    const uint64_t n_piece = ap->n_frag;
    const uint64_t *const start = ap->seq_off;
    const uint32_t *const len = ap->seq_len;
    const uint64_t text_len = ap->bases_end;
    const uint64_t last_dw = (text_len + 4) >> 2;  // the text is readable for 8 bytes behind its end
    const uint32_t *const text = reinterpret_cast<const uint32_t *>(ap->bases);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib; p < n_piece; p += n_waves) {
        const uint64_t o0 = start[p];
        const uint32_t n = len[p];
        if (n < 35u || o0 > text_len || text_len - o0 < n) continue;  // (wave-uniform; the host makes no such piece)
        const auto of_piece = enter(p);
        uint64_t carry_min = NH_FULL;
        walk_tiles(ap, S, lane, text, last_dw, o0, n, carry_min, [&](const uint32_t nruns, const uint32_t ps) {
            if (CLEAN) clean += (unsigned long long)(__popcll(__ballot(ps & 1u)) + __popcll(__ballot(ps & 2u)));
            per_tile(of_piece, nruns);
        });
        if (stop()) break;
    }
    return clean;
}

// COUNT and INSERT over the pieces of the host's text.
// MULTI (INSERT only): the value of a piece is its taxon's, and a cell that already holds the key under another value becomes the
// lowest common ancestor of the two.
// FILTER (INSERT only, builds with an exclusion list): a minimizer whose slot of the set is flagged is not inserted.
template <bool COUNT, bool MULTI, bool FILTER = false>
__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_build_pieces(const KArgs args_by_kernarg_pointer, const BuildDev b) {
    KArgsP ap = (KArgsP)__builtin_amdgcn_kernarg_segment_ptr();
    typedef WaveLdsT<true, 1, QCAP_GENERIC> WL;
    __shared__ WL lds_all[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WL &S = lds_all[wib];
    init_wave_lds<true>(S, lane);
    uint32_t *const table = const_cast<uint32_t *>(ap->db.table);
    const uint64_t cap = COUNT ? b.set_cap : ap->db.capacity;
    const uint64_t magic = COUNT ? b.set_magic : ap->db.cap_magic;
    const uint32_t vbits = ap->db.value_bits;
    struct {  // per lane
        unsigned long long claimed = 0;
        unsigned long long merges = 0, swaps = 0, inserts = 0;  // (MULTI): own key found under another value; values replaced; insertions
        bool gave_up = false;
    } tally;
    const unsigned long long clean = walk_pieces<!COUNT>(
        ap, S, lane, wib,
        [&](const uint64_t p) { return MULTI ? b.piece_value[p] : b.value; },  // the piece's value (wave-uniform)
        [&](const uint32_t mine, const uint32_t nruns) {
            // (the loop works on a copy of the lane's tally: updated through the closure's references the kernels compile with more
            // SGPR spills than the walk written out in place had, and the one-taxon INSERT takes 5.7 ms where it took 5.6:
            // profiles/build_refactor.txt)
            auto t = tally;
            for (uint32_t r = lane; r < nruns && !t.gave_up; r += 64) {
                const uint64_t mz = S.q[0][r];
                if (FILTER) {  // (every minimizer of the host is in the set: COUNT put it there)
                    unsigned long long word;
                    (void)set_find(b.set, b.set_cap, b.set_magic, mz, word);
                    if (word & SET_EXCLUDED) continue;
                }
                if (MULTI) t.inserts++;
                const uint64_t hc = fmix64(mz);
                uint64_t idx = mod_capacity(hc, cap, magic);
                bool placed = false;
                if (COUNT) {
                    const unsigned long long key = mz + 1;
                    for (uint64_t tries = 0; tries < cap; tries++) {
                        // (a slot never changes once it holds a key: only an empty one needs the compare-and-swap)
                        unsigned long long cur = __hip_atomic_load(&b.set[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (cur == 0) {
                            cur = atomicCAS(&b.set[idx], 0ull, key);
                            if (cur == 0) {
                                t.claimed++;
                                placed = true;
                                break;
                            }
                        }
                        if (cur == key) {
                            placed = true;
                            break;
                        }
                        idx++;
                        if (idx >= cap) idx = 0;
                        if ((tries & FULL_POLL) == FULL_POLL && __hip_atomic_load(b.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                    }
                } else {
                    const uint32_t compacted = (uint32_t)(hc >> (32 + vbits));
                    const uint32_t cell = (compacted << vbits) | mine;
                    for (uint64_t tries = 0; tries < cap; tries++) {
                        uint32_t cur = __hip_atomic_load(&table[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (cur == 0) {
                            cur = atomicCAS(&table[idx], 0u, cell);
                            if (cur == 0) {
                                t.claimed++;
                                placed = true;
                                break;
                            }
                        }
                        if ((cur >> vbits) == compacted) {
                            if (MULTI) {
                                // kraken2's CompareAndSet with LowestCommonAncestor: the larger id walks up its parent.  The key of a
                                // cell never changes and its value only moves towards the root, so a lane that loses the swap
                                // goes on from the value that won, at most as often as the tree is deep.
                                const uint32_t vmask = (1u << vbits) - 1u;
                                bool first = true;
                                for (;;) {
                                    const uint32_t v = cur & vmask;
                                    uint32_t x = v, y = mine;
                                    while (x != y) {
                                        if (x > y) x = b.parent[x];
                                        else y = b.parent[y];
                                    }
                                    if (first && v != mine) t.merges++;
                                    first = false;
                                    if (x == v) break;
                                    const uint32_t seen = atomicCAS(&table[idx], cur, (compacted << vbits) | x);
                                    if (seen == cur) {
                                        t.swaps++;
                                        break;
                                    }
                                    cur = seen;
                                }
                            }
                            placed = true;
                            break;
                        }
                        idx++;
                        if (idx >= cap) idx = 0;
                        if ((tries & FULL_POLL) == FULL_POLL && __hip_atomic_load(b.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                    }
                }
                if (!placed) {
                    __hip_atomic_store(b.full, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    t.gave_up = true;
                }
            }
            tally = t;
        },
        // a full table: no piece after this one can do anything but find it full again
        [&]() { return __hip_atomic_load(b.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; });
    unsigned long long &claimed = tally.claimed, &merges = tally.merges, &swaps = tally.swaps, &inserts = tally.inserts;
    for (int d = 32; d >= 1; d >>= 1) claimed += __shfl_xor(claimed, d, 64);
    if (lane == 0) {
        if (claimed) atomicAdd(&b.counters[0], claimed);
        if (!COUNT && clean) atomicAdd(&b.counters[1], clean);
    }
    if (MULTI) {
        for (int d = 32; d >= 1; d >>= 1)
            merges += __shfl_xor(merges, d, 64), swaps += __shfl_xor(swaps, d, 64), inserts += __shfl_xor(inserts, d, 64);
        if (lane == 0 && merges) atomicAdd(&b.counters[4], merges);
        if (lane == 0 && swaps) atomicAdd(&b.counters[5], swaps);
        if (lane == 0 && inserts) atomicAdd(&b.counters[6], inserts);
    }
}

// EXCLUDE: the pieces of the exclusion text, walked as COUNT walks the host's; every run-start minimizer is looked up in the
// finished set and flagged where it is found.  A miss -- nearly every minimizer of another genome -- writes nothing.
__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_exclude_pieces(const KArgs args_by_kernarg_pointer, const BuildDev b) {
    KArgsP ap = (KArgsP)__builtin_amdgcn_kernarg_segment_ptr();
    typedef WaveLdsT<true, 1, QCAP_GENERIC> WL;
    __shared__ WL lds_all[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WL &S = lds_all[wib];
    init_wave_lds<true>(S, lane);
    const uint64_t cap = b.set_cap, magic = b.set_magic;
    unsigned long long flagged = 0, lookups = 0;  // per lane
    const unsigned long long clean = walk_pieces<true>(
        ap, S, lane, wib, [](const uint64_t) { return 0; },
        [&](int, const uint32_t nruns) {
            for (uint32_t r = lane; r < nruns; r += 64) {
                unsigned long long word;
                const uint64_t idx = set_find(b.set, cap, magic, S.q[0][r], word);
                lookups++;
                // (several lanes may find one slot unflagged: the one whose atomicOr saw it so counts it)
                if (idx < cap && !(word & SET_EXCLUDED) && !(atomicOr(&b.set[idx], SET_EXCLUDED) & SET_EXCLUDED)) flagged++;
            }
        },
        []() { return false; });
    for (int d = 32; d >= 1; d >>= 1) flagged += __shfl_xor(flagged, d, 64), lookups += __shfl_xor(lookups, d, 64);
    if (lane == 0) {
        if (flagged) atomicAdd(&b.counters[7], flagged);
        if (lookups) atomicAdd(&b.counters[0], lookups);
        if (clean) atomicAdd(&b.counters[1], clean);
    }
}

// Cells per node of the finished table (several taxa): bins in LDS, one global atomic per non-zero bin and workgroup.  No occupied
// cell holds the value 0, so bin i counts the value i + 1: VALUE_BINS bins hold every node of the largest taxonomy.  The table is
// read four cells a lane; it is allocated, and zero, through the next multiple of four behind `cap`.
constexpr uint32_t VALUE_BINS = TAXA_MAX_NODES;
__global__ __launch_bounds__(256) void k_value_cells(const uint32_t *table, const uint64_t cap, const uint32_t vmask, const uint32_t nodes,
                                                     unsigned long long *cells) {
    __shared__ uint32_t bins[VALUE_BINS];
    for (uint32_t i = threadIdx.x; i < VALUE_BINS; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const uint64_t n4 = (cap + 3) >> 2, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4 *const t4 = reinterpret_cast<const uint4 *>(table);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 c = t4[i];
        for (uint32_t w : {c.x, c.y, c.z, c.w}) {
            const uint32_t bin = (w & vmask) - 1u;  // (an empty cell: 0 - 1 is no bin; nor is a value without a node)
            if (w != 0 && bin < nodes - 1u && bin < VALUE_BINS) atomicAdd(&bins[bin], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < VALUE_BINS && i < nodes - 1u; i += blockDim.x)
        if (bins[i]) atomicAdd(&cells[i + 1], (unsigned long long)bins[i]);
}

// the keys of the old set into the new, larger one (no key is in it twice: a plain claim of the first empty slot)
__global__ __launch_bounds__(256) void k_set_rehash(const unsigned long long *old, const uint64_t old_cap, unsigned long long *set,
                                                    const uint64_t cap, const uint64_t magic, int *full) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_cap; i += stride) {
        const unsigned long long key = old[i];
        if (key == 0) continue;
        uint64_t idx = mod_capacity(fmix64(key - 1), cap, magic);
        bool placed = false;
        for (uint64_t tries = 0; tries < cap; tries++) {
            if (atomicCAS(&set[idx], 0ull, key) == 0) {
                placed = true;
                break;
            }
            idx++;
            if (idx >= cap) idx = 0;
        }
        if (!placed) __hip_atomic_store(full, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
#define BUILD_TRY(expr)                                                                                                        \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) {                                                                                                \
            (void)hipGetLastError();                                                                                           \
            return set_error(_e == hipErrorOutOfMemory ? NH_EOOM : NH_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e));        \
        }                                                                                                                      \
    } while (0)

constexpr uint64_t DEFAULT_PIECE_KMERS = 16 * (TL - 4);  // 1984: 16 tiles, 1.7 % of the text read twice
constexpr uint64_t DEFAULT_BATCH_BYTES = 128ull << 20;
constexpr uint32_t TAXON_NODE = 2;                       // one taxon: three nodes, 0 the null sentinel, 1 root, 2 the taxon
constexpr int N_COUNTERS = 8;  // claimed, clean, `full` (an int), masked bases, then of several taxa: LCA merges, values replaced, insertions; EXCLUDE: slots flagged
const char *const DB_FILES[3] = {"hash.k2d", "opts.k2d", "taxo.k2d"};

double since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// one input file and the node (internal id) its sequences belong to
struct BuildInput {
    std::string path;
    uint32_t node;
};

// COUNT and INSERT read the host's inputs; EXCLUDE reads the exclusion list against the set of COUNT and is never masked
enum class Pass { COUNT, EXCLUDE, INSERT };

// what one pass found, every field from zero at its start
struct PassResult {
    unsigned long long claimed = 0;  // COUNT: slots, INSERT: cells, EXCLUDE: look-ups
    unsigned long long clean = 0;    // k-mers that are not ambiguous (INSERT, EXCLUDE)
    unsigned long long flagged = 0;  // EXCLUDE: slots flagged
    unsigned long long masked = 0;
    unsigned long long merges = 0, swaps = 0, inserts = 0;  // INSERT of several taxa
    uint64_t sequences = 0, bases = 0, kmers = 0;           // of the inputs read
    double seconds_read = 0, seconds_gpu = 0;
    double seconds_kernel = 0;  // of seconds_gpu: the pass's kernel alone (HIP events; the rest is copies, set growth and waits)
    double seconds_mask = 0;    // the mask kernel alone
};

struct Builder {
    // arguments
    uint64_t piece = DEFAULT_PIECE_KMERS, batch_cap = DEFAULT_BATCH_BYTES;
    bool mask = false;  // low-complexity masking
    int device = 0;
    unsigned threads = 0;
    int ambig_rule = 1;
    // the batch being filled (host)
    std::vector<char> text;
    std::vector<uint64_t> starts;
    std::vector<uint32_t> lens;
    std::vector<uint32_t> values;  // several taxa: the internal id of each piece's taxon
    uint32_t cur_value = TAXON_NODE;  // the taxon of the file being read (a sequence cut at a batch's end keeps it in the next batch)
    uint64_t batch_kmers = 0;
    std::vector<DustTile> tiles;  // masking: the tiles of the batch's chunks
    uint64_t ctx_bytes = 0;       // masking: bytes of the batch that are context, beside batch_cap
    // device
    hipStream_t stream = nullptr;
    int grid_max = 0;
    // (every buffer and event below is the builder's own: ~Builder selects the device, they go back behind it)
    DevBuf<char> d_text;
    DevBuf<uint64_t> d_starts;  // the pieces' arrays: regrown together, when a batch has more pieces than they hold
    DevBuf<uint32_t> d_lens;
    DevBuf<uint32_t> d_values;
    // several taxa: the node table and the cells per node, resident for the whole build
    bool multi = false;
    uint32_t node_count = 3, vbits = 2;
    std::vector<uint32_t> parent;  // 2^vbits entries
    DevBuf<uint32_t> d_parent;
    DevBuf<unsigned long long> d_cells;
    double t_cells = 0;  // k_value_cells alone
    DevBuf<char> d_raw;  // masking: the batch as it was uploaded, which the mask kernel reads while it writes d_text
    DevBuf<DustTile> d_tiles;
    int dust_grid = 0;
    DevBuf<unsigned long long> d_counters;  // N_COUNTERS: two counters, then `full` as an int, then the masked bases, ...
    DevBuf<unsigned long long> d_set;  // (d_set.cap: its slots)
    DevBuf<uint32_t> d_table;
    uint64_t capacity = 0;
    bool filter = false;  // the set carries the flags of an EXCLUDE pass: INSERT skips what is flagged
    Events<4> ev;  // around the pass's kernel [0, 1] and the mask kernel [2, 3]
    // the pass that is running, and what it has found so far
    Pass kind = Pass::INSERT;
    bool dust = false;  // it masks its text: `mask`, but never EXCLUDE
    PassResult res;
    std::vector<nh_build_taxon_stats> per_node;  // by internal id: sequences, bases and k-mers from the first pass over the host's inputs
    bool tallied = false;                        // that pass is over

    ~Builder() {
        if (device >= 0 && stream) (void)dev_set(device);
        if (stream) (void)hipStreamDestroy(stream);
    }

    int *d_full() const { return (int *)(d_counters.p + 2); }

    int init() {
        BUILD_TRY(dev_set(device));
        hipDeviceProp_t prop;
        BUILD_TRY(hipGetDeviceProperties(&prop, dev_phys(device)));
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_build_pieces<false, false>, WAVE * WAVES_PER_BLOCK, 0) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 4;
        }
        grid_max = prop.multiProcessorCount * (per_cu > 8 ? 8 : per_cu);
        BUILD_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        BUILD_TRY(ev.create());
        // (masking: up to 63 bases of context at either end of a batch)
        const size_t text_cap = batch_cap + (mask ? 2 * DUST_CONTEXT : 0) + 64;
        BUILD_TRY(d_text.reserve(text_cap));
        if (mask) {
            BUILD_TRY(d_raw.reserve(text_cap));
            dust_grid = dust_grid_max();
        }
        BUILD_TRY(d_counters.reserve(N_COUNTERS));
        if (multi) {
            BUILD_TRY(d_parent.reserve(parent.size()));
            BUILD_TRY(hipMemcpyAsync(d_parent, parent.data(), parent.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            BUILD_TRY(d_cells.reserve(node_count));
            BUILD_TRY(hipMemsetAsync(d_cells, 0, (size_t)node_count * sizeof(unsigned long long), stream));
            BUILD_TRY(hipStreamSynchronize(stream));
        }
        text.reserve(batch_cap);
        return NH_OK;
    }

    // COUNT: slots >= 2 x (keys in the set + keys this batch can add)
    int grow_set(uint64_t need_keys) {
        uint64_t need = 2 * need_keys + 64;
        const uint64_t set_cap = d_set.cap;
        if (need <= set_cap) return NH_OK;
        uint64_t ncap = set_cap ? set_cap : (1ull << 16);
        while (ncap < need) ncap *= 2;
        DevBuf<unsigned long long> nset;  // (beside the old set, which it is rehashed from)
        hipError_t he = nset.reserve(ncap);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            return set_error(NH_EOOM, "cannot allocate the counting set of the build (%llu slots, %.1f GiB, beside %.1f GiB in use): give the "
                             "table's size with `capacity` (--capacity) and the counting pass is skipped",
                             (unsigned long long)ncap, (double)ncap * 8 / (1ull << 30), (double)set_cap * 8 / (1ull << 30));
        }
        he = hipMemsetAsync(nset, 0, ncap * sizeof(unsigned long long), stream);
        if (he == hipSuccess && d_set) {
            const uint64_t want = (set_cap + 255) / 256;
            hipLaunchKernelGGL(k_set_rehash, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, stream, d_set, set_cap, nset, ncap,
                               ~0ull / ncap, d_full());
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipStreamSynchronize(stream);
        if (he != hipSuccess) return set_error(NH_EDEVICE, "growing the counting set: %s", hipGetErrorString(he));
        d_set = std::move(nset);  // (the old set goes back here)
        return NH_OK;
    }

    int alloc_table(uint64_t cap) {
        capacity = cap;
        const uint64_t cells = ((cap + 3) & ~3ull) + 32;
        hipError_t he = d_table.reserve(cells);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            return set_error(NH_EOOM, "cannot allocate the hash table of the build (%llu cells, %.1f GiB)", (unsigned long long)cap,
                             (double)cells * 4 / (1ull << 30));
        }
        BUILD_TRY(hipMemsetAsync(d_table, 0, cells * sizeof(uint32_t), stream));
        BUILD_TRY(hipStreamSynchronize(stream));
        return NH_OK;
    }

    // the batch to the device, one launch, its totals back
    int flush() {
        if (starts.empty() && tiles.empty()) {
            text.clear();
            batch_kmers = ctx_bytes = 0;
            return NH_OK;
        }
        auto t0 = std::chrono::steady_clock::now();
        const uint64_t n_piece = starts.size();
        if (kind == Pass::COUNT) {
            int rc = grow_set(res.claimed + batch_kmers);
            if (rc) return rc;
        }
        const uint64_t piece_cap = n_piece + n_piece / 2 + 1024;
        BUILD_TRY(d_starts.reserve(n_piece, piece_cap));
        BUILD_TRY(d_lens.reserve(n_piece, piece_cap));
        if (multi) BUILD_TRY(d_values.reserve(n_piece, piece_cap));
        BUILD_TRY(hipMemcpyAsync(d_text, text.data(), text.size(), hipMemcpyHostToDevice, stream));
        BUILD_TRY(hipMemsetAsync(d_text + text.size(), 0, 64, stream));
        if (n_piece) {
            BUILD_TRY(hipMemcpyAsync(d_starts, starts.data(), n_piece * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            BUILD_TRY(hipMemcpyAsync(d_lens, lens.data(), n_piece * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            if (multi && kind == Pass::INSERT) BUILD_TRY(hipMemcpyAsync(d_values, values.data(), n_piece * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        const bool masking = !tiles.empty();
        if (masking) {
            BUILD_TRY(d_tiles.reserve(tiles.size(), tiles.size() + tiles.size() / 2 + 1024));
            BUILD_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(DustTile), hipMemcpyHostToDevice, stream));
            BUILD_TRY(hipMemcpyAsync(d_raw, d_text, text.size() + 64, hipMemcpyDeviceToDevice, stream));
            BUILD_TRY(hipEventRecord(ev[2], stream));
            BUILD_TRY(launch_dust(d_raw, d_text, text.size(), d_tiles, tiles.size(), d_counters + 3, dust_grid, stream));
            BUILD_TRY(hipEventRecord(ev[3], stream));
        }
        KArgs ka;
        memset(&ka, 0, sizeof ka);
        DevDB &d = ka.db;
        d.table = d_table;
        d.n_copies = 1;
        d.copy_shift = 5;
        d.capacity = kind == Pass::INSERT ? capacity : 1;
        d.cap_magic = ~0ull / d.capacity;
        d.node_count = node_count;
        d.value_bits = vbits;
        d.vmask = (1u << vbits) - 1;
        d.k = 35, d.l = 31, d.window = 4;
        d.lmer_mask = (1ull << 62) - 1;
        d.spaced_mask = SPACED_MASK;
        d.toggle = TOGGLE_MASK & d.lmer_mask;
        d.min_hash = 0;
        d.revcom_version = 1;
        d.linear_probing = 1;
        d.ambig_rule = ambig_rule;
        ka.bases = (const uint8_t *)d_text.p;
        ka.seq_off = d_starts;
        ka.seq_len = d_lens;
        ka.bases_end = text.size();
        ka.n_frag = n_piece;
        BuildDev b;
        memset(&b, 0, sizeof b);
        b.set = d_set;
        b.set_cap = kind != Pass::INSERT || filter ? d_set.cap : 1;
        b.set_magic = ~0ull / b.set_cap;
        b.counters = d_counters;
        b.full = d_full();
        b.value = TAXON_NODE;
        b.piece_value = d_values;
        b.parent = d_parent;
        const uint64_t want = (n_piece + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
        const unsigned grid = (unsigned)(want < (uint64_t)grid_max ? want : (uint64_t)grid_max);
        void (*kernel)(KArgs, BuildDev) = nullptr;
        switch (kind) {
        case Pass::COUNT: kernel = k_build_pieces<true, false>; break;
        case Pass::EXCLUDE: kernel = k_exclude_pieces; break;
        case Pass::INSERT:
            kernel = multi ? (filter ? k_build_pieces<false, true, true> : k_build_pieces<false, true>)
                           : (filter ? k_build_pieces<false, false, true> : k_build_pieces<false, false>);
            break;
        }
        BUILD_TRY(hipEventRecord(ev[0], stream));
        // (no piece, masking: a batch of sequences too short for a k-mer)
        if (n_piece) hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, ka, b);
        BUILD_TRY(hipGetLastError());
        BUILD_TRY(hipEventRecord(ev[1], stream));
        unsigned long long out[N_COUNTERS] = {0, 0, 0, 0, 0, 0, 0, 0};
        BUILD_TRY(hipMemcpyAsync(out, d_counters, sizeof out, hipMemcpyDeviceToHost, stream));
        BUILD_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) res.seconds_kernel += ms * 1e-3;
        else (void)hipGetLastError();
        if (masking) {
            if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) res.seconds_mask += ms * 1e-3;
            else (void)hipGetLastError();
        }
        res.claimed = out[0];
        res.clean = out[1];
        res.masked = out[3];
        res.merges = out[4];
        res.swaps = out[5];
        res.inserts = out[6];
        res.flagged = out[7];
        int full;
        memcpy(&full, &out[2], sizeof full);
        text.clear();
        starts.clear();
        lens.clear();
        values.clear();
        tiles.clear();
        batch_kmers = ctx_bytes = 0;
        res.seconds_gpu += since(t0);
        if (full && kind == Pass::COUNT) return set_error(NH_EDEVICE, "the counting set of the build overflowed (%llu slots): this is a bug", (unsigned long long)d_set.cap);
        if (full)
            return set_error(NH_ECAPACITY, "the table of %llu cells is full: the input has more distinct minimizers than `capacity` holds "
                             "(leave capacity 0 and it is counted)", (unsigned long long)capacity);
        return NH_OK;
    }

    // one sequence into the batches: pieces of `piece` k-mers, the batch's end a cut like any other
    int add_sequence(const char *s, size_t n) {
        if (n < 35) return dust ? add_short(s, n) : NH_OK;
        const size_t nk = n - 34;
        size_t pos = 0;  // the first k-mer not yet in a piece (= its first base)
        while (pos < nk) {
            const size_t room = batch_cap + ctx_bytes - text.size();
            if (room < 35) {
                int rc = flush();
                if (rc) return rc;
                continue;
            }
            const size_t left = n - pos;
            const size_t take = left < room ? left : room;  // bases, >= 35
            const size_t mk = take - 34;                     // their k-mers
            // masking: the chunk with up to 63 bases of the sequence on either side; its masked bases are counted where they are
            // k-mer starts of this chunk, and through the sequence's end in its last chunk
            const size_t cl = !dust ? 0 : pos < DUST_CONTEXT ? pos : (size_t)DUST_CONTEXT;
            const size_t behind = n - (pos + take);
            const size_t cr = !dust ? 0 : behind < DUST_CONTEXT ? behind : (size_t)DUST_CONTEXT;
            const uint64_t t = text.size() + cl;
            text.insert(text.end(), s + pos - cl, s + pos + take + cr);
            if (dust) {
                dust_tiles(tiles, t - cl, cl + take + cr, cl, cl + (behind ? mk : take));
                ctx_bytes += cl + cr;
            }
            for (size_t p = 0; p < mk; p += piece) {
                const size_t pk = mk - p < piece ? mk - p : (size_t)piece;
                starts.push_back(t + p);
                lens.push_back((uint32_t)(pk + 34));
                if (multi) values.push_back(cur_value);
            }
            batch_kmers += mk;
            pos += mk;
        }
        return NH_OK;
    }

    // masking: a sequence too short for a k-mer has no piece, but its masked bases are counted like any other's
    int add_short(const char *s, size_t n) {
        if (n < 7) return NH_OK;  // (fewer than 7 bases hold no perfect interval)
        if (batch_cap + ctx_bytes - text.size() < n) {
            int rc = flush();
            if (rc) return rc;
        }
        dust_tiles(tiles, text.size(), n, 0, n);
        text.insert(text.end(), s, s + n);
        return NH_OK;
    }

    // the cells per node of the finished table into per_node (several taxa)
    int count_cells() {
        const uint64_t want = (capacity + 4095) / 4096;
        const unsigned grid = (unsigned)(want < (uint64_t)grid_max ? (want ? want : 1) : (uint64_t)grid_max);
        BUILD_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(k_value_cells, dim3(grid), dim3(256), 0, stream, d_table, capacity, (1u << vbits) - 1u, node_count, d_cells);
        BUILD_TRY(hipGetLastError());
        BUILD_TRY(hipEventRecord(ev[1], stream));
        std::vector<unsigned long long> out(node_count, 0);
        BUILD_TRY(hipMemcpyAsync(out.data(), d_cells, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        BUILD_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) t_cells = ms * 1e-3;
        else (void)hipGetLastError();
        for (uint32_t i = 1; i < node_count; i++) per_node[i].cells = out[i];
        return NH_OK;
    }

    // every record of every input through add_sequence -> what the pass found
    int pass(const std::vector<BuildInput> &inputs, Pass k, PassResult &out) {
        kind = k;
        dust = mask && kind != Pass::EXCLUDE;
        res = PassResult();
        BUILD_TRY(hipMemsetAsync(d_counters, 0, N_COUNTERS * sizeof(unsigned long long), stream));
        BUILD_TRY(hipStreamSynchronize(stream));
        const bool tally = kind != Pass::EXCLUDE && !tallied;
        int rc;
        SeqRecord rec;
        for (const BuildInput &in : inputs) {
            FastxReader rd;
            std::string err;
            auto t0 = std::chrono::steady_clock::now();
            if (rd.open(in.path.c_str(), err, threads) != 0) return set_error(NH_EIO, "%s", err.c_str());
            cur_value = in.node;
            nh_build_taxon_stats &pn = per_node[in.node];
            for (;;) {
                const int got = rd.next(rec, err);
                if (got < 0) return set_error(NH_EIO, "%s: %s", in.path.c_str(), err.c_str());
                if (got == 0) break;
                res.seconds_read += since(t0);
                const uint64_t n = rec.seq.size(), nk = n >= 35 ? n - 34 : 0;
                res.sequences++, res.bases += n, res.kmers += nk;
                if (tally) pn.sequences++, pn.bases += n, pn.kmers += nk;
                rc = add_sequence(rec.seq.data(), rec.seq.size());
                if (rc) return rc;
                t0 = std::chrono::steady_clock::now();
            }
            res.seconds_read += since(t0);
        }
        rc = flush();
        tallied = tallied || tally;
        out = res;
        return rc;
    }
};

bool file_there(const std::string &p) {
    struct stat st;
    return lstat(p.c_str(), &st) == 0;
}

std::string real_of(const std::string &p) {
    char buf[PATH_MAX];
    return realpath(p.c_str(), buf) ? std::string(buf) : std::string();
}

// is `input` one of the three files of out_dir (by inode where the file exists, by name where it does not yet)
bool input_is_output(const char *input, const std::string &out_dir) {
    struct stat si;
    const bool have_i = stat(input, &si) == 0;
    std::string in = input;
    const size_t slash = in.find_last_of('/');
    const std::string base = slash == std::string::npos ? in : in.substr(slash + 1);
    const std::string dir = slash == std::string::npos ? "." : slash == 0 ? "/" : in.substr(0, slash);
    for (const char *name : DB_FILES) {
        struct stat so;
        if (have_i && stat((out_dir + "/" + name).c_str(), &so) == 0 && so.st_dev == si.st_dev && so.st_ino == si.st_ino) return true;
        if (base == name) {
            const std::string a = real_of(dir), b = real_of(out_dir);
            if (!a.empty() && a == b) return true;
        }
    }
    return false;
}

std::vector<uint8_t> opts_image() {
    std::vector<uint8_t> ob(64, 0);
    const uint64_t v[4] = {35, 31, SPACED_MASK, TOGGLE_MASK};
    memcpy(ob.data(), v, 32);
    ob[32] = 1;  // dna_db
    const int32_t rv = 1;
    memcpy(ob.data() + 48, &rv, 4);  // (minimum_acceptable_hash_value at 40, db_version and db_type behind revcom_version: 0)
    return ob;
}

// "K2TAXDAT", node count, bytes of the name and the rank strings, 56-byte nodes {parent, first child, child count,
// name offset, rank offset, external id, godparent}, the two string tables.  The sentinel shares the root's name, "root".  The
// rank table holds the distinct rank strings in the order of their first use: "no rank" alone unless an extended base had others.
std::vector<uint8_t> taxo_image(const std::vector<TaxaNode> &nodes) {
    std::string names = nodes[1].name + '\0';
    std::string ranks;
    std::vector<std::pair<std::string, uint64_t>> rank_at;
    std::vector<uint64_t> recs(nodes.size() * 7, 0);
    for (size_t i = 1; i < nodes.size(); i++) {
        uint64_t *r = &recs[i * 7];
        r[0] = nodes[i].parent, r[1] = nodes[i].first_child, r[2] = nodes[i].children, r[5] = nodes[i].taxid;
        size_t k = 0;
        while (k < rank_at.size() && rank_at[k].first != nodes[i].rank) k++;
        if (k == rank_at.size()) {
            rank_at.push_back({nodes[i].rank, ranks.size()});
            ranks += nodes[i].rank;
            ranks += '\0';
        }
        r[4] = rank_at[k].second;
        if (i >= 2) {
            r[3] = names.size();
            names += nodes[i].name;
            names += '\0';
        }
    }
    std::vector<uint8_t> img;
    img.insert(img.end(), (const uint8_t *)"K2TAXDAT", (const uint8_t *)"K2TAXDAT" + 8);
    const uint64_t hdr[3] = {nodes.size(), names.size(), ranks.size()};
    img.insert(img.end(), (const uint8_t *)hdr, (const uint8_t *)hdr + 24);
    img.insert(img.end(), (const uint8_t *)recs.data(), (const uint8_t *)recs.data() + recs.size() * sizeof(uint64_t));
    img.insert(img.end(), names.begin(), names.end());
    img.insert(img.end(), ranks.begin(), ranks.end());
    return img;
}

bool write_all(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

bool write_file(const std::string &path, const std::vector<uint8_t> &img) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = write_all(f, img.data(), img.size());
    return (fclose(f) == 0) && ok;
}

// the three files under temporary names, then renamed into place; on any failure nothing of this call stays behind
int write_database(Builder &B, const nh_build_args *a, const std::vector<TaxaNode> &nodes, uint64_t size, const std::vector<uint8_t> *opts = nullptr) {
    const std::string dir = a->out_dir;
    bool made_dir = false;
    struct stat st;
    if (stat(dir.c_str(), &st) != 0) {
        if (mkdir(dir.c_str(), 0777) != 0) return set_error(NH_EIO, "cannot create %s: %s", dir.c_str(), strerror(errno));
        made_dir = true;
    }
    char suffix[48];
    snprintf(suffix, sizeof suffix, ".tmp%ld", (long)getpid());
    std::string tmp[3], fin[3];
    for (int i = 0; i < 3; i++) fin[i] = dir + "/" + DB_FILES[i], tmp[i] = fin[i] + suffix;
    auto fail = [&](int code, const std::string &msg) {
        for (const std::string &t : tmp) unlink(t.c_str());
        if (made_dir) rmdir(dir.c_str());
        return set_error(code, "%s", msg.c_str());
    };
    {   // hash.k2d: {capacity, size, key_bits, value_bits}, then the cells, fetched from the device a stretch at a time
        FILE *f = fopen(tmp[0].c_str(), "wb");
        if (!f) return fail(NH_EIO, "cannot write " + tmp[0] + ": " + strerror(errno));
        const uint64_t hdr[4] = {B.capacity, size, 32 - B.vbits, B.vbits};
        bool ok = write_all(f, hdr, sizeof hdr);
        const uint64_t step = 16ull << 20;  // cells
        std::vector<uint32_t> buf((size_t)(B.capacity < step ? B.capacity : step));
        hipError_t he = hipSuccess;
        for (uint64_t c = 0; ok && c < B.capacity; c += step) {
            const uint64_t n = B.capacity - c < step ? B.capacity - c : step;
            he = hipMemcpy(buf.data(), B.d_table + c, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
            if (he != hipSuccess) break;
            ok = write_all(f, buf.data(), n * sizeof(uint32_t));
        }
        ok = (fclose(f) == 0) && ok;
        if (he != hipSuccess) return fail(NH_EDEVICE, std::string("fetching the table: ") + hipGetErrorString(he));
        if (!ok) return fail(NH_EIO, "cannot write " + tmp[0]);
    }
    if (!write_file(tmp[1], opts ? *opts : opts_image())) return fail(NH_EIO, "cannot write " + tmp[1]);
    if (!write_file(tmp[2], taxo_image(nodes))) return fail(NH_EIO, "cannot write " + tmp[2]);
    for (int i = 0; i < 3; i++)
        if (rename(tmp[i].c_str(), fin[i].c_str()) != 0) return fail(NH_EIO, "cannot move " + tmp[i] + " into place: " + strerror(errno));
    return NH_OK;
}

// what the arguments ask for, once they have passed every check that needs no device
struct BuildPlan {
    bool grown = false, v3 = false;  // the caller's layout: masking is read; the taxa fields are read
    size_t stats_size = NH_BUILD_STATS_SIZE_V1;
    double lf = 0.7;
    std::vector<TaxaNode> nodes;     // [0] the sentinel, [1] the root, then the taxa in internal-id order
    std::vector<BuildInput> inputs;  // in the order they are read: by node, a node's files as given
};

// the database an extension starts from (nh_extend_db), as far as the host reads it
struct BasePlan {
    std::string dir;
    uint64_t capacity = 0, size = 0, old_vb = 0;
    std::vector<uint8_t> opts;    // opts.k2d as it is
    BaseTaxo taxo;
    std::vector<uint32_t> remap;  // internal id of the base -> internal id of the merged tree
};

// (the caller's layout is told by struct_size: one of an earlier layout gets that layout's stats and no more)
void layout_of(const nh_build_args *a, BuildPlan &P) {
    P.grown = a && a->struct_size >= NH_BUILD_ARGS_SIZE_V2;
    P.v3 = a && a->struct_size >= sizeof(nh_build_args);
    P.stats_size = P.v3 ? sizeof(nh_build_stats) : P.grown ? (size_t)NH_BUILD_STATS_SIZE_V2 : (size_t)NH_BUILD_STATS_SIZE_V1;
}

// ---- arguments: everything refused here is refused before any device is touched and before anything is created
int plan_build(const nh_build_args *a, BuildPlan &P, BasePlan *base = nullptr) {
    if (!a) return set_error(NH_EINVAL, "nh_build_db: null arguments");
    if (a->struct_size < NH_BUILD_ARGS_SIZE_V1)
        return set_error(NH_EINVAL, "nh_build_db: struct_size %u is smaller than nh_build_args (%u)", a->struct_size, NH_BUILD_ARGS_SIZE_V1);
    const char *taxa_file = P.v3 ? a->taxa_file : nullptr;
    if (taxa_file) {
        if (!*taxa_file) return set_error(NH_EINVAL, "nh_build_db: taxa_file is an empty path");
        if (a->n_fasta != 0 || a->fasta) return set_error(NH_EINVAL, "nh_build_db: taxa_file cannot be combined with fasta / n_fasta: the manifest lists the FASTA files");
        if (a->taxid != 0) return set_error(NH_EINVAL, "nh_build_db: taxa_file cannot be combined with taxid: the manifest gives the taxids");
        if (a->taxon_name) return set_error(NH_EINVAL, "nh_build_db: taxa_file cannot be combined with taxon_name: the manifest gives the names");
    } else {
        if (a->n_fasta == 0 || !a->fasta) return set_error(NH_EINVAL, "nh_build_db: no input (n_fasta 0)");
        for (uint32_t i = 0; i < a->n_fasta; i++)
            if (!a->fasta[i]) return set_error(NH_EINVAL, "nh_build_db: input %u is a null path", i);
    }
    if (!a->out_dir || !*a->out_dir) return set_error(NH_EINVAL, "nh_build_db: no output directory");
    P.lf = a->load_factor == 0 ? (base ? 0.95 : 0.7) : a->load_factor;
    if (!(P.lf > 0 && P.lf <= 0.95)) return set_error(NH_EINVAL, "nh_build_db: load factor %g is not in (0, 0.95]", a->load_factor);
    if (a->taxid == 1) return set_error(NH_EINVAL, "nh_build_db: taxid 1 is the root of the taxonomy, not a taxon to build");
    // (a probe-queue entry of the classifier packs the home cell and the 30-bit key into 63 bits)
    if (a->capacity >> 33) return set_error(NH_EINVAL, "nh_build_db: capacity %llu is not below 2^33", (unsigned long long)a->capacity);
    const std::string dir = a->out_dir;
    struct stat st;
    if (stat(dir.c_str(), &st) == 0 && !S_ISDIR(st.st_mode)) return set_error(NH_EINVAL, "nh_build_db: %s is not a directory", dir.c_str());
    if (taxa_file) {
        if (input_is_output(taxa_file, dir))
            return set_error(NH_EINVAL, "nh_build_db: the taxa manifest %s is a database file of the output directory %s", taxa_file, dir.c_str());
        std::string err;
        const int rc = base ? merge_taxa(taxa_file, base->taxo, P.nodes, base->remap, err) : parse_taxa(taxa_file, P.nodes, err);
        if (rc) return set_error(rc, "%s", err.c_str());
        for (size_t i = 2; i < P.nodes.size(); i++)
            for (const std::string &f : P.nodes[i].files) {
                if (input_is_output(f.c_str(), dir))
                    return set_error(NH_EINVAL, "nh_build_db: %s line %u: the input %s is a database file of the output directory %s", taxa_file,
                                     P.nodes[i].line, f.c_str(), dir.c_str());
                P.inputs.push_back({f, (uint32_t)i});
            }
    } else {
        for (uint32_t i = 0; i < a->n_fasta; i++)
            if (input_is_output(a->fasta[i], dir))
                return set_error(NH_EINVAL, "nh_build_db: the input %s is a database file of the output directory %s", a->fasta[i], dir.c_str());
    }
    if (!a->force)
        for (const char *name : DB_FILES)
            if (file_there(dir + "/" + name))
                return set_error(NH_EINVAL, "nh_build_db: %s already holds %s (`force` replaces a database)", dir.c_str(), name);
    if (!taxa_file && base) {  // one taxon on a base: a child of the root, or the node the base has for it
        const uint64_t taxid = a->taxid ? a->taxid : 9606;
        const std::string name = a->taxon_name ? a->taxon_name : taxid == 9606 ? "Homo sapiens" : "taxon" + std::to_string(taxid);
        std::string err;
        const int rc = merge_taxon(taxid, name, std::vector<std::string>(a->fasta, a->fasta + a->n_fasta), base->taxo, P.nodes, base->remap, err);
        if (rc) return set_error(rc, "%s", err.c_str());
        for (size_t i = 2; i < P.nodes.size(); i++)
            for (const std::string &f : P.nodes[i].files) P.inputs.push_back({f, (uint32_t)i});
    } else if (!taxa_file) {  // one taxon: the three nodes it always had
        const uint64_t taxid = a->taxid ? a->taxid : 9606;
        P.nodes.resize(3);
        P.nodes[1].taxid = 1, P.nodes[1].name = "root", P.nodes[1].first_child = 2, P.nodes[1].children = 1;
        P.nodes[2].taxid = taxid, P.nodes[2].parent = 1;
        if (a->taxon_name) P.nodes[2].name = a->taxon_name;
        else if (taxid == 9606) P.nodes[2].name = "Homo sapiens";
        else P.nodes[2].name = "taxon" + std::to_string(taxid);
        for (uint32_t i = 0; i < a->n_fasta; i++) P.inputs.push_back({a->fasta[i], TAXON_NODE});
    }
    return NH_OK;
}

// the per-node results into the caller's array (present layout only)
void give_taxon_stats(const nh_build_args *a, const BuildPlan &P, const std::vector<nh_build_taxon_stats> &per_node) {
    if (!P.v3 || !a->taxon_stats) return;
    for (uint32_t i = 1; i < per_node.size() && i - 1 < a->taxon_stats_cap; i++) a->taxon_stats[i - 1] = per_node[i];
}

// the per-node table of a plan before anything is read: the taxids, every count zero
std::vector<nh_build_taxon_stats> zero_per_node(const std::vector<TaxaNode> &nodes) {
    std::vector<nh_build_taxon_stats> per_node(nodes.size());
    for (size_t i = 0; i < nodes.size(); i++) memset(&per_node[i], 0, sizeof per_node[i]), per_node[i].taxid = nodes[i].taxid;
    return per_node;
}

// what a *_check call hands back of a plan that passed: the taxa and their zeroed table
void give_plan(const nh_build_args *a, const BuildPlan &P, nh_build_stats *stats) {
    give_taxon_stats(a, P, zero_per_node(P.nodes));
    if (stats && P.v3) stats->taxa = P.nodes.size() - 1;
}

// a caller's nh_exclude_stats or nh_extend_stats filled from v, its struct_size kept
template <class T>
void give_stats(T *xs, const T &v) {
    if (!xs) return;
    const uint32_t size = xs->struct_size;
    *xs = v;
    xs->struct_size = size, xs->reserved = 0;
}

int build_check(const nh_build_args *a, nh_build_stats *stats) {
    BuildPlan P;
    layout_of(a, P);
    if (stats) memset(stats, 0, P.stats_size);
    const int rc = plan_build(a, P);
    if (rc) return rc;
    give_plan(a, P, stats);
    return NH_OK;
}

// ---- nh_build_db_exclude: the checks of the exclusion list that need no device -----------------------------------
// (an exclusion list is in force only where x is there and names a file: without one the call is nh_build_db)
bool excluding_with(const nh_exclude_args *x) { return x && x->struct_size >= sizeof(nh_exclude_args) && x->n_fasta != 0; }

// the struct sizes: looked at even where the list is empty
int check_exclude_layout(const nh_exclude_args *x, const nh_exclude_stats *xs) {
    if (x && x->struct_size < sizeof(nh_exclude_args))
        return set_error(NH_EINVAL, "nh_build_db_exclude: struct_size %u is smaller than nh_exclude_args (%u)", x->struct_size, (unsigned)sizeof(nh_exclude_args));
    if (xs && xs->struct_size < sizeof(nh_exclude_stats))
        return set_error(NH_EINVAL, "nh_build_db_exclude: struct_size %u is smaller than nh_exclude_stats (%u)", xs->struct_size, (unsigned)sizeof(nh_exclude_stats));
    return NH_OK;
}

// the files of the list against out_dir, the host's inputs (P.inputs: plan_build has passed) and each other -> `files`
int plan_exclude(const nh_build_args *a, const nh_exclude_args *x, const BuildPlan &P, std::vector<BuildInput> &files) {
    if (!x->fasta) return set_error(NH_EINVAL, "nh_build_db_exclude: n_fasta is %u but fasta is null", x->n_fasta);
    for (uint32_t i = 0; i < x->n_fasta; i++)
        if (!x->fasta[i]) return set_error(NH_EINVAL, "nh_build_db_exclude: exclusion file %u is a null path", i);
    const std::string dir = a->out_dir;
    // (a file that does not exist has no real path: it is compared by its name and fails as unreadable later)
    auto id_of = [](const std::string &p) {
        const std::string r = real_of(p);
        return r.empty() ? p : r;
    };
    std::vector<std::string> host;
    for (const BuildInput &in : P.inputs) host.push_back(id_of(in.path));
    std::vector<std::string> seen;
    for (uint32_t i = 0; i < x->n_fasta; i++) {
        const char *f = x->fasta[i];
        if (input_is_output(f, dir))
            return set_error(NH_EINVAL, "nh_build_db_exclude: the exclusion file %s is a database file of the output directory %s", f, dir.c_str());
        const std::string id = id_of(f);
        for (size_t h = 0; h < host.size(); h++)
            if (host[h] == id)
                return set_error(NH_EINVAL, "nh_build_db_exclude: the exclusion file %s is also an input of the build (%s): every minimizer would be "
                                 "excluded", f, P.inputs[h].path.c_str());
        for (const std::string &s : seen)
            if (s == id) return set_error(NH_EINVAL, "nh_build_db_exclude: the exclusion file %s is given twice", f);
        seen.push_back(id);
        files.push_back({f, 0});
    }
    return NH_OK;
}

int exclude_check(const nh_build_args *a, const nh_exclude_args *x, nh_build_stats *stats, nh_exclude_stats *xs) {
    int rc = check_exclude_layout(x, xs);
    if (rc) return rc;
    if (!excluding_with(x)) return build_check(a, stats);
    BuildPlan P;
    layout_of(a, P);
    if (stats) memset(stats, 0, P.stats_size);
    rc = plan_build(a, P);
    if (rc) return rc;
    std::vector<BuildInput> files;
    rc = plan_exclude(a, x, P, files);
    if (rc) return rc;
    give_plan(a, P, stats);
    nh_exclude_stats v;
    memset(&v, 0, sizeof v);
    give_stats(xs, v);
    return NH_OK;
}

// The builder of a build or an extension, from the arguments and a plan that passed: the taxonomy's tables (value fields of at least
// min_vbits bits), the sizes of pieces and batches -- the environment knobs are read here -- and then the device.
int configure(Builder &B, const nh_build_args *a, const BuildPlan &P, bool multi, uint32_t min_vbits) {
    B.device = a->device;
    B.threads = a->threads;
    B.mask = P.grown && a->mask_low_complexity != 0;
    B.node_count = (uint32_t)P.nodes.size();
    B.multi = multi;
    B.vbits = value_bits_for(B.node_count);
    if (B.vbits < min_vbits) B.vbits = min_vbits;
    B.parent.assign((size_t)1 << B.vbits, 0);
    for (uint32_t i = 0; i < B.node_count; i++) B.parent[i] = P.nodes[i].parent;
    B.per_node = zero_per_node(P.nodes);
    if (a->piece_kmers) B.piece = a->piece_kmers < (1ull << 31) ? a->piece_kmers : (1ull << 31);
    if (const char *env = getenv("NOHUMAN_BUILD_BATCH")) {  // test knob: bytes of text per batch (sequences cut at the batches' ends)
        const long long v = atoll(env);
        if (v > 0) B.batch_cap = (uint64_t)v < 64 ? 64 : (uint64_t)v;
    }
    if (const char *env = getenv("NOHUMAN_OPT_AMBIGUITY_RULE")) B.ambig_rule = atoi(env) != 0 ? 1 : 0;  // as the classifier reads it
    else B.ambig_rule = NH_AMBIGUITY_DEFAULT == NH_AMBIGUITY_LAST_LMER ? 0 : 1;
    return B.init();
}

// the fields of nh_build_stats that a build and an extension fill alike.  `count` is null where no COUNT pass ran; the totals of the
// host's inputs are those of the first pass over them, as the per-node counts are, and the host's clocks cover both passes.
void fill_build_stats(nh_build_stats &s, const Builder &B, const PassResult *count, const PassResult &insert, uint64_t capacity, uint64_t size) {
    const PassResult &first = count ? *count : insert;
    s.seconds_insert = insert.seconds_gpu;
    s.seconds_read = insert.seconds_read + (count ? count->seconds_read : 0);
    s.sequences = first.sequences;
    s.bases = first.bases;
    s.kmers = first.kmers;
    s.ambiguous_kmers = first.kmers - insert.clean;
    s.capacity = capacity;
    s.size = size;
    s.masked_bases = insert.masked;
    s.seconds_mask = insert.seconds_mask + (count ? count->seconds_mask : 0);
    s.taxa = B.node_count - 1;
}

int no_kmer(const PassResult &r) {
    return set_error(NH_EDB, "the input holds no k-mer to build from: %llu sequences, %llu bases, every sequence shorter than 35 bases or "
                     "ambiguous throughout", (unsigned long long)r.sequences, (unsigned long long)r.bases);
}

int build_db(const nh_build_args *a, nh_build_stats *stats, const nh_exclude_args *x = nullptr, nh_exclude_stats *xs = nullptr) {
    int rc = check_exclude_layout(x, xs);
    if (rc) return rc;
    BuildPlan P;
    layout_of(a, P);
    const size_t stats_size = P.stats_size;
    if (stats) memset(stats, 0, stats_size);
    rc = plan_build(a, P);
    if (rc) return rc;
    const double lf = P.lf;
    std::vector<BuildInput> x_files;  // empty: a build as it ever was
    if (excluding_with(x)) {
        rc = plan_exclude(a, x, P, x_files);
        if (rc) return rc;
    }
    const bool excluding = !x_files.empty();
    // (an exclusion file that is not there should not cost a counting pass over the host first)
    for (const BuildInput &f : x_files)
        if (access(f.path.c_str(), R_OK) != 0) return set_error(NH_EIO, "cannot read the exclusion file %s: %s", f.path.c_str(), strerror(errno));
    nh_exclude_stats xv;
    memset(&xv, 0, sizeof xv);

    rc = check_device(a->device);
    if (rc) return rc;
    Builder B;
    rc = configure(B, a, P, P.nodes.size() > 3, 0);  // (a manifest of one taxon is the one-taxon build)
    if (rc) return rc;

    nh_build_stats s;
    memset(&s, 0, sizeof s);
    uint64_t capacity = a->capacity;
    PassResult count, excl, insert;
    const bool counted = !capacity || excluding;  // (an exclusion needs the set: the counting pass runs whatever the capacity)
    if (counted) {
        rc = B.pass(P.inputs, Pass::COUNT, count);
        if (rc) return rc;
        s.distinct_minimizers = count.claimed;
        s.seconds_count = count.seconds_gpu;
        if (!excluding) B.d_set.reset();
        if (s.distinct_minimizers == 0) return no_kmer(count);
        uint64_t kept = s.distinct_minimizers;
        if (excluding) {  // the exclusion input against the set
            rc = B.pass(x_files, Pass::EXCLUDE, excl);
            if (rc) return rc;
            xv.sequences = excl.sequences, xv.bases = excl.bases, xv.kmers = excl.kmers;
            xv.ambiguous_kmers = excl.kmers - excl.clean;
            xv.lookups = excl.claimed;
            xv.excluded_minimizers = excl.flagged;
            xv.kept_minimizers = kept = s.distinct_minimizers - excl.flagged;
            xv.seconds_read = excl.seconds_read;
            xv.seconds_exclude = excl.seconds_gpu;
            if (kept == 0)
                return set_error(NH_EDB, "every minimizer of the input is excluded: all %llu distinct minimizers are also in the exclusion input "
                                 "(%llu sequences, %llu bases)", (unsigned long long)s.distinct_minimizers, (unsigned long long)xv.sequences,
                                 (unsigned long long)xv.bases);
            B.filter = true;
        }
        if (!capacity) capacity = (uint64_t)ceil((double)kept / lf);
        if (capacity >> 33) return set_error(NH_ECAPACITY, "%llu distinct minimizers need a table of 2^33 cells or more", (unsigned long long)kept);
    }
    rc = B.alloc_table(capacity);
    if (rc) return rc;
    rc = B.pass(P.inputs, Pass::INSERT, insert);
    if (rc) return rc;
    fill_build_stats(s, B, counted ? &count : nullptr, insert, capacity, insert.claimed);
    if (s.size == 0) return no_kmer(counted ? count : insert);
    // (a table without one empty cell is no kraken2 table: a look-up of an absent key would never end there)
    if (s.size >= capacity)
        return set_error(NH_ECAPACITY, "the table of %llu cells is full: the input has more distinct minimizers than `capacity` holds "
                         "(leave capacity 0 and it is counted)", (unsigned long long)capacity);
    if (B.multi) {
        rc = B.count_cells();
        if (rc) return rc;
    } else {
        B.per_node[TAXON_NODE].cells = s.size;
    }
    auto t0 = std::chrono::steady_clock::now();
    rc = write_database(B, a, P.nodes, s.size);
    if (rc) return rc;
    s.seconds_write = since(t0);
    if (getenv("NOHUMAN_TRACE"))
        fprintf(stderr, "[nohuman trace] build: %llu k-mers, %llu ambiguous, %llu distinct minimizers, %llu cells of %llu; kernels alone: count %.4f s, "
                        "insert %.4f s, mask %.4f s for %llu masked bases (batches of %llu bytes, pieces of %llu k-mers)\n",
                (unsigned long long)s.kmers, (unsigned long long)s.ambiguous_kmers, (unsigned long long)s.distinct_minimizers,
                (unsigned long long)s.size, (unsigned long long)s.capacity, count.seconds_kernel, insert.seconds_kernel, s.seconds_mask,
                (unsigned long long)s.masked_bases, (unsigned long long)B.batch_cap,
                (unsigned long long)B.piece);
    if (getenv("NOHUMAN_TRACE") && B.multi)
        fprintf(stderr, "[nohuman trace] build taxa: %u nodes, value_bits %u; insertions %llu, of them %llu found their key under another "
                        "value (the LCA path), values replaced %llu; cells per node %.6f s\n", B.node_count - 1, B.vbits, insert.inserts, insert.merges,
                insert.swaps, B.t_cells);
    if (getenv("NOHUMAN_TRACE") && excluding)
        fprintf(stderr, "[nohuman trace] build exclude: %llu k-mers of the exclusion input, %llu look-ups, %llu of %llu distinct minimizers excluded; "
                        "kernels alone: exclude %.4f s (set of %llu slots)\n", (unsigned long long)xv.kmers, (unsigned long long)xv.lookups,
                (unsigned long long)xv.excluded_minimizers, (unsigned long long)s.distinct_minimizers, excl.seconds_kernel, (unsigned long long)B.d_set.cap);
    give_taxon_stats(a, P, B.per_node);
    if (stats) memcpy(stats, &s, stats_size);
    give_stats(xs, xv);
    return NH_OK;
}

// ---- nh_extend_db: the taxa of a build added to an existing database (nh_extend.hip) ---------------------------
bool read_whole(const std::string &path, std::vector<uint8_t> &out, size_t at_most) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.resize(at_most);
    const size_t n = fread(out.data(), 1, at_most, f);
    out.resize(n);
    fclose(f);
    return true;
}

// every check of an extension that needs no device; P.nodes is the merged tree, X.remap the way there from the base's ids
int plan_extend(const nh_build_args *a, const nh_extend_args *x, const nh_extend_stats *xs, BuildPlan &P, BasePlan &X) {
    if (!a || !x) return set_error(NH_EINVAL, "nh_extend_db: null arguments");
    if (a->struct_size < sizeof(nh_build_args))
        return set_error(NH_EINVAL, "nh_extend_db: struct_size %u is smaller than nh_build_args (%u)", a->struct_size, (unsigned)sizeof(nh_build_args));
    if (x->struct_size < sizeof(nh_extend_args))
        return set_error(NH_EINVAL, "nh_extend_db: struct_size %u is smaller than nh_extend_args (%u)", x->struct_size, (unsigned)sizeof(nh_extend_args));
    if (xs && xs->struct_size < sizeof(nh_extend_stats))
        return set_error(NH_EINVAL, "nh_extend_db: struct_size %u is smaller than nh_extend_stats (%u)", xs->struct_size, (unsigned)sizeof(nh_extend_stats));
    if (!x->base_dir || !*x->base_dir) return set_error(NH_EINVAL, "nh_extend_db: no base database (base_dir)");
    if (a->capacity != 0)
        return set_error(NH_EINVAL, "nh_extend_db: capacity %llu cannot be given: an extension keeps the capacity of its base (the 64-bit hashes that "
                         "another capacity would need are not in hash.k2d)", (unsigned long long)a->capacity);
    X.dir = x->base_dir;
    for (const char *name : DB_FILES) {
        struct stat st;
        if (stat((X.dir + "/" + name).c_str(), &st) != 0 || !S_ISREG(st.st_mode))
            return set_error(NH_EINVAL, "nh_extend_db: the base database %s holds no %s", X.dir.c_str(), name);
    }
    if (a->out_dir && *a->out_dir) {
        const std::string o = real_of(a->out_dir), b = real_of(X.dir);
        if (!o.empty() && o == b)
            return set_error(NH_EINVAL, "nh_extend_db: the output directory %s is the base database itself: an extension is written to a directory of its own", a->out_dir);
    }
    {   // hash.k2d: the header, and a file as long as it says
        const std::string path = X.dir + "/hash.k2d";
        std::vector<uint8_t> h;
        struct stat st;
        if (!read_whole(path, h, 32) || stat(path.c_str(), &st) != 0) return set_error(NH_EIO, "nh_extend_db: cannot read %s: %s", path.c_str(), strerror(errno));
        if (h.size() < 32) return set_error(NH_EDB, "nh_extend_db: %s is truncated: %llu bytes hold no header", path.c_str(), (unsigned long long)h.size());
        uint64_t hdr[4];
        memcpy(hdr, h.data(), 32);
        if (hdr[2] + hdr[3] != 32 || hdr[3] == 0 || hdr[3] > 31)
            return set_error(NH_EDB, "nh_extend_db: %s: key_bits %llu + value_bits %llu is not 32", path.c_str(), (unsigned long long)hdr[2], (unsigned long long)hdr[3]);
        if (hdr[0] == 0 || hdr[0] >> 33) return set_error(NH_EDB, "nh_extend_db: %s: capacity %llu is not in [1, 2^33)", path.c_str(), (unsigned long long)hdr[0]);
        if ((uint64_t)st.st_size != 32 + 4 * hdr[0])
            return set_error(NH_EDB, "nh_extend_db: %s is truncated: %llu bytes, but its %llu cells take %llu", path.c_str(), (unsigned long long)st.st_size,
                             (unsigned long long)hdr[0], (unsigned long long)(32 + 4 * hdr[0]));
        if (hdr[1] >= hdr[0]) return set_error(NH_EDB, "nh_extend_db: %s: size %llu leaves no empty cell in %llu", path.c_str(), (unsigned long long)hdr[1], (unsigned long long)hdr[0]);
        X.capacity = hdr[0], X.size = hdr[1], X.old_vb = hdr[3];
    }
    {   // opts.k2d: the geometry this builder writes, and no other
        const std::string path = X.dir + "/opts.k2d";
        if (!read_whole(path, X.opts, 4096)) return set_error(NH_EIO, "nh_extend_db: cannot read %s: %s", path.c_str(), strerror(errno));
        if (X.opts.size() < 52) return set_error(NH_EDB, "nh_extend_db: %s is truncated: %llu bytes", path.c_str(), (unsigned long long)X.opts.size());
        const std::vector<uint8_t> want = opts_image();
        const char *field = memcmp(X.opts.data(), want.data(), 8)             ? "k"
                            : memcmp(X.opts.data() + 8, want.data() + 8, 8)   ? "l"
                            : memcmp(X.opts.data() + 16, want.data() + 16, 8) ? "spaced_seed_mask"
                            : memcmp(X.opts.data() + 24, want.data() + 24, 8) ? "toggle_mask"
                            : X.opts[32] != want[32]                          ? "dna_db"
                            : memcmp(X.opts.data() + 40, want.data() + 40, 8) ? "minimum_acceptable_hash_value"
                            : memcmp(X.opts.data() + 48, want.data() + 48, 4) ? "revcom_version"
                                                                              : nullptr;
        if (field)
            return set_error(NH_EDB, "nh_extend_db: %s: %s is not that of the default geometry (k = 35, l = 31, the default masks, a DNA database, "
                             "revcom_version 1, minimum hash 0), the only one that can be extended", path.c_str(), field);
    }
    {
        std::string err;
        const int rc = read_base_taxo((X.dir + "/taxo.k2d").c_str(), X.taxo, err);
        if (rc) return set_error(rc, "%s", err.c_str());
    }
    return plan_build(a, P, &X);
}

void extend_plan_stats(const BuildPlan &P, const BasePlan &X, nh_extend_stats &xs) {
    xs.base_size = X.size;
    xs.base_nodes = X.taxo.taxid.size();
    xs.base_value_bits = X.old_vb;
    xs.nodes_added = P.nodes.size() - X.taxo.taxid.size();
}

int extend_check(const nh_build_args *a, const nh_extend_args *x, nh_build_stats *stats, nh_extend_stats *xs) {
    BuildPlan P;
    BasePlan X;
    layout_of(a, P);
    const int rc = plan_extend(a, x, xs, P, X);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    give_plan(a, P, stats);
    nh_extend_stats v;
    memset(&v, 0, sizeof v);
    extend_plan_stats(P, X, v);
    give_stats(xs, v);
    return NH_OK;
}

int extend_db(const nh_build_args *a, const nh_extend_args *x, nh_build_stats *stats, nh_extend_stats *xs) {
    BuildPlan P;
    BasePlan X;
    layout_of(a, P);
    int rc = plan_extend(a, x, xs, P, X);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    rc = check_device(a->device);
    if (rc) return rc;
    Builder B;
    // (MULTI for one added taxon too: its minimizers merge with the values of the base; the value field never shrinks)
    rc = configure(B, a, P, true, (uint32_t)X.old_vb);
    if (rc) return rc;

    nh_extend_stats v;
    memset(&v, 0, sizeof v);
    extend_plan_stats(P, X, v);
    // the base table into the one table-sized buffer there ever is, then re-keyed where it lies
    rc = B.alloc_table(X.capacity);
    if (rc) return rc;
    auto t0 = std::chrono::steady_clock::now();
    rc = ext_load_table((X.dir + "/hash.k2d").c_str(), B.d_table, X.capacity, B.stream);
    if (rc) return rc;
    v.seconds_load = since(t0);
    ExtendTable T;
    T.d_table = B.d_table, T.capacity = X.capacity, T.old_vb = (uint32_t)X.old_vb, T.new_vb = B.vbits;
    T.remap.assign(X.remap.begin(), X.remap.end());
    T.d_parent = B.d_parent, T.grid_max = B.grid_max, T.stream = B.stream;
    rc = ext_rekey(T);
    if (rc) return rc;
    const std::string hash_path = X.dir + "/hash.k2d";
    if (T.bad_value)
        return set_error(NH_EDB, "nh_extend_db: %s holds a cell whose value is no node of its taxonomy (%llu nodes)", hash_path.c_str(),
                         (unsigned long long)X.taxo.taxid.size());
    if (T.non_empty != X.size)
        return set_error(NH_EDB, "nh_extend_db: %s holds %llu non-empty cells, but its header gives the size %llu", hash_path.c_str(),
                         (unsigned long long)T.non_empty, (unsigned long long)X.size);
    v.seconds_rekey = T.seconds_rekey;
    v.shadowed_cells = T.shadowed;
    rc = B.count_cells();
    if (rc) return rc;
    std::vector<uint64_t> base_cells(B.node_count, 0);
    for (uint32_t i = 1; i < B.node_count; i++) base_cells[i] = B.per_node[i].cells;

    const uint64_t free_cells = X.capacity - X.size;
    PassResult insert;
    rc = B.pass(P.inputs, Pass::INSERT, insert);
    if (rc == NH_ECAPACITY)
        return set_error(NH_ECAPACITY, "nh_extend_db: the base table has %llu free cells of %llu and the addition needs more than that: the capacity of "
                         "an extension is its base's", (unsigned long long)free_cells, (unsigned long long)X.capacity);
    if (rc) return rc;
    nh_build_stats s;
    memset(&s, 0, sizeof s);
    fill_build_stats(s, B, nullptr, insert, X.capacity, X.size + insert.claimed);
    v.cells_added = insert.claimed;
    v.load = (double)s.size / (double)s.capacity;
    if (s.size >= X.capacity)
        return set_error(NH_ECAPACITY, "nh_extend_db: the base table has %llu free cells of %llu and the addition needs %llu, which leaves no empty "
                         "cell: the capacity of an extension is its base's", (unsigned long long)free_cells, (unsigned long long)X.capacity,
                         (unsigned long long)insert.claimed);
    if (v.load > P.lf)
        return set_error(NH_ECAPACITY, "nh_extend_db: the base table has %llu free cells of %llu and the addition needs %llu: the load would be %.4f, "
                         "above the ceiling of %.4f (load_factor)", (unsigned long long)free_cells, (unsigned long long)X.capacity,
                         (unsigned long long)insert.claimed, v.load, P.lf);
    BUILD_TRY(hipMemsetAsync(B.d_cells, 0, (size_t)B.node_count * sizeof(unsigned long long), B.stream));
    rc = B.count_cells();
    if (rc) return rc;
    t0 = std::chrono::steady_clock::now();
    rc = write_database(B, a, P.nodes, s.size, &X.opts);
    if (rc) return rc;
    s.seconds_write = since(t0);
    if (getenv("NOHUMAN_TRACE"))
        fprintf(stderr, "[nohuman trace] extend: base %llu cells of %llu at %llu value bits, %llu nodes; now %u value bits, %u nodes, table %s; "
                        "%llu shadowed; %llu cells added; load %.4f s, re-key %.6f s (the streaming pass alone %.6f s), insert kernels %.4f s\n",
                (unsigned long long)X.size, (unsigned long long)X.capacity, (unsigned long long)X.old_vb, (unsigned long long)X.taxo.taxid.size(),
                B.vbits, B.node_count, T.rekeyed ? "rewritten" : "as it was", (unsigned long long)T.shadowed, (unsigned long long)insert.claimed,
                v.seconds_load, v.seconds_rekey, T.seconds_pass, insert.seconds_kernel);
    give_taxon_stats(a, P, B.per_node);
    if (x->base_cells)
        for (uint32_t i = 1; i < B.node_count && i - 1 < x->base_cells_cap; i++) x->base_cells[i - 1] = base_cells[i];
    if (stats) memcpy(stats, &s, sizeof s);
    give_stats(xs, v);
    return NH_OK;
}

// an exported entry: no exception leaves the library
template <class F>
int guarded(const char *name, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return set_error(NH_EOOM, "%s: out of host memory", name);
    } catch (const std::exception &e) {
        return set_error(NH_EIO, "%s: %s", name, e.what());
    }
}

}  // namespace
}  // namespace nh

extern "C" int nh_build_check(const nh_build_args *args, nh_build_stats *stats) {
    return nh::guarded("nh_build_check", [&] { return nh::build_check(args, stats); });
}

extern "C" int nh_build_db(const nh_build_args *args, nh_build_stats *stats) {
    return nh::guarded("nh_build_db", [&] { return nh::build_db(args, stats); });
}

extern "C" int nh_exclude_check(const nh_build_args *b, const nh_exclude_args *x, nh_build_stats *bs, nh_exclude_stats *xs) {
    return nh::guarded("nh_exclude_check", [&] { return nh::exclude_check(b, x, bs, xs); });
}

extern "C" int nh_build_db_exclude(const nh_build_args *b, const nh_exclude_args *x, nh_build_stats *bs, nh_exclude_stats *xs) {
    return nh::guarded("nh_build_db_exclude", [&] { return nh::build_db(b, bs, x, xs); });
}

extern "C" int nh_extend_check(const nh_build_args *b, const nh_extend_args *x, nh_build_stats *bs, nh_extend_stats *xs) {
    return nh::guarded("nh_extend_check", [&] { return nh::extend_check(b, x, bs, xs); });
}

extern "C" int nh_extend_db(const nh_build_args *b, const nh_extend_args *x, nh_build_stats *bs, nh_extend_stats *xs) {
    return nh::guarded("nh_extend_db", [&] { return nh::extend_db(b, x, bs, xs); });
}
