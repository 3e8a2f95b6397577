// nh_dust.hip -- low-complexity masking on the GPU: symmetric DUST (Morgulis et al. 2006) at dustmasker's defaults, window 64
// bases and score threshold 2.0, both fixed (the model is tests/dust_model.py).
//
// The masked set is the union of the bases of all PERFECT triplet intervals [i, i + d] of a run of ACGTacgt: d <= 61,
// 10 r > 20 d, and no sub-interval with a higher score r / d (r = sum over the 64 triplet codes of n (n - 1) / 2).  In the form the
// kernel runs, for d = 1 .. 61 and every start i (r_{-1} = r_0 = 0, M_0 = 0):
//     r_d(i) = r_{d-1}(i) + r_{d-1}(i+1) - r_{d-2}(i+1) + [t_i == t_{i+d}]
//     B      = max(M_{d-1}(i), M_{d-1}(i+1))
//     perfect(i, d)  <=>  r_d(i) / d >= B  and  10 r_d(i) > 20 d
//     M_d(i) = max(r_d(i) / d, B)
//     reach(i) = 3 + the largest perfect d (0: none);  base b is masked  <=>  some start i <= b has b < i + reach(i)
// Fractions are compared by cross-multiplication (r <= 1891, d <= 61: every product is below 2^24); no floating point.
//
// One wave per tile.  A lane keeps DUST_LANE_STARTS consecutive starts in registers (r_{d-1}, r_{d-2}, M, reach, and the window of
// triplet codes t_{i+d}, which moves by one code a step: the d loop is unrolled by the lane's starts so that the window's slots
// are static registers), so the neighbour i + 1 is in the lane except at the lane's last start, which takes the three values of
// the next lane's first start by two cross-lane reads a step.  The triplet codes of the tile lie in LDS (one byte a start), read
// once a step and lane for the window's new code.  Step d of start i needs step d - 1 of start i + 1, so of the wave's 64 x 16 =
// 1024 starts the last 61 are not carried to the end (the trapezoid), and the first 63 are the context before the tile's own bases:
// 900 bases a tile, 88 % of the work is the tile's own (221 VGPRs, two waves a SIMD; with 8 starts a lane -- 388 bases a tile,
// 76 %, 117 VGPRs, four waves a SIMD -- the kernel measured 4 % slower: profiles/build_db_dust.txt).
//
// The kernel reads `src` and writes `dst`, a copy of src made before the launch: a tile reads its neighbours' bases as context
// while they are being masked, and an N written in place would end a run there.  Each base belongs to one tile, is written by
// that wave only, and what is written depends on src alone -- not on the order of the waves.
//
// k_rdust (below k_dust) is the same mask for the reads of a batch at classification time (--dust-reads): every
// sequence on its own, found through a scan of the sequence table instead of tiles cut on the host.
#include <hip/hip_runtime.h>
#include <string.h>

#include <exception>
#include <new>
#include <vector>

#include "nh_device.h"
#include "nh_dust.h"
#include "nh_internal.h"
#include "nh_outbuild.h"
#include "nh_scan.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

constexpr int DS = DUST_LANE_STARTS;
constexpr uint32_t DN = DUST_WAVE_STARTS;
constexpr uint32_t DUST_DEAD = 0xFF;  // the code of a triplet with a base outside ACGTacgt or outside the segment

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_dust(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                  const uint64_t text_len, const DustTile *__restrict__ tiles,
                                                                  const uint64_t n_tiles, unsigned long long *counter) {
    static_assert(DS % 8 == 0, "a lane's codes are written to LDS in 8-byte words");
    __shared__ __attribute__((aligned(8))) uint8_t lds_all[WAVES_PER_BLOCK][DN + 64];
    const uint32_t lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *const T = lds_all[wib];
    T[DN + lane] = DUST_DEAD;  // what the last lanes' windows read behind the wave's starts
    const uint32_t p0 = lane * DS;  // tile positions: position p is base start - 63 + p of the text
    unsigned long long turned = 0;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t ti = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib; ti < n_tiles; ti += n_waves) {
        const DustTile tl = tiles[ti];
        const uint64_t a = tl.start;
        const uint32_t n = tl.n, left = tl.left, right = tl.right;
        // (wave-uniform; the host makes no such tile)
        if (n == 0 || n > DUST_TILE_BASES || left > DUST_CONTEXT || right > DUST_CONTEXT || a < left || a > text_len ||
            text_len - a < (uint64_t)n + right)
            continue;
        const uint32_t lo = DUST_CONTEXT - left, hi = DUST_CONTEXT + n + right;  // the positions that hold text of the segment
        uint32_t c[DS + 2];
#pragma unroll
        for (int k = 0; k < DS + 2; k++) {
            const uint32_t p = p0 + k;
            uint32_t by = 0;
            if (p >= lo && p < hi) by = src[a + p - DUST_CONTEXT];
            const uint32_t up = by & 0xDFu;
            c[k] = (up == 'A' || up == 'C' || up == 'G' || up == 'T') ? ((up >> 1) & 3u) : 4u;
        }
        uint32_t t[DS], w[DS];
        uint32_t alive = 0;
        uint64_t packed[DS / 8];
#pragma unroll
        for (int q = 0; q < DS / 8; q++) packed[q] = 0;
#pragma unroll
        for (int j = 0; j < DS; j++) {
            const bool ok = ((c[j] | c[j + 1] | c[j + 2]) & 4u) == 0;
            t[j] = ok ? ((c[j] << 4) | (c[j + 1] << 2) | c[j + 2]) : DUST_DEAD;
            w[j] = t[j];
            alive |= (ok ? 1u : 0u) << j;
            packed[j / 8] |= (uint64_t)t[j] << (8 * (j % 8));
        }
        wave_sync();  // (the tile before has been read)
#pragma unroll
        for (int q = 0; q < DS / 8; q++) reinterpret_cast<uint64_t *>(T + p0)[q] = packed[q];
        wave_sync();
        uint32_t r1[DS], r2[DS], mn[DS], md[DS], reach[DS];
#pragma unroll
        for (int j = 0; j < DS; j++) r1[j] = r2[j] = mn[j] = reach[j] = 0, md[j] = 1;
        uint32_t nb_r2 = 0;  // r_{d-2} of the next lane's first start
        // d = d0 + u with d0 = 1 mod DS: the code of position j + d lies in window slot (j + u + 1) mod DS
        for (uint32_t d0 = 1; d0 <= 61; d0 += DS) {
#pragma unroll
            for (int u = 0; u < DS; u++) {
                const uint32_t d = d0 + u;
                if (d <= 61) {
                    w[u] = T[p0 + (DS - 1) + d];  // (replaces the code of position d - 1)
                    const uint32_t nb_r1 = __shfl_down(r1[0], 1, 64);
                    const uint32_t nb_m = __shfl_down(mn[0] | (md[0] << 16), 1, 64);
                    const uint32_t nb_mn = nb_m & 0xFFFFu, nb_md = nb_m >> 16;
#pragma unroll
                    for (int j = 0; j < DS; j++) {
                        const uint32_t tt = w[(j + u + 1) % DS];
                        const uint32_t x_r1 = j < DS - 1 ? r1[j + 1 < DS ? j + 1 : j] : nb_r1;
                        const uint32_t x_r2 = j < DS - 1 ? r2[j + 1 < DS ? j + 1 : j] : nb_r2;
                        const uint32_t x_mn = j < DS - 1 ? mn[j + 1 < DS ? j + 1 : j] : nb_mn;
                        const uint32_t x_md = j < DS - 1 ? md[j + 1 < DS ? j + 1 : j] : nb_md;
                        if (tt >= 64u) alive &= ~(1u << j);  // an interval never spans a dead triplet
                        const bool live = (alive >> j) & 1u;
                        uint32_t r = r1[j] + x_r1 - x_r2 + (t[j] == tt ? 1u : 0u);
                        r = live ? r : 0u;
                        const bool nb_larger = __umul24(x_mn, md[j]) > __umul24(mn[j], x_md);
                        const uint32_t bn = nb_larger ? x_mn : mn[j], bd = nb_larger ? x_md : md[j];
                        const bool ge = __umul24(r, bd) >= __umul24(bn, d);
                        if (live && ge && r > 2u * d) reach[j] = d + 3u;
                        r2[j] = r1[j];
                        r1[j] = r;
                        mn[j] = ge ? r : bn;
                        md[j] = ge ? d : bd;
                    }
                    nb_r2 = nb_r1;
                }
            }
        }
        // masked(p) <=> the largest start + reach among the starts up to p lies behind p (reach <= 64: no window is needed)
        uint32_t pm[DS];
#pragma unroll
        for (int j = 0; j < DS; j++) {
            const uint32_t end = reach[j] ? p0 + j + reach[j] : 0u;
            pm[j] = j ? (pm[j ? j - 1 : 0] > end ? pm[j ? j - 1 : 0] : end) : end;
        }
        uint32_t inc = pm[DS - 1];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o && v > inc) inc = v;
        }
        uint32_t before = __shfl_up(inc, 1, 64);
        if (lane == 0) before = 0;
#pragma unroll
        for (int j = 0; j < DS; j++) {
            const uint32_t p = p0 + j;
            const uint32_t m = pm[j] > before ? pm[j] : before;
            if (m > p && p >= DUST_CONTEXT && p < DUST_CONTEXT + n) {  // an own base of the tile: a + (p - 63) < text_len
                const uint32_t o = p - DUST_CONTEXT;
                dst[a + o] = 'N';
                if (o >= tl.cnt_lo && o < tl.cnt_hi) turned++;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) turned += __shfl_xor(turned, d, 64);
    if (lane == 0 && turned) atomicAdd(counter, turned);
}

// ---- the reads of a batch (nh_run_dust, nh_dust_reads_device) ----------------------------------------------------
// The same mask over millions of short sequences that lie inside FASTQ text, each masked on its own, with no tile cut on the host.
// The VIRTUAL TEXT is all sequences in table order, each followed by one separator position; sequence i begins at virtual offset
// voff(i) = the exclusive scan of len + 1.  k_rdust_sums writes the offsets inside blocks of OB_THREADS sequences (loc[]) and the
// blocks' sums, k_rdust_scan turns the sums into the blocks' offsets (blk[]; blk[nblk]: the virtual text's length), so voff(i) =
// blk[i / OB_THREADS] + loc[i].  Tile t of k_rdust owns the virtual positions [T t, T t + T), T = DUST_TILE_BASES; its wave
// carries k_dust's 1024 starts from virtual position T t - 63 on.  The wave finds the sequence of its first position by one
// lower bound over voff that all its lanes make together (64 probes a round: four rounds for 16 M sequences); every lane then
// finds the sequence of ITS first position between that one and as many sequences further as it lies positions further (a
// sequence takes at least one position), and walks its DS + 2 positions from there.  A separator, and a position outside the virtual
// text, is a dead code, so no triplet and no interval spans two sequences and a perfect interval's last base lies in front of its
// sequence's separator.  The lane keeps where its walk began (three registers) across the recurrence and walks again, only if one
// of its own positions is masked, to store 'N' at the bases' addresses in `out`; nothing else is written.  A sequence that leaves
// the text takes part as a separator alone -- nothing of it is read or written -- and sets ERR_RDUST.
//
// The recurrence is k_dust's, as a device function.  k_dust itself keeps its text: built on this function it compiled to 242
// VGPRs (251 with the mask returned as bits) instead of 221, still without scratch and at two waves a SIMD; the kernel the builder
// was measured with is left alone.
constexpr int ERR_RDUST = 512;

// a byte's 2-bit code; 4: a byte outside ACGTacgt
__device__ __forceinline__ uint32_t dust_code(uint32_t by) {
    const uint32_t up = by & 0xDFu;
    return (up == 'A' || up == 'C' || up == 'G' || up == 'T') ? ((up >> 1) & 3u) : 4u;
}

// k_dust's recurrence for one wave.  c: the codes (4 also for a position that holds no base) of the lane's positions p0 .. p0 + DS
// + 1, p0 = lane * DS; T: the wave's DN + 64 bytes of LDS, the last 64 dead.  Bit j of the result: position p0 + j is masked by a
// start of the wave (the first 63 positions lack the starts before them, the last 61 starts are not carried to the end).
__device__ __forceinline__ uint32_t dust_wave(const uint32_t (&c)[DS + 2], uint8_t *const T, const uint32_t p0, const uint32_t lane) {
    uint32_t t[DS], w[DS];
    uint32_t alive = 0;
    uint64_t packed[DS / 8];
#pragma unroll
    for (int q = 0; q < DS / 8; q++) packed[q] = 0;
#pragma unroll
    for (int j = 0; j < DS; j++) {
        const bool ok = ((c[j] | c[j + 1] | c[j + 2]) & 4u) == 0;
        t[j] = ok ? ((c[j] << 4) | (c[j + 1] << 2) | c[j + 2]) : DUST_DEAD;
        w[j] = t[j];
        alive |= (ok ? 1u : 0u) << j;
        packed[j / 8] |= (uint64_t)t[j] << (8 * (j % 8));
    }
    wave_sync();  // (the tile before has been read)
#pragma unroll
    for (int q = 0; q < DS / 8; q++) reinterpret_cast<uint64_t *>(T + p0)[q] = packed[q];
    wave_sync();
    uint32_t r1[DS], r2[DS], mn[DS], md[DS], reach[DS];
#pragma unroll
    for (int j = 0; j < DS; j++) r1[j] = r2[j] = mn[j] = reach[j] = 0, md[j] = 1;
    uint32_t nb_r2 = 0;
    for (uint32_t d0 = 1; d0 <= 61; d0 += DS) {
#pragma unroll
        for (int u = 0; u < DS; u++) {
            const uint32_t d = d0 + u;
            if (d <= 61) {
                w[u] = T[p0 + (DS - 1) + d];
                const uint32_t nb_r1 = __shfl_down(r1[0], 1, 64);
                const uint32_t nb_m = __shfl_down(mn[0] | (md[0] << 16), 1, 64);
                const uint32_t nb_mn = nb_m & 0xFFFFu, nb_md = nb_m >> 16;
#pragma unroll
                for (int j = 0; j < DS; j++) {
                    const uint32_t tt = w[(j + u + 1) % DS];
                    const uint32_t x_r1 = j < DS - 1 ? r1[j + 1 < DS ? j + 1 : j] : nb_r1;
                    const uint32_t x_r2 = j < DS - 1 ? r2[j + 1 < DS ? j + 1 : j] : nb_r2;
                    const uint32_t x_mn = j < DS - 1 ? mn[j + 1 < DS ? j + 1 : j] : nb_mn;
                    const uint32_t x_md = j < DS - 1 ? md[j + 1 < DS ? j + 1 : j] : nb_md;
                    if (tt >= 64u) alive &= ~(1u << j);
                    const bool live = (alive >> j) & 1u;
                    uint32_t r = r1[j] + x_r1 - x_r2 + (t[j] == tt ? 1u : 0u);
                    r = live ? r : 0u;
                    const bool nb_larger = __umul24(x_mn, md[j]) > __umul24(mn[j], x_md);
                    const uint32_t bn = nb_larger ? x_mn : mn[j], bd = nb_larger ? x_md : md[j];
                    const bool ge = __umul24(r, bd) >= __umul24(bn, d);
                    if (live && ge && r > 2u * d) reach[j] = d + 3u;
                    r2[j] = r1[j];
                    r1[j] = r;
                    mn[j] = ge ? r : bn;
                    md[j] = ge ? d : bd;
                }
                nb_r2 = nb_r1;
            }
        }
    }
    uint32_t pm[DS];
#pragma unroll
    for (int j = 0; j < DS; j++) {
        const uint32_t end = reach[j] ? p0 + j + reach[j] : 0u;
        pm[j] = j ? (pm[j ? j - 1 : 0] > end ? pm[j ? j - 1 : 0] : end) : end;
    }
    uint32_t inc = pm[DS - 1];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o && v > inc) inc = v;
    }
    uint32_t before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < DS; j++) bits |= ((pm[j] > before ? pm[j] : before) > p0 + j ? 1u : 0u) << j;
    return bits;
}

// sequence i as the pass takes it: its start and its length, 0 for a sequence that leaves the text (*bad) or lies behind the table
__device__ __forceinline__ uint32_t rd_seq(const ReadDustArgs &a, uint64_t i, uint64_t *start, bool *bad) {
    *start = 0;
    if (i >= a.n) return 0;
    const uint64_t s = a.seq_off[i];
    const uint32_t len = a.seq_len[i];
    if (s > a.ntext || len > a.ntext - s) {
        *bad = true;
        return 0;
    }
    *start = s;
    return len;
}

// the virtual offset of sequence i < n (after k_rdust_scan)
__device__ __forceinline__ uint64_t rd_voff(const ReadDustArgs &a, uint64_t i) { return a.blk[i / OB_THREADS] + a.loc[i]; }

__global__ __launch_bounds__(OB_THREADS) void k_rdust_sums(ReadDustArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    uint64_t start, total;
    bool bad = false;
    const uint64_t v = i < a.n ? (uint64_t)rd_seq(a, i, &start, &bad) + 1 : 0;
    const uint64_t ex = block_exclusive_scan(v, wsum, &total);
    if (i < a.n) a.loc[i] = ex;
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
    if (bad) atomicOr(a.error, ERR_RDUST);
}

__global__ __launch_bounds__(OB_THREADS) void k_rdust_scan(ReadDustArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t total = scan_block_sums(a.blk, a.nblk, wsum);
    if (threadIdx.x == 0) a.blk[a.nblk] = total;
}

// The lane's DS + 2 virtual positions from v on, (i, off) being where position max(v, 0) lies: f(k, real, addr) for each, real: the
// position holds a base, at text address addr.  Unrolled: k is a constant in f
template <class F>
__device__ __forceinline__ void rd_walk(const ReadDustArgs &a, int64_t v, uint64_t total, uint64_t i, uint32_t off, F f) {
    uint64_t s;
    bool ignore = false;
    uint32_t len = rd_seq(a, i, &s, &ignore);
#pragma unroll
    for (int k = 0; k < DS + 2; k++, v++) {
        if (v < 0 || (uint64_t)v >= total) {
            f(k, false, 0ull);
        } else if (off == len) {  // the separator: the next position begins the next sequence
            f(k, false, 0ull);
            i++, off = 0;
            len = rd_seq(a, i, &s, &ignore);
        } else {
            f(k, true, s + off);
            off++;
        }
    }
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_rdust(ReadDustArgs a) {
    __shared__ __attribute__((aligned(8))) uint8_t lds_all[WAVES_PER_BLOCK][DN + 64];
    const uint32_t lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *const T = lds_all[wib];
    T[DN + lane] = DUST_DEAD;
    const uint32_t p0 = lane * DS;  // wave positions: position p is virtual position T t - 63 + p
    const uint64_t total = a.blk[a.nblk];
    const uint64_t n_tiles = (total + DUST_TILE_BASES - 1) / DUST_TILE_BASES;
    unsigned long long turned = 0;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t ti = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib; ti < n_tiles; ti += n_waves) {
        const int64_t v0 = (int64_t)(ti * DUST_TILE_BASES) - (int64_t)DUST_CONTEXT;
        const uint64_t f0 = v0 > 0 ? (uint64_t)v0 : 0;  // the wave's first position inside the virtual text (T ti < total)
        // the last sequence that begins at or before f0, by all lanes together: it lies in [lo, hi), voff(lo) <= f0
        uint64_t lo = 0, hi = a.n;
        while (hi - lo > 1) {
            const uint64_t stride = (hi - lo + 63) / 64;
            const uint64_t idx = lo + (uint64_t)lane * stride;
            const int cnt = __popcll(__ballot(idx < hi && rd_voff(a, idx) <= f0));  // (at least 1: lane 0 probes lo)
            lo += (uint64_t)(cnt - 1) * stride;
            hi = lo + stride < hi ? lo + stride : hi;
        }
        // the lane's own: its first position inside the virtual text lies fl - f0 positions, so at most as many sequences, further
        const int64_t vl = v0 + (int64_t)p0;
        const uint64_t fl = vl > 0 ? (uint64_t)vl : 0;
        uint64_t li = a.n;
        uint32_t loff = 0;
        if (fl < total) {
            uint64_t x = lo, y = lo + (fl - f0);
            if (y > a.n - 1) y = a.n - 1;
            while (x < y) {
                const uint64_t mid = x + (y - x + 1) / 2;
                if (rd_voff(a, mid) <= fl) x = mid;
                else y = mid - 1;
            }
            li = x;
            loff = (uint32_t)(fl - rd_voff(a, x));  // (at most the sequence's length: a 32-bit number)
        }
        uint32_t c[DS + 2];
        rd_walk(a, vl, total, li, loff, [&](int k, bool real, uint64_t addr) { c[k] = real ? dust_code((uint8_t)a.text[addr]) : 4u; });
        uint32_t bits = dust_wave(c, T, p0, lane);
        // the wave's own positions
#pragma unroll
        for (int j = 0; j < DS; j++)
            if (p0 + j < DUST_CONTEXT || p0 + j >= DUST_CONTEXT + DUST_TILE_BASES) bits &= ~(1u << j);
        if (bits)  // (a masked position holds a base: an interval covers live triplets only; `real` is asked all the same)
            rd_walk(a, vl, total, li, loff, [&](int k, bool real, uint64_t addr) {
                if (k < DS && ((bits >> k) & 1u) && real) {
                    a.out[addr] = 'N';
                    turned++;
                }
            });
    }
    for (int d = 32; d >= 1; d >>= 1) turned += __shfl_xor(turned, d, 64);
    if (lane == 0 && turned && a.masked) atomicAdd(a.masked, turned);
}

}  // namespace

uint64_t read_dust_scratch_words(uint64_t n) { return n + (n + OB_THREADS - 1) / OB_THREADS + 1; }

int read_dust_grid_max() {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
        (void)hipGetLastError();
        cus = 256;
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_rdust, WAVE * WAVES_PER_BLOCK, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 2;
    }
    return cus * (per_cu > 8 ? 8 : per_cu);
}

hipError_t launch_read_dust(ReadDustArgs a, uint64_t *scratch, int grid_max, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.n > (1ull << 31)) return hipErrorInvalidValue;
    a.nblk = (a.n + OB_THREADS - 1) / OB_THREADS;
    a.blk = scratch, a.loc = scratch + a.nblk + 1;
    hipLaunchKernelGGL(k_rdust_sums, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_rdust_scan, dim3(1), dim3(OB_THREADS), 0, stream, a);
    // the virtual text is at most text_len + n positions when the sequences are disjoint; the waves loop over the tiles in any case
    const uint64_t tiles = (a.ntext + a.n) / DUST_TILE_BASES + 1;
    const uint64_t want = (tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const unsigned grid = (unsigned)(want < (uint64_t)grid_max ? want : (uint64_t)(grid_max > 0 ? grid_max : 1));
    hipLaunchKernelGGL(k_rdust, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, a);
    return hipGetLastError();
}

void dust_tiles(std::vector<DustTile> &out, uint64_t seg_start, uint64_t seg_len, uint64_t cnt_lo, uint64_t cnt_hi) {
    if (cnt_hi > seg_len) cnt_hi = seg_len;
    for (uint64_t off = 0; off < seg_len; off += DUST_TILE_BASES) {
        const uint64_t rest = seg_len - off;
        DustTile t;
        memset(&t, 0, sizeof t);
        t.start = seg_start + off;
        t.n = (uint32_t)(rest < DUST_TILE_BASES ? rest : DUST_TILE_BASES);
        t.left = (uint8_t)(off < DUST_CONTEXT ? off : DUST_CONTEXT);
        const uint64_t behind = rest - t.n;
        t.right = (uint8_t)(behind < DUST_CONTEXT ? behind : DUST_CONTEXT);
        const uint64_t lo = cnt_lo > off ? cnt_lo - off : 0, hi = cnt_hi > off ? cnt_hi - off : 0;
        t.cnt_lo = (uint32_t)(lo < t.n ? lo : t.n);
        t.cnt_hi = (uint32_t)(hi < t.n ? hi : t.n);
        out.push_back(t);
    }
}

int dust_grid_max() {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
        (void)hipGetLastError();
        cus = 256;
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_dust, WAVE * WAVES_PER_BLOCK, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 4;
    }
    return cus * (per_cu > 8 ? 8 : per_cu);
}

hipError_t launch_dust(const char *src, char *dst, uint64_t text_len, const DustTile *d_tiles, uint64_t n_tiles,
                       unsigned long long *d_count, int grid_max, hipStream_t stream) {
    if (n_tiles == 0) return hipSuccess;
    const uint64_t want = (n_tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const unsigned grid = (unsigned)(want < (uint64_t)grid_max ? want : (uint64_t)(grid_max > 0 ? grid_max : 1));
    hipLaunchKernelGGL(k_dust, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, (const uint8_t *)src, (uint8_t *)dst, text_len, d_tiles,
                       n_tiles, d_count);
    return hipGetLastError();
}

namespace {

#define DUST_TRY(expr)                                                                                                         \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) {                                                                                                \
            (void)hipGetLastError();                                                                                           \
            return set_error(_e == hipErrorOutOfMemory ? NH_EOOM : NH_EDEVICE, "nh_dust_mask: %s: %s", #expr, hipGetErrorString(_e)); \
        }                                                                                                                      \
    } while (0)

struct DustBuffers {  // (one call's: the caller has selected the device)
    DevBuf<char> src, dst;
    DevBuf<DustTile> tiles;
    DevBuf<unsigned long long> count;
    hipStream_t stream = nullptr;
    ~DustBuffers() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int dust_mask(int32_t device, char *text, uint64_t n_bytes, const uint64_t *seg_start, const uint64_t *seg_len, uint64_t n_seg,
              uint64_t *masked_bases) {
    if (masked_bases) *masked_bases = 0;
    if (!text) return set_error(NH_EINVAL, "nh_dust_mask: null text");
    if (n_seg && (!seg_start || !seg_len)) return set_error(NH_EINVAL, "nh_dust_mask: null segment list");
    for (uint64_t i = 0; i < n_seg; i++)
        if (seg_start[i] > n_bytes || seg_len[i] > n_bytes - seg_start[i])
            return set_error(NH_EINVAL, "nh_dust_mask: segment %llu (start %llu, length %llu) leaves the buffer of %llu bytes",
                             (unsigned long long)i, (unsigned long long)seg_start[i], (unsigned long long)seg_len[i], (unsigned long long)n_bytes);
    std::vector<DustTile> tiles;
    for (uint64_t i = 0; i < n_seg; i++) dust_tiles(tiles, seg_start[i], seg_len[i], 0, seg_len[i]);
    if (tiles.empty()) return NH_OK;  // nothing to mask: no device is needed
    int rc = check_device(device);
    if (rc) return rc;
    DUST_TRY(dev_set(device));
    DustBuffers B;
    DUST_TRY(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
    DUST_TRY(B.src.reserve(n_bytes + 64));
    DUST_TRY(B.dst.reserve(n_bytes + 64));
    DUST_TRY(B.tiles.reserve(tiles.size()));
    DUST_TRY(B.count.reserve(1));
    DUST_TRY(hipMemcpyAsync(B.src, text, n_bytes, hipMemcpyHostToDevice, B.stream));
    DUST_TRY(hipMemcpyAsync(B.dst, B.src, n_bytes, hipMemcpyDeviceToDevice, B.stream));
    DUST_TRY(hipMemcpyAsync(B.tiles, tiles.data(), tiles.size() * sizeof(DustTile), hipMemcpyHostToDevice, B.stream));
    DUST_TRY(hipMemsetAsync(B.count, 0, sizeof(unsigned long long), B.stream));
    DUST_TRY(launch_dust(B.src, B.dst, n_bytes, B.tiles, tiles.size(), B.count, dust_grid_max(), B.stream));
    unsigned long long turned = 0;
    DUST_TRY(hipMemcpyAsync(&turned, B.count, sizeof turned, hipMemcpyDeviceToHost, B.stream));
    DUST_TRY(hipStreamSynchronize(B.stream));
    DUST_TRY(hipMemcpy(text, B.dst, n_bytes, hipMemcpyDeviceToHost));
    if (masked_bases) *masked_bases = turned;
    return NH_OK;
}

}  // namespace
}  // namespace nh

extern "C" int nh_dust_mask(int32_t device, char *text, uint64_t n_bytes, const uint64_t *seg_start, const uint64_t *seg_len,
                            uint64_t n_seg, uint64_t *masked_bases) {
    try {
        return nh::dust_mask(device, text, n_bytes, seg_start, seg_len, n_seg, masked_bases);
    } catch (const std::bad_alloc &) {
        return nh::set_error(NH_EOOM, "nh_dust_mask: out of host memory");
    } catch (const std::exception &e) {
        return nh::set_error(NH_EIO, "nh_dust_mask: %s", e.what());
    }
}

extern "C" int nh_dust_reads_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                                    uint64_t n_seq, void *d_out, void *d_masked, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_text || !d_out || (n_seq && (!d_seq_starts || !d_seq_lens))) return nh::set_error(NH_EINVAL, "nh_dust_reads_device: null argument");
    if (n_seq > (1ull << 31)) return nh::set_error(NH_EINVAL, "nh_dust_reads_device: too many sequences for one launch");
    if (n_seq == 0) return NH_OK;
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::DevBuf<uint64_t> scratch;
    if (scratch.reserve(nh::read_dust_scratch_words(n_seq)) != hipSuccess) {
        (void)hipGetLastError();
        return nh::set_error(NH_EOOM, "nh_dust_reads_device: cannot allocate %llu words of scratch", (unsigned long long)nh::read_dust_scratch_words(n_seq));
    }
    nh::ReadDustArgs a{};
    a.text = (const char *)d_text, a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts, a.seq_len = (const uint32_t *)d_seq_lens, a.n = n_seq;
    a.out = (char *)d_out, a.masked = (unsigned long long *)d_masked;
    a.error = e->d_error + nh::LAUNCH_SLOTS;
    hipError_t he = nh::launch_read_dust(a, scratch, nh::read_dust_grid_max(), (hipStream_t)stream);
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);  // (the scratch is the launches' until they are done)
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "read DUST launch: %s", hipGetErrorString(he));
    return NH_OK;
}
