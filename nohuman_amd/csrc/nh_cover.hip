// nh_cover.hip -- where in each read the host k-mers lie (nh_run_intervals, --host-intervals): the covered intervals of every sequence
// of a batch as BED lines, built in HBM.  DESIGN.md 6.19; tests/intervals_model.py is the specification.
//
// A k-mer is a HOST k-mer when it is not ambiguous, its minimizer is looked up (minimum_acceptable_hash_value as in the classifier)
// and found with a non-zero value v, and -- a run with a host selection -- host_of[v] is set.  All of it depends on the k-mer alone,
// so this is a pass of its own behind the classifier, which is not touched, on the text the classifier read.  A base is covered when
// a host k-mer contains it; a sequence's intervals are its maximal runs of covered bases.
//
// k_cover_mark      a sequence is cut into pieces of `piece` k-mers (COVER_PIECE, NOHUMAN_COVER_PIECE) that overlap by k - 1 bases;
//                   the pieces of a batch are numbered by an exclusive scan of the sequences' piece counts (k_cover_piece_sizes,
//                   _scan, _starts: nh_outbuild.h's scheme) and a wave takes COVER_CHUNK consecutive pieces: one binary search, then a
//                   walk.  A piece is scanned a tile at a time with no carry INTO it: the first unambiguous k-mer of a piece
//                   starts a run whatever lay before, and a run start is one find-only look-up (nh_scan.h: find_cell).  The
//                   tile loop is walk_tiles' (nh_scan.h), written out: with its per-tile code in a closure this kernel reloads
//                   its arguments inside the loop and measured 0.6 % slower on long reads (profiles/tile_walk_refactor.txt);
//                   what differs from walk_tiles is the clamp alone, the last dword that holds a byte of the text.  `ps` says which run
//                   covers each k-mer; the tile's host k-mers, two ballots, are spread to a 128-bit mask, dilated by k (shifts and
//                   ORs of a 256-bit value the whole wave holds), shifted to the bit of the tile's first base and ORed into the
//                   bitmap, one bit a byte of the text: eight words at the most, a lane each.  A word whose new bits are zero is
//                   not touched -- a tile without a host k-mer skips the mask altogether --, every other word is written with
//                   atomicOr: neighbouring tiles (k - 1 bases in common), pieces and sequences share words, and bits only go from
//                   0 to 1.
// k_cover_ivl_*     sizes, scan, write: the bitmap into records {seq, start, end}, in sequence order, then by start, clipped to the
//                   sequence (two sequences back to back give two records).  One wave a sequence at a time, 64 sequences a wave; a
//                   lane takes a word: starts = w & ~(w << 1 | last bit of the word before), ends likewise, both with the words cut
//                   to the sequence; the k-th start and the k-th end of a sequence make its k-th record (wave prefix sums).
// k_cover_close     --host-bases-only's gap closing (tests/hitmask_model.py): an uncovered run of at most `gap` bases with a
//                   covered base on each side in the same sequence becomes covered.  One wave a sequence, a lane a word, as the
//                   interval builder; a lane takes the run ends of its word (covered, the next base not), looks for the sequence's
//                   next covered base -- the rest of its word, then the words behind it as far as `gap` reaches -- and ORs the
//                   bits between the two into the bitmap with atomicOr, a word at a time.  The uncovered runs are disjoint and a
//                   run is closed by the lane that holds the base in front of it alone, so what other lanes set meanwhile (bits
//                   in front of a covered base, never behind the last one a lane looks at) changes no lane's answer.  A run closes
//                   the sequences of its host fragments alone (the mask builder reads no other), so the kernel's sum is closed_bases.
// k_cover_line_*    sizes, scan, write on nh_outbuild.h: one line a record, <id> \t <start> \t <end> \t <mate> \t <taxid> \n, the
//                   id as nh_calls.hip's (read_id), decimal digits by division; the sizes also count the fragments with a record
//                   and the covered bases.
// Bounds: a sequence that leaves [0, ntext) has no piece and no record and sets ERR_COVER; loads of the text stay inside the dwords
// that hold bytes of it; a bitmap word is touched only where it holds a bit of a sequence; a list or a text above its capacity
// sets ERR_COVER_CAP, gives total 0 and writes nothing.  Plain C++, vector stores and atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "nh_device.h"
#include "nh_internal.h"
#include "nh_outbuild.h"
#include "nh_scan.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

constexpr uint32_t COVER_PIECE = 32 * (TL - 4);  // k-mers of a piece: 32 tiles, the classifier's segment (nh_device.h SEG_TILES)
constexpr uint32_t COVER_CHUNK = 8;              // consecutive pieces a wave claims: one binary search for all of them
constexpr uint32_t CK = 35;                      // k of the default geometry (cover_check_db)

// ---- the pieces ------------------------------------------------------------------------------------------------------------------
struct PieceArgs {
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    uint64_t n_seq, ntext, nblk;
    uint32_t piece;
    uint64_t *blk;     // nblk block sums / offsets, then [nblk] the total
    uint64_t *pstart;  // n_seq + 1: the first piece of every sequence, then the total
    int *error;
};

__device__ __forceinline__ bool seq_in_text(uint64_t o0, uint32_t n, uint64_t ntext) { return o0 <= ntext && ntext - o0 >= n; }

__device__ __forceinline__ uint64_t piece_count(const PieceArgs &a, uint64_t s, bool report) {
    if (s >= a.n_seq) return 0;
    const uint64_t o0 = a.seq_off[s];
    const uint32_t n = a.seq_len[s];
    if (!seq_in_text(o0, n, a.ntext)) {
        if (report) atomicOr(a.error, NH_ERR_COVER);
        return 0;
    }
    return n < CK ? 0 : ((uint64_t)(n - (CK - 1)) + a.piece - 1) / a.piece;
}

__global__ void __launch_bounds__(OB_THREADS) k_cover_piece_sizes(PieceArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    uint64_t total;
    (void)block_exclusive_scan(piece_count(a, (uint64_t)blockIdx.x * OB_THREADS + threadIdx.x, true), wsum, &total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(OB_THREADS) k_cover_piece_scan(PieceArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t total = scan_block_sums(a.blk, a.nblk, wsum);
    if (threadIdx.x == 0) a.blk[a.nblk] = a.pstart[a.n_seq] = total;
}

__global__ void __launch_bounds__(OB_THREADS) k_cover_piece_starts(PieceArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t s = (uint64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan(piece_count(a, s, false), wsum, &total);
    if (s < a.n_seq) a.pstart[s] = a.blk[blockIdx.x] + ex;
}

// ---- the mark pass ---------------------------------------------------------------------------------------------------------------
struct CoverDev {
    const uint64_t *pstart;  // n_seq + 1
    uint64_t n_seq;
    uint32_t piece;
    const uint8_t *host_of;  // NULL: every non-zero value is host
    uint64_t n_nodes;
    uint32_t *cover;         // ceil(ntext / 32) words
    uint64_t n_words;
};

// bit i of x -> bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// c |= c << s over 256 bits, 0 < s < 64
__device__ __forceinline__ void or_shifted(uint64_t (&c)[4], const uint32_t s) {
    c[3] |= (c[3] << s) | (c[2] >> (64 - s));
    c[2] |= (c[2] << s) | (c[1] >> (64 - s));
    c[1] |= (c[1] << s) | (c[0] >> (64 - s));
    c[0] |= c[0] << s;
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_cover_mark(const KArgs args_by_kernarg_pointer, const CoverDev m) {
    KArgsP ap = (KArgsP)__builtin_amdgcn_kernarg_segment_ptr();
    typedef WaveLdsT<true, 1, QCAP_GENERIC> WL;
    __shared__ WL lds_all[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WL &S = lds_all[wib];
    init_wave_lds<true>(S, lane);
    const uint32_t TQ = TL - 4u;  // k-mers of a full tile
    const uint64_t *const start = ap->seq_off;
    const uint32_t *const len = ap->seq_len;
    const uint64_t text_len = ap->bases_end;
    const uint32_t *const text = reinterpret_cast<const uint32_t *>(ap->bases);
    const uint32_t pl = (uint32_t)lane < PREF_LANES ? (uint32_t)lane : PREF_LANES - 1;
    const uint32_t *const table = ap->db.table;
    const uint64_t cap = ap->db.capacity;
    const uint64_t magic = ap->db.cap_magic;
    const uint64_t min_hash = ap->db.min_hash;
    const uint32_t vbits = ap->db.value_bits, vmask = ap->db.vmask;
    uint64_t prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tprev = 0;
    const uint64_t n_pieces = m.pstart[m.n_seq];
    if (n_pieces == 0 || text_len == 0) return;
    const uint64_t last_dw = (text_len - 1) >> 2;  // the last dword that holds a byte of the text
    const uint64_t n_chunks = (n_pieces + COVER_CHUNK - 1) / COVER_CHUNK;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t c = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib; c < n_chunks; c += n_waves) {
        const uint64_t p0 = c * COVER_CHUNK, p1 = p0 + COVER_CHUNK < n_pieces ? p0 + COVER_CHUNK : n_pieces;
        // the sequence of piece p0: pstart[s] <= p0 < pstart[s + 1] (wave-uniform)
        uint64_t s;
        {
            uint64_t lo = 0, hi = m.n_seq - 1;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (m.pstart[mid + 1] <= p0) lo = mid + 1;
                else hi = mid;
            }
            s = lo;
        }
        for (uint64_t p = p0; p < p1; p++) {
            while (s + 1 < m.n_seq && m.pstart[s + 1] <= p) s++;
            const uint64_t os = start[s];
            const uint32_t ns = len[s];
            const uint64_t j = p - m.pstart[s];
            // (wave-uniform; the sizes gave such a sequence no piece: the tests are the walk's own guard)
            if (ns < CK || !seq_in_text(os, ns, text_len) || j * m.piece >= (uint64_t)(ns - (CK - 1))) continue;
            const uint32_t k0 = (uint32_t)(j * m.piece);            // the piece's first k-mer
            const uint32_t nk_left = (ns - (CK - 1)) - k0;
            const uint32_t nk = nk_left < m.piece ? nk_left : m.piece;
            const uint64_t o0 = os + k0;                            // ... its first base
            const uint32_t n = nk + (CK - 1);                       // ... its bases
            uint64_t carry_min = NH_FULL;
            bool carry_host = false;  // the run that enters a tile: host or not
            uint32_t w;
            {
                uint64_t dw = (o0 >> 2) + pl;
                dw = dw < last_dw ? dw : last_dw;
                w = text[dw];
            }
            for (uint32_t q0 = 0; q0 < nk; q0 += TQ) {
                const uint64_t g0 = o0 + q0;
                const uint32_t nl_left = (n - 31u + 1) - q0;
                const uint32_t nlt = nl_left < (uint32_t)TL ? nl_left : (uint32_t)TL;
                const uint32_t nq_left = nk - q0;
                const uint32_t nqt = nq_left < TQ ? nq_left : TQ;
                // the next tile's dword is loaded while this one is scanned
                const bool more = nq_left > TQ;
                uint64_t dwn = ((g0 + TQ) >> 2) + pl;
                dwn = dwn < last_dw ? dwn : last_dw;
                uint32_t ps, w_next = 0;
                int last_lane;
                const uint32_t nruns = scan_tile<true, false>(ap, S, lane, w, (uint32_t)g0 & 3u, nlt, nqt, 0u, 0u, carry_min, ps, last_lane,
                                                              text + dwn, more, w_next, prof, tprev);
                wave_sync();
                // a tile holds at most TQ = 124 run starts: two a lane
                bool hit[2] = {false, false};
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const uint32_t r = (uint32_t)lane + 64u * t;
                    if (r >= nruns) continue;
                    const uint64_t mz = S.q[0][r];
                    // minimum_acceptable_hash_value: the classifier does not look such a minimizer up (taxon 0).  The hash is
                    // taken in front of the test, so that find_cell's own merges with it: one fmix64 a look-up, as before
                    const uint64_t hc = fmix64(mz);
                    uint64_t at;  // (the cell is of no use here)
                    const uint32_t v = min_hash != 0 && hc < min_hash ? 0u : find_cell(table, cap, magic, vbits, vmask, mz, at);
                    hit[t] = v != 0 && (m.host_of == nullptr || ((uint64_t)v < m.n_nodes && m.host_of[v] != 0));
                }
                const uint64_t hb0 = __ballot(hit[0]), hb1 = __ballot(hit[1]);
                // the lane's two k-mers: valid, and their run (1 + its index, 0: the run that entered the tile) is host
                const uint32_t r0 = ps >> 3, r1 = r0 + ((ps >> 2) & 1u);
                auto run_host = [&](uint32_t r) {
                    return r == 0 ? carry_host : r <= 64 ? ((hb0 >> (r - 1)) & 1ull) != 0 : ((hb1 >> ((r - 65) & 63u)) & 1ull) != 0;
                };
                const bool h0 = (ps & 1u) && run_host(r0), h1 = (ps & 2u) && run_host(r1);
                const uint64_t b0 = __ballot(h0), b1 = __ballot(h1);
                if (last_lane >= 0) carry_host = (((last_lane & 1) ? b1 : b0) >> (last_lane >> 1)) & 1ull;
                if (b0 | b1) {
                    // k-mer 2 t is bit t of b0, k-mer 2 t + 1 bit t of b1; k-mer q covers bases [q, q + k) of the tile: bits of c
                    uint64_t cv[4];
                    cv[0] = spread_bits((uint32_t)b0) | (spread_bits((uint32_t)b1) << 1);
                    cv[1] = spread_bits((uint32_t)(b0 >> 32)) | (spread_bits((uint32_t)(b1 >> 32)) << 1);
                    cv[2] = cv[3] = 0;
                    or_shifted(cv, 1), or_shifted(cv, 2), or_shifted(cv, 4), or_shifted(cv, 8), or_shifted(cv, 16);  // 32 bases
                    or_shifted(cv, CK - 32);
                    const uint32_t sh = (uint32_t)g0 & 31u;  // the tile's first base in its bitmap word (124 + 34 + 31 bits: four words)
                    if (sh) {
                        cv[3] = (cv[3] << sh) | (cv[2] >> (64 - sh));
                        cv[2] = (cv[2] << sh) | (cv[1] >> (64 - sh));
                        cv[1] = (cv[1] << sh) | (cv[0] >> (64 - sh));
                        cv[0] <<= sh;
                    }
                    uint32_t bits = 0;
#pragma unroll
                    for (int t = 0; t < 8; t++)
                        if (lane == t) bits = (uint32_t)(cv[t >> 1] >> (32 * (t & 1)));
                    const uint64_t wi = (g0 >> 5) + (uint64_t)lane;
                    if (bits && wi < m.n_words) atomicOr(m.cover + wi, bits);  // (a word with no new bit is not touched)
                }
                wave_sync();
                w = w_next;
            }
        }
    }
}

uint32_t cover_piece() {  // k-mers of a piece: tuning / test knob, read at every launch
    if (const char *env = getenv("NOHUMAN_COVER_PIECE")) {
        const long v = atol(env);
        if (v > 0 && v < (1l << 30)) return (uint32_t)v;
    }
    return COVER_PIECE;
}

// ---- the bitmap into records -----------------------------------------------------------------------------------------------------
// word i of the bitmap cut to the sequence [o0, end), whose words are [w0, w1]; 0 outside them (i - 1 of word 0 included)
__device__ __forceinline__ uint32_t seq_word(const uint32_t *cover, uint64_t i, uint64_t w0, uint64_t w1, uint64_t o0, uint64_t end) {
    if (i < w0 || i > w1) return 0;
    uint32_t w = cover[i];
    const uint64_t b0 = i << 5;
    if (o0 > b0) w &= 0xFFFFFFFFu << (uint32_t)(o0 - b0);
    if (end < b0 + 32) w &= 0xFFFFFFFFu >> (uint32_t)(b0 + 32 - end);
    return w;
}

__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, int lane) {
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    return incl - v;
}

// the sequence's words; false: it has no covered base to look for (too short for a k-mer, or outside the text: ERR_COVER)
__device__ __forceinline__ bool seq_words(const CoverIvlArgs &a, uint64_t s, bool report, int lane, uint64_t &o0, uint64_t &end, uint64_t &w0, uint64_t &w1) {
    o0 = a.seq_off[s];
    const uint32_t n = a.seq_len[s];
    if (!seq_in_text(o0, n, a.ntext)) {
        if (report && lane == 0) atomicOr(a.error, NH_ERR_COVER);
        return false;
    }
    if (n < CK) return false;
    end = o0 + n;
    w0 = o0 >> 5, w1 = (end - 1) >> 5;
    return true;
}

// One wave: the intervals of sequence s (wave-uniform).  WRITE: its records from rec[base]; returns their number
template <bool WRITE>
__device__ __forceinline__ uint32_t seq_intervals(const CoverIvlArgs &a, uint64_t s, int lane, uint64_t base) {
    uint64_t o0, end, w0, w1;
    if (!seq_words(a, s, !WRITE, lane, o0, end, w0, w1)) return 0;
    uint32_t cs = 0, ce = 0;  // the starts and ends of the words before this round's
    for (uint64_t it = w0; it <= w1; it += 64) {
        const uint64_t i = it + (uint64_t)lane;
        const uint32_t w = seq_word(a.cover, i, w0, w1, o0, end);
        uint32_t st = 0, en = 0;
        if (w) {
            const uint32_t before = seq_word(a.cover, i - 1, w0, w1, o0, end), after = seq_word(a.cover, i + 1, w0, w1, o0, end);
            st = w & ~((w << 1) | (before >> 31));
            en = w & ~((w >> 1) | (after << 31));
        }
        const uint32_t ns = (uint32_t)__popc(st), ne = (uint32_t)__popc(en);
        if (WRITE) {
            uint64_t xs = base + cs + wave_exclusive(ns, lane), xe = base + ce + wave_exclusive(ne, lane);
            while (st) {
                const uint32_t b = (uint32_t)__builtin_ctz(st);
                st &= st - 1;
                if (xs < a.cap) a.rec[3 * xs] = (uint32_t)s, a.rec[3 * xs + 1] = (uint32_t)((i << 5) + b - o0);
                xs++;
            }
            while (en) {
                const uint32_t b = (uint32_t)__builtin_ctz(en);
                en &= en - 1;
                if (xe < a.cap) a.rec[3 * xe + 2] = (uint32_t)((i << 5) + b + 1 - o0);
                xe++;
            }
        }
        cs += wave_sum(ns);
        if (WRITE) ce += wave_sum(ne);
    }
    return cs;
}

constexpr int IV_SEQS = OB_THREADS;  // sequences of one block: 64 a wave, one after another

// cnt[s]: the intervals of sequence s; blk[b]: those of block b
__global__ void __launch_bounds__(OB_THREADS) k_cover_ivl_sizes(CoverIvlArgs a) {
    __shared__ uint64_t wtot[OB_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * IV_SEQS + (uint64_t)wave * 64;
    uint32_t mine = 0;
    uint64_t sum = 0;
    for (int k = 0; k < 64 && first + k < a.n_seq; k++) {
        const uint32_t c = seq_intervals<false>(a, first + k, lane, 0);
        if (lane == k) mine = c;
        sum += c;
    }
    if (first + lane < a.n_seq) a.cnt[first + lane] = mine;
    if (lane == 0) wtot[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < OB_WAVES; w++) t += wtot[w];
        a.blk[blockIdx.x] = t;
    }
}

// total[0]: the records (0 where they do not fit: ERR_COVER_CAP), total[1]: the records there are
__global__ void __launch_bounds__(OB_THREADS) k_cover_ivl_scan(CoverIvlArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t total = scan_block_sums(a.blk, a.nblk, wsum);
    if (threadIdx.x == 0) {
        a.total[0] = total_fits(total, a.cap, a.error, NH_ERR_COVER_CAP) ? total : 0;
        a.blk[a.nblk] = total;
    }
}

__global__ void __launch_bounds__(OB_THREADS) k_cover_ivl_write(CoverIvlArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[IV_SEQS];
    __shared__ uint32_t s_cnt[IV_SEQS];
    if (a.blk[a.nblk] > a.cap) return;  // (block-uniform: the scan found the list too long, nothing is written)
    const uint64_t fb = (uint64_t)blockIdx.x * IV_SEQS;
    const uint32_t mine = fb + threadIdx.x < a.n_seq ? a.cnt[fb + threadIdx.x] : 0;
    s_cnt[threadIdx.x] = mine;
    uint64_t total;
    s_off[threadIdx.x] = block_exclusive_scan(mine, wsum, &total);
    __syncthreads();
    if (total == 0) return;
    const uint64_t base = a.blk[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 64; k++) {
        const int fl = wave * 64 + k;
        if (fb + fl >= a.n_seq) break;
        if (s_cnt[fl]) (void)seq_intervals<true>(a, fb + fl, lane, base + s_off[fl]);
    }
}

// ---- the gap closing -------------------------------------------------------------------------------------------------------------
constexpr unsigned CLOSE_MAX_BLOCKS = 1u << 16;

__global__ void __launch_bounds__(OB_THREADS) k_cover_close(CoverCloseArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * OB_WAVES;
    uint64_t closed = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * OB_WAVES + (threadIdx.x >> 6); s < a.n_seq; s += n_waves) {  // (wave-uniform)
        if (a.res != nullptr && a.res[s / (uint32_t)a.mates].call == 0) continue;  // (no host fragment: the mask builder does not ask)
        const uint64_t o0 = a.seq_off[s];
        const uint32_t n = a.seq_len[s];
        if (!seq_in_text(o0, n, a.ntext)) {
            if (lane == 0) atomicOr(a.error, NH_ERR_COVER);
            continue;
        }
        if (n < 3) continue;  // (no base with a neighbour on each side)
        const uint64_t end = o0 + n, w0 = o0 >> 5, w1 = (end - 1) >> 5;
        for (uint64_t it = w0; it <= w1; it += 64) {
            const uint64_t i = it + (uint64_t)lane;
            const uint32_t w = seq_word(a.cover, i, w0, w1, o0, end);
            if (!w) continue;
            uint32_t en = w & ~((w >> 1) | (seq_word(a.cover, i + 1, w0, w1, o0, end) << 31));  // covered, the next base not
            while (en) {
                const uint32_t b = (uint32_t)__builtin_ctz(en);
                en &= en - 1;
                const uint64_t e = (i << 5) + b + 1;  // the run's first base; the sequence's next covered base is the run's end
                const uint32_t rest = b == 31 ? 0u : w >> (b + 1);
                uint64_t nx = ~0ull;
                if (rest) nx = e + (uint32_t)__builtin_ctz(rest);
                else
                    for (uint64_t j = i + 1; j <= w1 && (j << 5) <= e + a.gap; j++) {
                        const uint32_t x = seq_word(a.cover, j, w0, w1, o0, end);
                        if (x) {
                            nx = (j << 5) + (uint32_t)__builtin_ctz(x);
                            break;
                        }
                    }
                if (nx == ~0ull || nx - e > a.gap) continue;  // (it touches the sequence's end, or is longer than the gap)
                for (uint64_t j = e >> 5; j <= (nx - 1) >> 5; j++) {  // (words of the sequence: e > o0, nx < end)
                    const uint64_t b0 = j << 5;
                    const uint32_t lo = e > b0 ? (uint32_t)(e - b0) : 0u, hi = nx < b0 + 32 ? (uint32_t)(nx - b0) : 32u;
                    atomicOr(a.cover + j, (hi == 32 ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u));
                }
                closed += nx - e;
            }
        }
    }
    if (a.closed == nullptr) return;
    const uint32_t lo = wave_sum((uint32_t)closed), hi = wave_sum((uint32_t)(closed >> 32));  // (a lane's sum is below 2^40: text_len)
    if (lane == 0 && (lo | hi)) atomicAdd(a.closed, ((unsigned long long)hi << 32) + lo);
}

// ---- the records into lines ------------------------------------------------------------------------------------------------------
constexpr int N_LFIELDS = 4;  // the numbers of a line: start, end, mate, taxid

struct IvLine {
    uint64_t id;     // absolute offset of the id in the batch's text
    uint32_t idlen;  // after TrimPairInfo
    uint64_t v[N_LFIELDS];
    uint32_t nd[N_LFIELDS];
    uint64_t len;    // bytes of the line, 0: none
    uint64_t frag;
};

// the line of record i; length 0 for a record that fails its bounds (error set)
__device__ inline IvLine load_ivline(const CoverLinesArgs &a, uint64_t i, uint64_t n_rec, bool report) {
    IvLine L{};
    if (i >= n_rec) return L;
    const uint32_t seq = a.ivl[3 * i], st = a.ivl[3 * i + 1], en = a.ivl[3 * i + 2];
    const uint64_t f = seq / (uint32_t)a.mates;
    bool ok = f < a.n && en > st;
    nh_result r{};
    if (ok) {
        r = a.res[f];
        ok = r.call < a.n_ext && read_id(a.text, a.ntext, a.rec, a.idlen, f, a.mates, &L.id, &L.idlen);
    }
    if (!ok) {
        if (report) atomicOr(a.error, NH_ERR_COVER);
        return L;
    }
    L.frag = f;
    L.v[0] = st, L.v[1] = en, L.v[2] = 1 + seq % (uint32_t)a.mates, L.v[3] = r.call ? a.ext[r.call] : 0;
    uint64_t tail = 0;
#pragma unroll
    for (int k = 0; k < N_LFIELDS; k++) {
        L.nd[k] = decimal_digits(L.v[k]);
        tail += 1 + L.nd[k];
    }
    L.len = (uint64_t)L.idlen + tail + 1;
    return L;
}

// blk: [b] the bytes of block b, [nblk + b] the fragments that begin in it, [2 nblk + b] its covered bases
__global__ void __launch_bounds__(OB_THREADS) k_cover_line_sizes(CoverLinesArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t n_rec = *a.n_ivl <= a.cap_ivl ? *a.n_ivl : 0;
    const uint64_t i = (uint64_t)blockIdx.x * OB_THREADS + threadIdx.x;
    const IvLine L = load_ivline(a, i, n_rec, true);
    // a fragment is counted at its first record (the records are in sequence order: a fragment's lie together)
    const bool first = L.len != 0 && (i == 0 || a.ivl[3 * (i - 1)] / (uint32_t)a.mates != a.ivl[3 * i] / (uint32_t)a.mates);
    uint64_t bytes, frags, covered;
    (void)block_exclusive_scan(L.len, wsum, &bytes);
    __syncthreads();
    (void)block_exclusive_scan(first ? 1 : 0, wsum, &frags);
    __syncthreads();
    (void)block_exclusive_scan(L.len ? L.v[1] - L.v[0] : 0, wsum, &covered);
    if (threadIdx.x == 0) {
        a.blk[blockIdx.x] = bytes;
        a.blk[a.nblk + blockIdx.x] = frags;
        a.blk[2 * a.nblk + blockIdx.x] = covered;
    }
}

// one workgroup: block sums -> block offsets; total: bytes, lines, fragments, covered bases
__global__ void __launch_bounds__(OB_THREADS) k_cover_line_scan(CoverLinesArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t n_rec = *a.n_ivl <= a.cap_ivl ? *a.n_ivl : 0;
    const uint64_t total = scan_block_sums(a.blk, a.nblk, wsum);
    uint64_t sums[2] = {0, 0};
    for (int q = 0; q < 2; q++)
        for (uint64_t c = 0; c < a.nblk; c += OB_THREADS) {
            const uint64_t i = c + threadIdx.x;
            uint64_t part;
            (void)block_exclusive_scan(i < a.nblk ? a.blk[(uint64_t)(1 + q) * a.nblk + i] : 0, wsum, &part);
            sums[q] += part;
            __syncthreads();  // (wsum is written again by the next chunk)
        }
    if (threadIdx.x == 0) {
        const bool fits = total_fits(total, a.cap, a.error, NH_ERR_COVER_CAP);
        a.total[0] = fits ? total : 0;
        a.total[1] = fits ? n_rec : 0;
        a.total[2] = fits ? sums[0] : 0;
        a.total[3] = fits ? sums[1] : 0;
    }
}

// byte p of the line (0 <= p < L.len)
__device__ inline uint8_t ivline_byte(const CoverLinesArgs &a, const IvLine &L, uint64_t p) {
    if (p < L.idlen) return (uint8_t)a.text[L.id + p];
    p -= L.idlen;
    uint64_t v = 0;
    uint32_t nd = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < N_LFIELDS; k++) {
        const uint64_t w = 1ull + L.nd[k];
        if (!found && p < w) v = L.v[k], nd = L.nd[k], found = true;
        if (!found) p -= w;
    }
    if (!found) return '\n';
    if (p == 0) return '\t';
    for (uint32_t j = nd - (uint32_t)p; j; j--) v /= 10;
    return (uint8_t)('0' + v % 10);
}

__global__ void __launch_bounds__(OB_THREADS) k_cover_line_write(CoverLinesArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[OB_THREADS];
    const uint64_t n_rec = *a.n_ivl <= a.cap_ivl ? *a.n_ivl : 0;
    const uint64_t fb = (uint64_t)blockIdx.x * OB_THREADS;
    if (fb >= n_rec) return;  // (block-uniform)
    block_offsets<1>(s_off, wsum, [&](uint32_t fl) { return load_ivline(a, fb + fl, n_rec, false).len; });
    const uint64_t base = a.blk[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < OB_THREADS / OB_WAVES; k++) {
        const int fl = wave * (OB_THREADS / OB_WAVES) + k;
        if (fb + fl >= n_rec) break;
        const IvLine L = load_ivline(a, fb + fl, n_rec, false);
        if (L.len == 0) continue;
        const uint64_t at = base + s_off[fl];
        if (at + L.len > a.cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0) atomicOr(a.error, NH_ERR_COVER_CAP);
            continue;
        }
        wave_write(
            a.out, at, L.len, lane, [&](uint64_t p) { return ivline_byte(a, L, p); },
            [&](uint64_t p, uint32_t *v) {
                if (p + 4 > L.idlen) return false;
                *v = text_dword(a.text, L.id + p);
                return true;
            });
    }
}

}  // namespace

int cover_check_db(const Engine *e) {
    const nh_db_info &i = e->info;
    const char *const what = "host intervals: the pass supports the default geometry and linear probing only";
    if (i.k != 35) return set_error(NH_EINVAL, "%s: k is %llu, not 35", what, (unsigned long long)i.k);
    if (i.l != 31) return set_error(NH_EINVAL, "%s: l is %llu, not 31", what, (unsigned long long)i.l);
    if (i.spaced_seed_mask != SPACED_MASK)
        return set_error(NH_EINVAL, "%s: spaced_seed_mask is 0x%llx, not 0x%llx", what, (unsigned long long)i.spaced_seed_mask, (unsigned long long)SPACED_MASK);
    if (i.toggle_mask != TOGGLE_MASK)
        return set_error(NH_EINVAL, "%s: toggle_mask is 0x%llx, not 0x%llx", what, (unsigned long long)i.toggle_mask, (unsigned long long)TOGGLE_MASK);
    if (i.revcom_version == 0) return set_error(NH_EINVAL, "%s: revcom_version is 0 (a legacy database)", what);
    if (!e->options.linear_probing) return set_error(NH_EINVAL, "%s: linear_probing is 0 in the engine's options", what);
    return NH_OK;
}

uint64_t cover_words(uint64_t ntext) { return (ntext + 31) >> 5; }
static uint64_t seq_blocks(uint64_t n_seq) { return (n_seq + OB_THREADS - 1) / OB_THREADS; }
uint64_t cover_mark_scratch_words(uint64_t n_seq) { return (n_seq + 1) + seq_blocks(n_seq) + 1; }
uint64_t cover_intervals_scratch_words(uint64_t n_seq) { return (n_seq + 1) / 2 + seq_blocks(n_seq) + 1; }
uint64_t cover_line_blocks(uint64_t cap_ivl) { return (cap_ivl + OB_THREADS - 1) / OB_THREADS; }

hipError_t launch_cover_mark(Engine *e, const CoverArgs &c, hipStream_t stream) {
    if (c.n_seq == 0 || c.ntext == 0) return hipSuccess;
    PieceArgs pa{};
    pa.seq_off = c.seq_off, pa.seq_len = c.seq_len, pa.n_seq = c.n_seq, pa.ntext = c.ntext, pa.nblk = seq_blocks(c.n_seq);
    pa.piece = cover_piece();
    pa.pstart = c.scratch, pa.blk = c.scratch + (c.n_seq + 1);
    pa.error = c.error;
    hipLaunchKernelGGL(k_cover_piece_sizes, dim3((unsigned)pa.nblk), dim3(OB_THREADS), 0, stream, pa);
    hipLaunchKernelGGL(k_cover_piece_scan, dim3(1), dim3(OB_THREADS), 0, stream, pa);
    hipLaunchKernelGGL(k_cover_piece_starts, dim3((unsigned)pa.nblk), dim3(OB_THREADS), 0, stream, pa);
    KArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.db = devdb_now(e);
    ka.bases = (const uint8_t *)c.text;
    ka.seq_off = c.seq_off;
    ka.seq_len = c.seq_len;
    ka.bases_end = c.ntext;
    ka.n_frag = c.n_seq;
    ka.mates = 1;
    CoverDev m{};
    m.pstart = pa.pstart, m.n_seq = c.n_seq, m.piece = pa.piece;
    m.host_of = c.host_of, m.n_nodes = c.n_nodes;
    m.cover = c.cover, m.n_words = cover_words(c.ntext);
    // the pieces there are is known on the device only: at least a piece a sequence's worth of waves, bounded by what the device holds
    const uint64_t by_text = c.ntext / ((uint64_t)pa.piece * COVER_CHUNK) + 1;
    const uint64_t want = (std::max<uint64_t>(by_text, (c.n_seq + COVER_CHUNK - 1) / COVER_CHUNK) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    static const int per_cu = blocks_per_cu(k_cover_mark, WAVE * WAVES_PER_BLOCK, 4);
    const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)std::max(1, e->n_cu) * per_cu);
    hipLaunchKernelGGL(k_cover_mark, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, ka, m);
    return hipGetLastError();
}

hipError_t launch_cover_intervals(const CoverIvlArgs &a_, hipStream_t stream) {
    if (a_.n_seq == 0) return hipMemsetAsync(a_.total, 0, sizeof(uint64_t), stream);
    CoverIvlArgs a = a_;
    a.nblk = seq_blocks(a.n_seq);
    a.cnt = (uint32_t *)a.scratch;
    a.blk = a.scratch + (a.n_seq + 1) / 2;
    hipLaunchKernelGGL(k_cover_ivl_sizes, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_cover_ivl_scan, dim3(1), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_cover_ivl_write, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cover_close(const CoverCloseArgs &a, hipStream_t stream) {
    if (a.n_seq == 0 || a.gap == 0) return hipSuccess;
    const uint64_t want = (a.n_seq + OB_WAVES - 1) / OB_WAVES;
    hipLaunchKernelGGL(k_cover_close, dim3((unsigned)std::min<uint64_t>(want, CLOSE_MAX_BLOCKS)), dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cover_lines(const CoverLinesArgs &a, hipStream_t stream) {
    if (a.n == 0 || a.nblk == 0) return hipMemsetAsync(a.total, 0, 4 * sizeof(uint64_t), stream);
    hipLaunchKernelGGL(k_cover_line_sizes, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_cover_line_scan, dim3(1), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_cover_line_write, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_host_cover_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                                    uint64_t n_seq, const void *d_host_of, uint64_t n_nodes, void *d_cover, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_text || !d_cover || (n_seq && (!d_seq_starts || !d_seq_lens))) return nh::set_error(NH_EINVAL, "nh_host_cover_device: null argument");
    if (((uintptr_t)d_text & 3) || ((uintptr_t)d_cover & 3)) return nh::set_error(NH_EINVAL, "nh_host_cover_device: the text and the bitmap must be 4-byte aligned");
    if (n_seq > (1ull << 32) || text_len >= (1ull << 40)) return nh::set_error(NH_EINVAL, "nh_host_cover_device: too many sequences or too much text for one launch");
    if (const int rc = nh::cover_check_db(e)) return rc;
    if (n_seq == 0 || text_len == 0) return NH_OK;
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::DevBuf<uint64_t> scratch;
    if (scratch.reserve(nh::cover_mark_scratch_words(n_seq)) != hipSuccess) {
        (void)hipGetLastError();
        return nh::set_error(NH_EOOM, "nh_host_cover_device: cannot allocate %llu words of scratch", (unsigned long long)nh::cover_mark_scratch_words(n_seq));
    }
    nh::CoverArgs c{};
    c.text = (const char *)d_text, c.ntext = text_len;
    c.seq_off = (const uint64_t *)d_seq_starts, c.seq_len = (const uint32_t *)d_seq_lens, c.n_seq = n_seq;
    c.host_of = (const uint8_t *)d_host_of, c.n_nodes = n_nodes;
    c.cover = (uint32_t *)d_cover, c.scratch = scratch;
    c.error = e->d_error + nh::LAUNCH_SLOTS;
    hipError_t he = nh::launch_cover_mark(e, c, (hipStream_t)stream);
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);  // (the scratch is the launches' until they are done)
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "host intervals, mark launch: %s", hipGetErrorString(he));
    return NH_OK;
}

extern "C" int nh_cover_intervals_device(nh_engine *e_, const void *d_cover, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                                         uint64_t n_seq, void *d_intervals, uint64_t cap_records, void *d_total, void *error_bits, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_cover || !d_total || !error_bits || (cap_records && !d_intervals) || (n_seq && (!d_seq_starts || !d_seq_lens)))
        return nh::set_error(NH_EINVAL, "nh_cover_intervals_device: null argument");
    if (((uintptr_t)d_cover & 3) || ((uintptr_t)d_intervals & 3) || ((uintptr_t)d_total & 7) || ((uintptr_t)error_bits & 3))
        return nh::set_error(NH_EINVAL, "nh_cover_intervals_device: the bitmap, the records and the error word must be 4-byte aligned, the total 8-byte aligned");
    if (n_seq > (1ull << 32) || text_len >= (1ull << 40)) return nh::set_error(NH_EINVAL, "nh_cover_intervals_device: too many sequences or too much text for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::DevBuf<uint64_t> scratch;
    if (n_seq && scratch.reserve(nh::cover_intervals_scratch_words(n_seq)) != hipSuccess) {
        (void)hipGetLastError();
        return nh::set_error(NH_EOOM, "nh_cover_intervals_device: cannot allocate %llu words of scratch", (unsigned long long)nh::cover_intervals_scratch_words(n_seq));
    }
    nh::CoverIvlArgs a{};
    a.cover = (const uint32_t *)d_cover, a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts, a.seq_len = (const uint32_t *)d_seq_lens, a.n_seq = n_seq;
    a.rec = (uint32_t *)d_intervals, a.cap = cap_records, a.total = (uint64_t *)d_total, a.scratch = scratch;
    a.error = (int *)error_bits;
    hipError_t he = nh::launch_cover_intervals(a, (hipStream_t)stream);
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "host intervals, interval launch: %s", hipGetErrorString(he));
    return NH_OK;
}

extern "C" int nh_cover_close_device(nh_engine *e_, void *d_cover, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens, uint64_t n_seq,
                                     uint32_t gap, void *d_closed_bases, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_cover || (n_seq && (!d_seq_starts || !d_seq_lens))) return nh::set_error(NH_EINVAL, "nh_cover_close_device: null argument");
    if (((uintptr_t)d_cover & 3) || ((uintptr_t)d_closed_bases & 7))
        return nh::set_error(NH_EINVAL, "nh_cover_close_device: the bitmap must be 4-byte aligned, the counter 8-byte aligned");
    if (gap > NH_HOST_GAP_MAX) return nh::set_error(NH_EINVAL, "nh_cover_close_device: gap %u is above NH_HOST_GAP_MAX (%d)", gap, NH_HOST_GAP_MAX);
    if (n_seq > (1ull << 32) || text_len >= (1ull << 40)) return nh::set_error(NH_EINVAL, "nh_cover_close_device: too many sequences or too much text for one launch");
    if (n_seq == 0 || gap == 0 || text_len == 0) return NH_OK;
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::CoverCloseArgs a{};
    a.cover = (uint32_t *)d_cover, a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts, a.seq_len = (const uint32_t *)d_seq_lens, a.n_seq = n_seq;
    a.gap = gap, a.res = nullptr, a.mates = 1, a.closed = (unsigned long long *)d_closed_bases;
    a.error = e->d_error + nh::LAUNCH_SLOTS;
    hipError_t he = nh::launch_cover_close(a, (hipStream_t)stream);
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "host bases only, closing launch: %s", hipGetErrorString(he));
    return NH_OK;
}
