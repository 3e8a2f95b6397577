// nh_cut.hip -- the text of a host-cut run, built in HBM (nh_run_hostcut, --host-cut): a single-end masked run whose host fragments
// are cut at the stretches the closed coverage covers and written as pieces, every other fragment whole.  DESIGN.md 6.23;
// tests/hostcut_model.py is the specification.
//
// An ITEM is {seq, a, b}: bases [a, b) of sequence seq.  A fragment whose call is 0 has one item, its whole record (0, slen), written
// as nh_run_mask writes an unclassified record.  A host fragment has one item for every maximal run of at least min_piece bases that
// the cover bitmap (one bit a byte of the text, after the closing) does not cover; its record is
//   header[0, 1 + idlen) ":<a>-<b>" header[1 + idlen, hlen) "\n" bases[a, b) ("\n+\n" qualities[a, b)) "\n"
// The output is not one record a fragment, so the builder has two stages, each nh_outbuild.h's sizes, scan and write:
//   k_cut_item_*  the item list.  A block takes OB_THREADS sequences, a lane has its own: a sequence that is not host counts one
//                 item without a look at the bitmap; the host sequences of a wave (a ballot) are walked by the whole wave one after
//                 the other, a lane a bitmap word, 64 words a round -- the interval builder's method on the COMPLEMENT of the bitmap
//                 cut to the sequence: starts = u & ~(u << 1 | last bit of the word before), ends likewise.  A run is made where it
//                 ENDS: its start is the last start at or below the end in the lane's own word, else the last start of the nearest
//                 lane in front that has one (one ballot and one shuffle a round), else the run that entered the round (wave-uniform
//                 carry).  So the length test against min_piece is the lane's own, no thread walks a long read's words, and a
//                 sequence shorter than k is what it is: one uncovered run.  The sizes count what the run reports (host bases,
//                 pieces, their bases, covered bases, bases in runs below min_piece, host fragments without a piece), a lane's sums
//                 reduced once a wave.
//   k_cut_*       the text: an item a thread for the lengths -- the sizes keep every item's offset in its block (ioff), so the write
//                 needs no scan of its own and any wave can take any item --, then a wave an item AND SPAN for the bytes: span y of
//                 an item is the aligned dwords [A + y * span, A + (y + 1) * span) of its output, A the dword of its first byte
//                 (span: CUT_SPAN = 16 KiB, NOHUMAN_CUT_SPAN).  The (item, span) pairs -- `rows` spans an item, those of the longest
//                 item the batch can hold -- are dealt to the waves of a grid that fills the device, in turn; a pair whose item ends
//                 in front of its span costs one load of the item's length (ilen).  The bytes are wave_write()'s: header, sequence
//                 slice and quality slice as text_dword() of their source position, the ":<a>-<b>" digits and the seams through the
//                 byte closure.  (One wave for 64 items one after the other, a long item whole, was measured first:
//                 profiles/host_cut.txt.)
// Bounds: a sequence that leaves [0, ntext) has no item (NH_ERR_CUT); a bitmap word is read only where it holds a bit of a sequence
// inside the text; a record whose fields leave the text, whose id is longer than its header (NH_ERR_CUT) or -- a FASTQ host record --
// whose quality line is not as long as its sequence (NH_ERR_CUT_QLEN) writes nothing; an item list or a text above its capacity
// sets NH_ERR_CUT_CAP, gives total 0 and writes nothing; every store lies inside [0, cap) of its buffer.  Plain C++, vector stores
// and atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "nh_internal.h"
#include "nh_outbuild.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

constexpr uint32_t CUT_K = 35;          // k of the geometry the mark pass supports (cover_check_db): the capacity's only use of it
constexpr int CI_SEQS = OB_THREADS;     // sequences of one block of the item list
constexpr int CB_ITEMS = OB_THREADS;    // items of one block of the text
constexpr uint32_t NO_RUN = 0xFFFFFFFFu;
constexpr uint32_t CUT_SPAN = 16u << 10;  // bytes of an item's output that one wave writes

struct CutDev {
    CutArgs a;
    uint32_t *cnt;   // n: the items of every sequence
    uint64_t *iblk;  // n_iblk block sums / offsets of the item list, then [n_iblk] the items there are
    uint64_t n_iblk;
    uint64_t *tblk;  // n_tblk block sums / offsets of the text, then [n_tblk] the bytes there are
    uint64_t n_tblk;
    uint64_t *ioff;  // cap_items: every item's offset in its block's text
    uint32_t *ilen;  // cap_items: every item's bytes (saturated: it decides which spans an item has, no more)
    uint32_t span;   // a multiple of 256
    uint32_t rows;   // spans an item: those of the longest there can be
};

__device__ __forceinline__ bool cut_seq_in_text(uint64_t o0, uint32_t n, uint64_t ntext) { return o0 <= ntext && ntext - o0 >= n; }

__device__ __forceinline__ uint64_t wave_total64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_exclusive32(uint32_t v, int lane) {
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    return incl - v;
}

// the bits of bitmap word i that belong to the sequence [o0, end), whose words are [w0, w1]; 0 outside them (i - 1 of word 0 included)
__device__ __forceinline__ uint32_t seq_bits(uint64_t i, uint64_t w0, uint64_t w1, uint64_t o0, uint64_t end) {
    if (i < w0 || i > w1) return 0;
    uint32_t m = 0xFFFFFFFFu;
    const uint64_t b0 = i << 5;
    if (o0 > b0) m &= 0xFFFFFFFFu << (uint32_t)(o0 - b0);
    if (end < b0 + 32) m &= 0xFFFFFFFFu >> (uint32_t)(b0 + 32 - end);
    return m;
}

// ... and those of them that are NOT covered (a word without a bit of the sequence is not loaded)
__device__ __forceinline__ uint32_t unc_word(const uint32_t *cover, uint64_t i, uint64_t w0, uint64_t w1, uint64_t o0, uint64_t end) {
    const uint32_t m = seq_bits(i, w0, w1, o0, end);
    return m ? m & ~cover[i] : 0u;
}

__device__ __forceinline__ uint32_t top_bit(uint32_t w) { return 31u - (uint32_t)__clz((int)w); }  // (w != 0)

// One wave: the pieces of host sequence s (wave-uniform; inside the text, not empty).  WRITE: its items from items[base]; else the
// lane's counts go up.  Returns the number of pieces.
template <bool WRITE>
__device__ __forceinline__ uint32_t seq_pieces(const CutArgs &a, uint64_t s, int lane, uint64_t base, uint64_t (&c)[CUT_COUNTS]) {
    const uint64_t o0 = a.seq_off[s];
    const uint64_t end = o0 + a.seq_len[s], w0 = o0 >> 5, w1 = (end - 1) >> 5;
    const uint32_t M = a.min_piece;
    uint32_t done = 0;       // the pieces that end in the words before this round's
    uint32_t open = NO_RUN;  // the start of the uncovered run that enters this round
    for (uint64_t it = w0; it <= w1; it += 64) {
        const uint64_t i = it + (uint64_t)lane;
        const uint32_t bits = seq_bits(i, w0, w1, o0, end);
        const uint32_t cw = bits ? a.cover[i] : 0u;
        const uint32_t u = bits & ~cw;
        uint32_t st = 0, en = 0;
        if (u) {
            const uint32_t before = unc_word(a.cover, i - 1, w0, w1, o0, end), after = unc_word(a.cover, i + 1, w0, w1, o0, end);
            st = u & ~((u << 1) | (before >> 31));
            en = u & ~((u >> 1) | (after << 31));
        }
        // positions count from the sequence's first base (word w0 begins at or in front of it: the sum with a bit of the sequence does not wrap)
        const uint32_t rel0 = (uint32_t)((i << 5) - o0);
        const uint32_t my_st = st ? rel0 + top_bit(st) : 0u, my_en = en ? rel0 + top_bit(en) : 0u;
        const uint64_t has_st = __ballot(st != 0), has_en = __ballot(en != 0);
        const uint64_t infront = has_st & ((1ull << lane) - 1ull);
        const uint32_t from = __shfl(my_st, infront ? 63 - __clzll((long long)infront) : 0, 64);
        const uint32_t prev_st = infront ? from : open;  // the last start in front of this lane's word
        // f(a, b): every run [a, b) that ends in this lane's word, in order
        auto runs = [&](auto f) {
            uint32_t e = en;
            while (e) {
                const uint32_t b = (uint32_t)__builtin_ctz(e);
                e &= e - 1;
                const uint32_t below = st & (0xFFFFFFFFu >> (31u - b));
                f(below ? rel0 + top_bit(below) : prev_st, rel0 + b + 1u);
            }
        };
        uint32_t np = 0;
        runs([&](uint32_t ra, uint32_t rb) {
            if (rb - ra >= M) {
                np++;
                if (!WRITE) c[CUT_PIECES]++, c[CUT_PIECE_BASES] += rb - ra;
            } else if (!WRITE) {
                c[CUT_SHORT_BASES] += rb - ra;
            }
        });
        if (!WRITE) c[CUT_CUT_BASES] += (uint32_t)__popc(bits & cw);
        if (WRITE) {
            uint64_t x = base + done + wave_exclusive32(np, lane);
            runs([&](uint32_t ra, uint32_t rb) {
                if (rb - ra < M) return;
                if (x < a.cap_items) a.items[3 * x] = (uint32_t)s, a.items[3 * x + 1] = ra, a.items[3 * x + 2] = rb;
                x++;
            });
        }
        done += (uint32_t)wave_total64(np);
        // the run that leaves the round open: the round's last start, unless an end lies at or behind it
        if (has_st) {
            const uint32_t S = __shfl(my_st, 63 - __clzll((long long)has_st), 64);
            const uint32_t E = __shfl(my_en, has_en ? 63 - __clzll((long long)has_en) : 0, 64);
            open = has_en && E >= S ? NO_RUN : S;
        } else if (has_en) {
            open = NO_RUN;
        }
    }
    return done;
}

// what the lane's own sequence is: 0 nothing (none, outside the text: error, or an empty host sequence), 1 whole, 2 host
__device__ __forceinline__ int seq_kind(const CutArgs &a, uint64_t s, bool report, uint32_t *len) {
    *len = 0;
    if (s >= a.n) return 0;
    const uint32_t n = a.seq_len[s];
    if (!cut_seq_in_text(a.seq_off[s], n, a.ntext)) {
        if (report) atomicOr(a.error, NH_ERR_CUT);
        return 0;
    }
    *len = n;
    return a.res[s].call == 0 ? 1 : 2;
}

// cnt[s]: the items of sequence s; iblk[b]: those of block b; the run's counts
__global__ void __launch_bounds__(OB_THREADS) k_cut_item_sizes(CutDev d) {
    __shared__ uint64_t wtot[OB_WAVES];
    const CutArgs &a = d.a;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * CI_SEQS + (uint64_t)wave * 64;
    uint64_t c[CUT_COUNTS] = {0, 0, 0, 0, 0, 0};
    uint32_t len;
    const int kind = seq_kind(a, first + lane, true, &len);
    uint32_t mine = kind == 1 ? 1u : 0u;
    if (kind == 2) {
        c[CUT_HOST_BASES] += len;
        if (len == 0) c[CUT_DROPPED]++;
    }
    uint64_t hosts = __ballot(kind == 2 && len != 0);
    while (hosts) {  // (wave-uniform)
        const int k = __builtin_ctzll(hosts);
        hosts &= hosts - 1;
        const uint32_t np = seq_pieces<false>(a, first + k, lane, 0, c);
        if (lane == k) {
            mine = np;
            if (np == 0) c[CUT_DROPPED]++;
        }
    }
    if (first + lane < a.n) d.cnt[first + lane] = mine;
    const uint64_t sum = wave_total64(mine);
    if (lane == 0) wtot[wave] = sum;
    if (a.counts != nullptr) {
#pragma unroll
        for (int q = 0; q < CUT_COUNTS; q++) {
            const uint64_t t = wave_total64(c[q]);
            if (lane == 0 && t) atomicAdd(a.counts + q, (unsigned long long)t);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < OB_WAVES; w++) t += wtot[w];
        d.iblk[blockIdx.x] = t;
    }
}

// total[1]: the items (0 where they do not fit: NH_ERR_CUT_CAP); iblk[n_iblk]: the items there are
__global__ void __launch_bounds__(OB_THREADS) k_cut_item_scan(CutDev d) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t total = scan_block_sums(d.iblk, d.n_iblk, wsum);
    if (threadIdx.x == 0) {
        d.a.total[1] = total_fits(total, d.a.cap_items, d.a.error, NH_ERR_CUT_CAP) ? total : 0;
        d.iblk[d.n_iblk] = total;
    }
}

__global__ void __launch_bounds__(OB_THREADS) k_cut_item_write(CutDev d) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[CI_SEQS];
    const CutArgs &a = d.a;
    if (d.iblk[d.n_iblk] > a.cap_items) return;  // (block-uniform: the scan found the list too long, nothing is written)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t s = (uint64_t)blockIdx.x * CI_SEQS + threadIdx.x;
    const uint32_t mine = s < a.n ? d.cnt[s] : 0;
    uint64_t total;
    const uint64_t at = d.iblk[blockIdx.x] + block_exclusive_scan(mine, wsum, &total);
    s_off[threadIdx.x] = at;
    __syncthreads();
    if (total == 0) return;
    uint32_t len;
    const int kind = mine ? seq_kind(a, s, false, &len) : 0;
    if (kind == 1 && at < a.cap_items) a.items[3 * at] = (uint32_t)s, a.items[3 * at + 1] = 0, a.items[3 * at + 2] = len;
    uint64_t c[CUT_COUNTS];  // (not counted again)
    uint64_t hosts = __ballot(kind == 2);
    while (hosts) {  // (wave-uniform)
        const int k = __builtin_ctzll(hosts);
        hosts &= hosts - 1;
        (void)seq_pieces<true>(a, (uint64_t)blockIdx.x * CI_SEQS + (uint64_t)wave * 64 + k, lane, s_off[wave * 64 + k], c);
    }
}

// ---- the items into text ---------------------------------------------------------------------------------------------------------
struct CItem {  // one item's fields, absolute offsets into the batch's text
    uint64_t h, s, q;       // the header, the first base written, the first quality written
    uint32_t hlen, head;    // the header's bytes; those in front of the coordinates (a whole record: all of them)
    uint32_t slen;          // bases (and, FASTQ, qualities) written
    uint32_t qlen;
    uint32_t va, vb, na, nb, clen;  // a piece's coordinates, their digits, the bytes of ":<a>-<b>" (a whole record: 0)
    uint64_t len;           // bytes of its output, 0: nothing (no item, or one that fails its checks: error set)
};

__device__ inline CItem load_citem(const CutArgs &a, uint64_t i, uint64_t n_items, bool report) {
    CItem r{};
    if (i >= n_items) return r;
    const uint32_t seq = a.items[3 * i], va = a.items[3 * i + 1], vb = a.items[3 * i + 2];
    bool ok = seq < a.n;
    uint4 fr{};
    uint64_t s0 = 0;
    uint32_t sl = 0, idl = 0;
    bool piece = false;
    if (ok) {
        fr = reinterpret_cast<const uint4 *>(a.rec)[seq];
        s0 = a.seq_off[seq], sl = a.seq_len[seq], idl = a.idlen[seq];
        piece = a.res[seq].call != 0;
    }
    const bool fastq = a.fastq != 0;
    const uint64_t h = fr.x, hlen = fr.y, q = fr.z, qlen = fastq ? fr.w : 0;
    ok = ok && h + hlen <= a.ntext && cut_seq_in_text(s0, sl, a.ntext) && (qlen == 0 || q + qlen <= a.ntext) && va <= vb && vb <= sl;
    if (piece) ok = ok && (uint64_t)idl + 1 <= hlen;
    if (!ok) {
        if (report) atomicOr(a.error, NH_ERR_CUT);
        return r;
    }
    if (piece && fastq && qlen != sl) {  // (a piece's qualities are a slice: the line must be the sequence's length)
        if (report) atomicOr(a.error, NH_ERR_CUT_QLEN);
        return r;
    }
    r.h = h, r.hlen = (uint32_t)hlen;
    if (piece) {
        r.head = 1 + idl, r.s = s0 + va, r.slen = vb - va, r.q = q + va, r.qlen = fastq ? vb - va : 0;
        r.va = va, r.vb = vb, r.na = decimal_digits(va), r.nb = decimal_digits(vb), r.clen = 2 + r.na + r.nb;
    } else {
        r.head = (uint32_t)hlen, r.s = s0, r.slen = sl, r.q = q, r.qlen = (uint32_t)qlen;
    }
    r.len = (uint64_t)r.hlen + r.clen + 1 + r.slen + 1 + (fastq ? 3ull + r.qlen : 0ull);
    return r;
}

// digit j (from the left) of v, which has nd digits
__device__ __forceinline__ uint8_t digit_of(uint32_t v, uint32_t nd, uint32_t j) {
    for (uint32_t t = nd - 1 - j; t; t--) v /= 10;
    return (uint8_t)('0' + v % 10);
}

// byte p of the item's output (0 <= p < r.len)
__device__ inline uint8_t citem_byte(const CutArgs &a, const CItem &r, uint64_t p) {
    if (p < r.head) return (uint8_t)a.text[r.h + p];
    p -= r.head;
    if (p < r.clen) {
        if (p == 0) return ':';
        p -= 1;
        if (p < r.na) return digit_of(r.va, r.na, (uint32_t)p);
        p -= r.na;
        if (p == 0) return '-';
        return digit_of(r.vb, r.nb, (uint32_t)p - 1);
    }
    p -= r.clen;
    const uint32_t rest = r.hlen - r.head;
    if (p < rest) return (uint8_t)a.text[r.h + r.head + p];
    p -= rest;
    if (p == 0) return '\n';
    p -= 1;
    if (p < r.slen) return (uint8_t)a.text[r.s + p];
    p -= r.slen;
    if (!a.fastq) return '\n';
    if (p < 3) return p == 1 ? '+' : '\n';
    p -= 3;
    if (p < r.qlen) return (uint8_t)a.text[r.q + p];
    return '\n';
}

// the items there are, as the item scan left them
__device__ __forceinline__ uint64_t items_now(const CutArgs &a) {
    const uint64_t n = a.total[1];
    return n <= a.cap_items ? n : 0;
}

__global__ void __launch_bounds__(OB_THREADS) k_cut_sizes(CutDev d) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t n_items = items_now(d.a);
    const uint64_t i = (uint64_t)blockIdx.x * CB_ITEMS + threadIdx.x;
    uint64_t total;
    const uint64_t len = load_citem(d.a, i, n_items, true).len;
    const uint64_t ex = block_exclusive_scan(len, wsum, &total);
    if (i < n_items) d.ioff[i] = ex, d.ilen[i] = len < 0xFFFFFFFFull ? (uint32_t)len : 0xFFFFFFFFu;
    if (threadIdx.x == 0) d.tblk[blockIdx.x] = total;
}

// total[0]: the bytes (0 where they do not fit: NH_ERR_CUT_CAP); tblk[n_tblk]: the bytes there are
__global__ void __launch_bounds__(OB_THREADS) k_cut_scan(CutDev d) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t total = scan_block_sums(d.tblk, d.n_tblk, wsum);
    if (threadIdx.x == 0) {
        d.a.total[0] = total_fits(total, d.a.cap, d.a.error, NH_ERR_CUT_CAP) ? total : 0;
        d.tblk[d.n_tblk] = total;
    }
}

constexpr unsigned CUT_MAX_BLOCKS = 1u << 13;

// pair t = item t / rows, span t % rows: the waves take the pairs in turn
__global__ void __launch_bounds__(OB_THREADS) k_cut_write(CutDev d) {
    const CutArgs &a = d.a;
    const uint64_t n_items = items_now(a);
    if (d.tblk[d.n_tblk] > a.cap) return;  // (a text too long: nothing is written)
    const int lane = threadIdx.x & 63;
    const bool fastq = a.fastq != 0;
    const uint64_t n_waves = (uint64_t)gridDim.x * OB_WAVES, n_pairs = n_items * d.rows;
    for (uint64_t t = (uint64_t)blockIdx.x * OB_WAVES + (threadIdx.x >> 6); t < n_pairs; t += n_waves) {  // (wave-uniform)
        const uint64_t i = d.rows == 1 ? t : t / d.rows;
        const uint64_t y = t - i * d.rows;
        if (y != 0 && y * d.span >= (uint64_t)d.ilen[i] + 3) continue;  // (the item ends in front of this span)
        const CItem r = load_citem(a, i, n_items, false);
        if (r.len == 0) continue;
        const uint64_t o = d.tblk[i / CB_ITEMS] + d.ioff[i], end = o + r.len;
        if (end > a.cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0 && y == 0) atomicOr(a.error, NH_ERR_CUT_CAP);
            continue;
        }
        const uint64_t A = (o & ~3ull) + y * d.span;
        if (A >= end) continue;
        const uint64_t stop = A + d.span < end ? A + d.span : end;
        const uint64_t pR = (uint64_t)r.head + r.clen;      // the rest of the header
        const uint64_t pB = (uint64_t)r.hlen + r.clen + 1;  // the bases
        const uint64_t pC = pB + r.slen + 3;                // the qualities
        // wave_write() on the span's dwords: an aligned dword inside the item from one field or four bytes, the item's first and
        // last partial dwords, which it shares with its neighbours, byte by byte
        for (uint64_t D = A + 4ull * lane; D < stop; D += 256) {
            if (D >= o && D + 4 <= end) {
                const uint64_t p = D - o;
                uint32_t v;
                if (p + 4 <= r.head) v = text_dword(a.text, r.h + p);
                else if (p >= pR && p + 4 <= pB - 1) v = text_dword(a.text, r.h + r.head + (p - pR));
                else if (p >= pB && p + 4 <= pB + r.slen) v = text_dword(a.text, r.s + (p - pB));
                else if (fastq && p >= pC && p + 4 <= pC + r.qlen) v = text_dword(a.text, r.q + (p - pC));
                else
                    v = (uint32_t)citem_byte(a, r, p) | (uint32_t)citem_byte(a, r, p + 1) << 8 | (uint32_t)citem_byte(a, r, p + 2) << 16 |
                        (uint32_t)citem_byte(a, r, p + 3) << 24;
                *reinterpret_cast<uint32_t *>(a.out + D) = v;
            } else {
                for (uint64_t x = D; x < D + 4; x++)
                    if (x >= o && x < end) a.out[x] = (char)citem_byte(a, r, x - o);
            }
        }
    }
}

uint32_t cut_span() {  // bytes a wave writes of an item: tuning / test knob, read at every launch
    if (const char *env = getenv("NOHUMAN_CUT_SPAN")) {
        const long v = atol(env);
        if (v > 0 && v < (1l << 30)) return (uint32_t)((v + 255) & ~255l);
    }
    return CUT_SPAN;
}

uint64_t seq_blocks(uint64_t n) { return (n + CI_SEQS - 1) / CI_SEQS; }
uint64_t item_blocks(uint64_t cap_items) { return (cap_items + CB_ITEMS - 1) / CB_ITEMS; }

}  // namespace

uint64_t cut_max_pieces(uint64_t slen, uint32_t min_piece) { return slen < min_piece ? 0 : (slen + CUT_K) / ((uint64_t)min_piece + CUT_K); }

uint64_t cut_scratch_words(uint64_t n, uint64_t cap_items) { return (n + 1) / 2 + seq_blocks(n) + 1 + item_blocks(cap_items) + 1 + cap_items + (cap_items + 1) / 2; }

hipError_t launch_cut(const CutArgs &a, hipStream_t stream) {
    if (a.n == 0) return hipMemsetAsync(a.total, 0, 2 * sizeof(uint64_t), stream);
    CutDev d{};
    d.a = a;
    d.n_iblk = seq_blocks(a.n), d.n_tblk = item_blocks(a.cap_items);
    d.cnt = (uint32_t *)a.scratch;
    d.iblk = a.scratch + (a.n + 1) / 2;
    d.tblk = d.iblk + d.n_iblk + 1;
    d.ioff = d.tblk + d.n_tblk + 1;
    // the spans of the longest item there can be
    d.span = cut_span();
    d.ilen = (uint32_t *)(d.ioff + a.cap_items);
    d.rows = (uint32_t)std::min<uint64_t>((a.max_item + 3) / d.span + 1, 1u << 20);  // (an item of a batch is below 4 GB)
    hipLaunchKernelGGL(k_cut_item_sizes, dim3((unsigned)d.n_iblk), dim3(OB_THREADS), 0, stream, d);
    hipLaunchKernelGGL(k_cut_item_scan, dim3(1), dim3(OB_THREADS), 0, stream, d);
    hipLaunchKernelGGL(k_cut_item_write, dim3((unsigned)d.n_iblk), dim3(OB_THREADS), 0, stream, d);
    if (d.n_tblk == 0) return hipMemsetAsync(a.total, 0, sizeof(uint64_t), stream);
    hipLaunchKernelGGL(k_cut_sizes, dim3((unsigned)d.n_tblk), dim3(OB_THREADS), 0, stream, d);
    hipLaunchKernelGGL(k_cut_scan, dim3(1), dim3(OB_THREADS), 0, stream, d);
    const uint64_t want = (a.cap_items * d.rows + OB_WAVES - 1) / OB_WAVES;
    hipLaunchKernelGGL(k_cut_write, dim3((unsigned)std::min<uint64_t>(want, CUT_MAX_BLOCKS)), dim3(OB_THREADS), 0, stream, d);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_host_cut_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_records, const void *d_seq_starts,
                                  const void *d_seq_lens, const void *d_idlen, const void *d_results, uint64_t n, int fastq, const void *d_cover,
                                  uint32_t min_piece, void *d_out, uint64_t cap, void *d_total, void *d_counts, void *error_bits, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_text || !d_cover || !d_total || !error_bits || (cap && !d_out) || (n && (!d_records || !d_seq_starts || !d_seq_lens || !d_idlen || !d_results)))
        return nh::set_error(NH_EINVAL, "nh_host_cut_device: null argument");
    if (((uintptr_t)d_text & 3) || ((uintptr_t)d_cover & 3) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_records & 15) || ((uintptr_t)error_bits & 3) ||
        ((uintptr_t)d_total & 7) || ((uintptr_t)d_counts & 7))
        return nh::set_error(NH_EINVAL, "nh_host_cut_device: the text, the bitmap, the output and the error word must be 4-byte aligned, the total and "
                                        "the counts 8-byte aligned, the record table 16-byte aligned");
    if (min_piece == 0 || min_piece > 0x7FFFFFFFu) return nh::set_error(NH_EINVAL, "nh_host_cut_device: min_piece %u is not in 1..2^31-1", min_piece);
    if (n >= (1ull << 32) || text_len >= (1ull << 32)) return nh::set_error(NH_EINVAL, "nh_host_cut_device: too many sequences or too much text for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    // ANY bitmap (the caller's may be forged: covered runs of one base): a covered base lies between two pieces, so sequences that
    // do not overlap hold at most (text_len + n) / (min_piece + 1) of them; a table that forges more meets the capacity, not the
    // end of a buffer
    const uint64_t cap_items = n + (text_len + n) / ((uint64_t)min_piece + 1) + 1;
    nh::DevBuf<uint64_t> scratch;
    nh::DevBuf<uint32_t> items;
    if (n && (scratch.reserve(nh::cut_scratch_words(n, cap_items)) != hipSuccess || items.reserve(3 * cap_items) != hipSuccess)) {
        (void)hipGetLastError();
        return nh::set_error(NH_EOOM, "nh_host_cut_device: cannot allocate the scratch and %llu items", (unsigned long long)cap_items);
    }
    nh::CutArgs a{};
    a.text = (const char *)d_text, a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts, a.seq_len = (const uint32_t *)d_seq_lens, a.rec = (const uint32_t *)d_records;
    a.idlen = (const uint32_t *)d_idlen, a.res = (const nh_result *)d_results, a.n = n, a.fastq = fastq != 0;
    a.cover = (const uint32_t *)d_cover, a.min_piece = min_piece;
    a.items = items, a.cap_items = cap_items, a.out = (char *)d_out, a.cap = cap, a.scratch = scratch;
    a.max_item = 2 * text_len + 64;  // (an item is a header and slices of two lines of the text: the entry does not know the longest)
    nh::DevBuf<uint64_t> totals;  // {bytes, items}: the caller takes the bytes
    if (totals.reserve(2) != hipSuccess) return nh::set_error(NH_EOOM, "nh_host_cut_device: cannot allocate the totals");
    a.total = totals, a.counts = (unsigned long long *)d_counts, a.error = (int *)error_bits;
    hipError_t he = nh::launch_cut(a, (hipStream_t)stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_total, totals, sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);  // (the scratch is the launches' until they are done)
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "host cut, builder launch: %s", hipGetErrorString(he));
    return NH_OK;
}
