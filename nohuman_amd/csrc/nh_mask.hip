// nh_mask.hip -- the masked text of a batch, built in HBM (nh_run_mask: every read written, a human read's bases as 'N').
//
// For every fragment, in input order, each mate's output receives the record nh_run's put_record() writes without a suffix:
//   FASTQ: header, "\n", sequence, "\n+\n", qualities, "\n"
//   FASTA: header, "\n", sequence, "\n"
// where the sequence is all 'N' (same length) when the fragment's call is not 0.  For a record already in that form in the
// batch's text, the bytes are the same as the normal keep_human = 0 output (the raw text); for the others (CRLF, "+id",
// trailing blanks, joined FASTA, no final newline) they are made from the parsed fields as the host's put_record() does.
//
// Four launches on the batch's stream, both mates in each (grid.y = mate); the scheme of sizes, scan and write and its
// parts are nh_outbuild.h's, the FAST blocks are this builder's own:
//   k_mask_sizes  per block of MB_FRAGS fragments: the sum of their output lengths, and whether the block is FAST: every
//                 record already in output form in the text (the same test as nh_fastx.h's raw_end, made on the device from
//                 the fields and a few bytes around them) and each record's text starting where the one before ends
//   k_mask_scan   per mate, one workgroup: block sums -> block offsets; the mate's total and (for the trace line) its
//                 number of FAST blocks
//   k_mask_copy   MB_SUB workgroups per block.  FAST block: its text is one contiguous range, copied 16 bytes a lane (aligned
//                 dwordx4 stores; the two partial chunks at the range's ends, shared with the neighbouring blocks, byte by
//                 byte).  Other blocks: the records' offsets, then one wave per record writes it; the fields that are
//                 copied as dwords are the header, the sequence (of a classified fragment: 'N' dwords) and the qualities
//   k_mask_fill   FAST blocks only: 'N' over the sequence ranges of the classified fragments, written as pieces of one field
// Every load stays inside the dwords that hold bytes of [0, ntext); every store inside [0, cap) of its mate's buffer.  A
// record whose fields lie outside the text or a total above the buffer sets bit 8 of the engine's error word and writes nothing.
//
// --host-bases-only (MaskArgs::cover): k_mask_copy and k_mask_fill in their HB form.  A classified fragment's
// sequence is the text's own, with 'N' where the bit of the SOURCE byte is set in the batch's cover bitmap: a sequence dword of
// the output is text_dword() of its source position, whose four bits (not aligned with the output dword; they may lie in two words
// of the bitmap) are expanded to a byte mask that selects 'N'.  The wave that writes a record counts its bits (popcount, one
// reduction and two atomics a wave).  A bitmap load stays inside cover_words(ntext): a bit is read for a byte of the text alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_internal.h"
#include "nh_outbuild.h"

namespace nh {

namespace {

constexpr int MB_PER_THREAD = 4;
constexpr int MB_FRAGS = OB_THREADS * MB_PER_THREAD;  // fragments of one block
constexpr int MB_SUB = 4;  // workgroups of k_mask_copy / k_mask_fill per block
constexpr int ERR_MASK = 8;
constexpr uint32_t NNNN = 0x4E4E4E4Eu;

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

struct MRec {  // one record's fields, absolute offsets into the batch's text
    uint64_t h, s, q;
    uint32_t hlen, slen, qlen;
    bool cls;      // its fragment is classified: the sequence is written as 'N'
    uint64_t len;  // bytes of its output, 0: nothing (no record, or a record that fails its bounds: error set)
};

__device__ inline MRec load_mrec(const MaskArgs &a, uint64_t f, int m, bool report) {
    MRec r{};
    if (f >= a.n) return r;
    const uint64_t i = f * (uint64_t)a.mates + (uint64_t)m;
    const uint4 fr = reinterpret_cast<const uint4 *>(a.rec)[i];
    const bool fastq = a.fastq[m] != 0;
    r.h = fr.x;
    r.hlen = fr.y;
    r.q = fr.z;
    r.qlen = fastq ? fr.w : 0;
    r.s = a.seq_off[i];
    r.slen = a.seq_len[i];
    r.cls = a.res[f].call != 0;
    const bool ok = r.h + r.hlen <= a.ntext && (r.slen == 0 || r.s + r.slen <= a.ntext) && (r.qlen == 0 || r.q + r.qlen <= a.ntext);
    if (!ok) {
        if (report) atomicOr(a.error, ERR_MASK);
        return r;
    }
    r.len = (uint64_t)r.hlen + 1 + r.slen + 1 + (fastq ? 3ull + r.qlen : 0ull);
    return r;
}

// text[r.h, r.h + r.len) is byte for byte the record's output (nh_fastx.h raw_end): "header\nseq\n+\nquals\n" / "header\nseq\n"
__device__ inline bool in_output_form(const MaskArgs &a, const MRec &r, bool fastq) {
    if (r.len == 0 || r.h + r.len > a.ntext) return false;
    const char *t = a.text;
    if (t[r.h + r.hlen] != '\n' || r.s != r.h + r.hlen + 1 || t[r.s + r.slen] != '\n') return false;
    if (!fastq) return true;
    return t[r.s + r.slen + 1] == '+' && t[r.s + r.slen + 2] == '\n' && r.q == r.s + r.slen + 3 && t[r.q + r.qlen] == '\n';
}

__global__ void __launch_bounds__(OB_THREADS) k_mask_sizes(MaskArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.y;
    const bool fastq = a.fastq[m] != 0;
    const uint64_t fb = (uint64_t)blockIdx.x * MB_FRAGS;
    const uint64_t fend = fb + MB_FRAGS < a.n ? fb + MB_FRAGS : a.n;
    const uint64_t f0 = fb + (uint64_t)threadIdx.x * MB_PER_THREAD;
    uint64_t mine = 0;
    bool fast = true;
    for (int j = 0; j < MB_PER_THREAD; j++) {
        const uint64_t f = f0 + j;
        const MRec r = load_mrec(a, f, m, true);
        mine += r.len;
        if (f >= a.n) continue;
        fast = fast && in_output_form(a, r, fastq);
        if (fast && f + 1 < fend)  // the next record of the block starts where this one ends
            fast = reinterpret_cast<const uint4 *>(a.rec)[(f + 1) * (uint64_t)a.mates + (uint64_t)m].x == r.h + r.len;
    }
    uint64_t total;
    (void)block_exclusive_scan(mine, wsum, &total);
    const int all_fast = __syncthreads_and(fast ? 1 : 0);
    if (threadIdx.x == 0) {
        a.blk[(uint64_t)m * a.nblk + blockIdx.x] = total;
        a.fast[(uint64_t)m * a.nblk + blockIdx.x] = all_fast ? 1u : 0u;
    }
}

// one workgroup per mate: block sums -> exclusive block offsets (in place), the mate's total and its number of FAST blocks
__global__ void __launch_bounds__(OB_THREADS) k_mask_scan(MaskArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.x;
    const uint64_t total = scan_block_sums(a.blk + (uint64_t)m * a.nblk, a.nblk, wsum);
    const uint32_t *fast = a.fast + (uint64_t)m * a.nblk;
    uint64_t nfast = 0;
    for (uint64_t c = 0; c < a.nblk; c += OB_THREADS) {
        const uint64_t i = c + threadIdx.x;
        nfast += (uint64_t)__syncthreads_count(i < a.nblk && fast[i] != 0);
    }
    if (threadIdx.x == 0) {
        a.total[m] = total_fits(total, a.cap[m], a.error, ERR_MASK) ? total : 0;
        a.total[2 + m] = nfast;
    }
}

// the cover bit of text byte p (p < ntext)
__device__ __forceinline__ uint32_t cover_bit(const uint32_t *cover, uint64_t p) { return (cover[p >> 5] >> (uint32_t)(p & 31)) & 1u; }

// the cover bits of the text bytes [src, src + 4), bit j: byte src + j (src + 3 < ntext: the second word holds the bit of src + 3)
__device__ __forceinline__ uint32_t cover_bits4(const uint32_t *cover, uint64_t src) {
    const uint64_t wi = src >> 5;
    const uint32_t sh = (uint32_t)(src & 31);
    uint32_t b = cover[wi] >> sh;
    if (sh > 28) b |= cover[wi + 1] << (32 - sh);
    return b & 0xFu;
}

// v with 'N' in the bytes whose bit of m (four bits) is set: bit j of m -> bit 8 j (the four shifted copies share no bit), -> byte j
__device__ __forceinline__ uint32_t select_n(uint32_t v, uint32_t m) {
    const uint32_t bytes = ((m * 0x00204081u) & 0x01010101u) * 0xFFu;
    return (v & ~bytes) | (NNNN & bytes);
}

__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// base p of a classified fragment's sequence as it is written; HB: the lane's count of the bases written as 'N' goes up
template <bool HB>
__device__ __forceinline__ uint8_t masked_base(const MaskArgs &a, const MRec &r, uint64_t p, uint32_t &nmask) {
    if (!HB) return (uint8_t)'N';
    const uint32_t c = cover_bit(a.cover, r.s + p);
    nmask += c;
    return c ? (uint8_t)'N' : (uint8_t)a.text[r.s + p];
}

// ... and the four from p on (p + 4 <= r.slen)
template <bool HB>
__device__ __forceinline__ uint32_t masked_dword(const MaskArgs &a, const MRec &r, uint64_t p, uint32_t &nmask) {
    if (!HB) return NNNN;
    const uint32_t m = cover_bits4(a.cover, r.s + p);
    nmask += (uint32_t)__popc(m);
    return select_n(text_dword(a.text, r.s + p), m);
}

// HB: what the wave's records added -- the sequence bases of its classified fragments, those written as 'N' -- to the run's counters
__device__ __forceinline__ void add_hb_counts(const MaskArgs &a, int lane, uint32_t host_bases, uint32_t nmask) {
    const uint32_t n = wave_total(nmask);  // (a batch's text is below 4 GB: no sum here leaves 32 bits)
    if (lane != 0) return;
    if (host_bases) atomicAdd(a.hb, (unsigned long long)host_bases);
    if (n) atomicAdd(a.hb + 1, (unsigned long long)n);
}

// byte p of the record's masked output (0 <= p < r.len)
template <bool HB>
__device__ inline uint8_t mrec_byte(const MaskArgs &a, const MRec &r, bool fastq, uint64_t p, uint32_t &nmask) {
    if (p < r.hlen) return (uint8_t)a.text[r.h + p];
    p -= r.hlen;
    if (p == 0) return '\n';
    p -= 1;
    if (p < r.slen) return r.cls ? masked_base<HB>(a, r, p, nmask) : (uint8_t)a.text[r.s + p];
    p -= r.slen;
    if (!fastq) return '\n';
    if (p < 3) return p == 1 ? '+' : '\n';
    p -= 3;
    if (p < r.qlen) return (uint8_t)a.text[r.q + p];
    return '\n';
}

// the 16 text bytes at src (src + 15 < ntext): four aligned dwords, a fifth only where the bytes reach into it
__device__ inline uint4 text_x4(const char *text, uint64_t src) {
    const uint64_t A = src & ~3ull;
    const uint32_t sh = (uint32_t)(src & 3);
    const u32x4a4 v = *reinterpret_cast<const u32x4a4 *>(text + A);
    if (sh == 0) return make_uint4(v.x, v.y, v.z, v.w);
    const uint32_t e = *reinterpret_cast<const uint32_t *>(text + A + 16);
    return make_uint4(__builtin_amdgcn_alignbyte(v.y, v.x, sh), __builtin_amdgcn_alignbyte(v.z, v.y, sh),
                      __builtin_amdgcn_alignbyte(v.w, v.z, sh), __builtin_amdgcn_alignbyte(e, v.w, sh));
}

// a FAST block: its records' text is [h0, h0 + L), written at out[base, base + L); false (error set): outside text or buffer
__device__ inline bool fast_range(const MaskArgs &a, int m, uint64_t fb, uint64_t base, uint64_t *h0, uint64_t *L, bool report) {
    const uint64_t last = (fb + MB_FRAGS < a.n ? fb + MB_FRAGS : a.n) - 1;
    const MRec r0 = load_mrec(a, fb, m, false), r1 = load_mrec(a, last, m, false);
    *h0 = r0.h;
    *L = r1.h + r1.len - r0.h;
    const bool ok = r0.len && r1.len && r1.h >= r0.h && r1.h + r1.len <= a.ntext && base + *L <= a.cap[m];
    if (!ok && report) atomicOr(a.error, ERR_MASK);
    return ok;
}

template <bool HB>
__global__ void __launch_bounds__(OB_THREADS) k_mask_copy(MaskArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[MB_FRAGS];
    const int m = blockIdx.y;
    const uint64_t blk = blockIdx.x / MB_SUB;
    const int u = blockIdx.x % MB_SUB;
    const bool fastq = a.fastq[m] != 0;
    const uint64_t fb = blk * MB_FRAGS;
    char *out = a.out[m];
    const uint64_t cap = a.cap[m];
    const uint64_t base = a.blk[(uint64_t)m * a.nblk + blk];
    if (a.fast[(uint64_t)m * a.nblk + blk]) {
        uint64_t h0, L;
        if (!fast_range(a, m, fb, base, &h0, &L, u == 0 && threadIdx.x == 0)) return;
        const uint64_t end = base + L;
        const uint64_t step = 16ull * OB_THREADS * MB_SUB;
        for (uint64_t D = (base & ~15ull) + 16ull * ((uint64_t)u * OB_THREADS + threadIdx.x); D < end; D += step) {
            if (D >= base && D + 16 <= end) {
                *reinterpret_cast<uint4 *>(out + D) = text_x4(a.text, h0 + (D - base));
            } else {  // the range's first or last chunk: the neighbouring blocks own the other bytes
                for (uint64_t x = D; x < D + 16; x++)
                    if (x >= base && x < end) out[x] = a.text[h0 + (x - base)];
            }
        }
        return;
    }
    block_offsets<MB_PER_THREAD>(s_off, wsum, [&](uint32_t fl) { return load_mrec(a, fb + fl, m, false).len; });
    const int lane = threadIdx.x & 63;
    const int gw = u * OB_WAVES + (threadIdx.x >> 6);
    uint32_t host_bases = 0, nmask = 0;  // (HB: the wave's, the lane's)
    // wave gw of the block's MB_SUB * OB_WAVES writes the records gw, gw + MB_SUB * OB_WAVES, ... one after another
    for (int fl = gw; fl < MB_FRAGS; fl += MB_SUB * OB_WAVES) {
        const MRec r = load_mrec(a, fb + fl, m, false);
        if (r.len == 0) continue;
        const uint64_t o = base + s_off[fl];
        if (o + r.len > cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0) atomicOr(a.error, ERR_MASK);
            continue;
        }
        if (HB && r.cls) host_bases += r.slen;
        const uint64_t pB = (uint64_t)r.hlen + 1, pC = pB + r.slen + 3;
        wave_write(
            out, o, r.len, lane, [&](uint64_t p) { return mrec_byte<HB>(a, r, fastq, p, nmask); },
            [&](uint64_t p, uint32_t *v) {
                if (p + 4 <= r.hlen) *v = text_dword(a.text, r.h + p);
                else if (p >= pB && p + 4 <= pB + r.slen) *v = r.cls ? masked_dword<HB>(a, r, p - pB, nmask) : text_dword(a.text, r.s + (p - pB));
                else if (fastq && p >= pC && p + 4 <= pC + r.qlen) *v = text_dword(a.text, r.q + (p - pC));
                else return false;
                return true;
            });
    }
    if (HB) add_hb_counts(a, lane, host_bases, nmask);
}

// FAST blocks: the copy wrote the raw text; 'N' over the sequences of the classified fragments (HB: over their covered bases, the
// others read from the text again)
template <bool HB>
__global__ void __launch_bounds__(OB_THREADS) k_mask_fill(MaskArgs a) {
    const int m = blockIdx.y;
    const uint64_t blk = blockIdx.x / MB_SUB;
    const int u = blockIdx.x % MB_SUB;
    if (!a.fast[(uint64_t)m * a.nblk + blk]) return;
    const uint64_t fb = blk * MB_FRAGS;
    const uint64_t base = a.blk[(uint64_t)m * a.nblk + blk];
    uint64_t h0, L;
    if (!fast_range(a, m, fb, base, &h0, &L, false)) return;  // (the copy reported it and wrote nothing)
    char *out = a.out[m];
    const int lane = threadIdx.x & 63;
    const int gw = u * OB_WAVES + (threadIdx.x >> 6);
    uint32_t host_bases = 0, nmask = 0;  // (HB: the wave's, the lane's)
    for (int fl = gw; fl < MB_FRAGS; fl += MB_SUB * OB_WAVES) {
        const uint64_t f = fb + fl;
        if (f >= a.n || a.res[f].call == 0) continue;
        const MRec r = load_mrec(a, f, m, false);
        if (r.len == 0 || r.slen == 0 || r.h < h0 || r.h + r.len > h0 + L) continue;
        if (HB) host_bases += r.slen;
        // (the sequence's first or last dword: the header's or the separator's bytes stay)
        wave_write(
            out, base + (r.h - h0) + r.hlen + 1, r.slen, lane, [&](uint64_t p) { return masked_base<HB>(a, r, p, nmask); },
            [&](uint64_t p, uint32_t *v) {
                *v = masked_dword<HB>(a, r, p, nmask);
                return true;
            });
    }
    if (HB) add_hb_counts(a, lane, host_bases, nmask);
}

}  // namespace

uint64_t mask_blocks(uint64_t n) { return (n + MB_FRAGS - 1) / MB_FRAGS; }

hipError_t launch_mask(const MaskArgs &a, hipStream_t stream) {
    if (a.n == 0) return hipMemsetAsync(a.total, 0, 4 * sizeof(uint64_t), stream);
    const dim3 grid((unsigned)a.nblk, (unsigned)a.mates), sub((unsigned)(a.nblk * MB_SUB), (unsigned)a.mates);
    hipLaunchKernelGGL(k_mask_sizes, grid, dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_mask_scan, dim3((unsigned)a.mates), dim3(OB_THREADS), 0, stream, a);
    if (a.cover) {
        hipLaunchKernelGGL(k_mask_copy<true>, sub, dim3(OB_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_mask_fill<true>, sub, dim3(OB_THREADS), 0, stream, a);
    } else {
        hipLaunchKernelGGL(k_mask_copy<false>, sub, dim3(OB_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_mask_fill<false>, sub, dim3(OB_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace nh
