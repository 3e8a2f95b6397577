// nh_split.hip -- the classified-out text of a batch, built in HBM (nh_run_split: the human reads of a split run).
//
// For every fragment whose call is not 0, in input order and contiguous, each mate's output receives exactly what
// nh_run's put_record() writes for a classified record under --classified-out (kraken2 classify.cc):
//   FASTQ: header, " kraken:taxid|<external id>", "\n", sequence, "\n+\n", qualities, "\n"
//   FASTA: header, " kraken:taxid|<external id>", "\n", sequence, "\n"
// The record is made from its parsed fields (header without trailing blanks, the sequence joined in place), never from
// its raw text, so CRLF and "+id" records come out normalised by the same rule as on the host.
//
// Three launches on the batch's stream, both mates in each (grid.y = mate); the scheme and its parts are nh_outbuild.h's:
//   k_hout_sizes  per block of HB_FRAGS fragments: the sum of their output lengths
//   k_hout_scan   per mate, one workgroup: block sums -> block offsets; the mate's total
//   k_hout_copy   per block: the records' offsets, then one wave per record writes it; the fields that are copied as
//                 dwords are the header, the sequence and the qualities
// Every load stays inside the dwords that hold bytes of [0, ntext); every store inside [0, cap) of its mate's buffer.
// A record whose fields lie outside the text, a call outside the taxon table or a total above the buffer sets bit 4 of
// the engine's error word and writes nothing.
//
// Per-taxon outputs (nh_run_taxa; k_tout_*, below k_hout_*): the same records sorted into up to NH_MAX_TAXON_OUTS bins in one
// pass.  bin_of[call] (a byte a taxonomy node, 0xFF: none) names the bin of a classified fragment; every bin is a region of
// its mate's ONE buffer, bin k starting at the 256-byte-aligned end of bin k - 1, records in input order inside it:
//   k_tout_sizes  per block and bin: the sum of the output lengths -> blk[(m * K + k) * nblk + block]
//   k_tout_scan   per mate, one workgroup: scan_block_sums() per bin; start[m][k], total[m][k]
//   k_tout_copy   per block: the records' offsets inside their bins -- K masked passes of block_offsets() into the one
//                 s_off[], a fragment being in exactly one bin -- then one wave per record writes it as k_hout_copy does
// The error bit of these three is 64; the rules are k_hout_*'s, and a bin index >= K (other than 0xFF) is an error too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_internal.h"
#include "nh_outbuild.h"

namespace nh {

namespace {

constexpr int HB_PER_THREAD = 4;
constexpr int HB_FRAGS = OB_THREADS * HB_PER_THREAD;  // fragments of one block
constexpr int ERR_HUMAN_OUT = 4;
constexpr int ERR_TAXON_OUT = 64;
constexpr uint32_t NO_BIN = 0xFF;  // bin_of: the node is in no selector's clade
constexpr uint32_t SFX_FIXED = 14;  // " kraken:taxid|"

__device__ __constant__ char kSfx[SFX_FIXED + 1] = " kraken:taxid|";

struct Rec {  // one record's fields, absolute offsets into the batch's text
    uint64_t h, s, q;
    uint32_t hlen, slen, qlen;
    uint64_t ext;
    uint32_t ndig;  // decimal digits of ext
    uint64_t len;   // bytes of its output, 0: not written
};

// the record of fragment f, mate m; len 0 for an unclassified fragment or a record that fails its bounds (error set)
__device__ inline Rec load_rec(const HumanOutArgs &a, uint64_t f, int m, bool report, int bit = ERR_HUMAN_OUT) {
    Rec r{};
    if (f >= a.n) return r;
    const uint32_t call = a.res[f].call;
    if (call == 0) return r;
    const uint64_t i = f * (uint64_t)a.mates + (uint64_t)m;
    const uint4 fr = reinterpret_cast<const uint4 *>(a.rec)[i];
    r.h = fr.x;
    r.hlen = fr.y;
    r.q = fr.z;
    r.qlen = a.fastq[m] ? fr.w : 0;
    r.s = a.seq_off[i];
    r.slen = a.seq_len[i];
    const bool ok = call < a.n_ext && r.h + r.hlen <= a.ntext && (r.slen == 0 || r.s + r.slen <= a.ntext) &&
                    (r.qlen == 0 || r.q + r.qlen <= a.ntext);
    if (!ok) {
        if (report) atomicOr(a.error, bit);
        return r;
    }
    r.ext = a.ext[call];
    r.ndig = decimal_digits(r.ext);
    r.len = (uint64_t)r.hlen + SFX_FIXED + r.ndig + 1 + r.slen + 1 + (a.fastq[m] ? 3ull + r.qlen : 0ull);
    return r;
}

__global__ void __launch_bounds__(OB_THREADS) k_hout_sizes(HumanOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.y;
    const uint64_t f0 = (uint64_t)blockIdx.x * HB_FRAGS + (uint64_t)threadIdx.x * HB_PER_THREAD;
    uint64_t mine = 0;
    for (int j = 0; j < HB_PER_THREAD; j++) mine += load_rec(a, f0 + j, m, true).len;
    uint64_t total;
    (void)block_exclusive_scan(mine, wsum, &total);
    if (threadIdx.x == 0) a.blk[(uint64_t)m * a.nblk + blockIdx.x] = total;
}

// one workgroup per mate: block sums -> exclusive block offsets (in place), the mate's total
__global__ void __launch_bounds__(OB_THREADS) k_hout_scan(HumanOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.x;
    const uint64_t total = scan_block_sums(a.blk + (uint64_t)m * a.nblk, a.nblk, wsum);
    if (threadIdx.x == 0) a.total[m] = total_fits(total, a.cap[m], a.error, ERR_HUMAN_OUT) ? total : 0;
}

// byte p of the record's output (0 <= p < r.len)
__device__ inline uint8_t rec_byte(const HumanOutArgs &a, const Rec &r, bool fastq, uint64_t p) {
    if (p < r.hlen) return (uint8_t)a.text[r.h + p];
    p -= r.hlen;
    if (p < SFX_FIXED) return (uint8_t)kSfx[p];
    p -= SFX_FIXED;
    if (p < r.ndig) {
        uint64_t v = r.ext;
        for (uint32_t k = r.ndig - 1 - (uint32_t)p; k; k--) v /= 10;
        return (uint8_t)('0' + v % 10);
    }
    p -= r.ndig;
    if (p == 0) return '\n';
    p -= 1;
    if (p < r.slen) return (uint8_t)a.text[r.s + p];
    p -= r.slen;
    if (!fastq) return '\n';
    if (p < 3) return p == 1 ? '+' : '\n';
    p -= 3;
    if (p < r.qlen) return (uint8_t)a.text[r.q + p];
    return '\n';
}

__global__ void __launch_bounds__(OB_THREADS) k_hout_copy(HumanOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[HB_FRAGS];
    const int m = blockIdx.y;
    const bool fastq = a.fastq[m] != 0;
    const uint64_t fb = (uint64_t)blockIdx.x * HB_FRAGS;
    block_offsets<HB_PER_THREAD>(s_off, wsum, [&](uint32_t fl) { return load_rec(a, fb + fl, m, false).len; });
    char *out = a.out[m];
    const uint64_t cap = a.cap[m];
    const uint64_t base = a.blk[(uint64_t)m * a.nblk + blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // wave w writes the records of fragments [w * 256, w * 256 + 256) of the block, one after another
    for (int k = 0; k < HB_FRAGS / OB_WAVES; k++) {
        const int fl = wave * (HB_FRAGS / OB_WAVES) + k;
        const Rec r = load_rec(a, fb + fl, m, false);
        if (r.len == 0) continue;
        const uint64_t o = base + s_off[fl];
        if (o + r.len > cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0) atomicOr(a.error, ERR_HUMAN_OUT);
            continue;
        }
        const uint64_t pB = (uint64_t)r.hlen + SFX_FIXED + r.ndig + 1, pC = pB + r.slen + 3;
        wave_write(
            out, o, r.len, lane, [&](uint64_t p) { return rec_byte(a, r, fastq, p); },
            [&](uint64_t p, uint32_t *v) {
                if (p + 4 <= r.hlen) *v = text_dword(a.text, r.h + p);
                else if (p >= pB && p + 4 <= pB + r.slen) *v = text_dword(a.text, r.s + (p - pB));
                else if (fastq && p >= pC && p + 4 <= pC + r.qlen) *v = text_dword(a.text, r.q + (p - pC));
                else return false;
                return true;
            });
    }
}

// ---- per-taxon outputs: the same records, binned

// the record of fragment f, mate m, and its bin; len 0 and NO_BIN for a fragment that is written to no bin
__device__ inline Rec load_bin_rec(const TaxonOutArgs &a, uint64_t f, int m, bool report, uint32_t *bin) {
    *bin = NO_BIN;
    if (f >= a.n) return Rec{};
    const uint32_t call = a.res[f].call;
    if (call == 0) return Rec{};
    uint32_t b = NO_BIN;
    if (call < a.n_ext) {  // (bin_of has n_ext entries; load_rec reports a call outside)
        b = a.bin_of[call];
        if (b == NO_BIN) return Rec{};
        if (b >= (uint32_t)a.K) {
            if (report) atomicOr(a.error, ERR_TAXON_OUT);
            return Rec{};
        }
    }
    const Rec r = load_rec(a, f, m, report, ERR_TAXON_OUT);
    if (r.len) *bin = b;
    return r;
}

__global__ void __launch_bounds__(OB_THREADS) k_tout_sizes(TaxonOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.y;
    const uint64_t f0 = (uint64_t)blockIdx.x * HB_FRAGS + (uint64_t)threadIdx.x * HB_PER_THREAD;
    uint64_t len[HB_PER_THREAD];
    uint32_t bin[HB_PER_THREAD];
    for (int j = 0; j < HB_PER_THREAD; j++) len[j] = load_bin_rec(a, f0 + j, m, true, &bin[j]).len;
    for (int k = 0; k < a.K; k++) {
        uint64_t mine = 0, total;
        for (int j = 0; j < HB_PER_THREAD; j++) mine += bin[j] == (uint32_t)k ? len[j] : 0;
        (void)block_exclusive_scan(mine, wsum, &total);
        if (threadIdx.x == 0) a.blk[((uint64_t)m * a.K + k) * a.nblk + blockIdx.x] = total;
        __syncthreads();  // (wsum is written again by the next bin)
    }
}

// one workgroup per mate: every bin's block sums -> exclusive block offsets (in place); the bins' starts and totals
__global__ void __launch_bounds__(OB_THREADS) k_tout_scan(TaxonOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int m = blockIdx.x;
    uint64_t at = 0;  // (every thread keeps the same running end)
    for (int k = 0; k < a.K; k++) {
        const uint64_t total = scan_block_sums(a.blk + ((uint64_t)m * a.K + k) * a.nblk, a.nblk, wsum);
        at = (at + 255) & ~255ull;
        if (threadIdx.x == 0) {
            a.start[m * a.K + k] = at;
            a.total[m * a.K + k] = total;
        }
        at += total;
    }
    if (threadIdx.x == 0 && !total_fits(at, a.cap[m], a.error, ERR_TAXON_OUT))
        for (int k = 0; k < a.K; k++) a.total[m * a.K + k] = 0;
}

__global__ void __launch_bounds__(OB_THREADS) k_tout_copy(TaxonOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[HB_FRAGS];
    __shared__ uint64_t s_base[NH_MAX_TAXON_OUTS];  // where this block's text begins in each bin
    const int m = blockIdx.y;
    const bool fastq = a.fastq[m] != 0;
    const uint64_t fb = (uint64_t)blockIdx.x * HB_FRAGS;
    // a thread's own records: length and bin, made once; a pass per bin leaves their offsets inside that bin
    uint64_t len[HB_PER_THREAD], off[HB_PER_THREAD];
    uint32_t bin[HB_PER_THREAD];
    for (int j = 0; j < HB_PER_THREAD; j++) {
        len[j] = load_bin_rec(a, fb + threadIdx.x * HB_PER_THREAD + j, m, false, &bin[j]).len;
        off[j] = 0;
    }
    for (int k = 0; k < a.K; k++) {
        block_offsets<HB_PER_THREAD>(s_off, wsum, [&](uint32_t fl) {
            const int j = fl % HB_PER_THREAD;
            return bin[j] == (uint32_t)k ? len[j] : 0;
        });
        for (int j = 0; j < HB_PER_THREAD; j++)  // (entries this thread wrote itself)
            if (bin[j] == (uint32_t)k) off[j] = s_off[threadIdx.x * HB_PER_THREAD + j];
    }
    for (int j = 0; j < HB_PER_THREAD; j++) s_off[threadIdx.x * HB_PER_THREAD + j] = off[j];
    if ((int)threadIdx.x < a.K) s_base[threadIdx.x] = a.start[m * a.K + threadIdx.x] + a.blk[((uint64_t)m * a.K + threadIdx.x) * a.nblk + blockIdx.x];
    __syncthreads();
    char *out = a.out[m];
    const uint64_t cap = a.cap[m];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < HB_FRAGS / OB_WAVES; k++) {
        const int fl = wave * (HB_FRAGS / OB_WAVES) + k;
        uint32_t b;
        const Rec r = load_bin_rec(a, fb + fl, m, false, &b);
        if (r.len == 0) continue;
        const uint64_t o = s_base[b] + s_off[fl];
        if (o + r.len > cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0) atomicOr(a.error, ERR_TAXON_OUT);
            continue;
        }
        const uint64_t pB = (uint64_t)r.hlen + SFX_FIXED + r.ndig + 1, pC = pB + r.slen + 3;
        wave_write(
            out, o, r.len, lane, [&](uint64_t p) { return rec_byte(a, r, fastq, p); },
            [&](uint64_t p, uint32_t *v) {
                if (p + 4 <= r.hlen) *v = text_dword(a.text, r.h + p);
                else if (p >= pB && p + 4 <= pB + r.slen) *v = text_dword(a.text, r.s + (p - pB));
                else if (fastq && p >= pC && p + 4 <= pC + r.qlen) *v = text_dword(a.text, r.q + (p - pC));
                else return false;
                return true;
            });
    }
}

}  // namespace

uint64_t human_out_blocks(uint64_t n) { return (n + HB_FRAGS - 1) / HB_FRAGS; }

hipError_t launch_human_out(const HumanOutArgs &a, hipStream_t stream) {
    if (a.n == 0) return hipMemsetAsync(a.total, 0, 2 * sizeof(uint64_t), stream);
    const dim3 grid((unsigned)a.nblk, (unsigned)a.mates);
    hipLaunchKernelGGL(k_hout_sizes, grid, dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_hout_scan, dim3((unsigned)a.mates), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_hout_copy, grid, dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_taxon_out(const TaxonOutArgs &a, hipStream_t stream) {
    if (a.K < 1 || a.K > NH_MAX_TAXON_OUTS) return hipErrorInvalidValue;
    if (a.n == 0) return hipMemsetAsync(a.total, 0, 2 * (size_t)a.K * sizeof(uint64_t), stream);
    const dim3 grid((unsigned)a.nblk, (unsigned)a.mates);
    hipLaunchKernelGGL(k_tout_sizes, grid, dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_tout_scan, dim3((unsigned)a.mates), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_tout_copy, grid, dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nh
