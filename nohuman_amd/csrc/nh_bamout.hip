// nh_bamout.hip -- BAM output (NH_CODEC_BAM): the records of a batch's BAM bytes in HBM, selected by their call and compacted (gfx950).
//
// The fifth builder on nh_outbuild.h.  A piece is a whole record as it lies in the input: its block_size field and the block_size
// bytes behind it, copied byte for byte -- tags, CIGAR, flags untouched.  Output o receives, in table order and contiguous, the
// records whose host-ness (call != 0) is want[o]; a split run's two outputs are made in one pass.  tests/bamout_model.py is the
// specification; DESIGN.md 6.17.  The records of a paired BAM (BamOutArgs::pairs; tests/bam_pair_model.py) are
// selected by their pair's call and written in file order: the work item is still a record, only where its offset and its result
// come from changes -- table[i] of the reader's pair table and res[i >> 1] -- and a record whose mate lies outside the BAM bytes
// has no bytes either.
//
// Three launches on the batch's stream, the scheme of nh_outbuild.h:
//   k_bout_sizes  per block of BO_RECS records and per output: the sum of 4 + block_size over the records that go there
//   k_bout_scan   per output, one workgroup: block sums -> block offsets; the output's total, 0 where it is above the buffer
//   k_bout_copy   per block and output: the records' offsets inside the block's bytes (block_offsets() into s_off[]), then the copy
// The copy's work item is a record or -- a long one: an ONT record with ML / mv tags runs to hundreds of kilobytes -- a span of at
// most `span` bytes of it, as in k_bam_fastq, and the items are found the same way, without a second table: the block's bytes are
// cut into slots of `span` bytes, a wave owns the items whose first byte lies in its slot -- the records that begin there (lower
// bound in s_off[], which ascends) and at most one later span of the record that reaches into the slot from before.  A record's
// length is the difference of two neighbours in s_off[].  The slots of a block are dealt to gridDim.y workgroups of four waves
// each (every one makes s_off[] again: a thousand loads), so a block of long records is the work of hundreds of waves and a block
// of 150-base records costs one binary search a slot.  Each item is written with wave_write(): aligned dwords of the output, 4
// bytes a lane; every dword comes from text_dword() (two aligned loads and v_alignbyte), the partial first and last dwords of an
// item are byte stores.
// Bounds: a record's length is only ever made by rec_len(), which reads block_size from the BAM bytes on the device and gives 0
// (and the error bit) unless the field and [off, off + 4 + block_size) lie inside [0, bam_len); the copy writes a record only if
// [o, o + len) lies inside its buffer.  Every load stays inside the dwords that hold bytes of [0, bam_len).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "nh_bam.h"
#include "nh_internal.h"
#include "nh_outbuild.h"

namespace nh {

namespace {

constexpr int BO_PER_THREAD = 4;
constexpr int BO_RECS = OB_THREADS * BO_PER_THREAD;  // records of one block
constexpr uint32_t BO_SPAN_DEFAULT = 16384;          // k_bam_fastq's (tools/bam_output_bench.py, profiles/bam_output.txt)
constexpr uint32_t BO_SPAN_MIN = 16, BO_SPAN_MAX = 1u << 24;
constexpr unsigned BO_MAX_Y = 64;  // workgroups that share one block's slots

// where record i lies in the BAM bytes: the reader's table, two words a record (the first is used) -- pairs: one word a record,
// the two of a pair side by side in file order
__device__ __forceinline__ uint64_t rec_off(const BamOutArgs &a, uint64_t i) { return a.table[a.pairs ? i : 2 * i]; }

// bytes of the record at `off` (4 + block_size), 0 (and the error bit, where `report`) for one outside the BAM bytes
__device__ __forceinline__ uint64_t len_at(const BamOutArgs &a, uint64_t off, bool report) {
    if (a.bam_len < 4 || off > a.bam_len - 4) {
        if (report) atomicOr(a.error, a.err_fields);
        return 0;
    }
    const uint32_t block_size = text_dword((const char *)a.bam, off);
    if (block_size > a.bam_len - 4 - off) {
        if (report) atomicOr(a.error, a.err_fields);
        return 0;
    }
    return 4ull + block_size;
}

// bytes of record i in the outputs, 0 for one outside the BAM bytes -- pairs: and for one whose mate is; *host: whether its
// call (pairs: its pair's) is not 0
__device__ __forceinline__ uint64_t rec_len(const BamOutArgs &a, uint64_t i, bool report, bool *host) {
    *host = false;
    if (i >= a.n) return 0;
    *host = a.res[a.pairs ? i >> 1 : i].call != 0;
    const uint64_t len = len_at(a, rec_off(a, i), report);
    if (a.pairs && len_at(a, rec_off(a, i ^ 1), false) == 0) return 0;  // (n is even: the mate is a record of the table)
    return len;
}

// ... of record i in output o: 0 as well for a record that does not go there
__device__ __forceinline__ uint64_t rec_len_in(const BamOutArgs &a, uint64_t i, int o) {
    bool host;
    const uint64_t len = rec_len(a, i, false, &host);
    return host == (a.want[o] != 0) ? len : 0;
}

__global__ void __launch_bounds__(OB_THREADS) k_bout_sizes(BamOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const uint64_t i0 = (uint64_t)blockIdx.x * BO_RECS + (uint64_t)threadIdx.x * BO_PER_THREAD;
    uint64_t len[BO_PER_THREAD];
    bool host[BO_PER_THREAD];
    for (int j = 0; j < BO_PER_THREAD; j++) len[j] = rec_len(a, i0 + j, true, &host[j]);
    for (int o = 0; o < a.n_out; o++) {
        uint64_t mine = 0, total;
        for (int j = 0; j < BO_PER_THREAD; j++) mine += host[j] == (a.want[o] != 0) ? len[j] : 0;
        (void)block_exclusive_scan(mine, wsum, &total);
        if (threadIdx.x == 0) a.blk[(uint64_t)o * a.nblk + blockIdx.x] = total;
        __syncthreads();  // (wsum is written again by the next output)
    }
}

// one workgroup per output: block sums -> exclusive block offsets (in place), the output's total
__global__ void __launch_bounds__(OB_THREADS) k_bout_scan(BamOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    const int o = blockIdx.x;
    const uint64_t total = scan_block_sums(a.blk + (uint64_t)o * a.nblk, a.nblk, wsum);
    if (threadIdx.x == 0) a.total[o] = total_fits(total, a.cap[o], a.error, a.err_total) ? total : 0;
}

__global__ void __launch_bounds__(OB_THREADS) k_bout_copy(BamOutArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[BO_RECS];
    const int o = blockIdx.z;
    if (a.total[o] == 0) return;  // (nothing goes there, or the scan found the total too large: nothing is written)
    const uint64_t ib = (uint64_t)blockIdx.x * BO_RECS;
    block_offsets<BO_PER_THREAD>(s_off, wsum, [&](uint32_t il) { return rec_len_in(a, ib + il, o); });
    const uint64_t T = s_off[BO_RECS - 1] + rec_len_in(a, ib + BO_RECS - 1, o);  // bytes of this block in the output
    const uint64_t base = a.blk[(uint64_t)o * a.nblk + blockIdx.x];
    const char *bam = (const char *)a.bam;
    char *out = a.out[o];
    const uint64_t cap = a.cap[o], span = a.span;
    const int lane = threadIdx.x & 63;
    for (uint64_t slot = (uint64_t)blockIdx.y * OB_WAVES + (threadIdx.x >> 6); slot * span < T; slot += (uint64_t)gridDim.y * OB_WAVES) {
        const uint64_t lo = slot * span, hi = lo + span;
        // the first record that begins at or behind lo
        uint32_t b = 0, e = BO_RECS;
        while (b < e) {
            const uint32_t m = b + (e - b) / 2;
            if (s_off[m] < lo) b = m + 1;
            else e = m;
        }
        // from the record before -- the span of it that begins in this slot, if it reaches that far -- over the records that begin here
        for (uint32_t i = b ? b - 1 : 0; i < BO_RECS; i++) {
            const uint64_t t = s_off[i];
            uint64_t p0 = 0;
            if (i + 1 == b) p0 = (lo - t + span - 1) / span * span;  // (t < lo: p0 >= span, and lo <= t + p0 < hi)
            else if (t >= hi) break;
            const uint64_t len = (i + 1 < BO_RECS ? s_off[i + 1] : T) - t;
            if (p0 >= len) continue;  // (a record that does not go here has no bytes)
            if (base + t > cap || len > cap - (base + t)) {  // (unreachable behind a scan that fits)
                if (lane == 0) atomicOr(a.error, a.err_total);
                continue;
            }
            const uint64_t src = rec_off(a, ib + i) + p0;  // (len != 0: rec_len() found the record inside the BAM bytes)
            wave_write(
                out, base + t + p0, (p0 + span < len ? p0 + span : len) - p0, lane, [&](uint64_t q) { return (uint8_t)bam[src + q]; },
                [&](uint64_t q, uint32_t *v) {
                    *v = text_dword(bam, src + q);
                    return true;
                });
        }
    }
}

uint32_t bam_out_span(uint32_t span) {
    if (span == 0) {
        span = BO_SPAN_DEFAULT;
        if (const char *env = getenv("NOHUMAN_BAM_SPAN")) {  // tuning / test knob (k_bam_fastq's)
            const long v = atol(env);
            if (v > 0) span = (uint32_t)std::min<long>(v, BO_SPAN_MAX);
        }
    }
    return std::max(BO_SPAN_MIN, std::min(BO_SPAN_MAX, span));
}

}  // namespace

uint64_t bam_out_blocks(uint64_t n) { return (n + BO_RECS - 1) / BO_RECS; }

hipError_t launch_bam_out(const BamOutArgs &a_, hipStream_t stream) {
    if (a_.n_out < 1 || a_.n_out > 2 || (a_.pairs && (a_.n & 1))) return hipErrorInvalidValue;
    if (a_.n == 0) return hipMemsetAsync(a_.total, 0, 2 * sizeof(uint64_t), stream);
    BamOutArgs a = a_;
    a.span = bam_out_span(a.span);
    // the workgroups a block's slots are dealt to: as many as the mean block has rounds of four slots
    const uint64_t slots = (a.bam_len / a.nblk + a.span - 1) / a.span;
    const unsigned Y = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((slots + OB_WAVES - 1) / OB_WAVES, BO_MAX_Y));
    hipLaunchKernelGGL(k_bout_sizes, dim3((unsigned)a.nblk), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_bout_scan, dim3((unsigned)a.n_out), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_bout_copy, dim3((unsigned)a.nblk, Y, (unsigned)a.n_out), dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nh

// nh_bam_select_device (pairs 0: n records) and nh_bam_select_pairs_device (pairs 1: n pairs)
static int bam_select(nh_engine *e_, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n, int pairs, const void *d_results, int want,
                      void *d_out, uint64_t out_cap, uint64_t *d_total, int *error_bits, void *stream) {
    const uint64_t n_records = pairs ? 2 * n : n;
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !error_bits || !d_total) return nh::set_error(NH_EINVAL, "null argument");
    if (n_records && (!d_bam || !d_table || !d_results || (!d_out && out_cap))) return nh::set_error(NH_EINVAL, "null argument");
    if (want != 0 && want != 1) return nh::set_error(NH_EINVAL, "want is %d: 0 selects the records with call == 0, 1 those with call != 0", want);
    if (((uintptr_t)d_bam | (uintptr_t)d_out | (uintptr_t)d_results) & 3)
        return nh::set_error(NH_EINVAL, "the BAM bytes, the results and the output must be 4-byte aligned");
    if (((uintptr_t)d_table | (uintptr_t)d_total) & 7) return nh::set_error(NH_EINVAL, "the table and the total must be 8-byte aligned");
    if (n_records > (1ull << 34) || n > (1ull << 34)) return nh::set_error(NH_EINVAL, "too many records for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::BamOutArgs a{};
    a.pairs = pairs;
    a.bam = (const uint8_t *)d_bam;
    a.bam_len = bam_len;
    a.table = (const uint64_t *)d_table;
    a.n = n_records;
    a.nblk = nh::bam_out_blocks(n_records);
    a.res = (const nh_result *)d_results;
    a.n_out = 1;
    a.want[0] = want;
    a.out[0] = (char *)d_out;
    a.cap[0] = out_cap;
    a.error = error_bits;
    a.err_fields = nh::BAM_ERR_FIELDS;
    a.err_total = nh::BAM_ERR_OUT;
    a.span = 0;
    nh::DevBuf<uint64_t> scratch;  // the block sums, then the two totals
    if (scratch.reserve(a.nblk + 2) != hipSuccess) return nh::set_error(NH_EOOM, "cannot allocate the builder's scratch");
    a.blk = scratch;
    a.total = scratch + a.nblk;
    hipStream_t s = (hipStream_t)stream;
    hipError_t he = nh::launch_bam_out(a, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_total, a.total, sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
    const hipError_t se = hipStreamSynchronize(s);  // (the scratch is this call's)
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "BAM select launch: %s", hipGetErrorString(he));
    return NH_OK;
}

extern "C" int nh_bam_select_device(nh_engine *e, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_records,
                                    const void *d_results, int want, void *d_out, uint64_t out_cap, uint64_t *d_total, int *error_bits,
                                    void *stream) {
    return bam_select(e, d_bam, bam_len, d_table, n_records, 0, d_results, want, d_out, out_cap, d_total, error_bits, stream);
}

extern "C" int nh_bam_select_pairs_device(nh_engine *e, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_pairs,
                                          const void *d_results, int want, void *d_out, uint64_t out_cap, uint64_t *d_total, int *error_bits,
                                          void *stream) {
    return bam_select(e, d_bam, bam_len, d_table, n_pairs, 1, d_results, want, d_out, out_cap, d_total, error_bits, stream);
}
