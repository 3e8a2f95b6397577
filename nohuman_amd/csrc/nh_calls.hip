// nh_calls.hip -- the read lists of a batch, built in HBM (nh_run_ex: the calls table and the human read ids).
//
// Two plain-text outputs, one line per fragment, in input order and contiguous:
//   output 0, the calls table, a line for EVERY fragment:
//     <C|U> \t <id> \t <external taxon id, 0 for U> \t <len>  or  <len1>|<len2> \t <total_kmers> \t <clade_hits> \t <hit_groups> \n
//     columns 1-4 are byte for byte columns 1-4 of nh_run's --output line of the fragment (format_batch, kraken2 classify.cc,
//     SURVEY.md A.6); columns 5-7 are the nh_result record as the classifier left it.  clade_hits / total_kmers is the
//     confidence that --confidence thresholds, so a threshold can be chosen from this table without running again.
//   output 1, the human ids: <id> \n for every fragment whose call is not 0.
// <id> is mate 1's header from the byte behind '@' / '>' for the id length the reader found (RecRef::idlen: up to the first
// space, tab or '\r'); a paired run drops a trailing "/1" or "/2" from an id longer than two bytes (kraken2 TrimPairInfo).
//
// Three launches on the batch's stream, both outputs in each (grid.y = output); the scheme and its parts are nh_outbuild.h's:
//   k_calls_sizes  per block of CB_FRAGS fragments: the sum of their line lengths and the number of lines
//   k_calls_scan   per output, one workgroup: block sums -> block offsets; the output's total bytes and lines
//   k_calls_write  per block: the lines' offsets, then one wave per line writes it; the only field that is copied as dwords
//                  is the id, the numbers are put together byte by byte (decimal digits by division, no printf).  Nothing
//                  is sized by the id's length.
// Every load stays inside the dwords that hold bytes of [0, ntext); every store inside [0, cap) of its output's buffer.  A record whose header lies outside the text, an id longer
// than its header, a call outside the taxon table or a total above the buffer sets bit 16 of the engine's error word and
// writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_internal.h"
#include "nh_outbuild.h"

namespace nh {

namespace {

constexpr int CB_FRAGS = OB_THREADS;  // fragments of one block: one a thread in the scans, 64 a wave in the write
constexpr int ERR_CALLS = 16;
constexpr int N_FIELDS = 6;  // the numbers of a table line: taxid, len1, len2 (paired), total_kmers, clade_hits, hit_groups

struct Line {  // one fragment's lines
    uint64_t id;     // absolute offset of the id in the batch's text
    uint32_t idlen;  // after TrimPairInfo
    uint32_t cls;    // call != 0
    uint64_t v[N_FIELDS];
    uint32_t nd[N_FIELDS];  // decimal digits of v[k]; 0: the field is absent (len2 of a single-end run)
    uint64_t len[2];        // bytes of its line in output 0 / 1, 0: none
};

// the lines of fragment f; both lengths 0 for a fragment that fails its bounds (error set)
__device__ inline Line load_line(const CallsArgs &a, uint64_t f, bool report) {
    Line L{};
    if (f >= a.n) return L;
    const nh_result r = a.res[f];
    const uint64_t i = f * (uint64_t)a.mates;
    uint32_t idl = 0;
    if (!(r.call < a.n_ext && read_id(a.text, a.ntext, a.rec, a.idlen, f, a.mates, &L.id, &idl))) {  // (the id: nh_outbuild.h, shared with nh_cover.hip)
        if (report) atomicOr(a.error, ERR_CALLS);
        L.id = 0;
        return L;
    }
    L.idlen = idl;
    L.cls = r.call != 0;
    L.v[0] = L.cls ? a.ext[r.call] : 0;
    L.v[1] = a.seq_len[i];
    L.v[2] = a.mates == 2 ? a.seq_len[i + 1] : 0;
    L.v[3] = r.total_kmers;
    L.v[4] = r.clade_hits;
    L.v[5] = r.hit_groups;
    uint64_t tail = 0;  // every number with the separator in front of it
#pragma unroll
    for (int k = 0; k < N_FIELDS; k++) {
        L.nd[k] = k == 2 && a.mates != 2 ? 0 : decimal_digits(L.v[k]);
        tail += L.nd[k] ? 1 + L.nd[k] : 0;
    }
    L.len[0] = a.want[0] ? 2ull + idl + tail + 1 : 0;
    L.len[1] = a.want[1] && (a.res_ids ? a.res_ids[f].call != 0 : L.cls != 0) ? (uint64_t)idl + 1 : 0;
    return L;
}

// blk: [o * nblk + b] the bytes of block b in output o, [(2 + o) * nblk + b] its lines
__global__ void __launch_bounds__(OB_THREADS) k_calls_sizes(CallsArgs a) {
    __shared__ uint64_t wsum[OB_WAVES], wcnt[OB_WAVES];
    const int o = blockIdx.y;
    const Line L = load_line(a, (uint64_t)blockIdx.x * CB_FRAGS + threadIdx.x, o == 0);
    const uint64_t len = o ? L.len[1] : L.len[0];
    uint64_t total, lines;
    (void)block_exclusive_scan(len, wsum, &total);
    (void)block_exclusive_scan(len != 0, wcnt, &lines);
    if (threadIdx.x == 0) {
        a.blk[(uint64_t)o * a.nblk + blockIdx.x] = total;
        a.blk[(uint64_t)(2 + o) * a.nblk + blockIdx.x] = lines;
    }
}

// one workgroup per output: block sums -> exclusive block offsets (in place), the output's total bytes and lines
__global__ void __launch_bounds__(OB_THREADS) k_calls_scan(CallsArgs a) {
    __shared__ uint64_t wsum[OB_WAVES], wcnt[OB_WAVES];
    const int o = blockIdx.x;
    const uint64_t total = scan_block_sums(a.blk + (uint64_t)o * a.nblk, a.nblk, wsum);
    const uint64_t *cnt = a.blk + (uint64_t)(2 + o) * a.nblk;
    uint64_t lines = 0;
    for (uint64_t c = 0; c < a.nblk; c += OB_THREADS) {
        const uint64_t i = c + threadIdx.x;
        uint64_t nl;
        (void)block_exclusive_scan(i < a.nblk ? cnt[i] : 0, wcnt, &nl);
        lines += nl;
        __syncthreads();  // (wcnt is written again by the next chunk)
    }
    if (threadIdx.x == 0) {
        const bool fits = total_fits(total, a.cap[o], a.error, ERR_CALLS);
        a.total[o] = fits ? total : 0;
        a.total[2 + o] = fits ? lines : 0;
    }
}

// byte p of the fragment's line in output o (0 <= p < L.len[o])
__device__ inline uint8_t line_byte(const CallsArgs &a, const Line &L, int o, uint64_t p) {
    if (o == 0) {
        if (p < 2) return p == 0 ? (L.cls ? 'C' : 'U') : '\t';
        p -= 2;
    }
    if (p < L.idlen) return (uint8_t)a.text[L.id + p];
    if (o != 0) return '\n';
    p -= L.idlen;
    // the number the byte lies in (or in front of which it is the separator), found without indexing by a variable
    uint64_t v = 0;
    uint32_t nd = 0;
    bool bar = false, found = false;
#pragma unroll
    for (int k = 0; k < N_FIELDS; k++) {
        const uint64_t w = L.nd[k] ? 1ull + L.nd[k] : 0;
        if (!found && p < w) v = L.v[k], nd = L.nd[k], bar = k == 2, found = true;
        if (!found) p -= w;
    }
    if (!found) return '\n';
    if (p == 0) return bar ? '|' : '\t';
    for (uint32_t j = nd - (uint32_t)p; j; j--) v /= 10;
    return (uint8_t)('0' + v % 10);
}

__global__ void __launch_bounds__(OB_THREADS) k_calls_write(CallsArgs a) {
    __shared__ uint64_t wsum[OB_WAVES];
    __shared__ uint64_t s_off[CB_FRAGS];
    const int o = blockIdx.y;
    const uint64_t fb = (uint64_t)blockIdx.x * CB_FRAGS;
    block_offsets<1>(s_off, wsum, [&](uint32_t fl) {
        const Line L = load_line(a, fb + fl, false);
        return o ? L.len[1] : L.len[0];
    });
    char *out = a.out[o];
    const uint64_t cap = a.cap[o];
    const uint64_t base = a.blk[(uint64_t)o * a.nblk + blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // wave w writes the lines of fragments [w * 64, w * 64 + 64) of the block, one after another
    for (int k = 0; k < CB_FRAGS / OB_WAVES; k++) {
        const int fl = wave * (CB_FRAGS / OB_WAVES) + k;
        if (fb + fl >= a.n) break;
        const Line L = load_line(a, fb + fl, false);
        const uint64_t len = o ? L.len[1] : L.len[0];
        if (len == 0) continue;
        const uint64_t at = base + s_off[fl];
        if (at + len > cap) {  // (the scan found the total too large: nothing is written)
            if (lane == 0) atomicOr(a.error, ERR_CALLS);
            continue;
        }
        const uint64_t pI = o ? 0 : 2;  // where the id starts in the line
        wave_write(
            out, at, len, lane, [&](uint64_t p) { return line_byte(a, L, o, p); },
            [&](uint64_t p, uint32_t *v) {
                if (!(p >= pI && p + 4 <= pI + L.idlen)) return false;
                *v = text_dword(a.text, L.id + (p - pI));
                return true;
            });
    }
}

}  // namespace

uint64_t calls_blocks(uint64_t n) { return (n + CB_FRAGS - 1) / CB_FRAGS; }

hipError_t launch_calls(const CallsArgs &a, hipStream_t stream) {
    if (a.n == 0) return hipMemsetAsync(a.total, 0, 4 * sizeof(uint64_t), stream);
    const dim3 grid((unsigned)a.nblk, 2);
    hipLaunchKernelGGL(k_calls_sizes, grid, dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_calls_scan, dim3(2), dim3(OB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_calls_write, grid, dim3(OB_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nh
