// nh_rstats.hip -- read statistics (nh_run_rstats, --read-stats): what `seqkit stats -a` or NanoPlot would be run for on the
// input and on the output of a run, counted in the run itself, where the text, the record table and the calls already lie in HBM.
//
// k_rstats, launched behind the classifier, adds for every sequence i of a batch to one of four accumulators acc[class][mate]
// (nh_read_class: class 1 where the fragment's call is not 0, both mates take the fragment's class; mate i % mates):
//   reads, bases            1 and len_i (a sequence of length 0 is a read)
//   min_len, max_len        atomic minimum / maximum (an empty accumulator holds all-ones / 0)
//   gc, other               bytes in "GCgc"; bytes not in "ACGTacgt"
//   qual_reads, qual_bases  reads and bases of the records that have qualities
//   qhist[94]               bases per Phred value q = byte - 33, the byte read as unsigned, clamped to 0 .. 93
// The bases are the text's: a run with a minimum base quality or a masked run counts the input's bases as well.  Integers only,
// sums and extrema only: the result does not depend on the order of anything and is bit-exact.  tests/rstats_model.py is the
// specification.  Median and N50 need every length: the host keeps a length histogram from what it holds anyway (nh_run.hip) and
// length_summary() below reads them off it; nh_read_stats_write() derives the ratios and prints the table.
//
// Bad records.  A record whose ranges leave the text, or whose quality line is not as long as its sequence (load_qseq,
// nh_qseq.h: the two lengths of the record table, or -- with the bare array of quality starts -- a '\n' among the len_i quality
// bytes or a byte above ' ' behind them) is not counted at all and sets bit 32 of the engine's error word, as in k_qmask.
//
// Mapping: k_qmask's (nh_qmask.hip).  A lane's unit is a 16-byte chunk aligned in the text; a workgroup takes 16 sequences at a
// time: a team of 16 lanes per sequence handles its first 32 chunks (512 bytes), what a sequence has beyond that is done by all
// 256 lanes together, sequence after sequence.  Nothing is stored to the text; what is new is the accumulation:
//   gc / other   four exact byte compares a dword on the case-folded bases (SWAR, no carry between bytes), popcounts kept in the
//                lane, summed over the team (head) or the wave (tail) by shuffles, then one LDS atomic;
//   qhist        in LDS, one copy per wave and accumulator (4 x 4 x 94 words): waves never contend.  A lane walks its chunk's 16
//                bytes and adds a RUN of equal bytes with one atomic (a dword equal to the run's byte four times over is taken at
//                once): Illumina's binned qualities are four values in long runs -- two or three atomics a chunk instead of 16;
//   the rest     one lane per sequence, 64-bit LDS atomics on the workgroup's copy of the four accumulators.
// A workgroup does not flush per 16 sequences -- at 2.5 M pairs that would be millions of global atomics on a few hundred
// addresses.  The grid is capped at the workgroups that are resident at once (the occupancy query: 5 a CU at 90 VGPRs, 1280 on
// 256 CUs; `max_workgroups` overrides it), each workgroup loops over its share of the groups of 16 and adds its non-zero LDS
// totals to HBM once, at its end: at most 408 atomics a workgroup, a few tens in practice.  (Measured, 1 M pairs of 150 bp: 1.21
// ms at 1280 workgroups, 1.24 at 2560, 1.51 at 2048 -- a second, partial round of workgroups -- 1.77 at 768, 4.80 at 256.)  The
// partial histogram words are 32-bit: a launch's text is below 4 GiB.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "nh_internal.h"
#include "nh_qseq.h"

namespace nh {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TEAM = 16;                     // lanes of a sequence's team
constexpr int RS_SEQS = RS_THREADS / RS_TEAM;   // sequences of a group
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_HEAD_STEPS = 2;                // chunks a lane of the team takes
constexpr uint32_t RS_HEAD = RS_TEAM * RS_HEAD_STEPS;  // chunks of a sequence its team handles
constexpr int RS_ACC = 4;                       // accumulators: 2 * class + mate
constexpr int RS_SCALARS = 8;                   // words of nh_read_class in front of qhist
constexpr int RS_WORDS = RS_SCALARS + NH_RS_QBINS;
constexpr int RS_HSTRIDE = 96;                  // words of one LDS histogram
constexpr int RS_WG_PER_CU = 5;                 // workgroups resident on a CU, where the occupancy query does not answer
constexpr int ERR_QMASK = 32;
enum { W_READS, W_BASES, W_MIN, W_MAX, W_GC, W_OTHER, W_QREADS, W_QBASES };

static_assert(sizeof(nh_read_class) == RS_WORDS * 8, "nh_read_class is eight words and the histogram");

// 0x80 in every byte of z that is zero; exact (nothing carries from one byte into the next), so its popcount counts
__device__ inline uint32_t zero_bytes(uint32_t z) { return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu); }

// the bytes lo .. hi - 1 of a chunk's 16 that lie in its dword k: 0x80 in each
__device__ inline uint32_t valid_bytes(uint32_t lo, uint32_t hi, uint32_t k) {
    const uint32_t a = lo > 4 * k ? min(lo - 4 * k, 4u) : 0u, b = hi > 4 * k ? min(hi - 4 * k, 4u) : 0u;
    if (b <= a) return 0;
    const uint32_t upto_b = b >= 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1, upto_a = (1u << (8 * a)) - 1;  // (a < b <= 4)
    return upto_b & ~upto_a & 0x80808080u;
}

// a dword of bases: G or C, and A, C, G or T, in either case, among its valid bytes.  'x' | 0x20 folds the case and maps no
// other byte onto a letter's.
__device__ inline void count_dword(uint32_t b, uint32_t valid, uint32_t *gc, uint32_t *acgt) {
    const uint32_t f = b | 0x20202020u;
    const uint32_t g = zero_bytes(f ^ 0x67676767u), c = zero_bytes(f ^ 0x63636363u);
    const uint32_t at = zero_bytes(f ^ 0x61616161u) | zero_bytes(f ^ 0x74747474u);
    *gc += (uint32_t)__popc((g | c) & valid);
    *acgt += (uint32_t)__popc((g | c | at) & valid);
}

// the bytes lo .. hi - 1 of the chunk b: *gc and *other grow
__device__ inline void count_chunk(const uint4 &b, uint32_t lo, uint32_t hi, uint32_t *gc, uint32_t *other) {
    uint32_t acgt = 0;
    if (lo == 0 && hi == 16) {
        count_dword(b.x, 0x80808080u, gc, &acgt);
        count_dword(b.y, 0x80808080u, gc, &acgt);
        count_dword(b.z, 0x80808080u, gc, &acgt);
        count_dword(b.w, 0x80808080u, gc, &acgt);
    } else {
        count_dword(b.x, valid_bytes(lo, hi, 0), gc, &acgt);
        count_dword(b.y, valid_bytes(lo, hi, 1), gc, &acgt);
        count_dword(b.z, valid_bytes(lo, hi, 2), gc, &acgt);
        count_dword(b.w, valid_bytes(lo, hi, 3), gc, &acgt);
    }
    *other += hi - lo - acgt;
}

__device__ inline uint32_t qbin(uint32_t byte) { return byte < 33 ? 0u : byte > 126 ? (uint32_t)NH_RS_QBINS - 1 : byte - 33; }

// the quality bytes lo .. hi - 1 of the chunk q into the LDS histogram h: one atomic per run of equal bytes
__device__ inline void hist_chunk(uint32_t *h, const uint4 &q, uint32_t lo, uint32_t hi) {
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
    uint32_t cur = 0, cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t w = d[k];
        if (cnt && lo <= 4 * k && hi >= 4 * k + 4 && w == cur * 0x01010101u) {
            cnt += 4;
            continue;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t x = 4 * k + j;
            if (x < lo || x >= hi) continue;
            const uint32_t byte = (w >> (8 * j)) & 0xFFu;
            if (cnt && byte != cur) {
                atomicAdd(&h[qbin(cur)], cnt);
                cnt = 0;
            }
            cur = byte;
            cnt++;
        }
    }
    if (cnt) atomicAdd(&h[qbin(cur)], cnt);
}

// the bytes of sequence r in the text's chunk [D, D + 16): lo .. hi - 1
__device__ inline void chunk_range(const QSeq &r, uint64_t D, uint32_t *lo, uint32_t *hi) {
    const uint64_t end = r.s + r.len;
    *lo = r.s > D ? (uint32_t)(r.s - D) : 0u;
    *hi = end - D >= 16 ? 16u : (uint32_t)(end - D);
}

__global__ void __launch_bounds__(RS_THREADS) k_rstats(RstatsArgs a, uint64_t ngroups) {
    __shared__ QSeq s_seq[RS_SEQS];
    __shared__ int s_bad[RS_SEQS];
    __shared__ int s_slot[RS_SEQS];
    __shared__ unsigned long long s_acc[RS_ACC][RS_SCALARS];
    __shared__ uint32_t s_hist[RS_WAVES][RS_ACC][RS_HSTRIDE];
    __shared__ int s_err;
    const int team = threadIdx.x / RS_TEAM, tl = threadIdx.x % RS_TEAM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool scan = a.rec == nullptr;  // the quality line's length is only known by reading it
    for (int x = threadIdx.x; x < RS_WAVES * RS_ACC * RS_HSTRIDE; x += RS_THREADS) (&s_hist[0][0][0])[x] = 0;
    if (threadIdx.x < RS_ACC * RS_SCALARS) s_acc[threadIdx.x / RS_SCALARS][threadIdx.x % RS_SCALARS] = threadIdx.x % RS_SCALARS == W_MIN ? ~0ull : 0ull;
    if (threadIdx.x == 0) s_err = 0;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {  // (the same trips for every thread of the workgroup)
        __syncthreads();  // the LDS is cleared; the group before is done with s_seq
        const uint64_t i = g * RS_SEQS + team;
        QSeq r = load_qseq(a, i);
        int slot = 0;
        if (i < a.n) slot = (a.res[a.mates == 2 ? i >> 1 : i].call != 0 ? 2 : 0) + (a.mates == 2 ? (int)(i & 1) : 0);
        const uint64_t D0 = r.s & ~3ull;
        // head: the team's chunks into registers; nothing is counted before the whole quality line has been seen
        uint4 hb[RS_HEAD_STEPS] = {}, hq[RS_HEAD_STEPS] = {};
        bool nl = false;
        for (int j = 0; j < RS_HEAD_STEPS; j++) {
            const uint32_t c = (uint32_t)(tl + RS_TEAM * j);
            if (c >= r.nch) continue;
            hb[j] = base_chunk(a, r, D0 + 16ull * c);
            if (r.q != NO_QUAL) {
                hq[j] = qual_chunk(a, r, D0 + 16ull * c);
                nl = nl || has_newline(hq[j]);
            }
        }
        const unsigned long long votes = __ballot(scan && nl);
        if ((votes >> (lane & ~(RS_TEAM - 1))) & ((1ull << RS_TEAM) - 1)) r.bad = true;
        if (tl == 0) {
            s_seq[team] = r;
            s_bad[team] = r.bad ? 1 : 0;
            s_slot[team] = slot;
        }
        __syncthreads();
        // tail, first pass (quality starts alone): a '\n' among the rest of a long sequence's qualities
        if (scan)
            for (int t = 0; t < RS_SEQS; t++) {
                const QSeq &x = s_seq[t];
                if (x.bad || x.nch <= RS_HEAD || x.q == NO_QUAL) continue;  // (the same for every thread of the workgroup)
                const uint64_t X0 = x.s & ~3ull;
                bool f = false;
                for (uint32_t c = RS_HEAD + threadIdx.x; c < x.nch; c += RS_THREADS) f = f || has_newline(qual_chunk(a, x, X0 + 16ull * c));
                if (__syncthreads_or(f ? 1 : 0) && threadIdx.x == 0) s_bad[t] = 1;
            }
        __syncthreads();
        const bool count = i < a.n && s_bad[team] == 0;
        uint32_t gc = 0, other = 0;
        if (count)
            for (int j = 0; j < RS_HEAD_STEPS; j++) {
                const uint32_t c = (uint32_t)(tl + RS_TEAM * j);
                if (c >= r.nch) continue;
                uint32_t lo, hi;
                chunk_range(r, D0 + 16ull * c, &lo, &hi);
                count_chunk(hb[j], lo, hi, &gc, &other);
                if (r.q != NO_QUAL) hist_chunk(s_hist[wave][slot], hq[j], lo, hi);
            }
        uint32_t both = gc | other << 16;  // (a team's head is 512 bytes + 3 at most)
        for (int d = RS_TEAM / 2; d > 0; d >>= 1) both += __shfl_xor(both, d, RS_TEAM);
        if (count && tl == 0) {
            unsigned long long *w = s_acc[slot];
            atomicAdd(&w[W_READS], 1ull);
            atomicMin(&w[W_MIN], (unsigned long long)r.len);
            atomicMax(&w[W_MAX], (unsigned long long)r.len);
            if (r.len) atomicAdd(&w[W_BASES], (unsigned long long)r.len);
            if (both & 0xFFFFu) atomicAdd(&w[W_GC], (unsigned long long)(both & 0xFFFFu));
            if (both >> 16) atomicAdd(&w[W_OTHER], (unsigned long long)(both >> 16));
            if (r.q != NO_QUAL) {
                atomicAdd(&w[W_QREADS], 1ull);
                if (r.len) atomicAdd(&w[W_QBASES], (unsigned long long)r.len);
            }
        }
        // tail: the workgroup together over what each of its sequences has beyond the head
        bool any_bad = false;
        for (int t = 0; t < RS_SEQS; t++) {
            if (s_bad[t]) {
                any_bad = true;
                continue;
            }
            const QSeq &x = s_seq[t];
            if (x.nch <= RS_HEAD) continue;
            const uint64_t X0 = x.s & ~3ull;
            const int xs = s_slot[t];
            uint32_t tgc = 0, tother = 0;
            for (uint32_t c = RS_HEAD + threadIdx.x; c < x.nch; c += RS_THREADS) {
                const uint64_t D = X0 + 16ull * c;
                uint32_t lo, hi;
                chunk_range(x, D, &lo, &hi);
                count_chunk(base_chunk(a, x, D), lo, hi, &tgc, &tother);
                if (x.q != NO_QUAL) hist_chunk(s_hist[wave][xs], qual_chunk(a, x, D), lo, hi);
            }
            for (int d = 32; d > 0; d >>= 1) {
                tgc += __shfl_down(tgc, d, 64);
                tother += __shfl_down(tother, d, 64);
            }
            if (lane == 0 && tgc) atomicAdd(&s_acc[xs][W_GC], (unsigned long long)tgc);
            if (lane == 0 && tother) atomicAdd(&s_acc[xs][W_OTHER], (unsigned long long)tother);
        }
        if (any_bad && threadIdx.x == 0) s_err = 1;
    }
    __syncthreads();
    // the workgroup's totals into HBM, once: only the words that hold something
    for (int x = threadIdx.x; x < RS_ACC * RS_WORDS; x += RS_THREADS) {
        const int k = x / RS_WORDS, w = x % RS_WORDS;
        unsigned long long *dst = a.acc + x;
        if (w >= RS_SCALARS) {
            unsigned long long v = 0;
            for (int wv = 0; wv < RS_WAVES; wv++) v += s_hist[wv][k][w - RS_SCALARS];
            if (v) atomicAdd(dst, v);
        } else if (s_acc[k][W_READS]) {
            const unsigned long long v = s_acc[k][w];
            if (w == W_MIN) atomicMin(dst, v);
            else if (w == W_MAX) atomicMax(dst, v);
            else if (v) atomicAdd(dst, v);
        }
    }
    if (threadIdx.x == 0 && s_err) atomicOr(a.error, ERR_QMASK);
}

}  // namespace

// workgroups of k_rstats that a CU holds at once (asked once; the calling thread has selected a device)
static int rstats_wg_per_cu() {
    static const int n = [] {
        int v = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_rstats, RS_THREADS, 0) == hipSuccess && v > 0 ? v : RS_WG_PER_CU;
    }();
    return n;
}

hipError_t launch_rstats(const RstatsArgs &a, int n_cu, uint32_t max_workgroups, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    const uint64_t ngroups = (a.n + RS_SEQS - 1) / RS_SEQS;
    const uint64_t cap = max_workgroups ? max_workgroups : (uint64_t)std::max(1, n_cu) * rstats_wg_per_cu();
    const uint64_t blocks = std::min(ngroups, std::min<uint64_t>(cap, 0x7FFFFFFFull));
    hipLaunchKernelGGL(k_rstats, dim3((unsigned)blocks), dim3(RS_THREADS), 0, stream, a, ngroups);
    return hipGetLastError();
}

void length_summary(const std::vector<std::pair<uint64_t, uint64_t>> &lens, uint64_t *median, uint64_t *n50) {
    uint64_t reads = 0, bases = 0;
    for (const auto &p : lens) reads += p.second, bases += p.first * p.second;
    *median = *n50 = 0;
    if (!reads) return;
    // the lower nearest-rank median: the element of 0-based index ceil(n / 2) - 1 of the ascending lengths
    const uint64_t idx = (reads + 1) / 2 - 1;
    uint64_t seen = 0;
    for (const auto &p : lens) {
        seen += p.second;
        if (seen > idx) {
            *median = p.first;
            break;
        }
    }
    // N50: the largest L such that the reads of length >= L hold at least half of the bases
    uint64_t acc = 0;
    for (size_t i = lens.size(); i-- > 0;) {
        if (!lens[i].second) continue;
        acc += lens[i].first * lens[i].second;
        if (2 * acc >= bases) {
            *n50 = lens[i].first;
            break;
        }
    }
}

}  // namespace nh

extern "C" int nh_read_stats_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_seq_starts,
                                    const void *d_seq_lens, const void *d_qual_starts, const void *d_results, uint64_t n_frag,
                                    uint32_t flags, void *d_acc, uint32_t max_workgroups, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_text || !d_seq_starts || !d_seq_lens || !d_qual_starts || !d_results || !d_acc) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_text & 3) || ((uintptr_t)d_acc & 7)) return nh::set_error(NH_EINVAL, "the text must be 4-byte aligned, the accumulators 8-byte aligned");
    if (text_len >= (1ull << 32)) return nh::set_error(NH_EINVAL, "read statistics: one launch takes less than 4 GiB of text");
    if (n_frag > (1ull << 33)) return nh::set_error(NH_EINVAL, "too many sequences for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::RstatsArgs a{};
    a.text = (const char *)d_text;
    a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts;
    a.seq_len = (const uint32_t *)d_seq_lens;
    a.qual_off = (const uint64_t *)d_qual_starts;
    a.mates = flags & NH_FLAG_PAIRED ? 2 : 1;
    a.n = n_frag * (uint64_t)a.mates;
    a.res = (const nh_result *)d_results;
    a.acc = (unsigned long long *)d_acc;
    a.error = e->d_error + nh::LAUNCH_SLOTS;
    const hipError_t he = nh::launch_rstats(a, e->n_cu, max_workgroups, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "read statistics launch: %s", hipGetErrorString(he));
    return NH_OK;
}

// ---- the table (host only) ----------------------------------------------------------------------------------------------------
namespace {

// a ratio of two of the integers: "NA" where the denominator is 0
void print_ratio(FILE *f, double num, uint64_t den) {
    if (!den) fputs("\tNA", f);
    else fprintf(f, "\t%.2f", num / (double)den);
}

void print_row(FILE *f, const char *set, int mate, const nh_read_class &c, uint64_t median, uint64_t n50) {
    fprintf(f, "%s\t%d\t%llu\t%llu\t%llu", set, mate + 1, (unsigned long long)c.reads, (unsigned long long)c.bases,
            (unsigned long long)(c.reads ? c.min_len : 0));
    print_ratio(f, (double)c.bases, c.reads);
    fprintf(f, "\t%llu\t%llu\t%llu", (unsigned long long)median, (unsigned long long)(c.reads ? c.max_len : 0), (unsigned long long)n50);
    print_ratio(f, 100.0 * (double)c.gc, c.bases);
    fprintf(f, "\t%llu", (unsigned long long)c.other);
    uint64_t q20 = 0, q30 = 0;
    double err = 0;
    for (int q = 0; q < NH_RS_QBINS; q++) {
        if (q >= 20) q20 += c.qhist[q];
        if (q >= 30) q30 += c.qhist[q];
        err += (double)c.qhist[q] * pow(10.0, -(double)q / 10.0);
    }
    print_ratio(f, 100.0 * (double)q20, c.qual_bases);
    print_ratio(f, 100.0 * (double)q30, c.qual_bases);
    if (!c.qual_bases) fputs("\tNA", f);
    else fprintf(f, "\t%.2f", -10.0 * log10(err / (double)c.qual_bases));
    fputc('\n', f);
}

}  // namespace

extern "C" int nh_read_stats_write(const nh_read_stats *st, const char *path) {
    if (!st || !path || !path[0]) return nh::set_error(NH_EINVAL, "nh_read_stats_write: null argument");
    if (st->mates != 1 && st->mates != 2) return nh::set_error(NH_EINVAL, "nh_read_stats_write: mates is %d, not 1 or 2", st->mates);
    FILE *f = fopen(path, "w");
    if (!f) return nh::set_error(NH_EIO, "cannot create %s: %s", path, strerror(errno));
    fputs("set\tmate\treads\tbases\tmin_len\tmean_len\tmedian_len\tmax_len\tN50\tgc_pct\tother_bases\tq20_pct\tq30_pct\tmean_qual\n", f);
    static const char *const names[3] = {"input", "nonhuman", "human"};
    for (int set = 0; set < 3; set++)
        for (int m = 0; m < st->mates; m++) {
            nh_read_class c;
            if (set) {
                c = st->cls[set - 1][m];
            } else {  // the input: the two classes together
                const nh_read_class &u = st->cls[0][m], &h = st->cls[1][m];
                memset(&c, 0, sizeof c);
                c.reads = u.reads + h.reads, c.bases = u.bases + h.bases, c.gc = u.gc + h.gc, c.other = u.other + h.other;
                c.qual_reads = u.qual_reads + h.qual_reads, c.qual_bases = u.qual_bases + h.qual_bases;
                for (int q = 0; q < NH_RS_QBINS; q++) c.qhist[q] = u.qhist[q] + h.qhist[q];
                c.min_len = !u.reads ? h.min_len : !h.reads ? u.min_len : std::min(u.min_len, h.min_len);
                c.max_len = std::max(u.reads ? u.max_len : 0, h.reads ? h.max_len : 0);
            }
            print_row(f, names[set], m, c, st->median_len[set][m], st->n50[set][m]);
        }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return nh::set_error(NH_EIO, "cannot write %s", path);
    return NH_OK;
}
