// nh_qmask.hip -- kraken2's --minimum-base-quality (classify.cc MaskLowQualityBases) as a pass in front of the classifier.
//
// k_qmask writes, for every sequence i of a batch, the bases of text[s_i, s_i + len_i) into out[s_i, s_i + len_i) -- a second
// buffer with the layout of the batch's text -- with 'N' where the base's quality byte q satisfies q - 33 < Q (Phred+33; the
// byte is read as unsigned).  A sequence without qualities (FASTA) is copied.  Nothing else of `out` is written: the classifier is
// then launched in place on `out` with the same (start, length) arrays and never interprets what surrounds a sequence; the
// builders, writers and encoders keep reading the text, so every output record keeps the input's bases.
//
// Where a sequence's qualities lie comes either from a u64 array of quality starts (nh_quality_mask_device; all-ones: none) or
// from the run's record table {header, header length, qualities, qualities length} (nh_run_minq).  A record whose quality line
// is not as long as its sequence, or whose ranges leave the text, sets bit 32 of the engine's error word and is not written at
// all.  With the record table the two lengths are compared; with the array of starts the quality line is read first: a '\n'
// among the len_i bytes (the line is shorter) or a byte above ' ' behind them (it is longer) is a mismatch.
//
// Mapping.  The kernel moves ~3 bytes per base and computes six integer operations a dword: occupancy is what hides the
// latency, and this kernel -- 52 VGPRs, 0.8 KB of LDS, 256 threads -- runs at the CU's limit of 8 waves a
// SIMD, so the mapping is chosen for lanes that have work.  A lane's unit is a 16-byte chunk of `out` (four aligned dwords: one
// dwordx4 load of bases, one or five dwords of qualities, one dwordx4 store).  A workgroup takes QM_SEQS = 16 sequences:
//   head  a team of 16 lanes per sequence handles its first 32 chunks (512 bytes) in two steps, results kept in registers.  A
//         150-base read is 10 or 11 chunks: 10.5 of a team's 16 lanes work, where a wave per read would use 38 of 64 lanes
//         for one step of dwords and leave 3 of 4 waves of address arithmetic without a byte to move;
//   tail  what a sequence has beyond 512 bytes is done by all 256 lanes of the workgroup together, 4 KB a step, sequence after
//         sequence: a long read is never one wave's serial loop (a 100-kilobase read is 25 steps of the workgroup; the
//         workgroups of the other reads run beside it).
// Chunks are aligned in the output (which has the text's offsets): the bases need no realignment, the qualities -- at another
// residue mod 4 in general -- are realigned with v_alignbyte.  A chunk that is not wholly inside its sequence goes dword by dword;
// a dword that is not wholly inside goes byte by byte (loads of qualities and stores): the neighbouring bytes belong to the
// header, the separator or another sequence.  Every load stays inside dwords that hold bytes of [0, ntext); every store inside
// the sequence ranges.  Masked bases are counted per lane, summed per wave, and added with one atomic a wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_internal.h"
#include "nh_qseq.h"

namespace nh {

namespace {

constexpr int QM_THREADS = 256;
constexpr int QM_TEAM = 16;                     // lanes of a sequence's team
constexpr int QM_SEQS = QM_THREADS / QM_TEAM;   // sequences of a workgroup
constexpr int QM_HEAD_STEPS = 2;                // chunks a lane of the team keeps in registers
constexpr uint32_t QM_HEAD = QM_TEAM * QM_HEAD_STEPS;  // chunks of a sequence its team handles
constexpr int ERR_QMASK = 32;
constexpr uint32_t NNNN = 0x4E4E4E4Eu;

// a byte of q below T (34 .. 126): its bit 7 set in the result.  (q | 0x80) - T borrows from no neighbour; bit 7 of a byte of
// the difference is clear exactly where the low seven bits of q are below T; a byte of 128 or more is no quality below T.
__device__ inline uint32_t below(uint32_t q, uint32_t T4) { return ~((q | 0x80808080u) - T4) & ~q & 0x80808080u; }

__device__ inline uint32_t mask_dword(uint32_t b, uint32_t q, uint32_t T4, uint32_t *cnt) {
    const uint32_t lt = below(q, T4);
    *cnt += (uint32_t)__popc(lt);
    const uint32_t m = (lt >> 7) * 0xFFu;
    return (b & ~m) | (NNNN & m);
}

// the chunk's output dwords (bytes outside the sequence: the text's, never stored); *nl: a '\n' among its qualities
__device__ inline uint4 eval_chunk(const QmaskArgs &a, const QSeq &r, uint64_t D, uint32_t T4, uint32_t *cnt, bool *nl) {
    uint4 b = base_chunk(a, r, D);
    if (r.q == NO_QUAL) return b;
    const uint4 q = qual_chunk(a, r, D);
    *nl = *nl || has_newline(q);
    b.x = mask_dword(b.x, q.x, T4, cnt);
    b.y = mask_dword(b.y, q.y, T4, cnt);
    b.z = mask_dword(b.z, q.z, T4, cnt);
    b.w = mask_dword(b.w, q.w, T4, cnt);
    return b;
}

__device__ inline void store_chunk(const QmaskArgs &a, const QSeq &r, uint64_t D, const uint4 &o) {
    const uint64_t end = r.s + r.len;
    if (D >= r.s && D + 16 <= end) {
        u32x4a4 v;
        v.x = o.x, v.y = o.y, v.z = o.z, v.w = o.w;
        *reinterpret_cast<u32x4a4 *>(a.out + D) = v;
        return;
    }
    const uint32_t d[4] = {o.x, o.y, o.z, o.w};
    for (int k = 0; k < 4; k++) {
        const uint64_t W = D + 4ull * k;
        if (W >= r.s && W + 4 <= end) {
            *reinterpret_cast<uint32_t *>(a.out + W) = d[k];
        } else {  // the sequence's first or last dword: its neighbours own the other bytes
            for (int j = 0; j < 4; j++)
                if (W + j >= r.s && W + j < end) a.out[W + j] = (char)(d[k] >> (8 * j));
        }
    }
}

__global__ void __launch_bounds__(QM_THREADS) k_qmask(QmaskArgs a) {
    __shared__ QSeq s_seq[QM_SEQS];
    __shared__ int s_bad[QM_SEQS];
    const int team = threadIdx.x / QM_TEAM, tl = threadIdx.x % QM_TEAM;
    const int lane = threadIdx.x & 63;
    const uint32_t T4 = a.thresh * 0x01010101u;
    const bool scan = a.rec == nullptr;  // the quality line's length is only known by reading it
    QSeq r = load_qseq(a, (uint64_t)blockIdx.x * QM_SEQS + team);
    const uint64_t D0 = r.s & ~3ull;
    // head: the team's chunks into registers; nothing is stored before the whole quality line has been seen
    uint4 ho[QM_HEAD_STEPS] = {};
    uint32_t hcnt = 0;
    bool nl = false;
    for (int j = 0; j < QM_HEAD_STEPS; j++) {
        const uint32_t c = (uint32_t)(tl + QM_TEAM * j);
        if (c < r.nch) ho[j] = eval_chunk(a, r, D0 + 16ull * c, T4, &hcnt, &nl);
    }
    const unsigned long long votes = __ballot(scan && nl);
    if ((votes >> (lane & ~(QM_TEAM - 1))) & ((1ull << QM_TEAM) - 1)) r.bad = true;
    if (tl == 0) {
        s_seq[team] = r;
        s_bad[team] = r.bad ? 1 : 0;
    }
    __syncthreads();
    // tail, first pass (quality starts alone): a '\n' among the rest of a long sequence's qualities
    if (scan)
        for (int t = 0; t < QM_SEQS; t++) {
            const QSeq &x = s_seq[t];
            if (x.bad || x.nch <= QM_HEAD || x.q == NO_QUAL) continue;  // (the same for every thread of the workgroup)
            const uint64_t X0 = x.s & ~3ull;
            bool f = false;
            for (uint32_t c = QM_HEAD + threadIdx.x; c < x.nch; c += QM_THREADS) f = f || has_newline(qual_chunk(a, x, X0 + 16ull * c));
            if (__syncthreads_or(f ? 1 : 0) && threadIdx.x == 0) s_bad[t] = 1;
        }
    __syncthreads();
    uint32_t cnt = 0;
    const bool bad = s_bad[team] != 0;
    if (!bad) {
        cnt = hcnt;
        for (int j = 0; j < QM_HEAD_STEPS; j++) {
            const uint32_t c = (uint32_t)(tl + QM_TEAM * j);
            if (c < r.nch) store_chunk(a, r, D0 + 16ull * c, ho[j]);
        }
    }
    // tail: the workgroup together over what each of its sequences has beyond the head
    bool any_bad = false;
    for (int t = 0; t < QM_SEQS; t++) {
        const QSeq &x = s_seq[t];
        if (s_bad[t]) {
            any_bad = true;
            continue;
        }
        const uint64_t X0 = x.s & ~3ull;
        bool ignore = false;
        for (uint32_t c = QM_HEAD + threadIdx.x; c < x.nch; c += QM_THREADS) {
            const uint64_t D = X0 + 16ull * c;
            store_chunk(a, x, D, eval_chunk(a, x, D, T4, &cnt, &ignore));
        }
    }
    if (any_bad && threadIdx.x == 0) atomicOr(a.error, ERR_QMASK);
    if (a.masked) {
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if (lane == 0 && cnt) atomicAdd(a.masked, (unsigned long long)cnt);
    }
}

}  // namespace

hipError_t launch_qmask(const QmaskArgs &a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + QM_SEQS - 1) / QM_SEQS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_qmask, dim3((unsigned)blocks), dim3(QM_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_quality_mask_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_seq_starts,
                                      const void *d_seq_lens, const void *d_qual_starts, uint64_t n_seq,
                                      uint32_t min_base_quality, void *d_out, void *d_masked, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (min_base_quality > 93) return nh::set_error(NH_EINVAL, "minimum base quality %u is not in 0..93", min_base_quality);
    if (!e || !d_text || !d_seq_starts || !d_seq_lens || !d_qual_starts || !d_out) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_text | (uintptr_t)d_out) & 3) return nh::set_error(NH_EINVAL, "the text and the output must be 4-byte aligned");
    if (n_seq > (1ull << 34)) return nh::set_error(NH_EINVAL, "too many sequences for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::QmaskArgs a{};
    a.text = (const char *)d_text;
    a.ntext = text_len;
    a.seq_off = (const uint64_t *)d_seq_starts;
    a.seq_len = (const uint32_t *)d_seq_lens;
    a.qual_off = (const uint64_t *)d_qual_starts;
    a.n = n_seq;
    a.mates = 1;
    a.thresh = min_base_quality + 33;
    a.out = (char *)d_out;
    a.masked = (unsigned long long *)d_masked;
    a.error = e->d_error + nh::LAUNCH_SLOTS;
    const hipError_t he = nh::launch_qmask(a, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "quality mask launch: %s", hipGetErrorString(he));
    return NH_OK;
}
