// nh_qseq.h -- where a batch's sequences and their qualities lie, and aligned loads of both: shared by the kernels that walk every
// sequence of a batch beside its quality line (nh_qmask.hip, nh_rstats.hip).  Device code only.
//
// A sequence's unit is a 16-byte chunk aligned in the text (four aligned dwords): the bases need no realignment, the qualities --
// at another residue mod 4 in general -- are realigned with v_alignbyte.  A chunk that is not wholly inside its sequence goes dword
// by dword; a dword that is not wholly inside goes byte by byte for the qualities: the neighbouring bytes belong to the header, the
// separator or another sequence.  Every load stays inside dwords that hold bytes of [0, ntext).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_internal.h"

namespace nh {

namespace {

constexpr uint64_t NO_QUAL = ~0ull;

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

struct QSeq {  // one sequence of the launch
    uint64_t s, q;     // starts of the bases and of the qualities (q == NO_QUAL: none, the bases are copied)
    uint32_t len;
    uint32_t nch;      // 16-byte chunks of `out` that hold its bytes (0: nothing to write)
    bool bad;          // fails its checks: error bit, nothing written
};

__device__ inline QSeq load_qseq(const QSeqSrc &a, uint64_t i) {
    QSeq r{};
    if (i >= a.n) return r;
    r.s = a.seq_off[i];
    r.len = a.seq_len[i];
    r.q = NO_QUAL;
    uint32_t qlen = r.len;
    if (a.rec) {
        if (a.fastq[a.mates == 2 ? (int)(i & 1) : 0]) {
            const uint4 fr = reinterpret_cast<const uint4 *>(a.rec)[i];
            r.q = fr.z;
            qlen = fr.w;
        }
    } else {
        r.q = a.qual_off[i];
    }
    r.bad = r.s > a.ntext || r.len > a.ntext - r.s;
    if (r.q != NO_QUAL) {
        r.bad = r.bad || qlen != r.len || r.q > a.ntext || r.len > a.ntext - r.q;
        // (the quality starts alone: the line is longer than the sequence when what follows the len bytes is no line end)
        if (!r.bad && !a.rec && r.q + r.len < a.ntext && (uint8_t)a.text[r.q + r.len] > (uint8_t)' ') r.bad = true;
    }
    if (!r.bad && r.len) r.nch = (uint32_t)((r.s + r.len - (r.s & ~3ull) + 15) >> 4);
    return r;
}

// the 4 text bytes at src (all inside the text): two aligned loads, the second only where the bytes reach into it
__device__ inline uint32_t text_dword(const char *text, uint64_t src) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(text + (src & ~3ull));
    const uint32_t sh = (uint32_t)(src & 3);
    const uint32_t lo = w[0];
    if (sh == 0) return lo;
    return __builtin_amdgcn_alignbyte(w[1], lo, sh);
}

// the qualities of the bases in out's chunk [D, D + 16) of sequence r, 0xFF for the bytes of the chunk outside the sequence
__device__ inline uint4 qual_chunk(const QSeqSrc &a, const QSeq &r, uint64_t D) {
    const uint64_t end = r.s + r.len;
    if (D >= r.s && D + 16 <= end) {
        const uint64_t qp = r.q + (D - r.s), A = qp & ~3ull;
        const uint32_t sh = (uint32_t)(qp & 3);
        const u32x4a4 v = *reinterpret_cast<const u32x4a4 *>(a.text + A);
        if (sh == 0) return make_uint4(v.x, v.y, v.z, v.w);
        const uint32_t e = *reinterpret_cast<const uint32_t *>(a.text + A + 16);
        return make_uint4(__builtin_amdgcn_alignbyte(v.y, v.x, sh), __builtin_amdgcn_alignbyte(v.z, v.y, sh),
                          __builtin_amdgcn_alignbyte(v.w, v.z, sh), __builtin_amdgcn_alignbyte(e, v.w, sh));
    }
    uint32_t d[4];
    for (int k = 0; k < 4; k++) {
        const uint64_t W = D + 4ull * k;
        d[k] = 0xFFFFFFFFu;
        if (W >= r.s && W + 4 <= end) {
            d[k] = text_dword(a.text, r.q + (W - r.s));
        } else {
            for (int j = 0; j < 4; j++) {
                const uint64_t x = W + j;
                if (x >= r.s && x < end)
                    d[k] = (d[k] & ~(0xFFu << (8 * j))) | (uint32_t)(uint8_t)a.text[r.q + (x - r.s)] << (8 * j);
            }
        }
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// the text's dwords of the chunk [D, D + 16): those that hold a byte of the sequence (the others: 0, never stored)
__device__ inline uint4 base_chunk(const QSeqSrc &a, const QSeq &r, uint64_t D) {
    const uint64_t end = r.s + r.len;
    if (D >= r.s && D + 16 <= end) {
        const u32x4a4 v = *reinterpret_cast<const u32x4a4 *>(a.text + D);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t d[4];
    for (int k = 0; k < 4; k++) {
        const uint64_t W = D + 4ull * k;
        d[k] = (W + 4 > r.s && W < end) ? *reinterpret_cast<const uint32_t *>(a.text + W) : 0u;
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

__device__ inline bool has_newline(uint32_t q) {
    const uint32_t z = q ^ 0x0A0A0A0Au;
    return ((z - 0x01010101u) & ~z & 0x80808080u) != 0;
}
__device__ inline bool has_newline(const uint4 &q) { return has_newline(q.x) || has_newline(q.y) || has_newline(q.z) || has_newline(q.w); }

}  // namespace

}  // namespace nh
