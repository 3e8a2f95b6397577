// nh_bam.hip -- BAM records in HBM to canonical FASTQ text in HBM (gfx950), on the output builders' toolkit (nh_outbuild.h).
//
// One launch writes the whole text.  The host knows every length (it chained the records), so there is neither a size pass nor
// a scan: the table says where each record's block_size field lies in the BAM bytes and where its '@' lies in the text.
// A work item is a record, or -- a long record -- a span of at most `span` bytes of its text; the items are found without
// a second table: the text is cut into slots of `span` bytes, a wave owns the items whose first byte lies in its slot.  Those
// are the records that begin there (lower bound in the table: its text offsets ascend) and at most one later span of the record
// that reaches into the slot from before.  So a 100 kb read is written by a dozen waves and a batch of 150 bp reads costs
// one binary search per slot.  Each item is written with wave_write(): aligned dwords, 4 bytes a lane; field_dword() has fast
// paths for the name, the bases (two packed bytes -> four letters through v_perm_b32 on the alphabet held in four registers;
// reverse strand: v_bfrev_b32 reverses the order of the four nibbles and the bits of each -- the IUPAC complement in BAM's
// code -- in one instruction) and the qualities (aligned load pair + v_alignbyte, + 0x21 a byte; reverse: from the mirrored
// position, byte-swapped; absent: the constant).
// Bounds: every wave derives the record's fields from its own fixed part and writes only if they lie inside the BAM bytes and the
// record's text inside the text; else it sets a bit of the error word and writes nothing of that record.  The host's validation
// makes that unreachable in a run; nh_bam_to_fastq_device takes any table without a fault.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "nh_bam.h"
#include "nh_internal.h"
#include "nh_outbuild.h"

namespace nh {

namespace {

constexpr uint32_t BAM_SPAN_DEFAULT = 16384;  // (tools/bam_input_bench.py, profiles/bam_input.txt: the best of 1 Ki .. 64 Ki on long reads, level from 8 Ki on 150 bp reads)
constexpr uint32_t BAM_SPAN_MIN = 16, BAM_SPAN_MAX = 1u << 24;

// "=ACMGRSVTWYHKDBN", four letters a register
constexpr uint32_t AL0 = 0x4D43413Du, AL1 = 0x56535247u, AL2 = 0x48595754u, AL3 = 0x4E42444Bu;

struct Rec {  // a record's fields as absolute offsets into the BAM bytes
    uint64_t name, seq, qual;
    uint32_t n, L;      // name length without the NUL, bases
    uint64_t len;       // bytes of FASTQ text
    bool rev, noq;
};

// the nibbles k .. k + 3 of the packed bases (k = 2 * byte + odd, high nibble first) of the four bytes w, one a byte
__device__ __forceinline__ uint32_t four_nibbles(uint32_t w, uint32_t odd) {
    uint32_t s = ((w & 0x0F0F0F0Fu) << 4) | ((w >> 4) & 0x0F0F0F0Fu);  // nibble m of the stream at bits [4m, 4m + 4)
    s = (s >> (4 * odd)) & 0xFFFFu;
    s = (s | (s << 8)) & 0x00FF00FFu;
    return (s | (s << 4)) & 0x0F0F0F0Fu;
}

// four codes (one a byte) -> four letters
__device__ __forceinline__ uint32_t four_letters(uint32_t codes) {
    const uint32_t sel = codes & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(AL1, AL0, sel), hi = __builtin_amdgcn_perm(AL3, AL2, sel);
    const uint32_t m = ((codes >> 3) & 0x01010101u) * 0xFFu;
    return (hi & m) | (lo & ~m);
}

__device__ __forceinline__ uint32_t letter(uint32_t code) {
    const uint32_t w = code & 8 ? (code & 4 ? AL3 : AL2) : (code & 4 ? AL1 : AL0);
    return (w >> (8 * (code & 3))) & 0xFFu;
}

__device__ __forceinline__ uint32_t rev4(uint32_t n) { return __builtin_bitreverse32(n) >> 28; }

// qualities + 33, a byte each without a carry into the next
__device__ __forceinline__ uint32_t plus33(uint32_t w) { return ((w & 0x7F7F7F7Fu) + 0x21212121u) ^ (w & 0x80808080u); }

// The record at bam[o ...): false (and a bit of *error) unless its fields lie in the BAM bytes and its text in [0, text_len)
__device__ __forceinline__ bool load_record(const BamFastqArgs &a, uint64_t o, uint64_t t, Rec *r) {
    const char *bam = (const char *)a.bam;
    if (a.bam_len < 36 || o > a.bam_len - 36) {
        atomicOr(a.error, BAM_ERR_FIELDS);
        return false;
    }
    const uint32_t w12 = text_dword(bam, o + 12), w16 = text_dword(bam, o + 16), L = text_dword(bam, o + 20);
    const uint32_t l_name = w12 & 0xFFu, n_cigar = w16 & 0xFFFFu, flag = w16 >> 16;
    r->name = o + 36;
    r->seq = r->name + l_name + 4ull * n_cigar;
    r->qual = r->seq + ((uint64_t)L + 1) / 2;
    r->n = l_name - 1;
    r->L = L;
    r->len = (uint64_t)(l_name - 1) + 2ull * L + 6;
    r->rev = (flag & 0x10u) != 0;
    if (l_name == 0 || L == 0 || r->qual + L > a.bam_len) {
        atomicOr(a.error, BAM_ERR_FIELDS);
        return false;
    }
    if (a.text_len > a.text_cap || t > a.text_len || r->len > a.text_len - t) {
        atomicOr(a.error, BAM_ERR_TEXT);
        return false;
    }
    r->noq = (uint8_t)bam[r->qual] == 0xFFu;
    return true;
}

// bytes [p0, p1) of the record's text, by one wave
__device__ __forceinline__ void write_span(const BamFastqArgs &a, const Rec &r, uint64_t t, uint64_t p0, uint64_t p1, int lane) {
    const char *bam = (const char *)a.bam;
    const uint64_t S = (uint64_t)r.n + 2, SE = S + r.L, Q = SE + 3, QE = Q + r.L;
    auto byte_at = [&](uint64_t q) -> uint32_t {
        const uint64_t p = q + p0;
        if (p == 0) return '@';
        if (p < S - 1) return (uint8_t)bam[r.name + p - 1];
        if (p < S) return '\n';
        if (p < SE) {
            const uint64_t j = p - S, k = r.rev ? r.L - 1 - j : j;
            const uint32_t b = (uint8_t)bam[r.seq + (k >> 1)], nib = (k & 1) ? b & 15u : b >> 4;
            return letter(r.rev ? rev4(nib) : nib);
        }
        if (p < Q) return p == SE + 1 ? '+' : '\n';
        if (p < QE) {
            if (r.noq) return '"';
            const uint64_t j = p - Q;
            return ((uint8_t)bam[r.qual + (r.rev ? r.L - 1 - j : j)] + 33u) & 0xFFu;
        }
        return '\n';
    };
    auto field_dword = [&](uint64_t q, uint32_t *v) -> bool {
        const uint64_t p = q + p0;
        if (p >= S && p + 4 <= SE) {  // four bases: the packed bytes behind them belong to the record (its qualities follow)
            const uint64_t j = p - S, k = r.rev ? r.L - 4 - j : j;
            const uint32_t c = four_nibbles(text_dword(bam, r.seq + (k >> 1)), (uint32_t)(k & 1));
            *v = four_letters(r.rev ? __builtin_bitreverse32(c) >> 4 : c);
            return true;
        }
        if (p >= Q && p + 4 <= QE) {
            if (r.noq) {
                *v = 0x22222222u;
                return true;
            }
            const uint64_t j = p - Q;
            const uint32_t w = text_dword(bam, r.qual + (r.rev ? r.L - 4 - j : j));
            *v = plus33(r.rev ? __builtin_bswap32(w) : w);
            return true;
        }
        if (p >= 1 && p + 4 <= S - 1) {
            *v = text_dword(bam, r.name + p - 1);
            return true;
        }
        return false;
    };
    wave_write(a.text, t + p0, p1 - p0, lane, byte_at, field_dword);
}

__global__ __launch_bounds__(OB_THREADS) void k_bam_fastq(const BamFastqArgs a, uint64_t n_slots) {
    const int lane = threadIdx.x & 63;
    const uint64_t span = a.span;
    for (uint64_t slot = (uint64_t)blockIdx.x * OB_WAVES + (threadIdx.x >> 6); slot < n_slots; slot += (uint64_t)gridDim.x * OB_WAVES) {
        const uint64_t lo = slot * span;
        const bool last = slot + 1 == n_slots;  // (the last slot takes what a table puts behind the text as well: refused there)
        const uint64_t hi = lo + span;
        // the first record whose text begins at or behind lo
        uint64_t b = 0, e = a.n;
        while (b < e) {
            const uint64_t m = b + (e - b) / 2;
            if (a.table[2 * m + 1] < lo) b = m + 1;
            else e = m;
        }
        // from the record before -- the span of it that begins in this slot, if it reaches that far -- over the records that begin here
        for (uint64_t i = b ? b - 1 : 0; i < a.n; i++) {
            const uint64_t o = a.table[2 * i], t = a.table[2 * i + 1];
            uint64_t p0 = 0;
            if (i + 1 == b) p0 = (lo - t + span - 1) / span * span;  // (t < lo: p0 >= span, and lo <= t + p0 < hi)
            else if (!last && t >= hi) break;
            Rec r;
            if (!load_record(a, o, t, &r) || p0 >= r.len) continue;
            write_span(a, r, t, p0, p0 + span < r.len ? p0 + span : r.len, lane);
        }
    }
}

}  // namespace

hipError_t launch_bam_fastq(const BamFastqArgs &a_, hipStream_t stream) {
    if (a_.n == 0) return hipSuccess;
    BamFastqArgs a = a_;
    if (a.span == 0) {
        a.span = BAM_SPAN_DEFAULT;
        if (const char *env = getenv("NOHUMAN_BAM_SPAN")) {  // tuning / test knob
            const long v = atol(env);
            if (v > 0) a.span = (uint32_t)std::min<long>(v, BAM_SPAN_MAX);
        }
    }
    a.span = std::max(BAM_SPAN_MIN, std::min(BAM_SPAN_MAX, a.span));
    const uint64_t n_slots = std::max<uint64_t>(1, (a.text_len + a.span - 1) / a.span);
    const uint64_t blocks = std::min<uint64_t>((n_slots + OB_WAVES - 1) / OB_WAVES, 1u << 16);
    hipLaunchKernelGGL(k_bam_fastq, dim3((unsigned)blocks), dim3(OB_THREADS), 0, stream, a, n_slots);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_bam_to_fastq_device(nh_engine *e_, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_records,
                                      void *d_text, uint64_t text_cap, uint64_t text_len, int *error_bits, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !error_bits) return nh::set_error(NH_EINVAL, "null argument");
    if (n_records && (!d_bam || !d_table || !d_text)) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_bam | (uintptr_t)d_text) & 3) return nh::set_error(NH_EINVAL, "the BAM bytes and the text must be 4-byte aligned");
    if ((uintptr_t)d_table & 7) return nh::set_error(NH_EINVAL, "the table must be 8-byte aligned");
    if (text_len > text_cap) return nh::set_error(NH_EINVAL, "text_len %llu is above text_cap %llu", (unsigned long long)text_len, (unsigned long long)text_cap);
    if (n_records > (1ull << 34)) return nh::set_error(NH_EINVAL, "too many records for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    nh::BamFastqArgs a{};
    a.bam = (const uint8_t *)d_bam;
    a.bam_len = bam_len;
    a.table = (const uint64_t *)d_table;
    a.n = n_records;
    a.text = (char *)d_text;
    a.text_cap = text_cap;
    a.text_len = text_len;
    a.error = error_bits;
    a.span = 0;
    const hipError_t he = nh::launch_bam_fastq(a, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "BAM to FASTQ launch: %s", hipGetErrorString(he));
    return NH_OK;
}
