// nh_scan.h -- the minimizer scanner of the gfx950 kernels: the per-wave LDS layout, the tile encoder and scan_tile, with
// the hash helpers (fmix64, mod_capacity), and what the passes beside the classifier share: the walk over a stretch of text
// (walk_tiles), the find-only probe (find_cell) and the constant-value claim (claim_cell).  Device code shared by the classifier
// (nh_kernels.hip), the database builder (nh_build.hip), the minimizer data (nh_mdata.hip) and the host intervals
// (nh_cover.hip): a k-mer is ambiguous, and has the minimizer it has, by ONE piece of code in all of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_device.h"

namespace nh {

#define NH_FULL 0xFFFFFFFFFFFFFFFFull
#ifndef NH_WIDE_CELLS
#define NH_WIDE_CELLS 16  // cells per round of an old lookup (8, 12 or 16)
#endif
#ifndef NH_WIDE_AFTER
#define NH_WIDE_AFTER 2  // rounds after which a lookup examines 16 cells per round instead of 4
#endif
#ifndef NH_R2_CELLS
#define NH_R2_CELLS 4    // cells of a lookup's second round
#endif

// window reads of idle lanes stay inside the candidate array: k-l+2 pad entries (k-l = 4 for
// kraken2's default geometry, <= 64 in general)
template <bool STD> struct CandPad { static constexpr int value = STD ? 6 : 66; };

#ifndef NH_MIN_WAVES
#define NH_MIN_WAVES 5  // waves per SIMD the hot variant is built for (LDS: 5 workgroups of 31.5 KB per CU)
#endif
#ifndef NH_NSLOT
#define NH_NSLOT 4
#endif
#ifndef NH_LPO
#define NH_LPO 4  // lanes that fetch an owner's probe round together (probe_queue_quad): 4 = 16 cells per round, 2 = 8
#endif
#ifndef NH_LPL
#define NH_LPL 1  // look-ups an owner lane holds in the short-read kernel's probe rounds (probe_queue_quad): 2 = probe_rounds_two_slots, measured and not adopted
#endif
#ifndef NH_PROBE_DESC
#define NH_PROBE_DESC 1  // the short-read kernel's one-slot probe round issues its wave-loads from the last to the first: all four in flight together
#endif
#ifndef NH_QCAP
#define NH_QCAP 256  // 5 waves per SIMD need <= 31 KB of LDS per workgroup (a 32 KB one fits only 4 times: profiles/r02_tuning.txt)
#endif
constexpr int NSLOT = NH_NSLOT;  // tiles scanned before one shared probe phase
static_assert(NSLOT <= 4, "carry_pack holds four 16-bit queue indices per group: one inherited-minimizer entry per tile");
constexpr int QCAP_SHORT = NH_QCAP;  // queue entries per group: a tile joins only if it is sure to fit (< 512)
#ifndef NH_QCAP_GENERIC
#define NH_QCAP_GENERIC 288  // the generic kernel keeps one packed stream instead of NSLOT: room for a longer queue
#endif
constexpr int QCAP_GENERIC = NH_QCAP_GENERIC;
constexpr uint32_t QTAX_SKIP = 0xFFFFFFFFu;  // queue entry dropped by the min-hash filter

constexpr int PKW = 18;  // words of a tile's packed stream: 16 of data + the 2 zero words a funnel read may touch

struct alignas(16) SlotLds {  // a scanned tile waiting for its probe results (written by lane 0)
    uint32_t f_lo, f_hi;    // fragment
    uint32_t koff, pad0;    // k-mer index of the tile within its fragment
    uint32_t nqt, qbase, nruns;
    uint32_t pad1;
    uint32_t last_lane;     // 2*lane+slot of the last unambiguous k-mer, 0xFFFFFFFF if none
    uint32_t flags;         // 1 = last tile of its fragment, 2 = last tile of mate 0, mate 1 follows
    uint32_t nk0, total_kmers;
};

// the generic kernel keeps the probe results apart from the queue entries; STD aliases them
template <bool STD, int QC> struct QTax { uint32_t v[2][QC]; };
template <int QC> struct QTax<true, QC> {};

// LDS slice of one wave.  NPK = tiles whose packed streams exist at a time (1: the generic kernel encodes
// and scans tile by tile; NSLOT: the short-read kernel encodes a batch first), QC = queue entries per
// group.  Both kernels are sized to 31 KB per workgroup: five workgroups per CU.
template <bool STD, int NPK, int QC>
struct WaveLdsT {
    static constexpr int QCAP = QC;
#if defined(NH_LDS_PAD) && NH_LDS_PAD > 0
    uint32_t occupancy_pad[NH_LDS_PAD / 4];  // tuning aid: lowers the number of resident workgroups
#endif
    unsigned long long acc[4];  // fragments, classified, bases, lookups of this wave (lane 0 adds)
    uint64_t last_dw;           // last readable dword of the bases buffer
    uint4 frag_state;        // FragState between post_group calls: nlist, hit_groups, carry_tax, overflow
    SlotLds slot[2][NSLOT];  // [parity of the group][tile]
    uint16_t ps[2][NSLOT][WAVE];  // per-lane packed k-mer state of the tiles in flight
    // 2-bit packed bases of a tile: base i' of the tile frame at bit 2*(255-i'); 64 B + zero pad.  One per
    // tile of a group: the short-read kernel encodes a whole batch of tiles before it scans them
    uint32_t pk[NPK][PKW];
    uint32_t pa[NPK][PKW];  // same layout, value 1 where the base is ambiguous
    // result records of the fragments the last post_group finished: stored to global memory by the next
    // turn, right before its probe phase (flush_records)
    uint4 stage_rec[NSLOT];
    uint64_t stage_f[NSLOT];
    uint32_t stage_n;
    uint64_t cand[TL + CandPad<STD>::value];
    uint64_t q[2][QC];  // [parity] queue: run-start minimizers, hashed in place (see probe_queue)
    QTax<STD, QC> qtax;       // taxon found for each queued run (generic kernel only, see tax_at)
    // (taxon, count) list of the fragment being post-processed: tiles are post-processed strictly
    // in input order, so one list (and one FragState, kept in registers) serves all fragments
    uint32_t list_tax[LIST_CAP];
    uint32_t list_cnt[LIST_CAP];
};

__device__ __forceinline__ void wave_sync() {
    // LDS operations of one wave are issued and serviced in order; only the compiler must be
    // kept from moving LDS accesses across the hand-off points.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// exact hc % capacity: q' = floor(hc * floor((2^64-1)/cap) / 2^64) is q, q-1 or q-2
__device__ __forceinline__ uint64_t mod_capacity(uint64_t hc, uint64_t cap, uint64_t magic) {
    uint64_t q = __umul64hi(hc, magic);
    uint64_t r = hc - q * cap;
    if (r >= cap) r -= cap;
    if (r >= cap) r -= cap;
    return r;
}

// Find-only look-up of one minimizer by linear probing: plain loads from its home on, the index wrapping at the table's end, until
// an empty cell or the compacted key; at most `cap` cells are looked at.  -> the value found (0: a miss) and, with it, in `at`
// the cell where the key matched.
__device__ __forceinline__ uint32_t find_cell(const uint32_t *table, const uint64_t cap, const uint64_t magic, const uint32_t vbits,
                                              const uint32_t vmask, const uint64_t mz, uint64_t &at) {
    const uint64_t hc = fmix64(mz);
    const uint32_t compacted = (uint32_t)(hc >> (32 + vbits));
    uint64_t idx = mod_capacity(hc, cap, magic);
    for (uint64_t tries = 0; tries < cap; tries++) {
        const uint32_t cell = table[idx];
        const uint32_t v = cell & vmask;
        if (v == 0) return 0;  // an empty cell ends the probe run
        if ((cell >> vbits) == compacted) {
            at = idx;
            return v;
        }
        idx++;
        if (idx >= cap) idx = 0;
    }
    return 0;
}

// kraken2 CompactHashTable::CompareAndSet with a constant value: claim the first empty cell of the probe sequence, or stop at a
// cell that already holds this compacted key (or after `cap` cells).  -> this lane claimed an empty cell.
__device__ __forceinline__ bool claim_cell(uint32_t *table, const uint64_t cap, const uint64_t magic, const uint32_t vbits,
                                           const uint32_t value, const uint64_t mz) {
    const uint64_t hc = fmix64(mz);
    const uint32_t compacted = (uint32_t)(hc >> (32 + vbits));
    const uint32_t cell = (compacted << vbits) | value;
    uint64_t idx = mod_capacity(hc, cap, magic);
    for (uint64_t tries = 0; tries < cap; tries++) {
        const uint32_t old = atomicCAS(&table[idx], 0u, cell);
        if (old == 0) return true;
        if ((old >> vbits) == compacted) return false;
        idx++;
        if (idx >= cap) idx = 0;
    }
    return false;
}

// reverse the 32 two-bit groups of x and complement every base
__device__ __forceinline__ uint64_t revcomp_word(uint64_t x) {
    const uint64_t br = __builtin_bitreverse64(x);
    return ~(((br & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((br & 0x5555555555555555ull) << 1));
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// number of set bits of a wave mask below this lane
__device__ __forceinline__ uint32_t below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Kernel arguments are read on demand from the kernarg segment (constant address space, scalar
// loads).  Each phase launders the pointer first, which stops the compiler from hoisting every
// argument load to the kernel entry and pinning ~50 SGPRs for the whole kernel.
typedef const __attribute__((address_space(4))) KArgs *KArgsP;
__device__ __forceinline__ KArgsP launder(KArgsP p) {
    const uint64_t v = (uint64_t)p;
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (KArgsP)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int src) {
    uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src);
    uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ bool is_a_ancestor_of_b(const uint32_t *parent, uint32_t a, uint32_t b) {
    if (!a || !b) return false;
    while (b > a) b = parent[b];
    return a == b;
}

__device__ __forceinline__ uint32_t lowest_common_ancestor(const uint32_t *parent, uint32_t a,
                                                           uint32_t b) {
    if (!a || !b) return a ? a : b;
    while (a != b) {
        if (a > b)
            a = parent[a];
        else
            b = parent[b];
    }
    return a;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// 4 ASCII bytes -> one byte of packed 2-bit codes (first base in bits 7:6); `diff` is non-zero in
// every byte that is not one of ACGTacgt (SWAR, no per-byte work on the common path)
__device__ __forceinline__ uint32_t encode4(uint32_t w, uint32_t &diff) {
    const uint32_t up = w & 0xDFDFDFDFu;          // fold case
    const uint32_t x = (up >> 1) & 0x03030303u;   // A0 C1 G3 T2
    const uint32_t code = x ^ ((x >> 1) & 0x01010101u);  // A0 C1 G2 T3
    const uint32_t tbit = (x >> 1) & ~x & 0x01010101u;   // 1 where the byte decodes as T
    const uint32_t recon = (0x41414141u | (x << 1)) ^ (tbit * 0x11u);  // canonical letter of code
    diff = recon ^ up;
    return (code * 0x40100401u) >> 24;
}

// exact per-base flags "real base of this read and not ACGTacgt", same packing as the codes
__device__ __forceinline__ uint32_t ambig4(uint32_t w, uint32_t p0, uint32_t lo, uint32_t hi) {
    uint32_t bad = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t ch = (w >> (8 * b)) & 0xDFu;
        const bool ok = (ch == 0x41u) | (ch == 0x43u) | (ch == 0x47u) | (ch == 0x54u);
        const uint32_t p = p0 + b;
        const bool real = (p >= lo) & (p < hi);
        bad |= ((real & !ok) ? 1u : 0u) << (6 - 2 * b);
    }
    return bad;
}

__device__ __forceinline__ uint64_t funnel_read(const uint32_t *pkd, uint32_t s) {
    const uint32_t d = s >> 5, r = s & 31u;
    const uint64_t lo = (uint64_t)pkd[d] | ((uint64_t)pkd[d + 1] << 32);
    const uint64_t hi = pkd[d + 2];
    return r ? ((lo >> r) | (hi << (64 - r))) : lo;
}

// per-fragment accumulation state of one wave (wave-uniform scalars)
struct FragState {
    uint32_t nlist;       // distinct taxa in the LDS list
    uint32_t hit_groups;  // minimizer_hit_groups
    uint64_t carry_min;   // kraken2 last_minimizer (NH_FULL = none)
    uint32_t carry_tax;   // kraken2 last_taxon
    bool overflow;
};

#define NH_STAMP(i)                                        \
    do {                                                   \
        if (PROF) {                                        \
            const uint64_t _t = __builtin_readcyclecounter(); \
            prof[i] += _t - tprev;                         \
            tprev = _t;                                    \
        }                                                  \
    } while (0)

// ENCODE one tile into the packed streams of `slot`: 4 bases per lane (dword stream `w`, tile frame
// starting `sh` bytes in), of which bytes [sh, sh + nbases) belong to this sequence.  What follows them
// is whatever lies behind the sequence in the caller's buffer (the next read, or -- when records are
// classified in place inside their FASTQ text -- a newline and the quality line): it must neither count
// as ambiguous nor send the tile down the slow path.  Returns "the tile has an ambiguous base".
template <bool STD, class WL>
__device__ __forceinline__ bool encode_tile(WL &S, const int lane, const uint32_t slot, const uint32_t w,
                                            const uint32_t sh, const uint32_t nbases) {
    uint32_t diff;
    const uint32_t codes = encode4(w, diff);
    reinterpret_cast<uint8_t *>(S.pk[slot])[63 - lane] = (uint8_t)codes;
    // bytes of this lane's dword that are bases of the sequence: frame positions [4 lane, 4 lane + 4) cut to [sh, hi)
    const uint32_t p0 = 4u * (uint32_t)lane, hi = sh + nbases;
    uint32_t m = 0xFFFFFFFFu;
    if (p0 < sh) m = sh - p0 >= 4u ? 0u : m << (8u * (sh - p0));
    if (p0 + 4u > hi) m = hi <= p0 ? 0u : m & (0xFFFFFFFFu >> (8u * (p0 + 4u - hi)));
    bool has_amb = __ballot((diff & m) != 0) != 0;
    if (has_amb) {  // exact flags, restricted to the bases of this tile
        const uint32_t bad = ambig4(w, p0, sh, hi);
        reinterpret_cast<uint8_t *>(S.pa[slot])[63 - lane] = (uint8_t)bad;
    }
    return has_amb;
}

// SCAN one encoded tile (streams of `slot`): l-mers [q0, q0+nlt) / k-mers [q0, q0+nqt) of a sequence
// whose tile frame starts `sh` bytes into its dword stream.  Appends the run-start minimizers to
// S.q[par][qbase ...], returns their number, and leaves in `ps` the lane's packed per-k-mer state
// (bit0/1 = k-mer 2t / 2t+1 is valid and unambiguous, bit 2 = k-mer 2t+1 starts a run, bits 3-10 = 1 + index of the run
// that covers k-mer 2t, 0 = continuation of the run that entered the tile).
template <bool STD, bool PROF, class WL>
__device__ __forceinline__ uint32_t scan_body(KArgsP ap, WL &S, const int lane, const uint32_t slot,
                                              const bool has_amb, const uint32_t sh, const uint32_t nlt,
                                              const uint32_t nqt, const uint32_t par,
                                              const uint32_t qbase, uint64_t &carry_min,
                                              uint32_t &ps, int &last_lane,
                                              uint64_t (&prof)[12], uint64_t &tprev) {
    ap = launder(ap);
    const uint32_t L = STD ? 31u : ap->db.l;
    const uint32_t W = STD ? 4u : ap->db.window;
    const uint64_t LMASK = STD ? ((1ull << 62) - 1) : ap->db.lmer_mask;
    const int RV = STD ? 1 : ap->db.revcom_version;
    const uint64_t SPACED = ap->db.spaced_mask, TOGGLE = ap->db.toggle;

    // ---- 2. two l-mers per lane -> candidates --------------------------------------------------
    {
        const uint32_t j1 = sh + 2u * lane + L;  // frame index of the last base of l-mer 2t+1
        const uint32_t s = 2u * (255u - j1);
        const uint64_t wv = funnel_read(S.pk[slot], s);
        const uint64_t lm1 = wv & LMASK;
        const uint64_t lm0 = (wv >> 2) & LMASK;
        uint64_t rc0, rc1;
        if (RV != 0) {
            const uint64_t R = revcomp_word(wv);  // one reverse complement serves both l-mers
            rc1 = R >> (64 - 2 * L);
            rc0 = (R >> (62 - 2 * L)) & LMASK;
        } else {  // legacy databases: complement of the un-shifted reversed word
            rc1 = revcomp_word(lm1) & LMASK;
            rc0 = revcomp_word(lm0) & LMASK;
        }
        const uint64_t c0 = (umin64(lm0, rc0) & SPACED) ^ TOGGLE;
        const uint64_t c1 = (umin64(lm1, rc1) & SPACED) ^ TOGGLE;
        bool dead0 = 2u * lane >= nlt, dead1 = 2u * lane + 1 >= nlt;
        if (has_amb) {
            const uint64_t wa = funnel_read(S.pa[slot], s);
            dead1 |= (wa & LMASK) != 0;
            dead0 |= ((wa >> 2) & LMASK) != 0;
        }
        ulonglong2 cc;
        cc.x = dead0 ? NH_FULL : c0;
        cc.y = dead1 ? NH_FULL : c1;
        *reinterpret_cast<ulonglong2 *>(&S.cand[2 * lane]) = cc;
    }
    wave_sync();

    // ---- 3. two k-mer minimizers per lane (window min) -----------------------------------------
    const uint32_t qi0 = 2u * lane, qi1 = 2u * lane + 1;
    uint64_t mz0, mz1;
    bool v0, v1;  // valid and non-ambiguous
    {
        uint64_t first, mid, last0, last1;
        if (STD) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(&S.cand[qi0]);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(&S.cand[qi0 + 2]);
            const ulonglong2 c = *reinterpret_cast<const ulonglong2 *>(&S.cand[qi0 + 4]);
            first = a.x;
            mid = umin64(umin64(a.y, b.x), umin64(b.y, c.x));
            last0 = c.x;
            last1 = c.y;
        } else if (W == 0) {
            first = S.cand[qi0];
            last1 = S.cand[qi1];
            last0 = first;
            mid = NH_FULL;
        } else {
            first = S.cand[qi0];
            mid = S.cand[qi0 + 1];
            for (uint32_t i = 2; i <= W; i++) mid = umin64(mid, S.cand[qi0 + i]);
            last0 = S.cand[qi0 + W];
            last1 = S.cand[qi1 + W];
        }
        uint64_t m0 = umin64(first, mid);
        uint64_t m1 = (!STD && W == 0) ? last1 : umin64(mid, last1);
        if (!STD && has_amb && W > L) {
            // kraken2's scanner empties its queue at an ambiguous base, so a k-mer's window holds only
            // the l-mers that lie wholly after the last ambiguous base.  While k-l <= l
            // every l-mer of the window before that base contains it (is +inf) and the plain min is
            // the same thing; beyond that, walk back from the last l-mer and stop at the first dead one.
            uint64_t a0 = NH_FULL, a1 = NH_FULL;
            bool open0 = true, open1 = true;
            for (uint32_t i = W + 1; i-- > 0;) {
                const uint64_t c0 = S.cand[qi0 + i], c1 = S.cand[qi1 + i];
                open0 &= c0 != NH_FULL;
                open1 &= c1 != NH_FULL;
                if (open0) a0 = umin64(a0, c0);
                if (open1) a1 = umin64(a1, c1);
            }
            m0 = a0;
            m1 = a1;
        }
        v0 = (qi0 < nqt) & (last0 != NH_FULL);
        v1 = (qi1 < nqt) & (last1 != NH_FULL);
        if (has_amb && ap->db.ambig_rule != 0) {
            // nh_options.ambiguity_rule 1 (mmscanner.h is_ambiguous(): queue_pos < k-l || last_ambig): a k-mer counts
            // only when k-l l-mers have been queued since the last ambiguous base, i.e. when every l-mer of its window
            // but the first is alive (the first may be dead: the window of the first clean k-mer holds k-l l-mers;
            // +inf drops out of the min by itself).  Rule 0 asks for the last l-mer only.
            if (STD) {
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(&S.cand[qi0]);
                const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(&S.cand[qi0 + 2]);
                const bool mid_alive = (b.x != NH_FULL) & (b.y != NH_FULL);
                v0 &= mid_alive & (a.y != NH_FULL);
                v1 &= mid_alive & (last0 != NH_FULL);
            } else {
                for (uint32_t i = 1; i < W; i++) {  // (i == W is last0 / last1)
                    v0 &= S.cand[qi0 + i] != NH_FULL;
                    v1 &= S.cand[qi1 + i] != NH_FULL;
                }
            }
        }
        mz0 = m0 ^ TOGGLE;
        mz1 = m1 ^ TOGGLE;
    }

    NH_STAMP(2);
    // ---- 4. run starts: minimizer differs from the previous non-ambiguous one -----------------
    uint64_t prev_in;
    if (!has_amb) {
        prev_in = __shfl_up(mz1, 1, 64);
        if (lane == 0) prev_in = carry_min;
    } else {
        // inclusive scan of "rightmost lane that holds a non-ambiguous k-mer"
        bool has = v0 | v1;
        uint64_t val = v1 ? mz1 : mz0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const bool h2 = __shfl_up((int)has, d, 64) != 0;
            const uint64_t x2 = __shfl_up(val, d, 64);
            if (lane >= d && !has) {
                has = h2;
                val = x2;
            }
        }
        const bool hx = __shfl_up((int)has, 1, 64) != 0;
        const uint64_t vx = __shfl_up(val, 1, 64);
        prev_in = (lane > 0 && hx) ? vx : carry_min;
    }
    const uint64_t prev1 = v0 ? mz0 : prev_in;
    const bool new0 = v0 & (mz0 != prev_in);
    const bool new1 = v1 & (mz1 != prev1);

    // ---- 5. append run starts to the LDS queue; remember the last minimizer --------------------
    const uint64_t b0 = __ballot(new0), b1 = __ballot(new1);
    const uint32_t ex = below(b0) + below(b1);
    const uint32_t nruns = __popcll(b0) + __popcll(b1);
    if (new0) S.q[par][qbase + ex] = mz0;
    if (new1) S.q[par][qbase + ex + (new0 ? 1u : 0u)] = mz1;
    const uint32_t r0p = ex + (new0 ? 1u : 0u);  // 1 + run index of k-mer 2t (0 = carried run)
    ps = (v0 ? 1u : 0u) | (v1 ? 2u : 0u) | (new1 ? 4u : 0u) | (r0p << 3);
    {
        const uint64_t m1 = __ballot(v1), m0 = __ballot(v0);
        last_lane = -1;
        if (m0 | m1) {
            const int l1 = m1 ? 63 - __builtin_clzll(m1) : -1;
            const int l0 = m0 ? 63 - __builtin_clzll(m0) : -1;
            if (l1 >= l0) {
                carry_min = readlane64(mz1, l1);
                last_lane = 2 * l1 + 1;
            } else {
                carry_min = readlane64(mz0, l0);
                last_lane = 2 * l0;
            }
        }
    }
    NH_STAMP(3);
    return nruns;
}


// One tile of the generic kernel: encode (slot 0), start the prefetch of a later tile, scan.
template <bool STD, bool PROF, class WL>
__device__ __forceinline__ uint32_t scan_tile(KArgsP ap, WL &S, const int lane,
                                              const uint32_t w,
                                              const uint32_t sh, const uint32_t nlt,
                                              const uint32_t nqt, const uint32_t par,
                                              const uint32_t qbase, uint64_t &carry_min,
                                              uint32_t &ps, int &last_lane,
                                              const uint32_t *pf_ptr, const bool pf_on,
                                              uint32_t &w_pref,
                                              uint64_t (&prof)[12], uint64_t &tprev) {
    const uint32_t L = STD ? 31u : launder(ap)->db.l;
    const bool has_amb = encode_tile<STD>(S, lane, 0u, w, sh, nlt + L - 1);
    wave_sync();
    // `w` has been consumed: start the load of the next tile's bases now, so that no wait for
    // `w` can be widened into a wait for the prefetch (vmcnt retires loads in issue order)
    if (pf_on) w_pref = *pf_ptr;
    NH_STAMP(1);
    return scan_body<STD, PROF>(ap, S, lane, 0u, has_amb, sh, nlt, nqt, par, qbase, carry_min, ps, last_lane, prof,
                                tprev);
}

// one-time LDS init of a wave: zero pads of the packed streams, sentinel tail of the candidate array
template <bool STD, class WL>
__device__ __forceinline__ void init_wave_lds(WL &S, const int lane) {
    if (lane == 0) S.stage_n = 0;
    for (int i = lane; i < (int)(sizeof(S.pk) / 4); i += 64) {
        (&S.pk[0][0])[i] = 0;
        (&S.pa[0][0])[i] = 0;
    }
    for (int i = lane; i < CandPad<STD>::value; i += 64) S.cand[TL + i] = NH_FULL;
    wave_sync();
}

constexpr uint32_t PREF_LANES = 42;  // dwords a tile can need: (3 + 128 + 30 + 3) / 4 <= 41

// The tile walk of the passes beside the classifier that take a closure well -- the builder's walk_pieces and k_insert_sequences;
// k_mdata_mark and k_cover_mark keep this loop written out (profiles/tile_walk_refactor.txt) -- at the default geometry, k = 35,
// l = 31: ONE stretch text[o0, o0 + n) a tile of TL - 4 k-mers at a time through scan_tile<true, false>, the next tile's dword
// loaded while this one is scanned.  The text is read as dwords and every dword index is clamped to `last_dw`, the last dword
// the caller may read: no load leaves text[0 .. last_dw] whatever o0 and n are.  The caller sees to it that n >= 35, that the
// stretch lies inside the text, and that both tests are wave-uniform: the whole wave walks, or none of it.  `carry_min` is the
// minimizer of the last unambiguous k-mer before the stretch (NH_FULL: none) and, afterwards, of the last one in it.
// per_tile(nruns, ps) is called between two wave_sync() with the tile's run-start minimizers in S.q[0][0 .. nruns), two a lane
// at the most; `ps` is scan_body's.
template <class WL, class PerTile>
__device__ __forceinline__ void walk_tiles(KArgsP ap, WL &S, const int lane, const uint32_t *const text, const uint64_t last_dw,
                                           const uint64_t o0, const uint32_t n, uint64_t &carry_min, PerTile &&per_tile) {
    const uint32_t TQ = TL - 4u;  // k-mers of a full tile
    const uint32_t pl = (uint32_t)lane < PREF_LANES ? (uint32_t)lane : PREF_LANES - 1;
    const uint32_t nk = n - 34u;
    uint64_t prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tprev = 0;
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
        per_tile(nruns, ps);
        wave_sync();
        w = w_next;
    }
}

}  // namespace nh
