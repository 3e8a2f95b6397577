// nh_mdata.hip -- minimizer data (nh_run_mdata, --report-minimizer-data): per taxon, how many minimizer hit groups the reads of a
// run produced and how many DISTINCT database minimizers they were (kraken2's --report-minimizer-data, the KrakenUniq idea), with
// the cells of the table per taxon as the denominator (kraken2-inspect's number).  DESIGN.md 6.13; tests/mdata_model.py is the
// specification.
//
// Every database minimizer lives in exactly one cell of the table, so one bit per cell counts distinct minimizers EXACTLY: no
// HyperLogLog, no sketches to merge, the same numbers whatever the batches, streams and devices, and clades that sum.
//
// k_mdata_mark, a pass of its own behind the classifier (which is not touched): one wave per fragment, both mates by the same
// wave (reset_per_mate = 0 carries the last minimizer across the mate border), a mate a tile at a time through the classifier's
// own scanner, carry_min from tile to tile and across the mate border -- a run start here is a run start there.  The tile loop
// is walk_tiles' (nh_scan.h), written out: with its per-tile code in a closure the kernel compiled with more exec-mask
// bookkeeping and missed the parent's timing in some legs (profiles/tile_walk_refactor.txt); as it stands it compiles to the
// code it had.  Every run start is looked up with a find-only linear probe over copy 0 of the resident table (nh_scan.h: find_cell; 64-bit cell
// indices, bounded by the capacity); a hit sets the bit of the cell WHERE THE KEY WAS FOUND and counts one hit group for the
// cell's value.
//   the bit      the word is read with a plain load first and the atomic OR issued only when the bit is clear: bits only go from 0
//                to 1, so a stale read costs one redundant atomic and nothing else.  In a host-heavy sample almost every hit is a
//                repeat, and a device atomic drops its line from L2 where a load keeps it (NOHUMAN_MDATA_ATOMIC=always disables
//                the test, for the A/B of tools/mdata_bench.py).
//   the groups   lanes with equal taxa are grouped by ballot, one sum per distinct taxon and tile -- and the sums are kept on the
//                wave, in 64 (taxon, count) entries of its LDS slice indexed by the taxon's low bits (the classifier's per-fragment
//                list, which this kernel has no other use for): an entry is added to d_groups when another taxon takes its place
//                and at the wave's end.  One atomic per distinct taxon and TILE was the first form, and it was the whole cost of
//                the kernel: on a database of one host every tile of the launch added to ONE word -- 1 M atomics on one address,
//                which retire at 46-88 per microsecond on this chip (nh_device.h) -- 12.4 ms for 1 M pairs where the classifier
//                takes 1.8 (profiles/minimizer_data.txt).  Now a human-only database is one atomic a wave.
// k_mdata_count: one lane per dword of the bitmap (32 cells).  A zero word is skipped without touching the table; otherwise the
// word's cells are loaded 16 bytes at a time and every marked cell with a value adds 1 to its value's bin.  Bins in LDS, one global
// atomic per non-zero bin and workgroup, while node_count <= MD_LDS_BINS (k_value_cells' scheme); above that 64-bit global
// atomics, runs of one value within a lane's word and equal values across the wave added up first.  marks == NULL: every cell
// counts, which gives the cells per taxon from the same kernel.
// Nothing here writes through anything but vector stores and atomics from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "nh_device.h"
#include "nh_internal.h"
#include "nh_scan.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

constexpr uint32_t MD_LDS_BINS = 4096;  // nodes up to which k_mdata_count keeps its bins in LDS (16 KB)

struct MarkDev {
    uint32_t *marks;             // one bit per cell, ceil(capacity / 32) words
    unsigned long long *groups;  // node_count counters
};

// One wave per fragment; TEST: look at the bitmap's word before the atomic.
template <bool TEST>
__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_mdata_mark(const KArgs args_by_kernarg_pointer, const MarkDev m) {
    KArgsP ap = (KArgsP)__builtin_amdgcn_kernarg_segment_ptr();
    typedef WaveLdsT<true, 1, QCAP_GENERIC> WL;
    __shared__ WL lds_all[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WL &S = lds_all[wib];
    static_assert(LIST_CAP == WAVE, "the wave's (taxon, count) entries: one a lane at the start and at the end");
    S.list_tax[lane] = 0;
    S.list_cnt[lane] = 0;
    init_wave_lds<true>(S, lane);
    const uint32_t TQ = TL - 4u;  // k-mers of a full tile
    const uint64_t n_frag = ap->n_frag;
    const uint32_t mates = (uint32_t)ap->mates;
    const bool reset = ap->db.reset_per_mate != 0;
    const uint64_t *const start = ap->seq_off;
    const uint32_t *const len = ap->seq_len;
    const uint64_t text_len = ap->bases_end;
    const uint64_t last_dw = (text_len + 4) >> 2;  // the text is readable for 8 bytes behind its end
    const uint32_t *const text = reinterpret_cast<const uint32_t *>(ap->bases);
    const uint32_t pl = (uint32_t)lane < PREF_LANES ? (uint32_t)lane : PREF_LANES - 1;
    const uint32_t *const table = ap->db.table;
    const uint64_t cap = ap->db.capacity;
    const uint64_t magic = ap->db.cap_magic;
    const uint32_t vbits = ap->db.value_bits, vmask = ap->db.vmask, nodes = ap->db.node_count;
    uint64_t prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tprev = 0;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t f = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib; f < n_frag; f += n_waves) {
        uint64_t carry_min = NH_FULL;
        for (uint32_t mate = 0; mate < mates; mate++) {
            if (reset) carry_min = NH_FULL;
            const uint64_t o0 = start[f * mates + mate];
            const uint32_t n = len[f * mates + mate];
            if (n < 35u || o0 > text_len || text_len - o0 < n) continue;  // (wave-uniform) no k-mer, or a range that leaves the text
            const uint32_t nk = n - 34u;
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
                // a tile holds at most TQ = 124 run starts: two a lane
                uint32_t tax[2] = {0u, 0u};
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const uint32_t r = (uint32_t)lane + 64u * s;
                    if (r >= nruns) continue;
                    uint64_t at = 0;
                    const uint32_t v = find_cell(table, cap, magic, vbits, vmask, S.q[0][r], at);
                    if (v == 0 || v >= nodes || at >= cap) continue;  // a miss (or a value that is no node: nh_open refuses such a table)
                    tax[s] = v;
                    uint32_t *const word = m.marks + (at >> 5);
                    const uint32_t bit = 1u << ((uint32_t)at & 31u);
                    if (!TEST || !(*word & bit)) atomicOr(word, bit);
                }
                // hit groups: one sum per distinct taxon of the tile, added to the wave's entry of that taxon (lane 0 keeps them)
                uint64_t p0 = __ballot(tax[0] != 0), p1 = __ballot(tax[1] != 0);
                while (p0 | p1) {
                    const uint32_t t = p0 ? (uint32_t)__builtin_amdgcn_readlane((int)tax[0], __builtin_ctzll(p0))
                                          : (uint32_t)__builtin_amdgcn_readlane((int)tax[1], __builtin_ctzll(p1));
                    const uint64_t e0 = __ballot(tax[0] == t), e1 = __ballot(tax[1] == t);
                    if (lane == 0) {
                        const uint32_t e = t & (uint32_t)(LIST_CAP - 1);
                        const uint32_t old_t = S.list_tax[e];
                        uint32_t c = S.list_cnt[e];
                        if (old_t != t || c > 0x7FFFFFFFu) {  // another taxon's entry (or a count near its 32 bits): out it goes
                            if (c) atomicAdd(&m.groups[old_t], (unsigned long long)c);
                            c = 0;
                            S.list_tax[e] = t;
                        }
                        S.list_cnt[e] = c + (uint32_t)(__popcll(e0) + __popcll(e1));
                    }
                    p0 &= ~e0;
                    p1 &= ~e1;
                }
                wave_sync();
                w = w_next;
            }
        }
    }
    // (an entry's taxon was checked against node_count before it went in)
    const uint32_t c = S.list_cnt[lane];
    if (c) atomicAdd(&m.groups[S.list_tax[lane]], (unsigned long long)c);
}

// the cells of bitmap word i that count: its marks, without the bits at and above the capacity
__device__ __forceinline__ uint32_t word_bits(const uint32_t *marks, const uint64_t i, const uint64_t cap) {
    uint32_t bits = marks ? marks[i] : 0xFFFFFFFFu;
    const uint64_t c0 = i << 5;
    if (cap - c0 < 32u) bits &= (1u << (uint32_t)(cap - c0)) - 1u;  // (c0 < cap: the caller's loop)
    return bits;
}

template <bool LDS_BINS>
__global__ __launch_bounds__(256) void k_mdata_count(const uint32_t *table, const uint64_t cap, const uint32_t vmask, const uint32_t nodes,
                                                     const uint32_t *marks, unsigned long long *counts) {
    __shared__ uint32_t bins[LDS_BINS ? MD_LDS_BINS : 1];
    if (LDS_BINS) {
        for (uint32_t i = threadIdx.x; i < MD_LDS_BINS; i += blockDim.x) bins[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const uint64_t n_words = (cap + 31) >> 5, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4 *const t4 = reinterpret_cast<const uint4 *>(table);
    // (the loop is uniform across a wave: its lanes take 64 consecutive words)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n_words; base += stride) {
        const uint64_t i = base + (uint64_t)lane;
        const uint32_t bits = i < n_words ? word_bits(marks, i, cap) : 0u;
        uint32_t cur = 0, cnt = 0;  // global bins: the run of one value the lane is in
        if (bits) {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t nib = (bits >> (4 * j)) & 0xFu;
                if (!nib) continue;  // (the table is allocated through the next multiple of four cells: a group with a cell below cap is whole)
                const uint4 c = t4[i * 8 + j];
                const uint32_t cell[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t v = cell[k] & vmask;
                    if (!((nib >> k) & 1u) || v == 0 || v >= nodes) continue;  // not marked, empty, or no node
                    if (LDS_BINS) {
                        atomicAdd(&bins[v], 1u);
                    } else if (v == cur) {
                        cnt++;
                    } else {
                        if (cnt) atomicAdd(&counts[cur], (unsigned long long)cnt);
                        cur = v, cnt = 1;
                    }
                }
            }
        }
        if (!LDS_BINS) {
            // a table of one taxon ends every lane's word in the same run: the wave adds those up, a few values at the most
            for (int round = 0; round < 4; round++) {
                const uint64_t pend = __ballot(cnt != 0);
                if (!pend) break;
                const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)cur, __builtin_ctzll(pend));
                const bool mine = cnt != 0 && cur == t;
                const uint32_t sum = wave_sum(mine ? cnt : 0u);
                if (lane == __builtin_ctzll(pend)) atomicAdd(&counts[t], (unsigned long long)sum);
                if (mine) cnt = 0;
            }
            if (cnt) atomicAdd(&counts[cur], (unsigned long long)cnt);
        }
    }
    if (LDS_BINS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < MD_LDS_BINS && i < nodes; i += blockDim.x)
            if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
    }
}

bool mark_always_atomic() {
    static const bool v = [] {
        const char *env = getenv("NOHUMAN_MDATA_ATOMIC");
        return env && !strcmp(env, "always");
    }();
    return v;
}

}  // namespace

int mdata_check_db(const Engine *e) {
    const nh_db_info &i = e->info;
    if (i.k != 35) return set_error(NH_EDB, "minimizer data: k is %llu; the pass supports the default geometry only (k = 35)", (unsigned long long)i.k);
    if (i.l != 31) return set_error(NH_EDB, "minimizer data: l is %llu; the pass supports the default geometry only (l = 31)", (unsigned long long)i.l);
    if (i.spaced_seed_mask != SPACED_MASK)
        return set_error(NH_EDB, "minimizer data: spaced_seed_mask is 0x%llx, not the default 0x%llx", (unsigned long long)i.spaced_seed_mask,
                         (unsigned long long)SPACED_MASK);
    if (i.toggle_mask != TOGGLE_MASK)
        return set_error(NH_EDB, "minimizer data: toggle_mask is 0x%llx, not the default 0x%llx", (unsigned long long)i.toggle_mask,
                         (unsigned long long)TOGGLE_MASK);
    if (i.minimum_acceptable_hash_value != 0)
        return set_error(NH_EDB, "minimizer data: minimum_acceptable_hash_value is %llu, not 0", (unsigned long long)i.minimum_acceptable_hash_value);
    if (i.revcom_version == 0) return set_error(NH_EDB, "minimizer data: revcom_version is 0 (a legacy database)");
    if (!e->options.linear_probing) return set_error(NH_EINVAL, "minimizer data: linear_probing is 0 in the engine's options; the pass probes linearly");
    return NH_OK;
}

uint64_t mdata_mark_words(const Engine *e) { return (e->info.capacity + 31) >> 5; }

hipError_t launch_mdata_mark(Engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens, uint64_t n_frag,
                             int mates, void *d_marks, void *d_groups, hipStream_t stream) {
    if (n_frag == 0) return hipSuccess;
    KArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.db = devdb_now(e);
    ka.bases = (const uint8_t *)d_text;
    ka.seq_off = (const uint64_t *)d_seq_starts;
    ka.seq_len = (const uint32_t *)d_seq_lens;
    ka.bases_end = text_len;
    ka.n_frag = n_frag;
    ka.mates = mates;
    MarkDev m;
    m.marks = (uint32_t *)d_marks;
    m.groups = (unsigned long long *)d_groups;
    const uint64_t want = (n_frag + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    static const int per_cu = blocks_per_cu(k_mdata_mark<true>, WAVE * WAVES_PER_BLOCK, 4);
    const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)std::max(1, e->n_cu) * per_cu);
    if (mark_always_atomic()) hipLaunchKernelGGL((k_mdata_mark<false>), dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, ka, m);
    else hipLaunchKernelGGL((k_mdata_mark<true>), dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), 0, stream, ka, m);
    return hipGetLastError();
}

hipError_t launch_mdata_count(Engine *e, const void *d_marks, void *d_counts, hipStream_t stream) {
    const uint64_t cap = e->info.capacity, words = (cap + 31) >> 5;
    const uint32_t nodes = (uint32_t)e->info.node_count, vmask = (uint32_t)((1ull << e->info.value_bits) - 1);
    if (words == 0 || nodes < 2) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((words + 255) / 256, (uint64_t)std::max(1, e->n_cu) * 8);
    if (nodes <= MD_LDS_BINS)
        hipLaunchKernelGGL((k_mdata_count<true>), dim3(grid), dim3(256), 0, stream, e->d_table, cap, vmask, nodes, (const uint32_t *)d_marks,
                           (unsigned long long *)d_counts);
    else
        hipLaunchKernelGGL((k_mdata_count<false>), dim3(grid), dim3(256), 0, stream, e->d_table, cap, vmask, nodes, (const uint32_t *)d_marks,
                           (unsigned long long *)d_counts);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_minimizer_marks_bytes(const nh_engine *e_, uint64_t *bytes) {
    const nh::Engine *e = (const nh::Engine *)e_;
    if (!e || !bytes) return nh::set_error(NH_EINVAL, "null argument");
    *bytes = nh::mdata_mark_words(e) * 4;
    return NH_OK;
}

extern "C" int nh_minimizer_mark_device(nh_engine *e_, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                                        uint64_t n_frag, uint32_t flags, void *d_marks, void *d_groups, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_text || !d_seq_starts || !d_seq_lens || !d_marks || !d_groups) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_text & 3) || ((uintptr_t)d_marks & 3) || ((uintptr_t)d_groups & 7))
        return nh::set_error(NH_EINVAL, "the text and the bitmap must be 4-byte aligned, the hit-group counters 8-byte aligned");
    if (n_frag > (1ull << 32)) return nh::set_error(NH_EINVAL, "too many fragments for one launch");
    const int rc = nh::mdata_check_db(e);
    if (rc) return rc;
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    const hipError_t he = nh::launch_mdata_mark(e, d_text, text_len, d_seq_starts, d_seq_lens, n_frag, flags & NH_FLAG_PAIRED ? 2 : 1, d_marks,
                                                d_groups, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "minimizer data, mark launch: %s", hipGetErrorString(he));
    return NH_OK;
}

extern "C" int nh_minimizer_count_device(nh_engine *e_, const void *d_marks, void *d_counts, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_counts) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_marks & 3) || ((uintptr_t)d_counts & 7)) return nh::set_error(NH_EINVAL, "the bitmap must be 4-byte aligned, the counters 8-byte aligned");
    const int rc = nh::mdata_check_db(e);
    if (rc) return rc;
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    const hipError_t he = nh::launch_mdata_count(e, d_marks, d_counts, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "minimizer data, count launch: %s", hipGetErrorString(he));
    return NH_OK;
}
