// nh_extend.hip -- the device side of nh_extend_db that is its own: the table of the base database into HBM, and the passes that
// turn it, in place, into a table of the merged taxonomy at the same capacity (include/nohuman_engine.h).
//
// A cell of hash.k2d is (fmix64(m) >> (32 + value_bits)) << value_bits | value and lives at or behind fmix64(m) % capacity.  With
// the capacity unchanged no cell moves.  A wider value field takes the low `delta` bits off the stored key, a renumbered taxonomy
// sends the value through a table: k_ext_rekey does both in one pass of 16 bytes a lane, the table (16-bit entries) in LDS.
//
// Shadowed cells.  Two cells of one probe run (a maximal cyclic stretch of non-empty cells) whose keys differed only in the bits
// that are gone now carry one key.  A look-up ends at the first of them it meets, and linear probing cannot delete the other (the
// home of a cell is not stored).  k_ext_shadow gives every cell of such a group the lowest common ancestor of the group's values,
// so that whichever cell a look-up meets answers for all minimizers the key now stands for; the cells stay in the table and in
// `size`.  A cell is counted as shadowed when a cell before it in its run has its key.  The group's LCA does not depend on
// which of its members have been replaced by it already, so the result does not depend on scheduling.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nh_extend.h"
#include "nh_internal.h"
#include "nohuman_engine.h"

namespace nh {
namespace {

#define EXT_TRY(expr)                                                                                                          \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) {                                                                                                \
            (void)hipGetLastError();                                                                                           \
            return set_error(_e == hipErrorOutOfMemory ? NH_EOOM : NH_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e));        \
        }                                                                                                                      \
    } while (0)

// out[0] non-empty cells, out[1] raised by a value that is 0 or no node of the base, out[2] shadowed cells
constexpr int EXT_COUNTERS = 3;

// The table is read (WRITE: and written back) four cells a lane; it is allocated, and zero, through the next multiple of four
// behind `cap`, and an empty cell stays empty.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_ext_rekey(uint32_t *table, const uint64_t cap, const uint32_t old_vb, const uint32_t delta,
                                                   const uint32_t new_vb, const uint16_t *remap, const uint32_t base_nodes,
                                                   unsigned long long *out) {
    __shared__ uint16_t lut[EXT_REMAP_MAX];
    __shared__ unsigned long long wave_sum[4];
    if (WRITE) {
        for (uint32_t i = threadIdx.x; i < EXT_REMAP_MAX; i += blockDim.x) lut[i] = i < base_nodes ? remap[i] : (uint16_t)0;
        __syncthreads();
    }
    const uint32_t old_mask = (1u << old_vb) - 1u;
    const uint64_t n4 = (cap + 3) >> 2, stride = (uint64_t)gridDim.x * blockDim.x;
    uint4 *const t4 = reinterpret_cast<uint4 *>(table);
    unsigned long long count = 0;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        uint4 c = t4[i];
        uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (w[j] == 0) continue;
            count++;
            const uint32_t v = w[j] & old_mask;
            if (v == 0 || v >= base_nodes || v >= EXT_REMAP_MAX) {
                bad = true;  // (the call fails; the cell is left as it is)
                continue;
            }
            if (WRITE) w[j] = (((w[j] >> old_vb) >> delta) << new_vb) | lut[v];
        }
        if (WRITE) t4[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = count;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&out[1], 1ull);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (s) atomicAdd(&out[0], s);
    }
}

__device__ __forceinline__ uint32_t ext_lca(const uint32_t *parent, uint32_t x, uint32_t y) {
    while (x != y) {
        if (x > y) x = parent[x];
        else y = parent[y];
    }
    return x;
}

__device__ __forceinline__ uint32_t ext_cell(const uint32_t *table, uint64_t i) {
    return __hip_atomic_load(&table[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane a cell.  A cell that finds its key in a cell before it in its run is shadowed: it walks its whole run (back to the
// empty cell before it, forward to the one behind it; both walks are cyclic and bounded by the capacity, so a run that wraps
// round the table's end or takes all of it but one cell is a run like any other), folds the values under its key into their LCA
// and writes that into every cell of the key.  Keys never change here, values only move to the group's LCA.
__global__ __launch_bounds__(256) void k_ext_shadow(uint32_t *table, const uint64_t cap, const uint32_t vb, const uint32_t *parent,
                                                    unsigned long long *out) {
    const uint32_t vmask = (1u << vb) - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long shadowed = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        const uint32_t c = ext_cell(table, i);
        if (c == 0) continue;
        const uint32_t key = c >> vb;
        bool hit = false;
        uint64_t j = i;
        for (uint64_t steps = 1; steps < cap; steps++) {
            j = j ? j - 1 : cap - 1;
            const uint32_t w = ext_cell(table, j);
            if (w == 0) break;
            if ((w >> vb) == key) {
                hit = true;
                break;
            }
        }
        if (!hit) continue;
        shadowed++;
        uint32_t lca = c & vmask;
        for (int dir = 0; dir < 2; dir++) {
            j = i;
            for (uint64_t steps = 1; steps < cap; steps++) {
                j = dir ? (j + 1 < cap ? j + 1 : 0) : (j ? j - 1 : cap - 1);
                const uint32_t w = ext_cell(table, j);
                if (w == 0) break;
                if ((w >> vb) == key) lca = ext_lca(parent, lca, w & vmask);
            }
        }
        const uint32_t cell = (key << vb) | lca;
        if (cell != c) __hip_atomic_store(&table[i], cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int dir = 0; dir < 2; dir++) {
            j = i;
            for (uint64_t steps = 1; steps < cap; steps++) {
                j = dir ? (j + 1 < cap ? j + 1 : 0) : (j ? j - 1 : cap - 1);
                const uint32_t w = ext_cell(table, j);
                if (w == 0) break;
                if ((w >> vb) == key && w != cell) __hip_atomic_store(&table[j], cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) shadowed += __shfl_xor(shadowed, d, 64);
    if ((threadIdx.x & 63) == 0 && shadowed) atomicAdd(&out[2], shadowed);
}

}  // namespace

int ext_load_table(const char *path, uint32_t *d_table, uint64_t capacity, hipStream_t stream) {
    FILE *f = fopen(path, "rb");
    if (!f) return set_error(NH_EIO, "nh_extend_db: cannot read %s: %s", path, strerror(errno));
    int rc = NH_OK;
    if (fseek(f, 32, SEEK_SET) != 0) rc = set_error(NH_EIO, "nh_extend_db: cannot read %s: %s", path, strerror(errno));
    const uint64_t step = 16ull << 20;  // cells
    std::vector<uint32_t> buf((size_t)(capacity < step ? capacity : step));
    for (uint64_t c = 0; rc == NH_OK && c < capacity; c += step) {
        const uint64_t n = capacity - c < step ? capacity - c : step;
        if (fread(buf.data(), sizeof(uint32_t), n, f) != n) {
            rc = set_error(NH_EDB, "nh_extend_db: %s is truncated: it ends inside the %llu cells of its header", path, (unsigned long long)capacity);
            break;
        }
        hipError_t he = hipMemcpyAsync(d_table + c, buf.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
        if (he == hipSuccess) he = hipStreamSynchronize(stream);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            rc = set_error(NH_EDEVICE, "nh_extend_db: copying the base table to the device: %s", hipGetErrorString(he));
        }
    }
    fclose(f);
    return rc;
}

int ext_rekey(ExtendTable &t) {
    const uint32_t base_nodes = (uint32_t)t.remap.size();
    if (base_nodes > EXT_REMAP_MAX || t.new_vb < t.old_vb || t.new_vb >= 32 || t.old_vb == 0)
        return set_error(NH_EINVAL, "nh_extend_db: %u nodes of the base at %u value bits cannot be renumbered to %u value bits", base_nodes, t.old_vb, t.new_vb);
    bool identity = t.new_vb == t.old_vb;
    for (uint32_t i = 0; i < base_nodes; i++) identity = identity && t.remap[i] == i;
    t.rekeyed = !identity;
    DevBuf<uint16_t> d_remap;  // (the three go back when the call returns, on every path: t's device is the thread's)
    DevBuf<unsigned long long> d_out;
    Events<3> ev;
    EXT_TRY(d_remap.reserve(EXT_REMAP_MAX));
    EXT_TRY(d_out.reserve(EXT_COUNTERS));
    EXT_TRY(hipMemsetAsync(d_remap, 0, (size_t)EXT_REMAP_MAX * sizeof(uint16_t), t.stream));
    EXT_TRY(hipMemcpyAsync(d_remap, t.remap.data(), (size_t)base_nodes * sizeof(uint16_t), hipMemcpyHostToDevice, t.stream));
    EXT_TRY(hipMemsetAsync(d_out, 0, EXT_COUNTERS * sizeof(unsigned long long), t.stream));
    EXT_TRY(ev.create());
    const uint64_t want = (((t.capacity + 3) >> 2) + 255) / 256;
    const unsigned grid = (unsigned)(want < (uint64_t)t.grid_max ? (want ? want : 1) : (uint64_t)t.grid_max);
    const uint32_t delta = t.new_vb - t.old_vb;
    EXT_TRY(hipEventRecord(ev[0], t.stream));
    if (identity)
        hipLaunchKernelGGL(k_ext_rekey<false>, dim3(grid), dim3(256), 0, t.stream, t.d_table, t.capacity, t.old_vb, delta, t.new_vb, d_remap,
                           base_nodes, d_out);
    else
        hipLaunchKernelGGL(k_ext_rekey<true>, dim3(grid), dim3(256), 0, t.stream, t.d_table, t.capacity, t.old_vb, delta, t.new_vb, d_remap,
                           base_nodes, d_out);
    EXT_TRY(hipGetLastError());
    EXT_TRY(hipEventRecord(ev[2], t.stream));
    unsigned long long out[EXT_COUNTERS] = {0, 0, 0};
    EXT_TRY(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, t.stream));
    EXT_TRY(hipStreamSynchronize(t.stream));
    t.non_empty = out[0];
    t.bad_value = out[1] != 0;
    if (delta > 0 && !t.bad_value) {  // (a bad value fails the call: nothing more is done to the table)
        const uint64_t want1 = (t.capacity + 255) / 256;
        const unsigned grid1 = (unsigned)(want1 < (uint64_t)t.grid_max ? (want1 ? want1 : 1) : (uint64_t)t.grid_max);
        hipLaunchKernelGGL(k_ext_shadow, dim3(grid1), dim3(256), 0, t.stream, t.d_table, t.capacity, t.new_vb, t.d_parent, d_out);
        EXT_TRY(hipGetLastError());
    }
    EXT_TRY(hipEventRecord(ev[1], t.stream));
    EXT_TRY(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, t.stream));
    EXT_TRY(hipStreamSynchronize(t.stream));
    t.shadowed = out[2];
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) t.seconds_rekey = ms * 1e-3;
    else (void)hipGetLastError();
    if (hipEventElapsedTime(&ms, ev[0], ev[2]) == hipSuccess) t.seconds_pass = ms * 1e-3;
    else (void)hipGetLastError();
    return NH_OK;
}

}  // namespace nh
