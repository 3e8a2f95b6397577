// nh_extend.h -- what nh_extend.hip gives nh_extend_db (nh_build.hip): the table of an existing database onto the device, re-keyed
// and renumbered in place for a larger taxonomy.  DESIGN.md 6.15; the model: tests/extend_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace nh {

constexpr uint32_t EXT_REMAP_MAX = 8192;  // entries of the renumbering table a workgroup keeps in LDS

struct ExtendTable {
    uint32_t *d_table = nullptr;  // capacity cells, allocated and zero through the next multiple of four
    uint64_t capacity = 0;
    uint32_t old_vb = 0, new_vb = 0;    // new_vb >= old_vb
    std::vector<uint16_t> remap;        // internal id of the base -> internal id of the merged tree ([0] = 0); at most EXT_REMAP_MAX
    const uint32_t *d_parent = nullptr; // the merged tree (2^new_vb entries)
    int grid_max = 0;
    hipStream_t stream = nullptr;
    // results
    uint64_t non_empty = 0, shadowed = 0;
    bool bad_value = false;  // a cell whose value is 0 or no node of the base
    bool rekeyed = false;    // the table was rewritten (false: read only, the cells are what the file held)
    double seconds_rekey = 0;  // both passes and the wait between them (HIP events)
    double seconds_pass = 0;   // of it: k_ext_rekey alone
};

// the cells of hash.k2d at `path` (behind its 32-byte header) into d_table, a stretch at a time.  NH_OK, NH_EIO, NH_EDEVICE.
int ext_load_table(const char *path, uint32_t *d_table, uint64_t capacity, hipStream_t stream);
// One streaming pass: counts the non-empty cells, checks every value against the base's nodes and -- unless the value field keeps
// its width and the renumbering is the identity -- rewrites every cell as ((cell >> old_vb) >> delta) << new_vb | remap[value].
// Where the key lost bits, a second pass gives the cells of one probe run that now share a key the LCA of their values.
int ext_rekey(ExtendTable &t);

}  // namespace nh
