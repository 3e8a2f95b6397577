// nh_host.hip -- the host selection (--host-taxid / --keep-taxid, nh_run_host): which classified fragments count as host.
//
// The table (host side).  One byte per node of the taxonomy, internal id: 1 where the deepest listed taxon that is the node or an
// ancestor of it is a HOST taxid, 0 where it is a KEEP taxid or no listed taxon lies above the node; entry 0 (unclassified) is 0.
// nh_open guarantees that parents lie below their children, so one pass from the root down fills it: a listed node takes its own
// list's value, any other node its parent's.  The same pass fills the per-taxon builder's bin_of (nh_run.hip).
//
// k_host_filter (device), behind the classifier on the slot's stream: a thread per fragment loads the 16-byte nh_result as one
// dwordx4, looks host_of[call] up -- n_nodes bytes, a few kilobytes for a host database, cache-resident for a standard one -- and
// stores the record to a second array with call = 0 where the fragment is not host; words 1-3 go through untouched.  The builders
// that remove, keep, mask, list or count host reads (nh_split, nh_mask, nh_calls' id list, nh_rstats) then read that array with
// the test they always had, call != 0, and are not edited; whatever reports the call keeps reading the classifier's array.
// out == in is allowed (a thread reads and writes its own record only).  Host and spared fragments are counted per wave with a
// ballot and added with one 64-bit atomic a workgroup and counter: every workgroup of a launch adds to the same two words, and
// atomics on one word are served one after the other, so the workgroup is the largest there is (1024 threads, 21 VGPRs: full
// occupancy) -- with 256 threads the 7800 atomics of a million fragments WERE the kernel's time (97 us; profiles/host_taxid.txt).
// A call >= n_nodes -- nothing the classifier writes: its values come from a table nh_open checked against the node count -- is
// never used as an index: the record gets call 0, is counted nowhere, and bit 128 of the engine's error word fails the next
// blocking call.
// The pass moves 32 bytes a fragment, 80 MB for 2.5 M fragments, beside the classifier's milliseconds (profiles/host_taxid.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "nh_internal.h"

namespace nh {

namespace {

constexpr int HF_THREADS = 1024;  // the largest workgroup: the fewest atomics on the two counters (a workgroup adds once to each)
constexpr int HF_WAVES = HF_THREADS / 64;
constexpr int ERR_HOST = 128;

__global__ void __launch_bounds__(HF_THREADS) k_host_filter(const uint4 *in, uint4 *out, uint64_t n, const uint8_t *host_of, uint64_t n_nodes,
                                                            unsigned long long *counts, int *error) {
    __shared__ uint32_t s_host[HF_WAVES], s_spared[HF_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * HF_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool host = false, spared = false, bad = false;
    if (i < n) {
        uint4 r = in[i];
        const uint32_t call = r.x;
        if ((uint64_t)call >= n_nodes) bad = true;  // (never an index)
        else if (call) host = host_of[call] != 0, spared = !host;
        if (!host) r.x = 0;
        out[i] = r;
    }
    if (__ballot(bad) && lane == 0) atomicOr(error, ERR_HOST);
    if (!counts) return;  // (the same for every thread of the launch)
    const unsigned long long bh = __ballot(host), bs = __ballot(spared);
    if (lane == 0) s_host[wave] = (uint32_t)__popcll(bh), s_spared[wave] = (uint32_t)__popcll(bs);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t h = 0, s = 0;
        for (int w = 0; w < HF_WAVES; w++) h += s_host[w], s += s_spared[w];
        if (h) atomicAdd(&counts[0], (unsigned long long)h);
        if (s) atomicAdd(&counts[1], (unsigned long long)s);
    }
}

inline uint64_t rd64(const uint8_t *p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

// the table of a taxonomy of nn nodes given by two accessors (internal id -> parent's internal id / external id)
template <class Parent, class External>
int fill_host_table(uint64_t nn, Parent parent, External external, const nh_host_filter *hf, uint8_t *host_of) {
    std::vector<uint8_t> own(nn, 0);  // 1: a host taxid, 2: a keep taxid
    for (uint32_t k = 0; k < hf->n_host + hf->n_keep; k++) {
        const uint64_t taxid = k < hf->n_host ? hf->host_taxids[k] : hf->keep_taxids[k - hf->n_host];
        uint64_t at = 0;
        for (uint64_t i = 1; i < nn && !at; i++)
            if (external(i) == taxid) at = i;
        if (!at) return set_error(NH_EINVAL, "nh_run_host: taxid %llu is not in the database's taxonomy", (unsigned long long)taxid);
        own[at] = k < hf->n_host ? 1 : 2;
    }
    if (nn) host_of[0] = 0;
    for (uint64_t i = 1; i < nn; i++) {  // (parents have smaller ids than their children)
        const uint64_t p = parent(i);
        host_of[i] = own[i] ? (uint8_t)(own[i] == 1) : (i > 1 && p >= 1 && p < i) ? host_of[p] : (uint8_t)0;
    }
    return NH_OK;
}

}  // namespace

// (a struct too small to hold the counts is given too: check_host_filter refuses it)
bool host_filter_given(const nh_host_filter *hf) { return hf && (hf->struct_size < sizeof(nh_host_filter) || hf->n_host || hf->n_keep); }

int check_host_filter(const nh_host_filter *hf) {
    if (!hf) return NH_OK;
    if (hf->struct_size < sizeof(nh_host_filter))
        return set_error(NH_EINVAL, "nh_run_host: struct_size %u is smaller than nh_host_filter (%zu bytes)", hf->struct_size, sizeof(nh_host_filter));
    if (hf->n_keep && !hf->n_host) return set_error(NH_EINVAL, "nh_run_host: keep taxids are given without a host taxid (n_keep %u, n_host 0)", hf->n_keep);
    if ((uint64_t)hf->n_host + hf->n_keep > NH_MAX_HOST_TAXA)
        return set_error(NH_EINVAL, "nh_run_host: %llu taxids are more than the %d a selection takes (host and keep together)",
                         (unsigned long long)hf->n_host + hf->n_keep, NH_MAX_HOST_TAXA);
    if ((hf->n_host && !hf->host_taxids) || (hf->n_keep && !hf->keep_taxids)) return set_error(NH_EINVAL, "nh_run_host: a null list of taxids with a count that is not 0");
    const uint32_t n = hf->n_host + hf->n_keep;
    auto at = [&](uint32_t k) { return k < hf->n_host ? hf->host_taxids[k] : hf->keep_taxids[k - hf->n_host]; };
    for (uint32_t k = 0; k < n; k++) {
        if (at(k) == 0) return set_error(NH_EINVAL, "nh_run_host: taxid 0 is not a taxon (a %s taxid)", k < hf->n_host ? "host" : "keep");
        for (uint32_t j = 0; j < k; j++)
            if (at(j) == at(k)) return set_error(NH_EINVAL, "nh_run_host: taxid %llu is given twice", (unsigned long long)at(k));
    }
    return NH_OK;
}

int host_table(const Engine *e, const nh_host_filter *hf, std::vector<uint8_t> &host_of) {
    const uint64_t nn = e->external.size();
    host_of.assign(std::max<uint64_t>(nn, 1), 0);
    return fill_host_table(nn, [&](uint64_t i) { return (uint64_t)e->parent[i]; }, [&](uint64_t i) { return e->external[i]; }, hf, host_of.data());
}

hipError_t launch_host_filter(const void *d_in, void *d_out, uint64_t n, const uint8_t *d_host_of, uint64_t n_nodes, unsigned long long *d_counts,
                              int *d_error, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + HF_THREADS - 1) / HF_THREADS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_host_filter, dim3((unsigned)blocks), dim3(HF_THREADS), 0, stream, (const uint4 *)d_in, (uint4 *)d_out, n, d_host_of, n_nodes,
                       d_counts, d_error);
    return hipGetLastError();
}

}  // namespace nh

extern "C" int nh_host_table_image(const void *taxo, size_t taxo_len, const nh_host_filter *hf, uint8_t *host_of, uint64_t cap, uint64_t *n_nodes) {
    if (!taxo || !hf || !host_of) return nh::set_error(NH_EINVAL, "null argument");
    const int crc = nh::check_host_filter(hf);
    if (crc) return crc;
    const uint8_t *tb = (const uint8_t *)taxo;
    if (taxo_len < 32 || memcmp(tb, "K2TAXDAT", 8) != 0) return nh::set_error(NH_EDB, "taxo.k2d: bad magic");
    const uint64_t nc = nh::rd64(tb + 8), nl = nh::rd64(tb + 16), rl = nh::rd64(tb + 24);
    if (nc == 0 || nc > 0xFFFFFFF0ull || nl > taxo_len || rl > taxo_len || taxo_len != 32 + 56 * nc + nl + rl)
        return nh::set_error(NH_EDB, "taxo.k2d: size does not match its header");
    if (n_nodes) *n_nodes = nc;
    if (cap < nc) return nh::set_error(NH_EINVAL, "nh_host_table_image: the table has room for %llu nodes, the taxonomy has %llu", (unsigned long long)cap, (unsigned long long)nc);
    for (uint64_t i = 1; i < nc; i++)
        if (nh::rd64(tb + 32 + 56 * i) >= i)
            return nh::set_error(NH_EDB, "taxo.k2d: parent id %llu of node %llu is not below it", (unsigned long long)nh::rd64(tb + 32 + 56 * i), (unsigned long long)i);
    return nh::fill_host_table(nc, [&](uint64_t i) { return nh::rd64(tb + 32 + 56 * i); }, [&](uint64_t i) { return nh::rd64(tb + 32 + 56 * i + 40); }, hf, host_of);
}

extern "C" int nh_host_filter_device(nh_engine *e_, const void *d_res_in, void *d_res_out, uint64_t n, const void *d_host_of, uint64_t n_nodes,
                                     void *d_counts, void *stream) {
    nh::Engine *e = (nh::Engine *)e_;
    if (!e || !d_res_in || !d_res_out || !d_host_of) return nh::set_error(NH_EINVAL, "null argument");
    if (((uintptr_t)d_res_in | (uintptr_t)d_res_out) & 15) return nh::set_error(NH_EINVAL, "the result arrays must be 16-byte aligned");
    if ((uintptr_t)d_counts & 7) return nh::set_error(NH_EINVAL, "the counters must be 8-byte aligned");
    if (n > (1ull << 38)) return nh::set_error(NH_EINVAL, "too many fragments for one launch");
    if (nh::dev_set(e->device) != hipSuccess) return nh::set_error(NH_EDEVICE, "hipSetDevice failed");
    const hipError_t he = nh::launch_host_filter(d_res_in, d_res_out, n, (const uint8_t *)d_host_of, n_nodes, (unsigned long long *)d_counts,
                                                 e->d_error + nh::LAUNCH_SLOTS, (hipStream_t)stream);
    if (he != hipSuccess) return nh::set_error(NH_EDEVICE, "host filter launch: %s", hipGetErrorString(he));
    return NH_OK;
}
