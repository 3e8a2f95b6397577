// nh_dust.h -- low-complexity masking (symmetric DUST, window 64, threshold 2.0) on the device: what nh_dust.hip gives the
// builder (nh_build.hip) and nh_dust_mask.  The definition: DESIGN.md 6.10; the model: tests/dust_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace nh {

#ifndef NH_DUST_LANE_STARTS
#define NH_DUST_LANE_STARTS 16  // (a multiple of 8; `make ab-dust8` builds the library with 8, which measured 4 % slower)
#endif
constexpr int DUST_LANE_STARTS = NH_DUST_LANE_STARTS;        // consecutive starts a lane keeps in registers
constexpr uint32_t DUST_WAVE_STARTS = 64 * DUST_LANE_STARTS; // starts a wave carries through the 61 steps
constexpr uint32_t DUST_CONTEXT = 63;                        // bases on either side that decide whether a base is masked
// of a wave's starts the last 61 lose their neighbours on the way (the trapezoid) and the first 63 belong to the tile before
constexpr uint32_t DUST_TILE_BASES = DUST_WAVE_STARTS - 61 - DUST_CONTEXT;

// One wave's work: the bases [start, start + n) of the text are its own -- no other tile writes them.  `left` / `right` are the
// bases of the same segment that lie before / behind them (at most 63 each; fewer only at the segment's ends).  Of the masked
// bases those at tile offsets [cnt_lo, cnt_hi) are counted.
struct DustTile {
    uint64_t start;
    uint32_t n;
    uint8_t left, right, pad[2];
    uint32_t cnt_lo, cnt_hi;
};

// the tiles of one segment [seg_start, +seg_len) appended to `out`; masked bases at segment offsets [cnt_lo, cnt_hi) are counted
void dust_tiles(std::vector<DustTile> &out, uint64_t seg_start, uint64_t seg_len, uint64_t cnt_lo, uint64_t cnt_hi);
// blocks that fill the current device once
int dust_grid_max();
// `dst` holds a copy of src[0, text_len): every masked base of every tile becomes N in dst, their number is added to *d_count.
// src is only read, so no tile sees what another one wrote.  A tile that leaves [0, text_len) is skipped.
hipError_t launch_dust(const char *src, char *dst, uint64_t text_len, const DustTile *d_tiles, uint64_t n_tiles,
                       unsigned long long *d_count, int grid_max, hipStream_t stream);

}  // namespace nh
