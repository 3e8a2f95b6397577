// nh_dust.h -- low-complexity masking (symmetric DUST, window 64, threshold 2.0) on the device: what nh_dust.hip gives the
// builder (nh_build.hip) and nh_dust_mask, and the runs with --dust-reads (nh_run.hip) and nh_dust_reads_device.  The definition:
// DESIGN.md 6.10 and 6.18; the model: tests/dust_model.py.
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


// The reads of one batch masked each on its own (k_rdust; nh_run_dust, nh_dust_reads_device): `out`, a buffer with the layout of
// the text that already holds the sequences (a copy of the text, or the quality mask's output), gets 'N' at every masked base
// of every sequence text[seq_off[i], +seq_len[i]); nothing else of it is written, the text is only read.
struct ReadDustArgs {
    const char *text;         // the batch's text (d_text), ntext bytes
    uint64_t ntext;
    const uint64_t *seq_off;  // n sequence starts (absolute), in any order
    const uint32_t *seq_len;  // n sequence lengths
    uint64_t n;               // sequences, at most 2^31
    char *out;                // ntext bytes
    unsigned long long *masked;  // NULL or one counter the waves add their masked bases to
    int *error;               // the engine's sticky error word (bit 512: a sequence that leaves the text; it is skipped)
    uint64_t nblk, *blk, *loc;   // (launch_read_dust's: the scratch, cut)
};
// words of scratch a launch over n sequences needs
uint64_t read_dust_scratch_words(uint64_t n);
// blocks of k_rdust that fill the current device once
int read_dust_grid_max();
// three launches on `stream`: the offsets of the sequences in the virtual text (two), the mask
hipError_t launch_read_dust(ReadDustArgs a, uint64_t *scratch, int grid_max, hipStream_t stream);

}  // namespace nh
