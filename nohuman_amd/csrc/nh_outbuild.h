// nh_outbuild.h -- what the builders of output text in HBM share (device only): nh_split.hip, nh_mask.hip, nh_calls.hip, nh_cover.hip.
//
// Each builder makes, per output (a mate's records, a list), one contiguous text out of pieces (records, lines) whose
// lengths are only known on the device, in three steps that are three launches on the batch's stream:
//   sizes  per block of pieces: the sum of their lengths -> blk[]                            (the builder's own kernel)
//   scan   per output, one workgroup: scan_block_sums() turns blk[] into the blocks' offsets in place and gives the
//          total; total_fits() compares it with the buffer
//   write  per block: block_offsets() makes the lengths again and scans them inside the block (s_off[]), then one wave
//          per piece writes it with wave_write(): aligned dwords of the output, 4 bytes a lane, 256 bytes a round.  A dword
//          that lies in one field of the piece comes from the builder's field_dword() (text_dword(): two aligned loads
//          and v_alignbyte, or a constant); a dword across fields is put together from four byte_at() calls; the first and
//          last partial dwords of a piece, which it shares with its neighbours, are written with byte stores.
// The kernel boundaries are the only hand-off between the launches.  The builder's loader checks that a piece's fields lie
// in the text, its write kernel that [o, o + len) lies in the buffer; nothing here loads or stores outside what it is given.
// All of it runs in blocks of OB_THREADS threads.  Everything is inlined: the builders stay separate translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nh {

constexpr int OB_THREADS = 256;
constexpr int OB_WAVES = OB_THREADS / 64;

__device__ __forceinline__ uint32_t decimal_digits(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}

// exclusive scan over the block's threads (OB_THREADS) of one value each; *total: the block's sum.  wsum: OB_WAVES words of
// LDS, written here: a __syncthreads() lies between two calls with the same wsum
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int w = 0; w < OB_WAVES; w++) {
        before += w < wave ? wsum[w] : 0;
        all += wsum[w];
    }
    *total = all;
    return before + incl - v;
}

// one workgroup: the block sums b[0, nblk) -> their exclusive scan, in place, OB_THREADS at a time; returns the total
__device__ __forceinline__ uint64_t scan_block_sums(uint64_t *b, uint64_t nblk, uint64_t *wsum) {
    uint64_t carry = 0;
    for (uint64_t c = 0; c < nblk; c += OB_THREADS) {
        const uint64_t i = c + threadIdx.x;
        const uint64_t v = i < nblk ? b[i] : 0;
        uint64_t sum;
        const uint64_t ex = block_exclusive_scan(v, wsum, &sum);
        if (i < nblk) b[i] = carry + ex;
        carry += sum;
        __syncthreads();  // (wsum is written again by the next chunk, or by the caller)
    }
    return carry;
}

// the scan's verdict, by one thread: a total above the buffer sets `bit` of the error word; false: nothing is to be written
__device__ __forceinline__ bool total_fits(uint64_t total, uint64_t cap, int *error, int bit) {
    if (total <= cap) return true;
    atomicOr(error, bit);
    return false;
}

// s_off[i] = the offset of piece i in its block's text, for the OB_THREADS * PER_THREAD pieces of the block: thread t makes
// the lengths len_of(t * PER_THREAD + j) again.  s_off is valid on return
template <int PER_THREAD, class LenOf>
__device__ __forceinline__ void block_offsets(uint64_t *s_off, uint64_t *wsum, LenOf len_of) {
    uint64_t len[PER_THREAD], mine = 0;
    for (int j = 0; j < PER_THREAD; j++) {
        len[j] = len_of(threadIdx.x * PER_THREAD + j);
        mine += len[j];
    }
    uint64_t total;
    uint64_t o = block_exclusive_scan(mine, wsum, &total);
    for (int j = 0; j < PER_THREAD; j++) {
        s_off[threadIdx.x * PER_THREAD + j] = o;
        o += len[j];
    }
    __syncthreads();
}

// the 4 text bytes at src (src + 3 < ntext): two aligned loads, the second only where the bytes reach into it
__device__ __forceinline__ uint32_t text_dword(const char *text, uint64_t src) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(text + (src & ~3ull));
    const uint32_t sh = (uint32_t)(src & 3);
    const uint32_t lo = w[0];
    if (sh == 0) return lo;
    return __builtin_amdgcn_alignbyte(w[1], lo, sh);
}

// Mate 1's id of fragment f, as every read list prints it: from the byte behind '@' / '>' of the header (rec: the run's record table,
// {header start, header length, ...} a sequence; mates sequences a fragment) for the id length the reader found (idlen[f]: up to the
// first space, tab or '\r'); a paired run drops a trailing "/1" or "/2" from an id longer than two bytes (kraken2 TrimPairInfo).
// false: the header lies outside the text, or the id is longer than its header -- nothing of the text is read then
__device__ __forceinline__ bool read_id(const char *text, uint64_t ntext, const uint32_t *rec, const uint32_t *idlen, uint64_t f, int mates, uint64_t *id,
                                        uint32_t *idl_out) {
    const uint2 hr = reinterpret_cast<const uint2 *>(rec)[2 * f * (uint64_t)mates];  // {header start, header length} of mate 1
    const uint64_t h = hr.x, hlen = hr.y;
    uint32_t idl = idlen[f];
    if (!(h + hlen <= ntext && (uint64_t)idl + 1 <= hlen)) return false;
    const uint64_t at = h + 1;
    if (mates == 2 && idl > 2 && text[at + idl - 2] == '/' && (text[at + idl - 1] == '1' || text[at + idl - 1] == '2')) idl -= 2;
    *id = at, *idl_out = idl;
    return true;
}

// One wave writes the piece out[o, o + len) (inside the buffer: the caller checked).  byte_at(p): byte p of the piece;
// field_dword(p, &v): whether bytes [p, p + 4) of the piece lie in one of its fields, and then v, the four of them
template <class ByteAt, class FieldDword>
__device__ __forceinline__ void wave_write(char *out, uint64_t o, uint64_t len, int lane, ByteAt byte_at, FieldDword field_dword) {
    const uint64_t end = o + len;
    for (uint64_t D = (o & ~3ull) + 4ull * lane; D < end; D += 256) {
        if (D >= o && D + 4 <= end) {
            const uint64_t p = D - o;
            uint32_t v;
            if (!field_dword(p, &v))
                v = (uint32_t)byte_at(p) | (uint32_t)byte_at(p + 1) << 8 | (uint32_t)byte_at(p + 2) << 16 | (uint32_t)byte_at(p + 3) << 24;
            *reinterpret_cast<uint32_t *>(out + D) = v;
        } else {  // the piece's first or last dword: its neighbours own the other bytes
            for (uint64_t x = D; x < D + 4; x++)
                if (x >= o && x < end) out[x] = (char)byte_at(x - o);
        }
    }
}

}  // namespace nh
