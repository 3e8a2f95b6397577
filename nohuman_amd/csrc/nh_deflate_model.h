// nh_deflate_model.h -- host model of the GPU gzip / BGZF encoder (nh_deflate.hip): the file the encoder writes for a text, computed
// on a CPU from the SAME lane-level and sequential functions (nh_deflate_core.h), the wave's 64 lanes run by a loop.  Host code only,
// header only: the library's nh_gzip_model_file (nh_deflate_model.cpp) and tools/deflate_model.cpp are two front ends over it.
//
// What is mirrored, from the kernel's code:
//   k_deflate        buckets empty at a region's start; a step's look-ups before its insertions; slot (p >> 6) % WAYS; positions with
//                    a full hash context enter the buckets, parsed or not; the lazy rule on the lengths as found, lane 63 never
//                    deferring; a match at SCAN_CAP extended up to min(n - pos, 258); a block ends once 32768 bytes are parsed or at
//                    the last step; the prices are the last block's lengths, stored blocks included.
//   finish_block     symbol 256 counted once; an alphabet with fewer than two used symbols gets its first unused ones counted once
//                    (the counts stay bumped: the size estimate sees them, as the kernel's does); sort key count << 9 | symbol;
//                    stored when bits >= 8 * bytes + 40.
//   the host side    chunks of `chunk` bytes cut into regions; every region of a chunk starts from the chunk's prior lengths; chunk
//                    k + 1's priors are region 0's lengths at the end of chunk k; chunk 0's come from the pilot (the first 16 regions
//                    under both candidate sets, the smaller total wins, a tie goes to set 1) or are forced; gzip and BGZF framing.
//   past the end     the match finder ranks candidates by lengths measured up to 31 bytes past a region's end before it clips them.
//                    Inside a chunk those bytes are the next region's; behind a chunk's last region they are what the device buffer
//                    holds there: zeros, or -- the encoder has two buffers that alternate -- the bytes chunk k - 2 left at the same
//                    offsets.  chunk_tail() reproduces that, so the model needs no buffer of a chunk's size.
#pragma once
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "nh_deflate_core.h"

namespace nh {
namespace dfl {
namespace model {

constexpr uint32_t PILOT_REGIONS = 16;
constexpr uint32_t BGZF_REGION_BYTES = 65280, BGZF_HEADER_BYTES = 18;

struct Options {
    uint32_t ways = 4;             // 4, 6, 8 (16: the tool only)
    uint32_t region = 65536;       // bytes of text per region (BGZF: 65280)
    uint64_t chunk = 128ull << 20; // bytes of text per kernel launch (BGZF: cut down to whole regions)
    int prices = -1;               // -1: pilot; 0 / 1: that starting set
    bool bgzf = false;
    uint32_t threads = 0;          // 0: up to 16, fewer on a smaller machine
    uint32_t block_bytes = 32768;  // (the tool's fourth argument; the kernel's BLOCK_IN)
};
struct Stats {
    uint64_t file_bytes = 0, regions = 0, price_set = 0;
    uint64_t dynamic_blocks = 0, stored_blocks = 0;
    uint64_t repaired15 = 0, repaired7 = 0;  // blocks in which a code had to be brought under its length limit (7: dynamic blocks)
    uint64_t longest_match = 0, longest_dist = 0, extended = 0;  // extended: matches longer than SCAN_CAP
    uint64_t tokens = 0, matches = 0, match_bytes = 0, header_bits = 0;
    void add(const Stats &o) {
        dynamic_blocks += o.dynamic_blocks;
        stored_blocks += o.stored_blocks;
        repaired15 += o.repaired15;
        repaired7 += o.repaired7;
        longest_match = std::max(longest_match, o.longest_match);
        longest_dist = std::max(longest_dist, o.longest_dist);
        extended += o.extended;
        tokens += o.tokens;
        matches += o.matches;
        match_bytes += o.match_bytes;
        header_bits += o.header_bits;
    }
};

struct BitWriter {
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    uint32_t nacc = 0;
    void put(uint32_t v, uint32_t n) {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        while (nacc >= 8) {
            out.push_back((uint8_t)acc);
            acc >>= 8;
            nacc -= 8;
        }
    }
    void align() {
        if (nacc) put(0, 8 - nacc);
    }
};

struct Tree {
    uint8_t lens[NLIT];
    uint16_t codes[NLIT];
};
struct Prior {  // the code lengths a region starts from (PRIOR_BYTES of the kernel)
    uint8_t llen[NLIT], dlen[NDIST];
};
inline Prior starting_prices(int set) {
    Prior p;
    for (int s = 0; s < NLIT; s++) p.llen[s] = s < 256 ? 6 : 7;
    for (int s = 0; s < NDIST; s++) p.dlen[s] = 5;
    if (set == 1)
        for (const char *c = "ACGTN"; *c; c++) p.llen[(int)*c] = 2;
    return p;
}

// the code of one alphabet from its counts, as build_tree_wave: freq is bumped where fewer than two symbols are used.  Returns
// whether the unrestricted code was deeper than maxbits (the Kraft repair ran).
inline bool build_tree(uint32_t *freq, int nsym, int maxbits, Tree &t) {
    int used = 0;
    for (int s = 0; s < nsym; s++) used += freq[s] != 0;
    for (int s = 0; used < 2 && s < nsym; s++)  // a code needs two symbols to be complete
        if (!freq[s]) {
            freq[s] = 1;
            used++;
        }
    uint32_t keys[NLIT];
    int n = 0;
    for (int s = 0; s < nsym; s++)
        if (freq[s]) keys[n++] = (freq[s] << 9) | (uint32_t)s;
    std::sort(keys, keys + n);
    uint32_t a[NLIT], depth[NLIT];
    uint16_t ss[NLIT];
    for (int i = 0; i < n; i++) {
        a[i] = depth[i] = keys[i] >> 9;
        ss[i] = (uint16_t)(keys[i] & 511u);
    }
    huff_depths_sorted(depth, n);  // (depth[0]: the rarest symbol's, the deepest)
    huff_lengths_sorted(a, ss, n, nsym, maxbits, t.lens);
    huff_codes(t.lens, nsym, maxbits, t.codes);
    return depth[0] > (uint32_t)maxbits;
}

struct Block {
    std::vector<uint32_t> tok;
    uint32_t lfreq[NLIT], dfreq[NDIST];
    uint32_t in_from = 0;
    void reset(uint32_t from) {
        tok.clear();
        memset(lfreq, 0, sizeof lfreq);
        memset(dfreq, 0, sizeof dfreq);
        in_from = from;
    }
};

inline void emit_block(BitWriter &bw, Block &b, const uint8_t *src, uint32_t in_to, Tree &lt, Tree &dt, Stats &st) {
    b.lfreq[256]++;
    bool rep15 = build_tree(b.lfreq, NLIT_USED, MAXBITS, lt);
    rep15 |= build_tree(b.dfreq, NDIST_USED, MAXBITS, dt);
    int hlit = NLIT_USED, hdist = NDIST_USED;
    while (hlit > 257 && lt.lens[hlit - 1] == 0) hlit--;
    while (hdist > 1 && dt.lens[hdist - 1] == 0) hdist--;
    uint8_t all[NLIT + NDIST];
    for (int i = 0; i < hlit; i++) all[i] = lt.lens[i];
    for (int i = 0; i < hdist; i++) all[hlit + i] = dt.lens[i];
    uint16_t items[NLIT + NDIST];
    uint32_t clfreq[NCL];
    const int ni = rle_lengths(all, hlit + hdist, items, clfreq);
    Tree ct;
    const bool rep7 = build_tree(clfreq, NCL, MAXBITS_CL, ct);
    st.repaired15 += rep15;  // (counted for stored blocks too: their lengths are the next block's prices)
    int hclen = NCL;
    while (hclen > 4 && ct.lens[cl_order(hclen - 1)] == 0) hclen--;
    uint64_t bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
    for (int i = 0; i < ni; i++) bits += ct.lens[items[i] & 31u] + cl_extra_bits(items[i] & 31u);
    const uint64_t hdr = bits;
    for (int s = 0; s < NLIT_USED; s++) bits += (uint64_t)b.lfreq[s] * (lt.lens[s] + (s > 256 ? len_extra_bits(s) : 0));
    for (int s = 0; s < NDIST_USED; s++) bits += (uint64_t)b.dfreq[s] * (dt.lens[s] + dist_extra_bits(s));
    const uint32_t nbytes = in_to - b.in_from;
    if (bits >= 8ull * nbytes + 40) {  // stored
        st.stored_blocks++;
        bw.put(0, 3);
        bw.align();
        bw.put(nbytes & 0xFFFF, 16);
        bw.put(~nbytes & 0xFFFF, 16);
        for (uint32_t i = 0; i < nbytes; i++) bw.put(src[b.in_from + i], 8);
        return;
    }
    st.dynamic_blocks++;
    st.repaired7 += rep7;
    st.header_bits += hdr;
    bw.put(0, 1);
    bw.put(2, 2);
    bw.put(hlit - 257, 5);
    bw.put(hdist - 1, 5);
    bw.put(hclen - 4, 4);
    for (int i = 0; i < hclen; i++) bw.put(ct.lens[cl_order(i)], 3);
    for (int i = 0; i < ni; i++) {
        const uint32_t s = items[i] & 31u;
        bw.put(ct.codes[s], ct.lens[s]);
        if (cl_extra_bits(s)) bw.put(items[i] >> 5, cl_extra_bits(s));
    }
    for (uint32_t t : b.tok) {
        if (t & 0x80000000u) {
            uint32_t sym, eb, ev, dsym, deb, dev;
            len_symbol((t >> 16) & 0xFFu, sym, eb, ev);
            dist_symbol(t & 0x7FFFu, dsym, deb, dev);
            bw.put(lt.codes[sym], lt.lens[sym]);
            if (eb) bw.put(ev, eb);
            bw.put(dt.codes[dsym], dt.lens[dsym]);
            if (deb) bw.put(dev, deb);
        } else {
            bw.put(lt.codes[t], lt.lens[t]);
        }
    }
    bw.put(lt.codes[256], lt.lens[256]);
}

// One region, as one wave does it: src[0..n), readable up to n + 64 (what lies there counts: see "past the end" above).  The
// region's stream is appended to bw, which ends on a byte boundary; `prior` holds the starting lengths and, on return, those of
// the region's last block.
template <int WAYS>
inline void deflate_region(BitWriter &bw, const uint8_t *src, uint32_t n, uint32_t block_bytes, bool final_region, Prior &prior,
                           Stats &st) {
    std::vector<uint16_t> bucket((size_t)WAYS << BUCKET_BITS, (uint16_t)EMPTY_ENTRY);
    Tree lt, dt;
    memset(&lt, 0, sizeof lt);
    memset(&dt, 0, sizeof dt);
    memcpy(lt.lens, prior.llen, NLIT);
    memcpy(dt.lens, prior.dlen, NDIST);
    Block b;
    b.reset(0);
    uint32_t carry = 0;
    for (uint32_t s = 0; s < n; s += 64) {
        uint32_t L[64], D[64], H[64];
        const Costs costs{lt.lens, dt.lens};
        const bool any = carry < s + 64;
        for (uint32_t lane = 0; lane < 64; lane++) {  // every lane: hash, bucket, match
            const uint32_t p = s + lane;
            L[lane] = 0;
            D[lane] = 0;
            H[lane] = 0;
            if (p >= n) continue;
            if (p + HASH_BYTES <= n) H[lane] = hash_at(load8(src + p));
            if (!any || p < carry) continue;
            int gain = 0;
            L[lane] = find_match<WAYS>(src, p, n, load16(src + p), &bucket[WAYS * hash_bucket(H[lane])], costs, D[lane], gain);
        }
        for (uint32_t lane = 0; lane < 64; lane++) {  // the step's positions enter the buckets after the look-ups
            const uint32_t p = s + lane;
            if (p + HASH_BYTES <= n) bucket[WAYS * hash_bucket(H[lane]) + ((p >> 6) % WAYS)] = make_entry(p);
        }
        if (any) {
            for (uint32_t lane = 0; lane < 63; lane++)  // lazy rule: a longer match one position on wins (lane 63 has no neighbour)
                if (L[lane] && L[lane] < 16 && L[lane + 1] > L[lane]) L[lane] = 0;  // (L[lane + 1] as found: not yet visited)
            uint32_t q = carry > s ? carry - s : 0;
            while (q < 64 && s + q < n) {
                const uint32_t p = s + q;
                uint32_t l = L[q];
                if (l == SCAN_CAP) {
                    const uint32_t room = n - p, cap = room < MAX_MATCH ? room : MAX_MATCH;
                    l = common_prefix(src + p - D[q], src + p, SCAN_CAP, cap);
                }
                if (l) {
                    uint32_t sym, eb, ev, dsym, deb, dev;
                    len_symbol(l - 3, sym, eb, ev);
                    dist_symbol(D[q] - 1, dsym, deb, dev);
                    b.tok.push_back(tok_match(l, D[q]));
                    b.lfreq[sym]++;
                    b.dfreq[dsym]++;
                    st.matches++;
                    st.match_bytes += l;
                    st.extended += l > SCAN_CAP;
                    st.longest_match = std::max<uint64_t>(st.longest_match, l);
                    st.longest_dist = std::max<uint64_t>(st.longest_dist, D[q]);
                } else {
                    b.tok.push_back(src[p]);
                    b.lfreq[src[p]]++;
                }
                st.tokens++;
                q += l ? l : 1;
            }
            carry = s + q;
        }
        if (carry - b.in_from >= block_bytes || s + 64 >= n) {
            const uint32_t to = carry < n ? carry : n;
            emit_block(bw, b, src, to, lt, dt, st);
            b.reset(to);
        }
    }
    bw.put(final_region ? 1 : 0, 3);  // empty stored block: the region ends on a byte boundary (BGZF: and its member's stream)
    bw.align();
    bw.put(0x0000, 16);
    bw.put(0xFFFF, 16);
    memcpy(prior.llen, lt.lens, NLIT);
    memcpy(prior.dlen, dt.lens, NDIST);
}
inline void deflate_region_ways(uint32_t ways, BitWriter &bw, const uint8_t *src, uint32_t n, uint32_t block_bytes, bool final_region,
                                Prior &prior, Stats &st) {
    if (ways == 4) deflate_region<4>(bw, src, n, block_bytes, final_region, prior, st);
    else if (ways == 6) deflate_region<6>(bw, src, n, block_bytes, final_region, prior, st);
    else if (ways == 16) deflate_region<16>(bw, src, n, block_bytes, final_region, prior, st);
    else deflate_region<8>(bw, src, n, block_bytes, final_region, prior, st);
}

// the 64 bytes behind chunk k's text of `fill` bytes in the device buffer it was copied to (chunk k - 2 used that buffer before)
inline void chunk_tail(const uint8_t *text, uint64_t chunk, uint64_t k, uint64_t fill, uint8_t *tail) {
    for (uint64_t j = 0; j < 64; j++) tail[j] = (k >= 2 && fill + j < chunk) ? text[(k - 2) * chunk + fill + j] : 0;
}

// tasks 0..n_tasks-1 on up to `threads` threads; what a task writes depends on its index alone
template <typename F>
inline void run_tasks(uint32_t n_tasks, uint32_t threads, const F &task) {
    const uint32_t nt = std::min(threads, n_tasks);
    if (nt <= 1) {
        for (uint32_t i = 0; i < n_tasks; i++) task(i);
        return;
    }
    std::atomic<uint32_t> next{0};
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nt; t++)
        pool.emplace_back([&] {
            for (uint32_t i; (i = next.fetch_add(1)) < n_tasks;) task(i);
        });
    for (std::thread &t : pool) t.join();
}

inline void put_le32(std::vector<uint8_t> &out, uint32_t v) {
    for (int i = 0; i < 4; i++) out.push_back((uint8_t)(v >> (8 * i)));
}

// The whole file for text[0..n).  region_sizes (optional, region_cap entries): the bytes of every region's deflate stream, in order.
inline void encode(const uint8_t *text, uint64_t n, Options o, std::vector<uint8_t> &out, Stats &st, uint32_t *region_sizes = nullptr,
                   uint64_t region_cap = 0) {
    if (o.bgzf) {
        o.region = BGZF_REGION_BYTES;
        o.chunk -= o.chunk % o.region;
    }
    uint32_t threads = o.threads;
    if (!threads) {
        const uint32_t hw = std::thread::hardware_concurrency();
        threads = hw ? std::min(hw, 16u) : 1u;
    }
    st = Stats();
    out.clear();
    static const uint8_t gzip_header[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    if (!o.bgzf) out.insert(out.end(), gzip_header, gzip_header + 10);
    struct Region {
        std::vector<uint8_t> stream;
        Stats st;
        Prior prior;
    };
    // a chunk's regions [r0, r1) from `prior`; the last region of the chunk sees the device buffer's bytes behind it
    auto run_chunk = [&](uint64_t k, uint64_t fill, uint32_t r0, uint32_t r1, const Prior &prior, std::vector<Region> &regs) {
        const uint8_t *base = text + k * o.chunk;
        const uint32_t nr = (uint32_t)((fill + o.region - 1) / o.region);
        // (the regions that can see past the chunk's text, the last one or two, work on a copy with the buffer's bytes behind it)
        uint32_t rs = nr - 1;
        while (rs > 0 && (uint64_t)rs * o.region + 64 > fill) rs--;
        const uint64_t end_from = (uint64_t)rs * o.region;
        std::vector<uint8_t> end(base + end_from, base + fill);
        end.resize(end.size() + 64);
        chunk_tail(text, o.chunk, k, fill, end.data() + (fill - end_from));
        regs.assign(r1 - r0, Region());
        run_tasks(r1 - r0, threads, [&](uint32_t i) {
            const uint32_t r = r0 + i;
            const uint64_t from = (uint64_t)r * o.region;
            const uint32_t len = (uint32_t)std::min<uint64_t>(o.region, fill - from);
            BitWriter bw;
            regs[i].prior = prior;
            deflate_region_ways(o.ways, bw, r >= rs ? end.data() + (from - end_from) : base + from, len, o.block_bytes, o.bgzf, regs[i].prior,
                                regs[i].st);
            regs[i].stream.swap(bw.out);
        });
    };
    Prior prior = starting_prices(1);
    uint64_t n_regions = 0;
    for (uint64_t k = 0; k * o.chunk < n; k++) {
        const uint64_t fill = std::min<uint64_t>(o.chunk, n - k * o.chunk);
        const uint32_t nr = (uint32_t)((fill + o.region - 1) / o.region);
        std::vector<Region> regs;
        if (k == 0) {
            int pick = o.prices;
            if (pick != 0 && pick != 1) {  // the pilot: the first regions under both sets (regions of the chunk as it is: a pilot
                                           // region's neighbours are the real run's)
                const uint32_t np = std::min(nr, PILOT_REGIONS);
                uint64_t tot[2] = {0, 0};
                for (int c = 0; c < 2; c++) {
                    run_chunk(0, fill, 0, np, starting_prices(c), regs);
                    for (const Region &r : regs) tot[c] += r.stream.size();
                }
                pick = tot[1] <= tot[0] ? 1 : 0;
            }
            st.price_set = (uint64_t)pick;
            prior = starting_prices(pick);
        }
        run_chunk(k, fill, 0, nr, prior, regs);
        for (uint32_t r = 0; r < nr; r++) {
            const Region &g = regs[r];
            st.add(g.st);
            if (region_sizes && n_regions + r < region_cap) region_sizes[n_regions + r] = (uint32_t)g.stream.size();
            if (o.bgzf) {
                const uint64_t from = k * o.chunk + (uint64_t)r * o.region;
                const uint32_t len = (uint32_t)std::min<uint64_t>(o.region, n - from);
                const uint32_t bsize = (uint32_t)g.stream.size() + 26u - 1u;
                const uint8_t head[BGZF_HEADER_BYTES] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
                out.insert(out.end(), head, head + BGZF_HEADER_BYTES);
                out.insert(out.end(), g.stream.begin(), g.stream.end());
                put_le32(out, (uint32_t)crc32(0, text + from, len));
                put_le32(out, len);
            } else {
                out.insert(out.end(), g.stream.begin(), g.stream.end());
            }
        }
        prior = regs[0].prior;
        n_regions += nr;
    }
    if (o.bgzf) {
        static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        out.insert(out.end(), eof, eof + 28);
    } else {
        out.push_back(0x03);  // final block: fixed codes, end of block only
        out.push_back(0x00);
        uint32_t crc = 0;
        for (uint64_t at = 0; at < n; at += 1u << 30) crc = (uint32_t)crc32(crc, text + at, (uInt)std::min<uint64_t>(1u << 30, n - at));
        put_le32(out, crc);
        put_le32(out, (uint32_t)n);
    }
    st.regions = n_regions;
    st.file_bytes = out.size();
}

}  // namespace model
}  // namespace dfl
}  // namespace nh
