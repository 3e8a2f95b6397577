// deflate_model.cpp -- command-line front end of the host model of the GPU gzip encoder (nohuman_amd/csrc/nh_deflate_model.h: the
// SAME lane-level and sequential functions as the kernel, nh_deflate_core.h, with the wave's 64 lanes run by a loop; the library's
// nh_gzip_model_file is the other front end, the one the GPU tests compare the encoder with).  Used to check the format logic against
// zlib's inflate on a CPU (tests/test_deflate_core.py) and to tune the match heuristics for ratio without a GPU: unlike the library's
// entry it takes any region from 64 bytes, any block size and 16 ways.  The text is one chunk.
//   g++ -O2 -std=c++17 -I nohuman_amd/csrc tools/deflate_model.cpp -o /tmp/deflate_model -lz -lpthread
//   deflate_model <in> <out.gz> [region_bytes] [block_bytes]
// Knobs (environment, tuning only): DFL_WAYS = 4 | 6 | 8 | 16 bucket width (8), DFL_INIT = the first prices (0: literals 6 bits like
// zlib's rules assume, 1: A C G T N 2 bits, -1: the encoder's pilot chooses; 1), DFL_BGZF = 1: BGZF members, DFL_THREADS.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "nh_deflate_model.h"

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: deflate_model <in> <out.gz> [region_bytes] [block_bytes]\n");
        return 2;
    }
    namespace m = nh::dfl::model;
    m::Options o;
    o.region = argc > 3 ? (uint32_t)atol(argv[3]) : 65536u;
    o.block_bytes = argc > 4 ? (uint32_t)atol(argv[4]) : 32768u;
    o.ways = getenv("DFL_WAYS") ? (uint32_t)atoi(getenv("DFL_WAYS")) : 8u;
    o.prices = getenv("DFL_INIT") ? atoi(getenv("DFL_INIT")) : 1;
    o.bgzf = getenv("DFL_BGZF") && atoi(getenv("DFL_BGZF"));
    o.threads = getenv("DFL_THREADS") ? (uint32_t)atoi(getenv("DFL_THREADS")) : 0u;
    if (o.region > nh::dfl::MAX_REGION || o.region < 64) {
        fprintf(stderr, "region out of range\n");
        return 2;
    }
    if (o.ways != 4 && o.ways != 6 && o.ways != 8 && o.ways != 16) {
        fprintf(stderr, "DFL_WAYS: 4, 6, 8 or 16\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<uint8_t> in;
    {
        std::vector<uint8_t> buf(1 << 20);
        size_t r;
        while ((r = fread(buf.data(), 1, buf.size(), f)) > 0) in.insert(in.end(), buf.begin(), buf.begin() + r);
    }
    fclose(f);
    const size_t n = in.size();
    o.chunk = ((uint64_t)n / o.region + 1) * o.region;  // one chunk
    std::vector<uint8_t> out;
    m::Stats st;
    m::encode(in.data(), n, o, out, st);
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    fprintf(stderr,
            "in %zu out %zu ratio %.3f  price set %llu  blocks dyn %llu stored %llu (length limit repaired in %llu + %llu)  header %.1f B/block  "
            "tokens %llu matches %llu (avg len %.1f, longest %llu, farthest %llu, %llu beyond the scan cap)\n",
            n, out.size(), (double)n / out.size(), (unsigned long long)st.price_set, (unsigned long long)st.dynamic_blocks,
            (unsigned long long)st.stored_blocks, (unsigned long long)st.repaired15, (unsigned long long)st.repaired7,
            st.dynamic_blocks ? st.header_bits / 8.0 / st.dynamic_blocks : 0.0, (unsigned long long)st.tokens,
            (unsigned long long)st.matches, st.matches ? (double)st.match_bytes / st.matches : 0.0,
            (unsigned long long)st.longest_match, (unsigned long long)st.longest_dist, (unsigned long long)st.extended);
    return 0;
}
