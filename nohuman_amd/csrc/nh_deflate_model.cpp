// nh_deflate_model.cpp -- nh_gzip_model_file: the host model of the GPU gzip / BGZF encoder (nh_deflate_model.h) behind the ABI, so
// that tests compare the encoder's files with it byte for byte wherever the library is.  Test / tool support; needs no GPU.
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>

#include "nh_deflate_model.h"
#include "nh_internal.h"
#include "nohuman_engine.h"

extern "C" int nh_gzip_model_file(const void *in, uint64_t n, const char *out_path, const nh_gzip_model_opts *opts, uint64_t *stats12) {
    namespace m = nh::dfl::model;
    if ((!in && n) || !out_path || !opts) return nh::set_error(NH_EINVAL, "nh_gzip_model_file: null argument");
    if (opts->ways != 4 && opts->ways != 6 && opts->ways != 8) return nh::set_error(NH_EINVAL, "nh_gzip_model_file: ways must be 4, 6 or 8");
    if (opts->prices < -1 || opts->prices > 1) return nh::set_error(NH_EINVAL, "nh_gzip_model_file: prices must be -1, 0 or 1");
    m::Options o;
    o.ways = opts->ways;
    // (rounded as the encoder rounds NOHUMAN_GZIP_REGION)
    const uint64_t rb = opts->region_bytes;
    o.region = (uint32_t)(rb < 4096 ? 4096 : rb > nh::dfl::MAX_REGION ? nh::dfl::MAX_REGION : (rb & ~63ull));
    o.bgzf = opts->bgzf != 0;
    if (o.bgzf) o.region = m::BGZF_REGION_BYTES;
    o.chunk = opts->chunk_bytes;
    if (o.chunk < o.region) return nh::set_error(NH_EINVAL, "nh_gzip_model_file: chunk_bytes must be at least the region's %u bytes", o.region);
    o.prices = opts->prices;
    o.threads = opts->threads;
    std::vector<uint8_t> file;
    m::Stats st;
    try {
        m::encode((const uint8_t *)in, n, o, file, st, opts->region_sizes, opts->region_sizes_cap);
    } catch (const std::exception &e) {
        return nh::set_error(NH_EOOM, "nh_gzip_model_file: %s", e.what());
    }
    int fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return nh::set_error(NH_EIO, "cannot create %s", out_path);
    bool ok = true;
    for (size_t at = 0; ok && at < file.size();) {
        const ssize_t w = ::write(fd, file.data() + at, file.size() - at);
        if (w < 0 && errno != EINTR) ok = false;
        if (w > 0) at += (size_t)w;
    }
    if (::close(fd) != 0 || !ok) return nh::set_error(NH_EIO, "write error on %s", out_path);
    if (stats12) {
        const uint64_t v[12] = {st.file_bytes, st.regions, st.price_set, st.dynamic_blocks, st.stored_blocks, st.repaired15,
                                st.repaired7, st.longest_match, st.longest_dist, st.extended, st.tokens, st.matches};
        for (int i = 0; i < 12; i++) stats12[i] = v[i];
    }
    return NH_OK;
}
