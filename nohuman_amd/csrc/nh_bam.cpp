// nh_bam.cpp -- the host side of BAM input (nh_bam.h): the record chain, the scalar transcoder, nh_bam_scan and BamReader.
// With NH_BAM_HOST_ONLY only what needs neither HIP nor the other readers is built (the stand-alone scan of tools/bam_scan_main.cpp).
#include "nh_bam.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>

namespace nh {

namespace {

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

const char BAM_ALPHABET[] = "=ACMGRSVTWYHKDBN";
// the IUPAC complement in BAM's code is the 4-bit reversal of the nibble
inline uint32_t rev4(uint32_t n) { return (n & 1) << 3 | (n & 2) << 1 | (n & 4) >> 1 | (n & 8) >> 3; }

}  // namespace

int BamStream::ensure(size_t n, std::string &err) {
    while (len_ - pos_ < n) {
        if (eof_) return 0;
        if (win_.size() < len_ + chunk) win_.resize(len_ + chunk + (win_.size() >> 1));
        const long got = read_(win_.data() + len_, chunk);
        if (got < 0) {
            err = name_ + ": read error";
            return -1;
        }
        if (got == 0) eof_ = true;
        len_ += (size_t)got;
    }
    return 1;
}

void BamStream::compact() {
    if (pos_ == 0) return;
    if (len_ > pos_) memmove(win_.data(), win_.data() + pos_, len_ - pos_);
    len_ -= pos_;
    pos_ = 0;
}

int BamStream::read_header(std::string &err) {
    header_.clear();
    size_t kept = pos_;  // the header's bytes up to here are in header_
    auto keep = [&] {
        header_.append((const char *)win_.data() + kept, pos_ - kept);
        kept = pos_;
    };
    auto need = [&](size_t n) -> int {
        const int rc = ensure(n, err);
        if (rc == 0) err = name_ + ": the BAM stream ends inside the header";
        return rc == 1 ? 0 : -1;
    };
    if (need(8)) return -1;
    if (memcmp(win_.data() + pos_, "BAM\1", 4) != 0) {
        err = name_ + ": not a BAM stream (no BAM\\1 magic)";
        return -1;
    }
    const int32_t l_text = (int32_t)le32(win_.data() + pos_ + 4);
    if (l_text < 0) {
        err = fmt("%s: BAM header: negative l_text (%d)", name_.c_str(), l_text);
        return -1;
    }
    pos_ += 8;
    if (need((size_t)l_text + 4)) return -1;
    pos_ += (size_t)l_text;
    const int32_t n_ref = (int32_t)le32(win_.data() + pos_);
    if (n_ref < 0) {
        err = fmt("%s: BAM header: negative n_ref (%d)", name_.c_str(), n_ref);
        return -1;
    }
    pos_ += 4;
    for (int32_t i = 0; i < n_ref; i++) {
        if (need(4)) return -1;
        const int32_t l_name = (int32_t)le32(win_.data() + pos_);
        if (l_name < 0) {
            err = fmt("%s: BAM header: reference %d has a negative l_name (%d)", name_.c_str(), i, l_name);
            return -1;
        }
        pos_ += 4;
        if (need((size_t)l_name + 4)) return -1;
        pos_ += (size_t)l_name + 4;
        if (pos_ > (8u << 20)) {
            keep();
            compact();
            kept = 0;
        }
    }
    keep();
    return 0;
}

bool bam_name_fields(const uint8_t *name, uint32_t n, uint32_t *hlen, uint32_t *idlen) {
    uint32_t e = n;
    while (e > 0 && strchr(" \t\n\v\f\r", name[e - 1]) && name[e - 1]) e--;
    if (e == 0 || memchr(name, '\n', n)) return false;
    uint32_t i = 0;
    while (i < e && name[i] != ' ' && name[i] != '\t' && name[i] != '\r') i++;
    *hlen = 1 + e;
    *idlen = i;
    return true;
}

// the refusal of a 0x1 record in a single-end file
int BamStream::refuse_paired(uint64_t ord, const char *name, int name_len, std::string &err) {
    err = fmt("%s: BAM record %llu (%.*s) is paired (flag 0x1) in a single-end BAM file (its first kept record has no flag 0x1): a paired BAM "
              "begins with a pair and holds nothing but collated pairs; or split the mates with `samtools fastq -1 R1.fq -2 R2.fq` and give both files",
              name_.c_str(), (unsigned long long)ord, name_len, name);
    return -1;
}

// a kept record of a paired file: the first of its pair is remembered, the second is held against it; -1: it breaks the chain
int BamStream::chain_pair(const BamRec &x, const uint8_t *name, std::string &err) {
    const unsigned long long ord = (unsigned long long)x.ordinal;
    const int nl = (int)x.name_len();
    if (!(x.flag & 0x1)) {
        err = fmt("%s: BAM record %llu (%.*s) is not paired (no flag 0x1) in a paired BAM file: every kept record of a paired BAM is a mate", name_.c_str(),
                  ord, nl, (const char *)name);
        return -1;
    }
    if (((x.flag & 0x40) != 0) == ((x.flag & 0x80) != 0)) {
        err = fmt("%s: BAM record %llu (%.*s) has %s of the flags 0x40 and 0x80: a mate is the first or the second of its pair", name_.c_str(), ord, nl,
                  (const char *)name, x.flag & 0x40 ? "both" : "neither");
        return -1;
    }
    if (!half_) {
        half_ = true;
        half_ord_ = x.ordinal;
        half_flag_ = x.flag;
        half_name_.assign((const char *)name, (size_t)nl);
        return 0;
    }
    if (half_name_.size() != (size_t)nl || memcmp(half_name_.data(), name, (size_t)nl) != 0) {
        err = fmt("%s: BAM record %llu (%.*s) follows record %llu (%s), which has another name and no mate: the file is not collated -- the two mates "
                  "of a pair must be neighbours (`samtools collate`)",
                  name_.c_str(), ord, nl, (const char *)name, (unsigned long long)half_ord_, half_name_.c_str());
        return -1;
    }
    if ((half_flag_ & 0xC0) == (x.flag & 0xC0)) {
        err = fmt("%s: BAM record %llu (%.*s) and record %llu are both mate %d of their pair (flag 0x%x)", name_.c_str(), ord, nl, (const char *)name,
                  (unsigned long long)half_ord_, x.flag & 0x40 ? 1 : 2, x.flag & 0xC0);
        return -1;
    }
    half_ = false;
    return 0;
}

int BamStream::next_pair(BamRec *a, BamRec *b, std::string &err) {
    int rc = next(a, err);
    if (rc != 1) return rc;
    holding = true;  // (*a points into the window: a stretch of skipped records in front of its mate does not compact it)
    rc = next(b, err);
    if (rc == 0) err = name_ + ": the BAM stream ends inside a pair";  // (unreachable: next() refuses the record without a partner)
    return rc == 1 ? 1 : -1;
}

int BamStream::next(BamRec *r, std::string &err) {
    for (;;) {
        const uint64_t ord = cnt_.records + 1;
        int rc = ensure(4, err);
        if (rc < 0) return -1;
        if (rc == 0) {
            if (len_ == pos_) {
                // (a file without a kept record is single-end: a 0x1 record among the skipped ones is refused as ever)
                if (!mode_known_ && early_ord_) return refuse_paired(early_ord_, early_name_.data(), (int)early_name_.size(), err);
                if (half_) {
                    err = fmt("%s: BAM record %llu (%s) is the last kept record and has no mate: the file is not collated, or a mate is missing or empty "
                              "(`samtools collate`)",
                              name_.c_str(), (unsigned long long)half_ord_, half_name_.c_str());
                    return -1;
                }
                return 0;
            }
            err = fmt("%s: the BAM stream ends inside record %llu", name_.c_str(), (unsigned long long)ord);
            return -1;
        }
        const int32_t block_size = (int32_t)le32(win_.data() + pos_);
        if (block_size < 32) {
            err = fmt("%s: BAM record %llu: block_size %d is smaller than the 32 bytes of its fixed part", name_.c_str(), (unsigned long long)ord,
                      block_size);
            return -1;
        }
        rc = ensure(36, err);
        if (rc < 0) return -1;
        if (rc == 0) {
            err = fmt("%s: the BAM stream ends inside record %llu", name_.c_str(), (unsigned long long)ord);
            return -1;
        }
        const uint8_t *p = win_.data() + pos_;
        BamRec x;
        x.off = pos_;
        x.block_size = (uint32_t)block_size;
        x.l_read_name = p[12];
        x.n_cigar = le16(p + 16);
        x.flag = le16(p + 18);
        x.l_seq = le32(p + 20);
        x.ordinal = ord;
        if (x.l_read_name == 0) {
            err = fmt("%s: BAM record %llu: l_read_name is 0", name_.c_str(), (unsigned long long)ord);
            return -1;
        }
        const uint64_t fields = 32ull + x.l_read_name + 4ull * x.n_cigar + ((uint64_t)x.l_seq + 1) / 2 + x.l_seq;
        if ((uint64_t)x.block_size < fields) {
            err = fmt("%s: BAM record %llu: block_size %d is smaller than its fields (%llu bytes: l_read_name %u, n_cigar_op %u, l_seq %u)",
                      name_.c_str(), (unsigned long long)ord, block_size, (unsigned long long)fields, x.l_read_name, x.n_cigar, x.l_seq);
            return -1;
        }
        rc = ensure(4 + (size_t)x.block_size, err);
        if (rc < 0) return -1;
        if (rc == 0) {
            err = fmt("%s: the BAM stream ends inside record %llu", name_.c_str(), (unsigned long long)ord);
            return -1;
        }
        p = win_.data() + pos_;
        if (p[36 + x.l_read_name - 1] != 0) {
            err = fmt("%s: BAM record %llu: the read name is not NUL-terminated", name_.c_str(), (unsigned long long)ord);
            return -1;
        }
        const bool is_kept = !(x.flag & 0x900) && x.l_seq != 0;
        if (x.flag & 0x1) {
            if (mode_known_ && !paired_) return refuse_paired(ord, (const char *)p + 36, (int)x.name_len(), err);
            if (!mode_known_ && !is_kept && !early_ord_) {  // (refused once the first kept record shows a single-end file)
                early_ord_ = ord;
                early_name_.assign((const char *)p + 36, x.name_len());
            }
        }
        if (is_kept && !mode_known_) {
            if (!(x.flag & 0x1) && early_ord_) return refuse_paired(early_ord_, early_name_.data(), (int)early_name_.size(), err);
            mode_known_ = true;
            paired_ = (x.flag & 0x1) != 0;
        }
        cnt_.records++;
        pos_ += 4 + (size_t)x.block_size;
        if (x.flag & 0x900) cnt_.skipped_secondary++;
        else if (x.l_seq == 0) cnt_.skipped_empty++;
        else {
            uint32_t hlen, idlen;
            if (x.text_len() > 0xFFFFFFF0ull) {
                err = fmt("%s: BAM record %llu: its FASTQ text (%llu bytes) cannot be addressed with a batch's 32-bit offsets", name_.c_str(),
                          (unsigned long long)ord, (unsigned long long)x.text_len());
                return -1;
            }
            if (!bam_name_fields(p + 36, x.name_len(), &hlen, &idlen)) {
                err = fmt("%s: BAM record %llu: the read name cannot stand in a FASTQ header line (empty, blank or with a line feed)", name_.c_str(),
                          (unsigned long long)ord);
                return -1;
            }
            if (paired_ && chain_pair(x, p + 36, err)) return -1;
            cnt_.reads++;
            cnt_.bases += x.l_seq;
            if (x.flag & 0x10) cnt_.reverse_complemented++;
            if (p[x.qual() - x.off] == 0xFF) cnt_.missing_qualities++;
            *r = x;
            return 1;
        }
        if (!holding && pos_ > (8u << 20)) compact();  // (a stretch of skipped records: nobody points into the window)
    }
}

void bam_transcode(const uint8_t *bam, const BamRec &r, char *out) {
    const uint32_t n = r.name_len(), L = r.l_seq;
    const uint8_t *seq = bam + r.seq(), *qual = bam + r.qual();
    const bool rev = (r.flag & 0x10) != 0, noq = qual[0] == 0xFF;
    char *o = out;
    *o++ = '@';
    memcpy(o, bam + r.name(), n);
    o += n;
    *o++ = '\n';
    for (uint32_t j = 0; j < L; j++) {
        const uint32_t k = rev ? L - 1 - j : j;
        const uint32_t nib = (k & 1) ? seq[k >> 1] & 15u : seq[k >> 1] >> 4;
        *o++ = BAM_ALPHABET[rev ? rev4(nib) : nib];
    }
    *o++ = '\n';
    *o++ = '+';
    *o++ = '\n';
    for (uint32_t j = 0; j < L; j++) *o++ = noq ? '"' : (char)(uint8_t)(qual[rev ? L - 1 - j : j] + 33);
    *o++ = '\n';
}

int bam_scan_stream(BamStream &s, BamCounts *counts, uint64_t *digest, std::string &err, BamPairCounts *pairs) {
    if (s.read_header(err)) return -1;
    // [0]: every kept record in file order; [1], [2]: the mates of a paired file
    uint64_t hs[3] = {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}, mate_bases[3] = {0, 0, 0};
    auto mix1 = [](uint64_t h, const char *p, size_t len) {
        for (size_t i = 0; i < len; i++) h = (h ^ (unsigned char)p[i]) * 0x100000001b3ull;
        return (h ^ 0) * 0x100000001b3ull;
    };
    int mate = 0;
    auto mix = [&](const char *p, size_t len) {
        hs[0] = mix1(hs[0], p, len);
        if (mate) hs[mate] = mix1(hs[mate], p, len);
    };
    std::vector<char> text;
    for (;;) {
        BamRec r;
        const int rc = s.next(&r, err);
        if (rc < 0) return -1;
        if (rc == 0) break;
        text.resize((size_t)r.text_len());
        bam_transcode(s.data(), r, text.data());
        uint32_t hlen = 0, idlen = 0;
        (void)bam_name_fields(s.data() + r.name(), r.name_len(), &hlen, &idlen);
        mate = !s.paired() ? 0 : r.flag & 0x40 ? 1 : 2;
        mate_bases[mate] += r.l_seq;
        mix(text.data(), hlen);
        mix(text.data() + r.name_len() + 2, r.l_seq);
        mix(text.data() + r.name_len() + 5 + r.l_seq, r.l_seq);
        if (s.cursor() > (8u << 20)) s.compact();
    }
    *counts = s.counts();
    *digest = hs[0];
    if (pairs) {
        pairs->paired = s.paired();
        pairs->pairs = s.paired() ? s.counts().reads / 2 : 0;
        pairs->bases1 = mate_bases[1], pairs->bases2 = mate_bases[2];
        pairs->digest1 = hs[1], pairs->digest2 = hs[2];
    }
    return 0;
}

bool bam_wants(const char *path) {
    if (!path) return false;
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> m(65536 + 64);
    const size_t got = fread(m.data(), 1, m.size(), f);
    fclose(f);
    // 1f 8b, deflate, FEXTRA alone; then XLEN bytes of subfields, among them 'B' 'C' 2 0 BSIZE
    if (got < 18 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return false;
    const size_t xlen = le16(m.data() + 10);
    if (12 + xlen > got) return false;
    size_t bsize = 0;
    for (size_t at = 12; at + 4 <= 12 + xlen;) {
        const size_t slen = le16(m.data() + at + 2);
        if (at + 4 + slen > 12 + xlen) return false;
        if (m[at] == 'B' && m[at + 1] == 'C' && slen == 2) bsize = le16(m.data() + at + 4) + 1;
        at += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || bsize > got) return false;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    uint8_t magic[4] = {0, 0, 0, 0};
    z.next_in = m.data() + 12 + xlen;
    z.avail_in = (uInt)(bsize - 12 - xlen - 8);
    z.next_out = magic;
    z.avail_out = 4;
    const int rc = inflate(&z, Z_SYNC_FLUSH);
    const bool four = z.avail_out == 0 && (rc == Z_OK || rc == Z_STREAM_END || rc == Z_BUF_ERROR);
    inflateEnd(&z);
    return four && memcmp(magic, "BAM\1", 4) == 0;
}

}  // namespace nh

#ifndef NH_BAM_HOST_ONLY
#include <condition_variable>
#include <mutex>

#include "nh_internal.h"

namespace nh {

bool bam_sniff(const char *path, size_t max_recs, uint64_t max_text, const std::function<void(const BamRec &)> &each) {
    if (!bam_wants(path)) return false;
    ByteSource src;
    std::string err;
    if (src.open(path, err) != 0) return false;
    BamStream bs;
    bs.open([&](uint8_t *b, size_t n) { return src.read(b, n); }, path);
    bs.chunk = 1u << 20;
    if (bs.read_header(err) != 0) return false;
    bs.holding = true;
    BamRec br;
    uint64_t t = 0;
    for (size_t i = 0; i < max_recs && t < max_text && bs.next(&br, err) == 1; i++) {
        if (each) each(br);
        t += br.text_len();
    }
    return bs.paired();  // (known with the first kept record, also where that record is then refused)
}

bool bam_paired(const char *path) { return path && bam_sniff(path, 1, ~0ull, nullptr); }

// Buffers of one batch in flight: page-locked staging of the batch's BAM bytes and its table, their copies in HBM, the text.
struct BamSet {
    int dev = -1;
    hipStream_t stream = nullptr;
    uint8_t *h_bam = nullptr, *d_bam = nullptr;
    uint64_t *h_tab = nullptr, *d_tab = nullptr;
    char *d_text = nullptr;
    int *h_err = nullptr, *d_err = nullptr;
    size_t cap_bam = 0, cap_tab = 0, cap_text = 0;
    int held = 0;  // the halves handed out that point into the set and have not been released: 1 a single-end batch, 2 a paired one
};

class BamReaderImpl {
public:
    ~BamReaderImpl() { close(); }

    int open(const char *path, const int *devices, int n_devices, std::string &err, unsigned gz_threads, int paired) {
        close();
        if (n_devices < 1) {
            err = "BamReader: no device";
            return -1;
        }
        if (src_.open(path, err, gz_threads ? gz_threads : 1, -1) != 0) return -1;
        stream_.open([this](uint8_t *b, size_t n) { return src_.read(b, n); }, path);
        if (stream_.read_header(err)) {
            if (!src_.error().empty()) err = std::string(path) + ": " + src_.error();
            src_.close();
            return -1;
        }
        sets_.assign((size_t)(SETS_PER_DEVICE * n_devices), BamSet());
        for (size_t i = 0; i < sets_.size(); i++) sets_[i].dev = devices[i % (size_t)n_devices];
        path_ = path;
        paired_ = paired < 0 ? bam_paired(path) : paired != 0;
        open_ = true;
        return 0;
    }

    void next_batch(HalfBatch &hb, size_t max_recs, size_t max_text) {
        hb.reset();
        hb.format = FMT_FASTQ;
        if (!open_ || done_) {
            hb.eof = true;
            return;
        }
        if (max_recs == 0) max_recs = 1;
        max_text = std::min<size_t>(max_text ? max_text : (size_t)3u << 30, (size_t)3u << 30);
        stream_.holding = false;
        stream_.compact();
        recs_.clear();
        uint64_t text = 0;
        std::string err;
        while (recs_.size() < max_recs && text < max_text) {
            BamRec r;
            const int rc = stream_.next(&r, err);
            if (rc < 0) {
                hb.error = src_.error().empty() ? err : path_ + ": " + src_.error();
                done_ = true;
                return;
            }
            if (rc == 0) {
                done_ = true;
                break;
            }
            if (stream_.paired() != paired_) {  // (the request found a single-end file)
                hb.error = path_ + ": the input changed while it was read (it was a single-end BAM when the run was checked)";
                done_ = true;
                return;
            }
            if (text + r.text_len() > 0xFFFFFFF0ull) {
                hb.error = path_ + ": BAM record " + std::to_string(r.ordinal) + ": its FASTQ text cannot be addressed with the batch's 32-bit offsets";
                done_ = true;
                return;
            }
            stream_.holding = true;
            recs_.push_back(r);
            text += r.text_len();
        }
        hb.eof = done_;
        if (recs_.empty()) return;
        // the span of BAM bytes the kept records occupy (skipped ones in between travel along)
        const size_t b0 = recs_.front().off, b1 = recs_.back().off + 4 + recs_.back().block_size;
        BamSet &s = sets_[(size_t)(batches_ % sets_.size())];
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return s.held == 0; });
        }
        std::string derr = reserve(s, b1 - b0, recs_.size(), (size_t)text);
        if (derr.empty()) {
            memcpy(s.h_bam, stream_.data() + b0, b1 - b0);
            hb.recs.resize(recs_.size());
            uint64_t t = 0;
            for (size_t i = 0; i < recs_.size(); i++) {
                const BamRec &r = recs_[i];
                s.h_tab[2 * i] = r.off - b0;
                s.h_tab[2 * i + 1] = t;
                RecRef &x = hb.recs[i];
                (void)bam_name_fields(stream_.data() + r.name(), r.name_len(), &x.hlen, &x.idlen);
                x.h = (uint32_t)t;
                x.s = (uint32_t)(t + r.name_len() + 2);
                x.slen = x.qlen = r.l_seq;
                x.q = x.s + r.l_seq + 3;
                t += r.text_len();
                x.raw_end = x.hlen == 1 + r.name_len() ? (uint32_t)t : 0;
            }
            derr = transcode(s, b1 - b0, recs_.size(), (size_t)text);
        }
        if (!derr.empty()) {
            hb.recs.clear();
            hb.error = path_ + ": " + derr;
            hb.eof = done_ = true;
            return;
        }
        // (the host text buffer is a token, as for the batches of DevFastqReader: whoever needs the bytes fetches them)
        hb.text.clear();
        if (!hb.text.reserve(64)) {
            hb.recs.clear();
            hb.error = "out of memory";
            return;
        }
        hb.text.set_size((size_t)text);
        hb.dev_text = (const uint8_t *)s.d_text;
        hb.dev_device = s.dev;
        hb.dev_bam = s.d_bam;
        hb.dev_bam_table = s.d_tab;
        hb.bam_len = b1 - b0;
        hb.host_text_valid = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            s.held = 1;
        }
        hb.release = releaser(&s);
        batches_++;
    }

    // A paired file: the pairs of the batch chained, their BAM bytes uploaded once, both mates' texts written by one launch.
    void next_batch(HalfBatch &h1, HalfBatch &h2, size_t max_recs, size_t max_text) {
        h1.reset();
        h2.reset();
        h1.format = h2.format = FMT_FASTQ;
        if (!open_ || done_) {
            h1.eof = h2.eof = true;
            return;
        }
        auto fail = [&](const std::string &msg) {
            h1.recs.clear();
            h2.recs.clear();
            h1.error = h2.error = msg;
            h1.eof = h2.eof = done_ = true;
        };
        if (max_recs == 0) max_recs = 1;
        // (the two texts lie in one buffer, and in one batch of the pipeline behind: together below its 32-bit offsets)
        max_text = std::min<size_t>(max_text ? max_text : (size_t)0x7F000000u, (size_t)0x7F000000u);
        stream_.holding = false;
        stream_.compact();
        recs_.clear();  // (file order: the pair p is recs_[2p], recs_[2p + 1])
        uint64_t text[2] = {0, 0};
        std::string err;
        while (recs_.size() / 2 < max_recs && text[0] < max_text && text[1] < max_text) {
            BamRec a, b;
            const int rc = stream_.next_pair(&a, &b, err);
            if (rc < 0) return fail(src_.error().empty() ? err : path_ + ": " + src_.error());
            if (rc == 0) {
                done_ = true;
                break;
            }
            if (!stream_.paired()) return fail(path_ + ": the input changed while it was read (it was a paired BAM when the run was checked)");
            const BamRec &m1 = a.flag & 0x40 ? a : b, &m2 = a.flag & 0x40 ? b : a;
            if (text[0] + m1.text_len() > 0x7FFFFF00ull || text[1] + m2.text_len() > 0x7FFFFF00ull)
                return fail(path_ + ": BAM record " + std::to_string(a.ordinal) + ": the FASTQ text of its pair cannot be addressed with the batch's 32-bit offsets");
            recs_.push_back(a);
            recs_.push_back(b);
            text[0] += m1.text_len();
            text[1] += m2.text_len();
        }
        h1.eof = h2.eof = done_;
        if (recs_.empty()) return;
        const size_t P = recs_.size() / 2;
        const size_t b0 = recs_.front().off, b1 = recs_.back().off + 4 + recs_.back().block_size;
        const size_t base2 = ((size_t)text[0] + 255) & ~(size_t)255, ntext = base2 + (size_t)text[1];
        BamSet &s = sets_[(size_t)(batches_ % sets_.size())];
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return s.held == 0; });
        }
        // the table: 2P records of k_bam_fastq's (mate 1's, then mate 2's: the text offsets ascend), then a word a record in file order
        std::string derr = reserve(s, b1 - b0, 3 * P, ntext);
        if (derr.empty()) {
            memcpy(s.h_bam, stream_.data() + b0, b1 - b0);
            h1.recs.resize(P);
            h2.recs.resize(P);
            uint64_t t[2] = {0, 0};
            for (size_t p = 0; p < P; p++) {
                const BamRec &a = recs_[2 * p], &b = recs_[2 * p + 1];
                s.h_tab[4 * P + 2 * p] = a.off - b0;
                s.h_tab[4 * P + 2 * p + 1] = b.off - b0;
                for (int m = 0; m < 2; m++) {
                    const BamRec &r = ((a.flag & 0x40) != 0) == (m == 0) ? a : b;
                    s.h_tab[2 * (m * P + p)] = r.off - b0;
                    s.h_tab[2 * (m * P + p) + 1] = (m ? base2 : 0) + t[m];
                    RecRef &x = (m ? h2 : h1).recs[p];
                    (void)bam_name_fields(stream_.data() + r.name(), r.name_len(), &x.hlen, &x.idlen);
                    x.h = (uint32_t)t[m];
                    x.s = (uint32_t)(t[m] + r.name_len() + 2);
                    x.slen = x.qlen = r.l_seq;
                    x.q = x.s + r.l_seq + 3;
                    t[m] += r.text_len();
                    x.raw_end = x.hlen == 1 + r.name_len() ? (uint32_t)t[m] : 0;
                }
            }
            derr = transcode(s, b1 - b0, 2 * P, ntext, 3 * P);
        }
        if (!derr.empty()) return fail(path_ + ": " + derr);
        for (int m = 0; m < 2; m++) {
            HalfBatch &hb = m ? h2 : h1;
            hb.text.clear();
            if (!hb.text.reserve(64)) return fail("out of memory");
            hb.text.set_size((size_t)text[m]);
            hb.dev_text = (const uint8_t *)s.d_text + (m ? base2 : 0);
            hb.dev_device = s.dev;
            hb.host_text_valid = false;
        }
        h1.dev_bam = s.d_bam;
        h1.dev_bam_table = s.d_tab + 4 * P;
        h1.bam_len = b1 - b0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            s.held = 2;  // (the halves are let go of independently: the set is free when both have been)
        }
        h1.release = h2.release = releaser(&s);
        batches_++;
    }

    bool paired() const { return paired_; }
    const BamCounts &counts() const { return stream_.counts(); }
    std::string take_header() { return stream_.take_header(); }

    void close() {
        if (!open_) return;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] {
                for (const BamSet &s : sets_)
                    if (s.held) return false;
                return true;
            });
        }
        for (BamSet &s : sets_) {
            if (!s.stream) continue;
            (void)dev_set(s.dev);
            (void)hipStreamSynchronize(s.stream);
            (void)hipStreamDestroy(s.stream);
            if (s.h_bam) (void)hipHostFree(s.h_bam);
            if (s.h_tab) (void)hipHostFree(s.h_tab);
            if (s.h_err) (void)hipHostFree(s.h_err);
            if (s.d_bam) (void)hipFree(s.d_bam);
            if (s.d_tab) (void)hipFree(s.d_tab);
            if (s.d_text) (void)hipFree(s.d_text);
            if (s.d_err) (void)hipFree(s.d_err);
        }
        sets_.clear();
        src_.close();
        open_ = false;
    }

private:
    enum { SETS_PER_DEVICE = 4 };

    // what a half's release does: one hold less on its set
    std::function<void()> releaser(BamSet *sp) {
        return [this, sp] {
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (sp->held > 0) sp->held--;
            }
            cv_.notify_all();
        };
    }

    // grow-only: room for the batch (a quarter more than asked for, so that batches of about one size allocate once)
    std::string reserve(BamSet &s, size_t bam, size_t n, size_t text) {
        if (dev_set(s.dev) != hipSuccess) return "hipSetDevice failed";
        if (!s.stream) {
            if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return "cannot create a stream";
            if (host_malloc(&s.h_err, sizeof(int)) != hipSuccess || dev_malloc(&s.d_err, sizeof(int)) != hipSuccess) return "cannot allocate the BAM reader's buffers";
        }
        auto room = [](size_t x) { return x + x / 4 + 64; };
        if (bam > s.cap_bam) {
            if (s.h_bam) (void)hipHostFree(s.h_bam);
            if (s.d_bam) (void)hipFree(s.d_bam);
            s.h_bam = s.d_bam = nullptr;
            s.cap_bam = 0;
            if (host_malloc(&s.h_bam, room(bam)) != hipSuccess || dev_malloc(&s.d_bam, room(bam)) != hipSuccess) return "cannot allocate the BAM reader's buffers";
            s.cap_bam = room(bam) - 8;
        }
        if (n > s.cap_tab) {
            if (s.h_tab) (void)hipHostFree(s.h_tab);
            if (s.d_tab) (void)hipFree(s.d_tab);
            s.h_tab = s.d_tab = nullptr;
            s.cap_tab = 0;
            if (host_malloc(&s.h_tab, room(n) * 16) != hipSuccess || dev_malloc(&s.d_tab, room(n) * 16) != hipSuccess) return "cannot allocate the BAM reader's buffers";
            s.cap_tab = room(n);
        }
        if (text > s.cap_text) {
            if (s.d_text) (void)hipFree(s.d_text);
            s.d_text = nullptr;
            s.cap_text = 0;
            if (dev_malloc(&s.d_text, room(text)) != hipSuccess) return "cannot allocate the BAM reader's buffers";
            s.cap_text = room(text) - 8;
        }
        return "";
    }

    // the batch's bytes and table to the device, k_bam_fastq, the error word back; waits for all of it
    // (tab: the table's size in records of 16 bytes where it is more than the n the kernel reads: a paired batch's pair table behind them)
    std::string transcode(BamSet &s, size_t bam, size_t n, size_t text, size_t tab = 0) {
        *s.h_err = 0;
        hipError_t he = hipMemcpyAsync(s.d_bam, s.h_bam, bam, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess) he = hipMemcpyAsync(s.d_tab, s.h_tab, std::max(n, tab) * 16, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess) he = hipMemsetAsync(s.d_err, 0, sizeof(int), s.stream);
        if (he == hipSuccess) {
            BamFastqArgs a{};
            a.bam = s.d_bam;
            a.bam_len = bam;
            a.table = s.d_tab;
            a.n = n;
            a.text = s.d_text;
            a.text_cap = s.cap_text;
            a.text_len = text;
            a.error = s.d_err;
            a.span = 0;
            he = launch_bam_fastq(a, s.stream);
        }
        if (he == hipSuccess) he = hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, s.stream);
        if (he == hipSuccess) he = hipStreamSynchronize(s.stream);
        if (he != hipSuccess) return std::string("BAM to FASTQ on the device: ") + hipGetErrorString(he);
        if (*s.h_err) return "BAM to FASTQ on the device: a record outside its bytes or its text (error bits " + std::to_string(*s.h_err) + ")";
        return "";
    }

    ByteSource src_;
    BamStream stream_;
    std::string path_;
    std::vector<BamSet> sets_;
    std::vector<BamRec> recs_;
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t batches_ = 0;
    bool open_ = false, done_ = false, paired_ = false;
};

BamReader::BamReader() : impl_(new BamReaderImpl()) {}
BamReader::~BamReader() { delete impl_; }
int BamReader::open(const char *path, const int *devices, int n_devices, std::string &err, unsigned gz_threads, int paired) {
    return impl_->open(path, devices, n_devices, err, gz_threads, paired);
}
void BamReader::next_batch(HalfBatch &hb, size_t max_recs, size_t max_text) { impl_->next_batch(hb, max_recs, max_text); }
void BamReader::next_batch(HalfBatch &h1, HalfBatch &h2, size_t max_recs, size_t max_text) { impl_->next_batch(h1, h2, max_recs, max_text); }
bool BamReader::paired() const { return impl_->paired(); }
const BamCounts &BamReader::counts() const { return impl_->counts(); }
std::string BamReader::take_header() { return impl_->take_header(); }
void BamReader::close() { impl_->close(); }

}  // namespace nh

// nh_bam_scan and nh_bam_scan_pairs (pinfo given): one pass over the file
static int bam_scan_file(const char *who, const char *path, uint32_t threads, nh_bam_info *info, nh_bam_pair_info *pinfo) {
    if (!path || !info) return nh::set_error(NH_EINVAL, "%s: null argument", who);
    if (info->struct_size < sizeof(nh_bam_info))
        return nh::set_error(NH_EINVAL, "%s: struct_size %u is smaller than nh_bam_info (%zu bytes)", who, info->struct_size, sizeof(nh_bam_info));
    if (pinfo && pinfo->struct_size < sizeof(nh_bam_pair_info))
        return nh::set_error(NH_EINVAL, "%s: struct_size %u is smaller than nh_bam_pair_info (%zu bytes)", who, pinfo->struct_size, sizeof(nh_bam_pair_info));
    {
        FILE *f = fopen(path, "rb");
        if (!f) return nh::set_error(NH_EIO, "cannot open %s", path);
        fclose(f);
    }
    if (!nh::bam_wants(path)) return nh::set_error(NH_EINVAL, "%s: not a BAM file (no BGZF member that inflates to BAM\\1)", path);
    nh::ByteSource src;
    std::string err;
    if (src.open(path, err, threads ? threads : 1, -1) != 0) return nh::set_error(NH_EIO, "%s", err.c_str());
    nh::BamStream s;
    s.open([&](uint8_t *b, size_t n) { return src.read(b, n); }, path);
    nh::BamCounts c;
    nh::BamPairCounts pc;
    uint64_t digest = 0;
    if (nh::bam_scan_stream(s, &c, &digest, err, &pc) != 0) {
        if (!src.error().empty()) err = std::string(path) + ": " + src.error();
        return nh::set_error(NH_EIO, "%s", err.c_str());
    }
    info->records = c.records;
    info->reads = c.reads;
    info->bases = c.bases;
    info->skipped_secondary = c.skipped_secondary;
    info->skipped_empty = c.skipped_empty;
    info->reverse_complemented = c.reverse_complemented;
    info->missing_qualities = c.missing_qualities;
    info->digest = digest;
    if (pinfo) {
        pinfo->paired = pc.paired;
        pinfo->pairs = pc.pairs;
        pinfo->bases1 = pc.bases1, pinfo->bases2 = pc.bases2;
        pinfo->digest1 = pc.digest1, pinfo->digest2 = pc.digest2;
    }
    return NH_OK;
}

extern "C" int nh_bam_scan(const char *path, uint32_t threads, nh_bam_info *info) { return bam_scan_file("nh_bam_scan", path, threads, info, nullptr); }

extern "C" int nh_bam_scan_pairs(const char *path, uint32_t threads, nh_bam_info *info, nh_bam_pair_info *pairs) {
    if (!pairs) return nh::set_error(NH_EINVAL, "nh_bam_scan_pairs: null argument");
    return bam_scan_file("nh_bam_scan_pairs", path, threads, info, pairs);
}

extern "C" int nh_bam_paired(const char *path) { return nh::bam_paired(path) ? 1 : 0; }
#endif
