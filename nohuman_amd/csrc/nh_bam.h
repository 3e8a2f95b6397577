// nh_bam.h -- BAM input: unaligned or aligned reads, single-end or collated pairs, transcoded to canonical FASTQ text.
//
// The BGZF stream is inflated on the host (ByteSource: BGZF is multi-member gzip), the records are chained by their
// block_size and validated there (BamStream), and the per-base work -- 4-bit bases to ASCII, qualities + 33, the reverse
// complement of reverse-strand records, "@name\nSEQ\n+\nQUAL\n" -- is done by k_bam_fastq (nh_bam.hip) on the batch's BAM bytes in
// HBM.  What leaves BamReader is what DevFastqReader hands out: a FASTQ text in device memory and its record table.
// A file whose first kept record has flag 0x1 is paired: its kept records are taken two at a time, the 0x40 record is mate 1, and
// the reader hands out two halves, one a mate (tests/bam_pair_model.py).
// tests/bam_model.py is the specification; DESIGN.md 6.16.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "nh_fastx.h"
#ifndef NH_BAM_HOST_ONLY
#include <hip/hip_runtime.h>

#include "nohuman_engine.h"
#endif

namespace nh {

// the FASTQ text one kept record transcodes to: '@' name '\n' bases "\n+\n" qualities '\n'
inline uint64_t bam_text_len(uint32_t name_len, uint32_t l_seq) { return (uint64_t)name_len + 2ull * l_seq + 6; }

struct BamRec {  // one record as chained on the host; offsets into the window it was chained in
    size_t off;          // its block_size field
    uint32_t block_size, l_read_name, n_cigar, flag, l_seq;
    uint64_t ordinal;    // 1-based, all records of the file counted
    size_t name() const { return off + 36; }
    size_t seq() const { return off + 36 + l_read_name + 4 * (size_t)n_cigar; }
    size_t qual() const { return seq() + ((size_t)l_seq + 1) / 2; }
    uint32_t name_len() const { return l_read_name - 1; }
    uint64_t text_len() const { return bam_text_len(name_len(), l_seq); }
};

struct BamCounts {
    uint64_t records = 0, reads = 0, bases = 0, skipped_secondary = 0, skipped_empty = 0, reverse_complemented = 0, missing_qualities = 0;
};
// what a scan says of a paired file besides: the pairs, each mate's bases, nh_fastx_scan's digest of each mate's FASTQ
struct BamPairCounts {
    bool paired = false;
    uint64_t pairs = 0, bases1 = 0, bases2 = 0, digest1 = 0, digest2 = 0;
};

// The inflated BAM stream as a window of bytes and a cursor: header, then record by record.  The source is any function that
// fills a buffer (ByteSource::read; the stand-alone scan of the sanitizer build reads with zlib).
class BamStream {
public:
    typedef std::function<long(uint8_t *, size_t)> ReadFn;  // bytes read, 0 at the end, -1 on error
    void open(ReadFn read, const std::string &name) {
        read_ = std::move(read);
        name_ = name;
        if (const char *env = getenv("NOHUMAN_BAM_CHUNK")) {  // test knob: records and fixed parts cut at every offset
            const long v = atol(env);
            if (v > 0) chunk = (size_t)v;
        }
    }
    // the magic, the text and the references: 0, or -1 with err set
    int read_header(std::string &err);
    // the header read_header() stepped over, byte for byte (BAM output copies it); take_header() moves it out
    const std::string &header_bytes() const { return header_; }
    std::string take_header() { return std::move(header_); }
    // The next KEPT record (secondary, supplementary and empty ones are counted and stepped over): 1 and *r (offsets into
    // data(), valid until the next compact()), 0 at the end of the stream, -1 malformed (err set: the record's ordinal).
    // The first kept record says whether the file is paired (its flag 0x1).  In a single-end file a 0x1 record is refused; in a
    // paired one the kept records are chained two by two -- both 0x1, one 0x40 and one 0x80, one name -- and the record that
    // breaks the chain is refused, as is a last one without a partner.
    int next(BamRec *r, std::string &err);
    // The next pair of a paired file, in file order (*a lies in front of *b; the mate 1 is the one with flag 0x40): 1, 0 at the
    // end, -1 malformed -- before either record has been handed out.  Sets `holding` for the second record's sake.
    int next_pair(BamRec *a, BamRec *b, std::string &err);
    // whether the file is paired: known once next() has returned (1 or 0)
    bool paired() const { return paired_; }
    const uint8_t *data() const { return win_.data(); }
    size_t cursor() const { return pos_; }
    // drops the bytes in front of the cursor (the records handed out so far are gone)
    void compact();
    const BamCounts &counts() const { return cnt_; }
    size_t chunk = 4u << 20;  // bytes per read of the source
    bool holding = false;     // the caller keeps records of this window: next() does not compact it over skipped ones

private:
    int ensure(size_t n, std::string &err);  // n bytes at the cursor: 1, 0 the stream ends before, -1 read error
    ReadFn read_;
    std::string name_;
    std::vector<uint8_t> win_;
    std::string header_;
    size_t pos_ = 0, len_ = 0;
    bool eof_ = false;
    BamCounts cnt_;
    // the first 0x1 record in front of the first kept one (a skipped one): the refusal of a file that turns out single-end
    uint64_t early_ord_ = 0;
    std::string early_name_;
    bool mode_known_ = false, paired_ = false;
    // a paired file: the first record of the pair in hand
    bool half_ = false;
    uint64_t half_ord_ = 0;
    uint32_t half_flag_ = 0;
    std::string half_name_;
    int refuse_paired(uint64_t ord, const char *name, int name_len, std::string &err);
    int chain_pair(const BamRec &x, const uint8_t *name, std::string &err);
};

// One record's FASTQ text in plain C++ (the rules of the kernel): text_len() bytes at out.  bam: the window r points into.
void bam_transcode(const uint8_t *bam, const BamRec &r, char *out);
// header / id of a kept record as every reader here states them: hlen without trailing white space, the id up to the first
// blank; false: the name cannot stand in a FASTQ header line (a line feed in it, nothing but white space)
bool bam_name_fields(const uint8_t *name, uint32_t name_len, uint32_t *hlen, uint32_t *idlen);

// the scan behind nh_bam_scan on any source: counts and nh_fastx_scan's digest of the FASTQ the stream transcodes to (a paired
// file: of its kept records in file order); pairs, where given: what nh_bam_scan_pairs adds
int bam_scan_stream(BamStream &s, BamCounts *counts, uint64_t *digest, std::string &err, BamPairCounts *pairs = nullptr);

// Is the file a BAM: its first gzip member carries the BGZF extra field and inflates to a stream that begins "BAM\1"
bool bam_wants(const char *path);

#ifndef NH_BAM_HOST_ONLY
// Is the file a paired BAM: a BAM whose first kept record has flag 0x1 (false for anything else, an unreadable file included)
bool bam_paired(const char *path);
// The sniff behind it, and behind the run's estimate of a batch: the first kept records of the file -- up to max_recs of them, or
// max_text bytes of their FASTQ text -- handed to `each`; returns whether the file is paired (false: no BAM, or unreadable)
bool bam_sniff(const char *path, size_t max_recs, uint64_t max_text, const std::function<void(const BamRec &)> &each);

class BamReaderImpl;
// BlockReader's shape on a BAM file; the batches are born on a device (DevFastqReader's hand-over).
class BamReader {
public:
    BamReader();
    ~BamReader();
    BamReader(const BamReader &) = delete;
    BamReader &operator=(const BamReader &) = delete;
    // devices: the GPUs of the run -- batch b is transcoded on devices[b mod n] and says so (HalfBatch::dev_device); its BAM bytes
    // and its table stay there until the batch is released (HalfBatch::dev_bam, dev_bam_table, bam_len: BAM output reads them)
    // paired: what the run's request found (1 / 0) -- the file is not asked again, and a stream that turns out otherwise fails
    // the batch; -1: ask the file (bam_paired)
    int open(const char *path, const int *devices, int n_devices, std::string &err, unsigned gz_threads = 0, int paired = -1);
    // up to max_recs records, cut after the record that reaches max_text bytes of FASTQ text (BlockReader::next_batch's rule);
    // hb.eof at the end of the input, hb.error on malformed input or a device failure
    void next_batch(HalfBatch &hb, size_t max_recs, size_t max_text);
    // A paired file (paired()): two halves of as many records, mate 1's and mate 2's, cut only at pair borders -- up to max_recs
    // pairs, cut after the pair at which either mate's text reaches max_text.  The BAM bytes are uploaded once; the two texts are
    // two regions of one buffer (the second aligned to 256 bytes), written by one launch of k_bam_fastq whose table lists mate 1's
    // records and then mate 2's.  h1 carries the BAM bytes and, as dev_bam_table, two words a PAIR: where its two records lie,
    // in file order (BAM output).  The buffers are free when BOTH halves have been released.  An error is set in both halves.
    void next_batch(HalfBatch &h1, HalfBatch &h2, size_t max_recs, size_t max_text);
    bool paired() const;  // (from open() on: what it was told, or found)
    const BamCounts &counts() const;
    // the input's header, byte for byte: handed out once (BAM output writes it in front of each file), empty from then on
    std::string take_header();
    void close();  // waits until every batch handed out has been released

private:
    BamReaderImpl *impl_;
};

// k_bam_fastq (nh_bam.hip).  table: two uint64 a record -- where its block_size field lies in bam, where its '@' lies in text.
// error: one word, BAM_ERR_* are set in it.  span 0: NOHUMAN_BAM_SPAN, else the default.
enum { BAM_ERR_FIELDS = 1, BAM_ERR_TEXT = 2, BAM_ERR_OUT = 4 };  // (BAM_ERR_OUT: nh_bam_select_device's total above its buffer)
struct BamFastqArgs {
    const uint8_t *bam;
    uint64_t bam_len;
    const uint64_t *table;
    uint64_t n;
    char *text;
    uint64_t text_cap, text_len;
    int *error;
    uint32_t span;
};
hipError_t launch_bam_fastq(const BamFastqArgs &a, hipStream_t stream);

// BAM output (nh_bamout.hip; NH_CODEC_BAM): the records of a batch's BAM bytes selected by their call and compacted, each copied
// whole (4 + block_size bytes), in table order, for up to two outputs in one pass: output o takes the records whose host-ness
// (res[i].call != 0) is want[o].  table: the reader's, two uint64 a record, the first -- where the record's block_size field
// lies in bam -- is used.  A record whose block_size field or whose bytes do not lie inside [0, bam_len) sets err_fields in
// *error and is written nowhere; an output whose total is above its cap sets err_total, gets nothing and total 0.
struct BamOutArgs {
    const uint8_t *bam;
    uint64_t bam_len;
    const uint64_t *table;
    uint64_t n, nblk;         // nblk = bam_out_blocks(n)
    const nh_result *res;     // n results
    int n_out;                // 1 or 2
    int want[2];
    char *out[2];
    uint64_t cap[2];
    uint64_t *blk;            // n_out * nblk words of scratch
    uint64_t *total;          // 2 words
    int *error;
    int err_fields, err_total;
    uint32_t span;            // 0: NOHUMAN_BAM_SPAN, else the default
    // Pairs (a paired BAM): n counts records, two a pair; table is the reader's pair table -- ONE word a record, the pair's two
    // records in file order -- and record i takes the result of its pair, res[i >> 1].  A record outside the BAM bytes is
    // written nowhere, and neither is its mate.
    int pairs;
};
uint64_t bam_out_blocks(uint64_t n);
hipError_t launch_bam_out(const BamOutArgs &a, hipStream_t stream);
#endif

}  // namespace nh
