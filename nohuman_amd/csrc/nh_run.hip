// nh_run.hip -- whole-run entry nh_run(): files in, kraken2-compatible files out.
//
// Replaces, for the caller at /root/reference/src/main.rs:270, what the kraken2 subprocess does
// with the argv of src/main.rs:210-267: read 1-2 FASTQ/FASTA inputs (plain/gzip/bzip2), classify
// every fragment, write the kept fragments UNCOMPRESSED to kraken_out.fq or kraken_out_1.fq +
// kraken_out_2.fq (src/main.rs:252-256,308-309,333), optionally the per-read kraken output
// (--output) and return the counts nohuman scrapes from stderr (src/lib.rs:61-97).
// kraken2 units restated: classify.cc ProcessFiles / output formatting.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "nh_bam.h"
#include "nh_codec.h"
#include "nh_dust.h"
#include "nh_fastx.h"
#include "nh_gunzip.h"
#include "nh_internal.h"
#include "nohuman_engine.h"

namespace nh {

// What one batch puts into one output file: slices of the batch's raw text (the normal case: nothing is copied) and of
// a scratch string (reformatted records), in output order
struct Spans {
    std::vector<struct iovec> iov;
    std::vector<char> is_scratch;  // per span: iov_base is an offset into scratch
    std::string scratch;
    void clear() {
        iov.clear();
        is_scratch.clear();
        scratch.clear();
    }
};

struct OutFile {
    int fd = -1;
    std::string path;
    Spans sp;  // the batch being formatted (the writer moves it into the flusher's job and gets a cleared one back)
    std::string &scratch = sp.scratch;
    std::unique_ptr<StreamEncoder> enc;  // set: the spans go through a streaming encoder
    int open(const char *p, int codec = NH_CODEC_NONE, unsigned codec_threads = 1, int device = -1) {
        path = p;
        fd = ::open(p, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        if (fd < 0) return set_error(NH_EIO, "cannot create %s", p);
        if (codec != NH_CODEC_NONE) {
            enc.reset(make_encoder(codec, fd, codec_threads ? codec_threads : 1, p, device));
            if (!enc) return NH_EINVAL;  // message set by make_encoder
        }
        return NH_OK;
    }
    void add_raw(const char *p, size_t n) {
        if (!n) return;
        std::vector<struct iovec> &iov = sp.iov;
        if (!iov.empty() && !sp.is_scratch.back() && (const char *)iov.back().iov_base + iov.back().iov_len == p) {
            iov.back().iov_len += n;
            return;
        }
        iov.push_back({(void *)p, n});
        sp.is_scratch.push_back(0);
    }
    // the caller appended [from, scratch.size()) to scratch
    void add_scratch(size_t from) {
        const size_t n = sp.scratch.size() - from;
        if (!n) return;
        std::vector<struct iovec> &iov = sp.iov;
        if (!iov.empty() && sp.is_scratch.back() && (size_t)iov.back().iov_base + iov.back().iov_len == from) {
            iov.back().iov_len += n;
            return;
        }
        iov.push_back({(void *)from, n});
        sp.is_scratch.push_back(1);
    }
    int flush(Spans &x) {  // write all spans of x, then forget them
        std::vector<struct iovec> &iov = x.iov;
        for (size_t i = 0; i < iov.size(); i++)
            if (x.is_scratch[i]) iov[i].iov_base = (void *)(x.scratch.data() + (size_t)iov[i].iov_base);
        size_t i = 0;
        int rc = NH_OK;
        if (enc) {
            for (; i < iov.size() && rc == NH_OK; i++) rc = enc->write(iov[i].iov_base, iov[i].iov_len);
            i = iov.size();
            const int src = enc->settle();  // the batch's buffers (host and device) go back to the pipeline after this
            if (rc == NH_OK) rc = src;
        }
        while (i < iov.size()) {
            const int cnt = (int)std::min<size_t>(iov.size() - i, 512);
            ssize_t w = ::writev(fd, &iov[i], cnt);
            if (w < 0) {
                if (errno == EINTR) continue;
                rc = set_error(NH_EIO, "write error on %s", path.c_str());
                break;
            }
            size_t left = (size_t)w;  // consume whole spans, shorten a partly written one
            while (i < iov.size() && left >= iov[i].iov_len) left -= iov[i++].iov_len;
            if (left) {
                iov[i].iov_base = (char *)iov[i].iov_base + left;
                iov[i].iov_len -= left;
            }
        }
        x.clear();
        return rc;
    }
    int close() {
        int rc = NH_OK;
        if (enc) {
            rc = enc->finish();
            enc.reset();
        }
        if (fd >= 0 && ::close(fd) != 0 && rc == NH_OK) rc = set_error(NH_EIO, "write error on %s", path.c_str());
        fd = -1;
        return rc;
    }
    ~OutFile() {
        enc.reset();
        if (fd >= 0) ::close(fd);
    }
};

// kraken2 TrimPairInfo: drop a trailing /1 or /2 from ids longer than two characters
static void trim_pair_info(std::string &id) {
    size_t sz = id.size();
    if (sz <= 2) return;
    if (id[sz - 2] == '/' && (id[sz - 1] == '1' || id[sz - 1] == '2')) id.erase(sz - 2);
}

// kraken2 AddHitlistString
static void append_hitlist(std::string &dst, const Engine *e, const uint32_t *taxa, uint64_t n) {
    if (n == 0) {
        dst += "0:0";
        return;
    }
    char tmp[64];
    uint64_t i = 0;
    bool first = true;
    while (i < n) {
        uint32_t t = taxa[i];
        uint64_t j = i;
        while (j < n && taxa[j] == t) j++;
        if (t == TAXON_MATE_BORDER) {
            for (uint64_t r = i; r < j; r++) {
                if (!first) dst += ' ';
                dst += "|:|";
                first = false;
            }
        } else {
            if (!first) dst += ' ';
            if (t == TAXON_AMBIGUOUS)
                snprintf(tmp, sizeof tmp, "A:%llu", (unsigned long long)(j - i));
            else
                snprintf(tmp, sizeof tmp, "%llu:%llu", (unsigned long long)e->external[t],
                         (unsigned long long)(j - i));
            dst += tmp;
            first = false;
        }
        i = j;
    }
}

// kraken2 reports.cc ReportKrakenStyle / KrakenReportDFS (reached through
// nohuman's -r/--kraken-report, /root/reference/src/main.rs:97-99,226-228).  Lowest-confidence part
// of the restatement: the line format is "%6.2f\tclade\ttaxon\trank\ttaxid\t<2*depth spaces>name".
struct TaxoView {
    uint64_t n = 0;
    const uint8_t *nodes = nullptr;
    const char *names = nullptr, *ranks = nullptr;
    uint64_t field(uint64_t i, int k) const {
        uint64_t v;
        memcpy(&v, nodes + 56 * i + 8 * k, 8);
        return v;
    }
};

// md_clade (kraken2's --report-minimizer-data; NULL: the report as it always was): {minimizers_clade, distinct_clade} per node, two
// more columns behind the read counts
static void report_dfs(FILE *f, const TaxoView &t, const std::vector<uint64_t> &clade,
                       const std::vector<uint64_t> &own, uint64_t total, uint64_t id, char rank_code,
                       int rank_depth, int depth, const std::vector<uint64_t> *md_clade = nullptr) {
    if (clade[id] == 0) return;  // clades absent from the sample are not printed
    const std::string rank = t.ranks + t.field(id, 4);
    if (rank == "superkingdom" || rank == "domain") { rank_code = 'D'; rank_depth = 0; }
    else if (rank == "kingdom") { rank_code = 'K'; rank_depth = 0; }
    else if (rank == "phylum") { rank_code = 'P'; rank_depth = 0; }
    else if (rank == "class") { rank_code = 'C'; rank_depth = 0; }
    else if (rank == "order") { rank_code = 'O'; rank_depth = 0; }
    else if (rank == "family") { rank_code = 'F'; rank_depth = 0; }
    else if (rank == "genus") { rank_code = 'G'; rank_depth = 0; }
    else if (rank == "species") { rank_code = 'S'; rank_depth = 0; }
    else rank_depth++;
    std::string rank_str(1, rank_code);
    if (rank_depth != 0) rank_str += std::to_string(rank_depth);
    fprintf(f, "%6.2f\t%llu\t%llu\t", 100.0 * (double)clade[id] / (double)total, (unsigned long long)clade[id], (unsigned long long)own[id]);
    if (md_clade) fprintf(f, "%llu\t%llu\t", (unsigned long long)md_clade[0][id], (unsigned long long)md_clade[1][id]);
    fprintf(f, "%s\t%llu\t", rank_str.c_str(), (unsigned long long)t.field(id, 5));
    for (int i = 0; i < depth; i++) fputs("  ", f);
    fprintf(f, "%s\n", t.names + t.field(id, 3));
    const uint64_t first = t.field(id, 1), cnt = t.field(id, 2);
    std::vector<uint64_t> kids(cnt);
    for (uint64_t i = 0; i < cnt; i++) kids[i] = first + i;
    std::stable_sort(kids.begin(), kids.end(),
                     [&](uint64_t x, uint64_t y) { return clade[x] > clade[y]; });
    for (uint64_t c : kids) report_dfs(f, t, clade, own, total, c, rank_code, rank_depth, depth + 1, md_clade);
}

static TaxoView taxo_view(const Engine *e) {
    TaxoView t;
    const uint8_t *img = e->taxo_image.data();
    memcpy(&t.n, img + 8, 8);
    uint64_t name_len;
    memcpy(&name_len, img + 16, 8);
    t.nodes = img + 32;
    t.names = (const char *)(img + 32 + 56 * t.n);
    t.ranks = t.names + name_len;
    return t;
}

static int write_report(const Engine *e, const char *path, const std::vector<uint64_t> &own,
                        uint64_t total, uint64_t unclassified, const std::vector<uint64_t> *md_clade = nullptr) {
    const TaxoView t = taxo_view(e);
    std::vector<uint64_t> clade(own);
    for (uint64_t i = t.n; i-- > 1;)  // children have larger ids than their parents
        if (clade[i]) clade[t.field(i, 0)] += clade[i];
    FILE *f = fopen(path, "w");
    if (!f) return set_error(NH_EIO, "cannot create %s", path);
    if (unclassified != 0)
        fprintf(f, "%6.2f\t%llu\t%llu\t%sU\t0\tunclassified\n",
                100.0 * (double)unclassified / (double)total, (unsigned long long)unclassified,
                (unsigned long long)unclassified, md_clade ? "0\t0\t" : "");
    if (t.n > 1 && total) report_dfs(f, t, clade, own, total, 1, 'R', -1, 0, md_clade);
    if (fclose(f) != 0) return set_error(NH_EIO, "write error on %s", path);
    return NH_OK;
}

// Minimizer data (nh_run_mdata): the per-node numbers of a run -- own counts in, clade sums made here (children have larger ids
// than their parents) -- the struct array and the table.
struct MdataNumbers {
    std::vector<uint64_t> v[8];  // reads, minimizers, distinct, db_cells: [2 * quantity] clade, [2 * quantity + 1] own
};
static void mdata_clades(const TaxoView &t, MdataNumbers &m) {
    for (int q = 0; q < 4; q++) {
        m.v[2 * q + 1].resize(t.n, 0);
        m.v[2 * q] = m.v[2 * q + 1];
        for (uint64_t i = t.n; i-- > 1;) {
            const uint64_t p = t.field(i, 0);
            if (p < i) m.v[2 * q][p] += m.v[2 * q][i];
        }
    }
}
static int write_mdata_table(const TaxoView &t, const MdataNumbers &m, const char *path) {
    FILE *f = fopen(path, "w");
    if (!f) return set_error(NH_EIO, "cannot create %s: %s", path, strerror(errno));
    fputs("taxid\tname\treads_clade\treads_own\tminimizers_clade\tminimizers_own\tdistinct_clade\tdistinct_own\tdb_cells_clade\tdb_cells_own\tcoverage_pct\n", f);
    for (uint64_t i = 1; i < t.n; i++) {
        if (!m.v[0][i] && !m.v[2][i]) continue;
        fprintf(f, "%llu\t%s", (unsigned long long)t.field(i, 5), t.names + t.field(i, 3));
        for (int k = 0; k < 8; k++) fprintf(f, "\t%llu", (unsigned long long)m.v[k][i]);
        if (m.v[6][i]) fprintf(f, "\t%.4f\n", 100.0 * (double)m.v[4][i] / (double)m.v[6][i]);
        else fputs("\tNA\n", f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return set_error(NH_EIO, "cannot write %s", path);
    return NH_OK;
}

// ---- the pipeline -----------------------------------------------------------------------------------
// reader thread(s): inflate + parse one input file each into HalfBatches (bounded queue)
// main thread:      pair the halves, copy their raw text (page-locked batch buffers) to the device as it
//                   is and classify the sequences in place: (start, length) per sequence; H2D + classify +
//                   D2H asynchronously on one of two stream slots per device (batch b -> device
//                   b mod G, database replicated per device: SURVEY.md section 8e)
// writer thread:    format and write the outputs of finished batches in input order
static size_t estimate_batch_frags(const char *path, size_t *mean_record_bytes) {
    std::string err;
    *mean_record_bytes = 0;
    HalfBatch hb;
    if (bam_wants(path)) {  // the first kept records of a BAM: their lengths as the FASTQ text they become
        uint32_t t = 0;
        (void)bam_sniff(path, 256, 64u << 20, [&](const BamRec &br) {
            RecRef x{};
            x.s = t + br.name_len() + 2, x.slen = x.qlen = br.l_seq, x.q = x.s + br.l_seq + 3;
            t += (uint32_t)br.text_len();
            hb.recs.push_back(x);
        });
    } else {
        BlockReader r;
        if (r.open(path, err) != 0) return 1u << 18;
        r.next_batch(hb, 256, 64u << 20);
    }
    if (hb.recs.empty()) return 1u << 18;
    uint64_t sum = 0;
    for (const RecRef &x : hb.recs) sum += x.slen;
    const uint64_t mean = sum / hb.recs.size() + 1;
    const RecRef &lastr = hb.recs.back();
    *mean_record_bytes = (size_t)((lastr.q + lastr.qlen + 2 > lastr.s + lastr.slen + 2 ? lastr.q + lastr.qlen + 2
                                                                                   : lastr.s + lastr.slen + 2) /
                                  hb.recs.size() + 1);
    uint64_t frags = (96ull << 20) / mean;
    if (frags < 256) frags = 256;
    if (frags > (1u << 18)) frags = 1u << 18;
    return (size_t)frags;
}

template <class T>
class BoundedQueue {
public:
    explicit BoundedQueue(size_t cap) : cap_(cap) {}
    void push(T &&v) {
        std::unique_lock<std::mutex> lk(mu_);
        not_full_.wait(lk, [&] { return q_.size() < cap_ || closed_; });
        if (closed_) return;
        q_.push_back(std::move(v));
        not_empty_.notify_one();
    }
    bool pop(T &out) {  // false when closed and drained
        std::unique_lock<std::mutex> lk(mu_);
        not_empty_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        not_full_.notify_one();
        return true;
    }
    void close() {
        std::lock_guard<std::mutex> lk(mu_);
        closed_ = true;
        not_empty_.notify_all();
        not_full_.notify_all();
    }

private:
    std::mutex mu_;
    std::condition_variable not_full_, not_empty_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false;
};

// What the two input files contribute to one launch: records [off, off + n) of each half.  Normally a half is used whole
// (both readers cut at the same record counts); where a reader had to cut by TEXT (a batch's record text is addressed with 32
// bits), or the two files came from different readers after a handover, the halves differ in length and the longer one is used
// in parts: the halves are shared, and go back to their pool (device-born ones: to their reader) when the last part is through.
// A shared half is READ-ONLY once its first part has been queued (the writer used to fetch a device-born half's
// text into hb.text in place while the main thread read its size for the next part and the flusher of the part before still
// held spans into the old buffer): the halves' text lengths are taken when the half arrives (len1 / len2), and a part that
// must have the bytes on the host after all (a kept record that is rewritten: CRLF, "+id") fetches them into a buffer of its own.
struct Batch {
    std::shared_ptr<HalfBatch> h1, h2;
    size_t off1 = 0, off2 = 0;
    size_t len1 = 0, len2 = 0;  // bytes of text of the two halves (the whole half's, also for a part)
    std::unique_ptr<char[]> fetch1, fetch2;  // this part's own host copy of a half's text (see above), else null
    size_t n = 0;
    int slot = -1;  // stream slot that carries its results
    int dev_index = 0;  // index of the slot's device among the run's engines
    // the batch's text in the slot's device buffer: file 1's at byte 0, file 2's behind it at base2() (len2 is 0 without one)
    size_t base2() const { return (len1 + 8 + 255) & ~(size_t)255; }
    size_t ntext() const { return h2 ? base2() + len2 : len1; }
    // the words of fragment i in the -k lines' taxa: one a k-mer of each mate, and the mates' border
    uint64_t kmer_taxa(size_t i, uint64_t k) const {
        const uint64_t l1 = h1->recs[off1 + i].slen, l2 = h2 ? h2->recs[off2 + i].slen : 0;
        return (l1 >= k ? l1 - k + 1 : 0) + (h2 ? (l2 >= k ? l2 - k + 1 : 0) + 1 : 0);
    }
};

// One builder's side of a slot: the texts (one a mate, or one a list) that nh_split / nh_mask / nh_calls.hip make in HBM behind
// the classifier, the builder's scratch, its totals as they come back with the results (in the order its kernel writes them:
// *Args::total), and the page-locked copies the writer makes where the consumer cannot take the HBM range.
struct BuiltOut {
    DevBuf<uint64_t> d_blk;  // block sums / offsets, then the totals (d_total), then what else the builder keeps (*Args)
    DevBuf<char> d_out[2];
    PinBuf<char> h_out[2];
    uint64_t *d_total = nullptr;  // where in d_blk the batch's launch leaves its totals
    PinBuf<uint64_t> h_total;
    EventPair ev;  // NOHUMAN_TRACE: around the builder's launches (its kernel time)
};

// The pinned host + device buffers of one in-flight batch.  A slot owns them and its stream: they go back when the slot does, under
// the slot's device -- ~Slot selects it and destroys the stream, the members free themselves behind it -- and a slot is made in
// place and never copied or moved (Pipeline::slots).
struct Slot {
    Engine *e = nullptr;
    hipStream_t stream = nullptr;
    // The sequences are classified IN PLACE: the raw text of the batch (both mate files' record text, as
    // read) is copied to the device as it is, and the kernel gets (start, length) of every sequence.
    PinBuf<uint64_t> h_off;   // n_seq starts into d_text
    PinBuf<uint32_t> h_len;   // n_seq lengths
    PinBuf<nh_result> h_res;
    PinBuf<uint32_t> h_taxa;
    PinBuf<uint64_t> h_taxa_off;
    PinBuf<int> h_flag;  // the engine's sticky error bits as of the end of this slot's batch (copied on its stream)
    DevBuf<char> d_text;
    DevBuf<uint64_t> d_off, d_taxa_off;
    DevBuf<uint32_t> d_len, d_taxa;
    DevBuf<nh_result> d_res;
    uint64_t n_taxa = 0;
    bool busy = false;
    // the record table, per sequence {h, hlen, q, qlen}: what the builders, the quality mask and the read statistics read
    PinBuf<uint32_t[4]> h_rec;
    DevBuf<uint32_t[4]> d_rec;
    // read lists: mate 1's id lengths beside the record table
    PinBuf<uint32_t> h_idl;
    DevBuf<uint32_t> d_idl;
    BuiltOut human;  // split runs (nh_run_split): the classified-out records per mate; totals: bytes[2]
    BuiltOut mask;   // masked runs (nh_run_mask): every record per mate; totals: bytes[2], FAST blocks[2]
    BuiltOut lists;  // read lists (nh_run_ex): the calls table [0] and the human ids [1]; totals: bytes[2], lines[2]
    BuiltOut taxon;  // per-taxon outputs (nh_run_taxa): one buffer a mate, K bins in it; totals: start[2][K], bytes[2][K]
    BuiltOut bam;    // BAM output (NH_CODEC_BAM): the selected records of out1 [0] and, a split run, of human_out1 [1]; totals: bytes[2]
    // host intervals (nh_run_intervals): the BED lines [0] and the interval records they are made from [1]; totals: bytes, lines,
    // fragments, covered bases -- and the bitmap k_cover_mark ORs into, one bit a byte of the batch's text, zeroed per batch
    BuiltOut cover;
    DevBuf<uint32_t> d_cover;
    // runs with a minimum base quality (nh_run_minq): the text-sized buffer the classifier reads instead of d_text -- the
    // sequences with 'N' where the quality is low (nh_qmask.hip; the record table tells where the qualities lie) -- allocated
    // when first needed, and the masked bases of the slot's batches, read once, at the end of the run
    DevBuf<char> d_qtext;
    DevBuf<unsigned long long> d_qcnt;
    EventPair qev;  // NOHUMAN_TRACE: around k_qmask
    // runs that mask the reads' low-complexity stretches (nh_run_dust): d_qtext is reserved for them as well -- a copy of the text,
    // or the quality mask's output, in which k_rdust (nh_dust.hip) writes 'N' --, the scratch of its scan, the masked bases of the
    // slot's batches, the blocks that fill the slot's device once
    DevBuf<uint64_t> d_dscr;
    DevBuf<unsigned long long> d_dcnt;
    int dust_grid = 0;
    EventPair duev;  // NOHUMAN_TRACE: around the three launches of the read DUST
    EventPair rev;   // NOHUMAN_TRACE: around k_rstats (runs with read statistics)
    EventPair mev;   // NOHUMAN_TRACE: around k_mdata_mark (runs with minimizer data)
    // runs with a host selection (nh_run_host): the results with call = 0 where the fragment is not host (nh_host.hip) -- what
    // decides host-ness on the device (d_hres: the builders that remove, mask, list or count host reads) and on the host (h_hres:
    // the writer); d_res / h_res keep the true calls.  Empty in a run without a selection: the host-ness is then h_res's call != 0
    DevBuf<nh_result> d_hres;
    PinBuf<nh_result> h_hres;
    EventPair hev;  // NOHUMAN_TRACE: around k_host_filter
    // the results that decide which fragments are host reads
    const nh_result *host_res() const { return h_hres ? h_hres : h_res; }

    Slot() = default;
    Slot(const Slot &) = delete;
    Slot &operator=(const Slot &) = delete;
    ~Slot() {
        if (e) (void)dev_set(e->device);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// what a buffer that must hold `need` is allocated with: some room, so that batches a little larger do not reallocate
static size_t grow(size_t need) { return need + need / 4 + 4096; }
// room for n elements in a buffer of a slot, grown by grow(); false: the allocation failed, the caller words the message
template <class B>
static bool have(B &buf, size_t n) { return buf.reserve(n, grow(n)) == hipSuccess; }

static int slot_reserve(Slot &s, size_t ntext, size_t nfrag, size_t ntaxa) {
    if (dev_set(s.e->device) != hipSuccess) return set_error(NH_EDEVICE, "hipSetDevice failed");
    if (!s.h_flag) {
        if (s.h_flag.reserve(1, 16) != hipSuccess) return set_error(NH_EOOM, "cannot allocate batch buffers");
        *s.h_flag = 0;
    }
    if (!have(s.d_text, ntext + 64)) return set_error(NH_EOOM, "cannot allocate batch buffers (%zu bytes)", grow(ntext + 64));
    // (2 * cap + 2 starts and lengths, cap results, cap + 1 offsets: all eight grow at the same batch)
    const size_t cap = grow(nfrag), ns = 2 * cap + 2;
    if (s.h_off.reserve(2 * nfrag + 2, ns) != hipSuccess || s.h_len.reserve(2 * nfrag + 2, ns) != hipSuccess ||
        s.h_res.reserve(nfrag, cap) != hipSuccess || s.h_taxa_off.reserve(nfrag + 1, cap + 1) != hipSuccess ||
        s.d_off.reserve(2 * nfrag + 2, ns) != hipSuccess || s.d_len.reserve(2 * nfrag + 2, ns) != hipSuccess ||
        s.d_res.reserve(nfrag, cap) != hipSuccess || s.d_taxa_off.reserve(nfrag + 1, cap + 1) != hipSuccess)
        return set_error(NH_EOOM, "cannot allocate batch buffers (%zu fragments)", cap);
    if (!have(s.h_taxa, ntaxa) || !have(s.d_taxa, ntaxa)) return set_error(NH_EOOM, "cannot allocate k-mer taxa buffers");
    return NH_OK;
}

// a builder's buffers of a slot: blk_words words of scratch, out_cap[i] bytes of text for each of its n_out outputs;
// `what` names the text buffers in the error message
static int built_reserve(BuiltOut &o, size_t blk_words, const size_t out_cap[2], int n_out, const char *what) {
    if (!have(o.d_blk, blk_words)) return set_error(NH_EOOM, "cannot allocate batch buffers");
    for (int i = 0; i < n_out; i++)
        if (!have(o.d_out[i], out_cap[i])) return set_error(NH_EOOM, "cannot allocate %s (%zu bytes)", what, grow(out_cap[i]));
    return NH_OK;
}

// a page-locked array of a slot and its twin in HBM: n elements (`what`: their name in the message)
template <class T>
static int slot_reserve_pair(PinBuf<T> &h, DevBuf<T> &d, size_t n, const char *what) {
    if (have(h, n) && have(d, n)) return NH_OK;
    return set_error(NH_EOOM, "cannot allocate batch buffers (%zu %s)", grow(n), what);
}
// the record table of nrec sequences of a slot (read statistics need nothing else)
static int slot_reserve_rec(Slot &s, size_t nrec) { return slot_reserve_pair(s.h_rec, s.d_rec, nrec, "records"); }
// mate 1's id lengths of n fragments of a slot (read lists)
static int slot_reserve_idl(Slot &s, size_t n) { return slot_reserve_pair(s.h_idl, s.d_idl, n, "id lengths"); }

// ntext bytes of masked text of a slot: what the classifier reads in a run with a minimum base quality or with --dust-reads
static int slot_reserve_qtext(Slot &s, size_t ntext) {
    return have(s.d_qtext, ntext + 64) ? NH_OK : set_error(NH_EOOM, "cannot allocate the masked text (%zu bytes)", grow(ntext + 64));
}
// one of a slot's counters of masked bases: allocated once, zeroed on the slot's stream; `what` names it in the message
static int slot_counter(Slot &s, DevBuf<unsigned long long> &c, const char *what) {
    if (c.reserve(1) != hipSuccess) return set_error(NH_EOOM, "cannot allocate batch buffers");
    if (hipMemsetAsync(c, 0, 8, s.stream) != hipSuccess) return set_error(NH_EDEVICE, "cannot clear the %s's counter", what);
    return NH_OK;
}

// the read DUST's buffers of a slot: ntext bytes of masked text, the scan's scratch for nseq sequences, the counter
static int slot_reserve_dust(Slot &s, size_t ntext, size_t nseq) {
    const int trc = slot_reserve_qtext(s, ntext);
    if (trc) return trc;
    const size_t words = (size_t)read_dust_scratch_words(nseq);
    if (!have(s.d_dscr, words)) return set_error(NH_EOOM, "cannot allocate the read DUST's scratch (%zu words)", grow(words));
    if (s.d_dcnt) return NH_OK;
    s.dust_grid = read_dust_grid_max();
    return slot_counter(s, s.d_dcnt, "read DUST");
}

// the quality mask's buffers of a slot: the record table of nrec sequences, ntext bytes of masked text, the counter
static int slot_reserve_qmask(Slot &s, size_t ntext, size_t nrec) {
    const int rrc = slot_reserve_rec(s, nrec);
    if (rrc) return rrc;
    const int trc = slot_reserve_qtext(s, ntext);
    if (trc) return trc;
    return s.d_qcnt ? NH_OK : slot_counter(s, s.d_qcnt, "quality mask");
}

// page-locked text buffers of the batches (RawBuf allocator): the H2D copy of a batch's raw text runs
// asynchronously straight from where the reader inflated / read it
// A host that cannot page-lock that much (memlock / cgroup limits) gets pageable memory instead -- the
// asynchronous copy accepts it and merely stages it itself; a 64-byte header says which kind a block is.
static std::atomic<int> g_pageable_batches{0};
// Page-locking a batch buffer costs ~40 ms and releasing it as much again: a run of a few seconds spent 0.4-0.7 s of its wall
// time on its dozen buffers.  Released buffers are kept for the process's next run (at most PINNED_KEEP of them; nh_close
// of an engine empties the store, NOHUMAN_PINNED_CACHE=0 turns it off).
static constexpr size_t PINNED_KEEP = 16;
static std::mutex g_pinned_mu;
static std::vector<void *> g_pinned_store;  // block starts (header: [0] kind, [1] usable bytes)
static bool pinned_cache_on() {
    static const bool on = !(getenv("NOHUMAN_PINNED_CACHE") && getenv("NOHUMAN_PINNED_CACHE")[0] == '0');
    return on;
}
static void *pinned_alloc(size_t n) {
    void *p = nullptr;
    static const bool no_pin = getenv("NOHUMAN_NO_PINNED") != nullptr;  // test knob: exercise the fallback
    if (!no_pin && pinned_cache_on() && n >= ((size_t)8u << 20)) {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        for (size_t i = 0; i < g_pinned_store.size(); i++) {
            const uint64_t cap = ((uint64_t *)g_pinned_store[i])[1];
            if (cap >= n && cap <= n + n / 2) {
                p = g_pinned_store[i];
                g_pinned_store.erase(g_pinned_store.begin() + (long)i);
                return (char *)p + 64;
            }
        }
    }
    if (!no_pin && host_malloc(&p, n + 64, hipHostMallocPortable) == hipSuccess) {
        ((uint64_t *)p)[0] = 1;
        ((uint64_t *)p)[1] = n;
        return (char *)p + 64;
    }
    (void)hipGetLastError();
    if (posix_memalign(&p, 64, n + 64) != 0) return nullptr;
    ((uint64_t *)p)[0] = 2;
    ((uint64_t *)p)[1] = n;
    g_pageable_batches++;
    return (char *)p + 64;
}
static void pinned_free(void *q) {
    void *p = (char *)q - 64;
    if (*(uint64_t *)p == 1) {
        if (pinned_cache_on() && ((uint64_t *)p)[1] >= ((size_t)8u << 20)) {
            std::lock_guard<std::mutex> lk(g_pinned_mu);
            if (g_pinned_store.size() < PINNED_KEEP) {
                g_pinned_store.push_back(p);
                return;
            }
        }
        (void)hipHostFree(p);
    } else {
        free(p);
    }
}
void run_cache_trim() {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    for (void *p : g_pinned_store) (void)hipHostFree(p);
    g_pinned_store.clear();
}

// folds the counters of one run into the engine's running totals (nh_stats_get)
__global__ void k_add_counters(unsigned long long *dst, const unsigned long long *src) {
    atomicAdd(&dst[threadIdx.x], src[threadIdx.x]);
}

struct RunState {
    const nh_run_args *a;
    std::vector<Engine *> engines;
    bool paired, want_k;
    // results of the run
    uint64_t total = 0, classified = 0, total_bases = 0;
    uint64_t hit_groups = 0;  // the fragments' nh_result.hit_groups summed: the checker of the minimizer data's count
    // split runs (NOHUMAN_TRACE): what the classified-out builder made, and the bytes of record text the run copied back to
    // the host -- classified-out text for host encoders, and batches of the reader on the GPU fetched for the other side
    uint64_t human_records = 0, human_bytes = 0;
    double human_kernel_ms = 0;  // NOHUMAN_TRACE: the builder's launches, by events on the slots' streams
    // masked runs (NOHUMAN_TRACE): records masked and written, the bytes the mask builder made, its kernel time
    uint64_t mask_masked = 0, mask_records = 0, mask_bytes = 0, mask_nblk = 0, mask_fast = 0;
    double mask_kernel_ms = 0;
    // read lists (NOHUMAN_TRACE): lines and bytes of the calls table [0] and the human ids [1], the builder's kernel time
    uint64_t list_lines[2] = {0, 0}, list_bytes[2] = {0, 0};
    double list_kernel_ms = 0;
    // per-taxon outputs: the fragments of every selector (nh_taxon_out.fragments); NOHUMAN_TRACE: the bytes the binned builder
    // made, its kernel time
    uint64_t taxon_frags[NH_MAX_TAXON_OUTS] = {}, taxon_records = 0, taxon_bytes = 0;
    double taxon_kernel_ms = 0;
    // runs with a minimum base quality (NOHUMAN_TRACE): the bases k_qmask replaced, its kernel time
    uint64_t qmask_masked = 0;
    double qmask_kernel_ms = 0;
    // runs with --dust-reads: the bases k_rdust masked (nh_read_dust.masked_bases), the kernel time of its three launches
    uint64_t dust_masked = 0;
    double dust_kernel_ms = 0;
    // runs with read statistics: the exact length histogram of each [class][mate] -- a vector for the lengths below 2^20, a map
    // above -- that the writer keeps from the batch's lengths and calls (median and N50 need every length), k_rstats' time
    std::vector<uint64_t> len_hist[2][2];
    std::map<uint64_t, uint64_t> len_long[2][2];
    double rstats_kernel_ms = 0;
    double mdata_kernel_ms = 0;  // NOHUMAN_TRACE: k_mdata_mark, by events on the slots' streams
    // runs with a host selection: the classified fragments that are host / spared as the writer saw them (the checker of the
    // devices' counters), k_host_filter's time
    uint64_t host_frags = 0, spared_frags = 0;
    double host_kernel_ms = 0;
    // host intervals: the fragments with a line, the lines and the covered bases as the devices counted them (nh_host_intervals),
    // the bytes of the lines, the kernel time of the mark pass and the two builders
    uint64_t cover_frags = 0, cover_ivls = 0, cover_bases = 0, cover_bytes = 0;
    double cover_kernel_ms = 0;
    // host bases only: {host, masked, closed} bases as the devices counted them (nh_host_bases), fetched once at the end, and the
    // sequence bases of the host fragments as the writer saw them
    uint64_t hb_bases[3] = {0, 0, 0}, hb_host_written = 0;
    // host cut: the CUT_COUNTS counts as the devices counted them (nh_host_cut; closed_bases is hb_bases[2], the writer's check
    // hb_host_written), the items the builder made
    uint64_t cut_counts[CUT_COUNTS] = {}, cut_items = 0;
    // BAM output (NOHUMAN_TRACE): the records and bytes the builder selected per output, its kernel time
    uint64_t bam_records[2] = {0, 0}, bam_bytes[2] = {0, 0};
    double bam_kernel_ms = 0;
    // in1's reader says once what it reads: a BAM's header, byte for byte (BamReader::take_header), or "" for anything else.  A run
    // with BAM output waits for it and writes it in front of every record output
    std::mutex hdr_mu;
    std::condition_variable hdr_cv;
    bool hdr_set = false;
    std::string bam_header;
    void set_bam_header(std::string h) {
        {
            std::lock_guard<std::mutex> lk(hdr_mu);
            bam_header = std::move(h);
            hdr_set = true;
        }
        hdr_cv.notify_all();
    }
    std::atomic<uint64_t> text_fetched{0};
    std::vector<uint64_t> dev_counts;  // per device {fragments, classified, bases, 0} as the writer saw them (checker)
    std::vector<uint64_t *> d_run_counters;  // per device: the counters the classify kernels of THIS run add to (HBM)
    std::vector<uint64_t> call_counts;
    // first error of any thread
    std::mutex err_mu;
    int err_code = NH_OK;
    std::string err_msg;
    void fail(int code, const std::string &msg) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (err_code == NH_OK) {
            err_code = code;
            err_msg = msg;
        }
    }
    bool failed() {
        std::lock_guard<std::mutex> lk(err_mu);
        return err_code != NH_OK;
    }
};

// Recycles batch buffers (~100 MB each) between the writer and the readers, so that steady state
// neither allocates nor page-faults.
class BatchPool {
public:
    ~BatchPool() {
        if (filler_.joinable()) filler_.join();
    }
    std::unique_ptr<HalfBatch> get() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!free_.empty()) {
                std::unique_ptr<HalfBatch> hb = std::move(free_.back());
                free_.pop_back();
                return hb;
            }
        }
        return make();
    }
    void put(std::unique_ptr<HalfBatch> hb) {
        if (!hb) return;
        if (hb->release) {  // a batch born on the GPU: its text buffer goes back to the device reader
            hb->release();
            hb->release = nullptr;
        }
        std::lock_guard<std::mutex> lk(mu_);
        free_.push_back(std::move(hb));
    }
    // Page-locking ~100 MB takes tens of milliseconds: a helper makes the first buffers while the reader
    // already fills the ones it has, instead of the reader stopping for each of them.
    void start_prefill(int n) {
        filler_ = std::thread([this, n] {
            for (int i = 0; i < n && !stop_.load(); i++) put(make());
        });
    }
    void stop() { stop_.store(true); }
    size_t first_reserve = 0;

private:
    std::unique_ptr<HalfBatch> make() {
        std::unique_ptr<HalfBatch> hb(new HalfBatch());
        hb->text.set_allocator(pinned_alloc, pinned_free);
        if (first_reserve) hb->text.reserve(first_reserve);  // one allocation instead of a dozen growing ones
        return hb;
    }
    std::mutex mu_;
    std::vector<std::unique_ptr<HalfBatch>> free_;
    std::thread filler_;
    std::atomic<bool> stop_{false};
};

// NOHUMAN_TRACE: the time between a slot's pair of events is added to *sum (the slot's stream was synchronised: both have
// completed; without the trace there are no events)
static void add_event_ms(const EventPair &ev, double *sum) {
    float ms = 0;
    if (ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *sum += ms;
}

// The span of built text the writer hands on, output i's `tot` bytes: in HBM where the consumer takes the range, else copied
// to the slot's page-locked buffer and counted as fetched.  `what` / `item` name the buffers / the text in the error messages.
static char *built_span(BuiltOut &o, int i, size_t tot, bool in_hbm, RunState &rs, int *wrc, const char *what, const char *item) {
    if (in_hbm) return o.d_out[i];
    if (!have(o.h_out[i], tot)) *wrc = set_error(NH_EOOM, "cannot allocate %s (%zu bytes)", what, tot);
    if (!*wrc && hipMemcpy(o.h_out[i], o.d_out[i], tot, hipMemcpyDeviceToHost) != hipSuccess)
        *wrc = set_error(NH_EDEVICE, "fetching a batch's %s from the device failed", item);
    rs.text_fetched += tot;
    return o.h_out[i];
}

struct StageClock {  // NOHUMAN_TRACE=1: where the wall time of a run goes, per thread
    std::atomic<uint64_t> ns[12];
    StageClock() {
        for (auto &x : ns) x = 0;
    }
    static uint64_t now() {
        return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                   std::chrono::steady_clock::now().time_since_epoch())
            .count();
    }
};
enum { ST_READ1 = 0, ST_READ2, ST_RPUSH1, ST_RPUSH2, ST_MPOP, ST_MSLOT, ST_MGATHER, ST_MLAUNCH, ST_WPOP, ST_WSYNC, ST_WFORMAT, ST_WWRITE };

// the host reader's loop: batches of an opened BlockReader (or BamReader: the same next_batch) into the queue, behind `skip`
// records that are read and dropped (the reader on the GPU handed them out before it handed the file over)
template <class Reader>
static void host_read(Reader &r, BoundedQueue<std::unique_ptr<HalfBatch>> *out, RunState *rs, BatchPool *pool, StageClock *clk, int which,
                      size_t batch_frags, size_t batch_text, uint64_t skip) {
    while (skip) {
        std::unique_ptr<HalfBatch> hb = pool->get();
        r.next_batch(*hb, (size_t)std::min<uint64_t>(skip, batch_frags), batch_text);
        if (!hb->error.empty()) {
            rs->fail(NH_EIO, hb->error);
            return;
        }
        const size_t n = hb->recs.size();
        const bool eof = hb->eof;
        pool->put(std::move(hb));
        skip -= std::min<uint64_t>(skip, n);
        if (eof || rs->failed()) {  // (the file ends inside what the device reader read: it cannot be the same file)
            if (skip) rs->fail(NH_EIO, "the input changed while it was read");
            return;
        }
    }
    for (;;) {
        std::unique_ptr<HalfBatch> hb = pool->get();
        hb->recs.reserve(batch_frags);
        uint64_t t0 = StageClock::now();
        r.next_batch(*hb, batch_frags, batch_text);
        uint64_t t1 = StageClock::now();
        clk->ns[ST_READ1 + which] += t1 - t0;
        if (!hb->error.empty()) {
            rs->fail(NH_EIO, hb->error);
            break;
        }
        const bool eof = hb->eof;
        out->push(std::move(hb));
        clk->ns[ST_RPUSH1 + which] += StageClock::now() - t1;
        if (eof || rs->failed()) break;
    }
}

// Which reader a gzip input starts on when NOHUMAN_GZ_READER does not say.  Measured (tools/reader_choice.py,
// profiles/r05_reader_choice.txt; run time with the reader on the GPU / with the host reader on 16 cores):
//   outputs gzip-encoded on the GPU (the text never leaves HBM): 0.45-0.94 at every size from 50 MB to 1 GB a file, paired
//     and single-end, and 0.79-0.92 on long reads                                                      -> the GPU
//   short reads, only classified reads kept / --output wanted (the text is fetched, little is written): 0.33-0.78 -> the GPU
//   outputs written by the host (plain, bzip2, xz, zstd: every kept byte crosses PCIe and goes through
//     writev): 0.78-0.98 below 128 MiB a file, 1.09-1.21 from there to 1 GiB, 0.88 at 4 GiB             -> the host in between
//   long reads (batches few and large: nothing flows before the first 512 MiB piece is through) with outputs written by the
//     host or nothing kept: 1.14-1.26                                                                  -> the host
static bool device_reader_pays(const char *path, size_t mean_record_bytes, bool host_text_wanted, bool bulk_by_host) {
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) return false;
    if (const char *e = getenv("NOHUMAN_GZDEV_MIN_BYTES")) return (uint64_t)st.st_size >= (uint64_t)atoll(e);  // tuning / test knob
    if (!host_text_wanted) return true;
    if (mean_record_bytes > 4096) return false;
    // bulk_by_host: most of the input is expected to leave through the host (the default mode keeps the non-human reads; a
    // --keep-human-reads run keeps few).  Between 128 MiB and 2 GiB a file -- one to four pieces, little to pipeline -- the
    // host reader is the faster one then; above, the GPU reader's pieces overlap the writes (50 M pairs: 25.5 against 22.3)
    const uint64_t sz = (uint64_t)st.st_size;
    return !(bulk_by_host && sz >= ((uint64_t)128u << 20) && sz < ((uint64_t)2u << 30));
}

// a paired BAM's loop: both mates' halves from one reader, one thread -- mate 1's into out1, mate 2's into out2
static void paired_bam_read(BamReader &br, BoundedQueue<std::unique_ptr<HalfBatch>> *out1, BoundedQueue<std::unique_ptr<HalfBatch>> *out2, RunState *rs,
                            BatchPool *pool1, BatchPool *pool2, StageClock *clk, size_t batch_frags, size_t batch_text) {
    for (;;) {
        std::unique_ptr<HalfBatch> h1 = pool1->get(), h2 = pool2->get();
        h1->recs.reserve(batch_frags);
        h2->recs.reserve(batch_frags);
        const uint64_t t0 = StageClock::now();
        br.next_batch(*h1, *h2, batch_frags, batch_text);
        const uint64_t t1 = StageClock::now();
        clk->ns[ST_READ1] += t1 - t0;
        if (!h1->error.empty()) {
            rs->fail(NH_EIO, h1->error);
            break;
        }
        const bool eof = h1->eof;
        out1->push(std::move(h1));
        out2->push(std::move(h2));
        clk->ns[ST_RPUSH1] += StageClock::now() - t1;
        if (eof || rs->failed()) break;
    }
}

// out2 / pool2: given for a paired BAM alone -- the one reader of the run feeds both queues, and closes both on every way out
static void reader_main(const char *path, BoundedQueue<std::unique_ptr<HalfBatch>> *out, BoundedQueue<std::unique_ptr<HalfBatch>> *out2, RunState *rs,
                        BatchPool *pool, BatchPool *pool2, StageClock *clk, int which, size_t batch_frags, size_t batch_text,
                        unsigned gz_threads, std::vector<int> gz_devices, bool device_reader, unsigned hybrid_threads) {
    struct CloseSecond {  // (a queue closed twice stays closed)
        BoundedQueue<std::unique_ptr<HalfBatch>> *q;
        ~CloseSecond() {
            if (q) q->close();
        }
    } close_second{out2};
    const int gz_device = gz_devices.empty() ? -1 : gz_devices[0];
    // BAM: inflated and chained on the host, transcoded to FASTQ text on the GPU (nh_bam.h); the batches are born there
    const bool is_bam = bam_wants(path);
    if (which == 0 && !is_bam) rs->set_bam_header("");
    if (is_bam) {
        BamReader br;
        std::string err;
        if (gz_devices.empty() || br.open(path, gz_devices.data(), (int)gz_devices.size(), err, gz_threads, out2 != nullptr) != 0) {
            rs->fail(NH_EIO, gz_devices.empty() ? std::string(path) + ": BAM input needs a device" : err);
            if (which == 0) rs->set_bam_header("");
            out->close();
            return;
        }
        if (which == 0) rs->set_bam_header(br.take_header());
        if (out2) paired_bam_read(br, out, out2, rs, pool, pool2, clk, batch_frags, batch_text);
        else host_read(br, out, rs, pool, clk, which, batch_frags, batch_text, 0);
        if (getenv("NOHUMAN_TRACE")) {
            const BamCounts &c = br.counts();
            fprintf(stderr, "[nohuman trace] BAM reader: %llu records, %llu kept, %llu secondary or supplementary and %llu empty skipped, %llu reverse-complemented\n",
                    (unsigned long long)c.records, (unsigned long long)c.reads, (unsigned long long)c.skipped_secondary,
                    (unsigned long long)c.skipped_empty, (unsigned long long)c.reverse_complemented);
        }
        out->close();
        if (out2) out2->close();  // (before close() waits: the main thread must see the end of both)
        br.close();  // (waits for the batches still in the pipeline: they point into its buffers)
        return;
    }
    // gzip FASTQ: the whole reader on the GPU (inflate, record index; the text stays in HBM) where that pays (the caller
    // decides: device_reader) or NOHUMAN_GZ_READER says "device"; "host": the host decoders; "device-text": inflate on the
    // GPU, records parsed on the host (BlockReader)
    uint64_t skip = 0;  // records the reader on the GPU handed out before it handed the file over
    {
        const char *how = getenv("NOHUMAN_GZ_READER");
        const bool named = how && !strcmp(how, "device");
        if (gz_device >= 0 && device_reader) {
            DevFastqReader dr;
            std::string derr;
            // (the run's devices, this file's first: piece i of the stream is inflated, indexed and classified on device i mod G)
            const int orc = dr.open(path, gz_devices.data(), (int)gz_devices.size(), derr, hybrid_threads);
            if (orc < 0) {
                if (named) {  // asked for by name: no silent change of reader
                    rs->fail(NH_EIO, derr);
                    out->close();
                    return;
                }
                fprintf(stderr, "nohuman: WARN %s: the gzip reader on GPU %d could not be set up (%s); reading on the host\n", path, gz_device,
                        derr.c_str());
            }
            bool fell_back = orc != 0;
            while (!fell_back) {
                std::unique_ptr<HalfBatch> hb = pool->get();
                uint64_t t0 = StageClock::now();
                // (paired inputs: both files' readers cut at the same record counts; single-end batches are cut by text as well)
                const int rc = dr.next_batch(*hb, batch_frags, rs->paired ? 0 : batch_text);
                uint64_t t1 = StageClock::now();
                clk->ns[ST_READ1 + which] += t1 - t0;
                if (rc == 1) {
                    // no four-line FASTQ: the host parser reads the file (FASTA, wrapped lines, its error messages) -- or the
                    // reader on the GPU could not go on: the host reader does, behind the records already handed out
                    pool->put(std::move(hb));
                    if (!dr.handover_reason().empty()) {
                        if (named) {
                            rs->fail(NH_EIO, dr.handover_reason());
                            break;
                        }
                        skip = dr.records_handed();
                        fprintf(stderr, "nohuman: WARN %s: the gzip reader on GPU %d stopped (%s); the host reader goes on from record %llu\n", path,
                                gz_device, dr.handover_reason().c_str(), (unsigned long long)skip);
                    }
                    fell_back = true;
                    break;
                }
                if (!hb->error.empty()) {
                    rs->fail(NH_EIO, hb->error);
                    break;
                }
                const bool eof = hb->eof;
                out->push(std::move(hb));
                clk->ns[ST_RPUSH1 + which] += StageClock::now() - t1;
                if (eof || rs->failed()) break;
            }
            if (!fell_back) {
                out->close();
                dr.close();  // (waits for the batches still in the pipeline: they point into its buffers)
                return;
            }
            if (skip == 0) dr.close();
            else {
                // the batches it handed out are still in the pipeline and point into its buffers: the host reader starts now, the
                // device reader's buffers go when they are through (close() waits for them)
                BlockReader r;
                std::string err;
                if (r.open(path, err, gz_threads, -1) != 0) {
                    rs->fail(NH_EIO, err);
                    out->close();
                    dr.close();
                    return;
                }
                host_read(r, out, rs, pool, clk, which, batch_frags, batch_text, skip);
                out->close();
                dr.close();
                return;
            }
        }
    }
    BlockReader r;
    std::string err;
    // (the GPU inflates for the host parser only when asked for by name: "device-text", or "device" and the text is no FASTQ)
    const char *how = getenv("NOHUMAN_GZ_READER");
    if (r.open(path, err, gz_threads, how && (!strcmp(how, "device-text") || !strcmp(how, "device")) ? gz_device : -1) != 0) {
        rs->fail(NH_EIO, err);
        out->close();
        return;
    }
    host_read(r, out, rs, pool, clk, which, batch_frags, batch_text, 0);
    out->close();
}

static inline void put_record(std::string &dst, const char *text, int format, const RecRef &r, const char *suffix) {
    dst.append(text + r.h, r.hlen);
    if (suffix) dst += suffix;
    dst += '\n';
    dst.append(text + r.s, r.slen);
    if (format == FMT_FASTQ) {
        dst += "\n+\n";
        dst.append(text + r.q, r.qlen);
    }
    dst += '\n';
}

// decide + format one finished batch into the span lists of the output files (runs on the writer
// thread, batches arrive in input order)
// (emit false: a masked run -- its records are built on the device, only the counts and the -k lines are made here)
static void format_batch(RunState *rs, const Batch &b, const Slot &s, OutFile &o1, OutFile &o2, OutFile &ok, bool emit = true) {
    const nh_run_args *a = rs->a;
    const Engine *e = s.e;
    const bool keep_class = a->keep_human != 0;
    const char *t1 = b.fetch1 ? b.fetch1.get() : b.h1->text.data();
    const char *t2 = !rs->paired ? nullptr : b.fetch2 ? b.fetch2.get() : b.h2->text.data();
    char tmp[128];
    uint64_t bases = 0, classified = 0, hit_groups = 0, host = 0;
    const nh_result *const hres = s.host_res();  // (a host selection: call = 0 where the fragment is not host; else h_res)
    const RecRef *const R1 = b.h1->recs.data() + b.off1;
    const RecRef *const R2 = rs->paired ? b.h2->recs.data() + b.off2 : nullptr;
    for (size_t i = 0; i < b.n; i++) {
        const RecRef &r1 = R1[i];
        const uint32_t call = s.h_res[i].call;
        const bool is_class = call != 0;
        // host-ness decides what is emitted and how; the call what is reported (the counts, the -k line, the suffix): a spared
        // fragment -- classified, not host -- is written exactly as an unclassified one is
        const bool is_host = hres[i].call != 0;
        classified += is_class;
        host += is_host;
        hit_groups += s.h_res[i].hit_groups;
        rs->call_counts[call] += is_class;
        bases += r1.slen + (rs->paired ? R2[i].slen : 0);
        if (emit && is_host == keep_class) {
            if (!is_host && r1.raw_end) {
                o1.add_raw(t1 + r1.h, r1.raw_end - r1.h);
            } else {
                const char *suffix = nullptr;
                if (is_host) {
                    snprintf(tmp, sizeof tmp, " kraken:taxid|%llu", (unsigned long long)e->external[call]);
                    suffix = tmp;
                }
                const size_t from = o1.scratch.size();
                put_record(o1.scratch, t1, b.h1->format, r1, suffix);
                o1.add_scratch(from);
            }
            if (rs->paired) {
                const RecRef &r2 = R2[i];
                if (!is_host && r2.raw_end) {
                    o2.add_raw(t2 + r2.h, r2.raw_end - r2.h);
                } else {
                    const size_t from = o2.scratch.size();
                    put_record(o2.scratch, t2, b.h2->format, r2, is_host ? tmp : nullptr);
                    o2.add_scratch(from);
                }
            }
        }
        if (rs->want_k) {
            const uint64_t ext = is_class ? e->external[call] : 0;
            std::string &bufk = ok.scratch;
            std::string id(t1 + r1.h + 1, r1.idlen);
            if (rs->paired) trim_pair_info(id);
            bufk += is_class ? "C\t" : "U\t";
            bufk += id;
            snprintf(tmp, sizeof tmp, "\t%llu\t", (unsigned long long)ext);
            bufk += tmp;
            if (rs->paired)
                snprintf(tmp, sizeof tmp, "%u|%u\t", r1.slen, R2[i].slen);
            else
                snprintf(tmp, sizeof tmp, "%u\t", r1.slen);
            bufk += tmp;
            append_hitlist(bufk, e, s.h_taxa + s.h_taxa_off[i], s.h_taxa_off[i + 1] - s.h_taxa_off[i]);
            bufk += '\n';
        }
    }
    if (rs->want_k) ok.add_scratch(0);
    rs->total += b.n;
    rs->classified += classified;
    rs->host_frags += host;
    rs->spared_frags += classified - host;
    rs->hit_groups += hit_groups;
    rs->total_bases += bases;
    uint64_t *dc = &rs->dev_counts[4 * (size_t)b.dev_index];
    dc[0] += b.n;
    dc[1] += classified;
    dc[2] += bases;
}

// the engine's internal -> external taxon ids in its HBM (once per engine): the digits of "kraken:taxid|N" built there
static int ensure_device_external(Engine *e) {
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->d_external) return NH_OK;
    if (dev_set(e->device) != hipSuccess) return set_error(NH_EDEVICE, "hipSetDevice failed");
    const size_t n = std::max<size_t>(1, e->external.size());
    DevBuf<uint64_t> d;
    if (d.reserve(n) != hipSuccess) return set_error(NH_EOOM, "cannot allocate the taxon id table on device %d", e->device);
    if (!e->external.empty() && hipMemcpy(d, e->external.data(), e->external.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        return set_error(NH_EDEVICE, "cannot copy the taxon id table to device %d", e->device);
    e->d_external = d.p, d.p = nullptr;  // (the engine's from here on: it frees it with its other fields)
    return NH_OK;
}

// ---- the request of a whole run ------------------------------------------------------------------
// What an nh_run* entry was asked for, in one place: make_request fills it from the entry's arguments, check_request refuses a
// bad one before any device is touched, run_devices / run_engine / run_engines carry it out.
struct RunRequest {
    // the entry: nh_run_split and nh_run_mask take the human outputs as bare paths and always check them, nh_run_ex wants its
    // extras; RUN is nh_run and every entry from nh_run_minq upwards without extras (with extras they ask what nh_run_ex asks: EX)
    enum Form { RUN, SPLIT, MASK, EX } form = RUN;
    const char *who = "nh_run";  // the entry's name, for messages
    const nh_run_args *a = nullptr;
    // the run is paired: in2 is given, or in1 is a paired BAM (nh_bam.h).  Found once, by make_request; everything that asks reads it here
    bool paired = false;
    const nh_run_extras *x = nullptr;  // the caller's extras as given: what is wrong with the struct itself is said in check_request's order
    // hout1 set: a split run (nh_run_split) -- a->keep_human is 0, hout1 / hout2 receive the classified records
    const char *hout1 = nullptr, *hout2 = nullptr;
    // a masked run (nh_run_mask) -- a->keep_human is 0, out1 / out2 receive every record, a classified one's bases as 'N'
    bool mask = false;
    // set (nh_run_ex): the calls table / the human read ids, built in HBM beside whatever else the run writes
    const char *calls = nullptr, *ids = nullptr;
    // > 0 (nh_run_minq): kraken2's --minimum-base-quality -- the classifier reads a copy of each batch's sequences in which the
    // bases of a FASTQ record with a quality below minq are 'N' (k_qmask, in front of it on the slot's stream); every output is made
    // from the batch's text as before, so the records written keep their bases.  0: nothing of this runs.
    uint32_t minq = 0;
    // either set (nh_run_rstats): read statistics -- k_rstats behind the classifier on the slot's stream adds every sequence of the
    // batch to the device's four accumulators (nh_rstats.hip), fetched once, at the end; the writer keeps the lengths by class for
    // median and N50.  Both NULL: nothing of this runs.
    const char *rs_path = nullptr;
    nh_read_stats *rs_out = nullptr;
    // n_touts > 0 (nh_run_taxa): per-taxon outputs -- k_tout_* behind the classifier on the slot's stream sort the classified
    // records of the batch into the selectors' bins (nh_split.hip), a span a bin and mate goes to the selector's file.  0: nothing runs.
    nh_taxon_out *touts = nullptr;
    uint32_t n_touts = 0;
    // asking for something (nh_run_mdata): minimizer data -- k_mdata_mark behind the classifier on the slot's stream marks the cell
    // of every hit group in the device's bitmap and counts the group for its taxon (nh_mdata.hip), on the text the classifier read;
    // k_mdata_count reads the bitmap once, at the end (several devices: the union of their bitmaps -- a minimizer hit on two devices
    // is one).  NULL, or nothing asked for: nothing of this runs.
    nh_minimizer_data *md = nullptr;
    // set (nh_run_host with a taxid): the host selection -- k_host_filter behind the classifier on the slot's stream writes the
    // batch's results a second time, call = 0 where the fragment is not a host fragment (nh_host.hip); everything that removes, keeps,
    // masks, lists or counts HOST reads then reads that array (the writer its copy), everything that reports the CALL the
    // classifier's.  NULL: nothing of this runs.
    nh_host_filter *hf = nullptr;
    // given (nh_run_dust): the struct as the caller gave it -- check_request looks at its size --, and `dust` where it enables the
    // pass: every sequence of every batch is masked by symmetric DUST on its own (k_rdust in front of the classifier on the slot's
    // stream, behind the quality mask) in the copy the classifier and the minimizer data's marks read; the outputs keep the
    // input's bases, as with minq.  Not enabled: nothing of this runs.
    nh_read_dust *rd = nullptr;
    bool dust = false;
    // given (nh_run_intervals): the struct as the caller gave it -- check_request looks at its size --, and `hi_path` where it asks
    // for the report: k_cover_mark behind the classifier (and the host filter's table) on the slot's stream marks the bases that host
    // k-mers cover in the text the classifier read, k_cover_ivl_* / k_cover_line_* make the BED lines of the batch (nh_cover.hip).
    // No path: nothing of this runs.
    nh_host_intervals *hi = nullptr;
    const char *hi_path = nullptr;
    // given (nh_run_hostbases): the struct as the caller gave it -- check_request looks at its size --, and `hbo` where it enables the
    // mode: a masked run whose mask builder reads the batch's cover bitmap -- the same mark pass as the host intervals', then the
    // closing of the uncovered runs of at most hb->gap bases (nh_cover.hip) -- and writes 'N' over the covered bases of a host fragment
    // alone (nh_mask.hip).  Not enabled: nothing of this runs.
    nh_host_bases *hb = nullptr;
    bool hbo = false;
    // given (nh_run_hostcut): the struct as the caller gave it -- check_request looks at its size --, and `cut` where it enables the
    // mode: a single-end masked run with the same mark pass and closing (hc->gap), whose out1 is made by the cut builder (nh_cut.hip):
    // a host fragment as its uncovered pieces of at least hc->min_piece bases, every other fragment whole.  Not enabled: nothing runs.
    nh_host_cut *hc = nullptr;
    bool cut = false;
};

// The request of an entry: its args, its extras (NULL where it has none, or was given none) or the bare human paths of
// nh_run_split / nh_run_mask, and as much of nh_run_host's tail as the entry has
RunRequest make_request(RunRequest::Form form, const nh_run_args *a, const nh_run_extras *x, const char *h1 = nullptr, const char *h2 = nullptr,
                        uint32_t minq = 0, const char *rs_path = nullptr, nh_read_stats *rs_out = nullptr, nh_taxon_out *touts = nullptr,
                        uint32_t n_touts = 0, nh_minimizer_data *md = nullptr, nh_host_filter *hf = nullptr, nh_read_dust *rd = nullptr,
                        nh_host_intervals *hi = nullptr, nh_host_bases *hb = nullptr, nh_host_cut *hc = nullptr) {
    static const char *const names[] = {"nh_run", "nh_run_split", "nh_run_mask", "nh_run_ex"};
    RunRequest r;
    r.form = form == RunRequest::RUN && x ? RunRequest::EX : form;
    r.who = names[r.form];
    r.a = a, r.x = x;
    r.paired = a && (a->in2 || (a->in1 && bam_paired(a->in1)));
    r.hout1 = h1, r.hout2 = h2, r.mask = form == RunRequest::MASK;
    if (x && x->struct_size >= sizeof(nh_run_extras))  // (a smaller struct: check_request refuses it, nothing else of it is read)
        r.hout1 = x->human_out1, r.hout2 = x->human_out2, r.mask = x->mask != 0, r.calls = x->calls, r.ids = x->human_ids;
    r.minq = minq, r.rs_path = rs_path, r.rs_out = rs_out, r.touts = touts, r.n_touts = n_touts, r.md = md;
    r.hf = host_filter_given(hf) ? hf : nullptr;  // (no taxid listed: the run of nh_run_mdata, and the struct is not looked at again)
    r.rd = rd, r.dust = rd && rd->struct_size >= sizeof(nh_read_dust) && rd->enable != 0;
    r.hi = hi, r.hi_path = hi && hi->struct_size >= sizeof(nh_host_intervals) ? hi->path : nullptr;
    r.hb = hb, r.hbo = hb && hb->struct_size >= sizeof(nh_host_bases) && hb->enable != 0;
    r.hc = hc, r.cut = hc && hc->struct_size >= sizeof(nh_host_cut) && hc->enable != 0;
    return r;
}

// ---- the files a request names ----------------------------------------------------------------------
// `candidate` names the file `other` names: the same string, or candidate is an existing regular file and other has its device and
// inode.  (Which of the two is tested for being regular cannot be seen: two names of one inode have one mode.)
static bool same_file(const char *candidate, const char *other) {
    if (!strcmp(candidate, other)) return true;
    struct stat sc, so;
    return stat(candidate, &sc) == 0 && S_ISREG(sc.st_mode) && stat(other, &so) == 0 && so.st_dev == sc.st_dev && so.st_ino == sc.st_ino;
}

// One file of a request.  The kinds are in the order of the checks: a feature's files are checked against the files of the kinds
// before it (and the read lists and the selectors' files among themselves).
enum FileKind { F_INPUT, F_OUTPUT, F_HUMAN, F_LIST, F_RSTATS, F_TAXON, F_MDATA, F_COVER };
struct RunFile {
    const char *path;   // never NULL; may be empty
    FileKind kind;
    const char *who;    // the words of a message about it: "<who>: <words> <path> is the input ..."
    std::string words;
};

// The files r names, inputs first, of the kinds up to `last` -- what is behind it may not have been checked yet (r.a is not NULL)
static std::vector<RunFile> request_files(const RunRequest &r, FileKind last) {
    std::vector<RunFile> f;
    auto add = [&](const char *p, FileKind k, const char *who, std::string words) {
        if (p && k <= last) f.push_back({p, k, who, std::move(words)});
    };
    const nh_run_args *a = r.a;
    for (const char *p : {a->in1, a->in2}) add(p, F_INPUT, "nh_run", "input");
    for (const char *p : {a->out1, a->out2, a->kraken_output, a->report}) add(p, F_OUTPUT, r.mask ? "nh_run_mask" : "nh_run", "output");
    for (const char *p : {r.hout1, r.hout2}) add(p, F_HUMAN, r.mask ? "nh_run_mask" : "nh_run_split", "human output");
    add(r.calls, F_LIST, "nh_run_ex", "calls");
    add(r.ids, F_LIST, "nh_run_ex", "human_ids");
    add(r.rs_path, F_RSTATS, "nh_run_rstats", "the read statistics table");
    for (uint32_t i = 0; last >= F_TAXON && r.touts && i < r.n_touts; i++)
        for (int m = 0; m < 2; m++) add(m ? r.touts[i].out2 : r.touts[i].out1, F_TAXON, "nh_run_taxa", "outs[" + std::to_string(i) + "].out" + std::to_string(m + 1));
    if (last >= F_MDATA && r.md) add(r.md->table, F_MDATA, "nh_run_mdata", "the minimizer table");
    add(r.hi_path, F_COVER, "nh_run_intervals", "the host intervals' file");
    return f;
}

// files[c] against the `upto` files in front: NH_EINVAL, with c's words, for the first that it also names.  (An output given as
// an empty path is not written: it collides with nothing.  An input is compared as it is.)
static int check_collision(const std::vector<RunFile> &files, size_t c, size_t upto) {
    const RunFile &f = files[c];
    for (size_t i = 0; i < upto; i++) {
        const RunFile &o = files[i];
        if ((o.kind != F_INPUT && !o.path[0]) || !same_file(f.path, o.path)) continue;
        if (o.kind == F_INPUT) return set_error(NH_EINVAL, "%s: %s %s is the input %s", f.who, f.words.c_str(), f.path, o.path);
        if (o.kind == F_LIST && f.kind == F_LIST) return set_error(NH_EINVAL, "nh_run_ex: calls and human_ids are the same file %s", f.path);
        if (o.kind == F_TAXON && f.kind == F_TAXON) return set_error(NH_EINVAL, "%s: %s %s is also %s", f.who, f.words.c_str(), f.path, o.words.c_str());
        return set_error(NH_EINVAL, "%s: %s %s is also the output %s", f.who, f.words.c_str(), f.path, o.path);
    }
    return NH_OK;
}

// every file of `kind` against the files of the kinds before it; the read lists and the selectors' files also against the earlier
// ones of their own kind (human_out1 against human_out2 is check_split_args' own test, by name only)
static int check_files(const RunRequest &r, FileKind kind) {
    const std::vector<RunFile> files = request_files(r, kind);
    size_t first = 0;
    while (first < files.size() && files[first].kind != kind) first++;
    for (size_t c = first; c < files.size(); c++)
        if (const int rc = check_collision(files, c, kind == F_LIST || kind == F_TAXON ? c : first)) return rc;
    return NH_OK;
}

// ---- check_request: what is wrong with a request, said before any device is touched -----------------
// the human outputs of a split run, and of a masked run that has them
static int check_split_args(const RunRequest &r) {
    const nh_run_args *a = r.a;
    const char *h1 = r.hout1, *h2 = r.hout2, *who = r.mask ? "nh_run_mask" : "nh_run_split";
    if (!h1 || !h1[0]) return set_error(NH_EINVAL, "%s: human_out1 is required", who);
    if (a->keep_human != 0) return set_error(NH_EINVAL, "%s: keep_human must be 0 (the human reads go to human_out1 / human_out2)", who);
    // (BAM output of a paired BAM: one file holds both mates -- check_out_codec refuses a human_out2 there)
    if (r.paired && !h2 && a->out_codec != NH_CODEC_BAM) return set_error(NH_EINVAL, "%s: paired input needs human_out2", who);
    if (!r.paired && h2) return set_error(NH_EINVAL, "%s: human_out2 is given without in2", who);
    if (h2 && !strcmp(h1, h2)) return set_error(NH_EINVAL, "%s: human_out1 and human_out2 are the same file", who);
    return check_files(r, F_HUMAN);
}

// a masked run: out1 / out2 receive every record, so none of the run's own outputs may be an input
static int check_mask_args(const RunRequest &r) {
    if (r.a->keep_human != 0) return set_error(NH_EINVAL, "nh_run_mask: keep_human must be 0 (the human reads are masked, not kept)");
    if (r.hout1 || r.hout2) {
        const int rc = check_split_args(r);
        if (rc) return rc;
    }
    const std::vector<RunFile> files = request_files(r, F_OUTPUT);
    size_t inputs = 0;
    while (inputs < files.size() && files[inputs].kind == F_INPUT) inputs++;
    for (size_t c = inputs; c < files.size(); c++)
        if (files[c].path[0])
            if (const int rc = check_collision(files, c, inputs)) return rc;
    return NH_OK;
}

// the read lists (the calls table, the human ids): a list names no input and no other output of the run
static int check_list_args(const RunRequest &r) {
    const std::vector<RunFile> files = request_files(r, F_LIST);
    for (size_t c = 0; c < files.size(); c++) {
        if (files[c].kind != F_LIST) continue;
        if (!files[c].path[0]) return set_error(NH_EINVAL, "nh_run_ex: %s is an empty path", files[c].words.c_str());
        if (const int rc = check_collision(files, c, c)) return rc;
    }
    return NH_OK;
}

// what nh_run_ex checks, and nh_run_split / nh_run_mask for the fields they share with it: the struct, the human outputs or the
// mask, the read lists
static int check_extras(const RunRequest &r) {
    if (!r.a) return set_error(NH_EINVAL, "%s: null arguments", r.who);
    if (r.form == RunRequest::EX) {
        if (!r.x) return set_error(NH_EINVAL, "nh_run_ex: null extras");
        if (r.x->struct_size < sizeof(nh_run_extras))
            return set_error(NH_EINVAL, "nh_run_ex: struct_size %u is smaller than nh_run_extras (%zu bytes)", r.x->struct_size, sizeof(nh_run_extras));
    }
    int rc = NH_OK;
    if (r.mask) rc = check_mask_args(r);
    else if (r.hout1 || r.hout2 || r.form == RunRequest::SPLIT) rc = check_split_args(r);
    if (rc) return rc;
    return check_list_args(r);
}

// nh_run_rstats' table: it names no input and no other output of the run
static int check_rstats_args(const RunRequest &r) {
    if (!r.rs_path) return NH_OK;
    if (!r.a) return set_error(NH_EINVAL, "nh_run_rstats: null arguments");
    if (!r.rs_path[0]) return set_error(NH_EINVAL, "nh_run_rstats: read_stats_path is an empty path");
    return check_files(r, F_RSTATS);
}

// nh_run_taxa's selectors: their number, their taxids, their files -- a per-taxon file names no input and no other output of the run
static int check_taxon_args(const RunRequest &r) {
    const nh_run_args *a = r.a;
    const nh_taxon_out *outs = r.touts;
    const uint32_t n = r.n_touts;
    if (n == 0) return NH_OK;
    if (!a) return set_error(NH_EINVAL, "nh_run_taxa: null arguments");
    if (n > NH_MAX_TAXON_OUTS) return set_error(NH_EINVAL, "nh_run_taxa: n_outs %u is above NH_MAX_TAXON_OUTS (%d)", n, NH_MAX_TAXON_OUTS);
    if (!outs) return set_error(NH_EINVAL, "nh_run_taxa: outs is NULL with n_outs %u", n);
    if (a->keep_human != 0) return set_error(NH_EINVAL, "nh_run_taxa: keep_human must be 0 (the classified reads go to the selectors' files)");
    for (uint32_t i = 0; i < n; i++) {
        const nh_taxon_out &t = outs[i];
        if (!t.out1 || !t.out1[0]) return set_error(NH_EINVAL, "nh_run_taxa: outs[%u].out1 is required", i);
        if (t.out2 && !t.out2[0]) return set_error(NH_EINVAL, "nh_run_taxa: outs[%u].out2 is an empty path", i);
        if (r.paired && !t.out2) return set_error(NH_EINVAL, "nh_run_taxa: paired input needs outs[%u].out2", i);
        if (!r.paired && t.out2) return set_error(NH_EINVAL, "nh_run_taxa: outs[%u].out2 is given without in2", i);
        for (uint32_t j = 0; j < i; j++)
            if (outs[j].taxid == t.taxid) {
                if (t.taxid == NH_TAXON_OTHER) return set_error(NH_EINVAL, "nh_run_taxa: outs[%u].taxid: `other` is given twice", i);
                return set_error(NH_EINVAL, "nh_run_taxa: outs[%u].taxid %llu is given twice", i, (unsigned long long)t.taxid);
            }
    }
    return check_files(r, F_TAXON);
}

// nh_run_mdata's own arguments: the struct, and a table that names no input and no other output of the run
static int check_mdata_args(const RunRequest &r) {
    const nh_minimizer_data *md = r.md;
    if (!md) return NH_OK;
    if (md->struct_size < sizeof(nh_minimizer_data))
        return set_error(NH_EINVAL, "nh_run_mdata: struct_size %u is smaller than nh_minimizer_data (%zu bytes)", md->struct_size, sizeof(nh_minimizer_data));
    if (!r.a) return set_error(NH_EINVAL, "nh_run_mdata: null arguments");
    if (md->in_report && !(r.a->report && r.a->report[0])) return set_error(NH_EINVAL, "nh_run_mdata: in_report is set without a report (args->report)");
    if (md->taxa && md->taxa_cap == 0) return set_error(NH_EINVAL, "nh_run_mdata: taxa is given with taxa_cap 0");
    if (md->table && !md->table[0]) return set_error(NH_EINVAL, "nh_run_mdata: table is an empty path");
    return check_files(r, F_MDATA);
}

// nh_run_intervals' own arguments: the struct, and a file that names no input and no other output of the run
static int check_cover_args(const RunRequest &r) {
    const nh_host_intervals *hi = r.hi;
    if (!hi) return NH_OK;
    if (hi->struct_size < sizeof(nh_host_intervals))
        return set_error(NH_EINVAL, "nh_run_intervals: struct_size %u is smaller than nh_host_intervals (%zu bytes)", hi->struct_size, sizeof(nh_host_intervals));
    if (!r.hi_path) return NH_OK;
    if (!r.a) return set_error(NH_EINVAL, "nh_run_intervals: null arguments");
    if (!r.hi_path[0]) return set_error(NH_EINVAL, "nh_run_intervals: path is an empty path");
    return check_files(r, F_COVER);
}

// nh_run_hostbases' own arguments: the struct, a masked run, the gap
static int check_hostbases_args(const RunRequest &r) {
    const nh_host_bases *hb = r.hb;
    if (!hb) return NH_OK;
    if (hb->struct_size < sizeof(nh_host_bases))
        return set_error(NH_EINVAL, "nh_run_hostbases: struct_size %u is smaller than nh_host_bases (%zu bytes)", hb->struct_size, sizeof(nh_host_bases));
    if (!r.hbo) return NH_OK;
    if (!r.a) return set_error(NH_EINVAL, "nh_run_hostbases: null arguments");
    if (!r.mask) return set_error(NH_EINVAL, "nh_run_hostbases: enable is set without a masked run (extras->mask): the mode writes every read, host bases as N");
    if (hb->gap > NH_HOST_GAP_MAX) return set_error(NH_EINVAL, "nh_run_hostbases: gap %u is above NH_HOST_GAP_MAX (%d)", hb->gap, NH_HOST_GAP_MAX);
    return NH_OK;
}

// nh_run_hostcut's own arguments: the struct, a masked run that is not a host-bases-only run, the gap, the shortest piece, one input
static int check_hostcut_args(const RunRequest &r) {
    const nh_host_cut *hc = r.hc;
    if (!hc) return NH_OK;
    if (hc->struct_size < sizeof(nh_host_cut))
        return set_error(NH_EINVAL, "nh_run_hostcut: struct_size %u is smaller than nh_host_cut (%zu bytes)", hc->struct_size, sizeof(nh_host_cut));
    if (!r.cut) return NH_OK;
    if (!r.a) return set_error(NH_EINVAL, "nh_run_hostcut: null arguments");
    if (!r.mask) return set_error(NH_EINVAL, "nh_run_hostcut: enable is set without a masked run (extras->mask): the mode writes every read, host reads as their pieces");
    if (r.hbo) return set_error(NH_EINVAL, "nh_run_hostcut: enable is set together with an enabled nh_host_bases: a host stretch is cut out or written as N, not both");
    if (hc->gap > NH_HOST_GAP_MAX) return set_error(NH_EINVAL, "nh_run_hostcut: gap %u is above NH_HOST_GAP_MAX (%d)", hc->gap, NH_HOST_GAP_MAX);
    if (hc->min_piece == 0 || hc->min_piece > 0x7FFFFFFFu) return set_error(NH_EINVAL, "nh_run_hostcut: min_piece %u is not in 1..2147483647", hc->min_piece);
    if (r.paired)
        return set_error(NH_EINVAL, "nh_run_hostcut: paired input (%s): the mode is single-end only, the pieces of two mates cannot stay in step",
                         r.a->in2 ? "in2 is given" : "in1 is a paired BAM");
    return NH_OK;
}

// The container of the record outputs: a codec there is none of, and what BAM output (NH_CODEC_BAM: the selected records of a BAM
// in1, copied) does not go with -- a second input, a masked run, per-taxon outputs (the last two: not built yet), an in1 that is
// no BAM file.  (A request without arguments is refused by its entry.)
static int check_out_codec(const RunRequest &r) {
    const nh_run_args *a = r.a;
    if (!a) return NH_OK;
    if (a->out_codec < NH_CODEC_NONE || a->out_codec > NH_CODEC_BAM) return set_error(NH_EINVAL, "nh_run: unknown out_codec %d", a->out_codec);
    // (a paired BAM makes a paired run without an in2: said here, before any device is touched; with an in2 run_engines says it)
    if (a->out_codec != NH_CODEC_BAM && r.paired && !a->in2 && !a->out2) return set_error(NH_EINVAL, "nh_run: paired input needs out2");
    if (a->out_codec != NH_CODEC_BAM) return NH_OK;
    if (a->in2) return set_error(NH_EINVAL, "nh_run: BAM output (out_codec %d) with in2 %s: BAM input is single-end, so is BAM output", NH_CODEC_BAM, a->in2);
    if (r.paired && a->out2) return set_error(NH_EINVAL, "nh_run: BAM output (out_codec %d) of a paired BAM with out2 %s: one BAM file holds both mates", NH_CODEC_BAM, a->out2);
    if (r.paired && r.hout2)
        return set_error(NH_EINVAL, "nh_run: BAM output (out_codec %d) of a paired BAM with human_out2 %s: one BAM file holds both mates", NH_CODEC_BAM, r.hout2);
    if (r.mask) return set_error(NH_EINVAL, "nh_run_mask: BAM output (out_codec %d) of a masked run is not supported: a masked record is not a record of the input", NH_CODEC_BAM);
    if (r.n_touts) return set_error(NH_EINVAL, "nh_run_taxa: BAM output (out_codec %d) with per-taxon outputs is not supported", NH_CODEC_BAM);
    if (!a->in1 || !bam_wants(a->in1))
        return set_error(NH_EINVAL, "nh_run: BAM output (out_codec %d) needs a BAM in1: %s is not a BAM file, and a FASTQ record has no BAM record to copy",
                         NH_CODEC_BAM, a->in1 ? a->in1 : "(null)");
    return NH_OK;
}

// Every entry's checks, in one order: the host selection's own, the minimum base quality (the highest printable quality is '~',
// Phred 93), the read DUST's struct, the extras (the mask or the human outputs, then the read lists), the read statistics' table, the selectors, the
// minimizer data, the host intervals, the host bases, the host cut, the container.  What an entry cannot ask for is not set in its request and checks nothing.
int check_request(const RunRequest &r) {
    int rc = check_host_filter(r.hf);
    if (!rc && r.minq > 93) rc = set_error(NH_EINVAL, "minimum base quality %u is not in 0..93 (Phred+33)", r.minq);
    if (!rc && r.rd && r.rd->struct_size < sizeof(nh_read_dust))
        rc = set_error(NH_EINVAL, "nh_run_dust: struct_size %u is smaller than nh_read_dust (%zu bytes)", r.rd->struct_size, sizeof(nh_read_dust));
    if (!rc && r.form != RunRequest::RUN) rc = check_extras(r);
    if (!rc) rc = check_rstats_args(r);
    if (!rc) rc = check_taxon_args(r);
    if (!rc) rc = check_mdata_args(r);
    if (!rc) rc = check_cover_args(r);
    if (!rc) rc = check_hostbases_args(r);
    if (!rc) rc = check_hostcut_args(r);
    if (!rc) rc = check_out_codec(r);
    return rc;
}
// A BAM is one input, paired or not: NH_EINVAL -- before any device is touched -- for a BAM in1 beside an in2, and for a BAM in2
int check_bam_inputs(const nh_run_args *a) {
    if (!a || !a->in2) return NH_OK;
    if (bam_wants(a->in2)) return set_error(NH_EINVAL, "nh_run: in2 %s is a BAM file: BAM input is single-end, give it alone as in1", a->in2);
    if (a->in1 && bam_wants(a->in1))
        return set_error(NH_EINVAL, "nh_run: in1 %s is a BAM file and in2 is given: BAM input is single-end (split a paired BAM with `samtools fastq -1 -2`)", a->in1);
    return NH_OK;
}

// ---- the parts of a run that happen once, before the first batch or after the last ------------------
// The output files of a run
struct RunFiles {
    OutFile o1, o2, ok;  // the kept records of mate 1 / mate 2, the per-read kraken output
    OutFile h1, h2;      // the classified records of a split run
    OutFile oc, oi;      // the read lists (calls, human ids): plain text whatever the codec of the records
    OutFile ohi;         // the host intervals: plain text as well
    OutFile tx[2][NH_MAX_TAXON_OUTS];  // the selectors' files, [mate][selector]
};

// fn(file, i) on out1 [0] and, side by side with it on threads of their own, on out2 [1] and the human outputs of a split run [2],
// [3]: a GPU encoder takes 70 ms to set up -- page-locked buffers, a trial of its prices -- and its last chunks as long to finish.
// The first error in that order.
template <class F>
static int record_files_side_by_side(RunFiles &f, bool paired, bool split_files, F fn) {
    OutFile *const of[4] = {&f.o1, paired ? &f.o2 : nullptr, split_files ? &f.h1 : nullptr, split_files && paired ? &f.h2 : nullptr};
    int rc[4] = {NH_OK, NH_OK, NH_OK, NH_OK};
    std::string err[4];
    std::thread t[4];
    for (int i = 1; i < 4; i++)
        if (of[i])
            t[i] = std::thread([&, i] {
                rc[i] = fn(*of[i], i);
                if (rc[i]) err[i] = g_last_error;
            });
    rc[0] = fn(f.o1, 0);
    for (std::thread &x : t)
        if (x.joinable()) x.join();
    for (int i = 1; i < 4 && !rc[0]; i++)
        if (rc[i]) return set_error(rc[i], "%s", err[i].c_str());
    return rc[0];
}

// Creates them.  gzip output is encoded on the GPU (nh_deflate.hip); with two devices each mate file has its own: mate 1's files on
// the first device, mate 2's on the second.
static int open_run_files(RunFiles &f, const RunRequest &r, const std::vector<Engine *> &engines, bool paired, bool want_k) {
    const nh_run_args *a = r.a;
    const int dev1 = engines[0]->device, dev2 = engines[engines.size() > 1 ? 1 : 0]->device;
    const char *const paths[4] = {a->out1, a->out2, r.hout1, r.hout2};
    int rc = record_files_side_by_side(f, paired, r.hout1 != nullptr,
                                       [&](OutFile &of, int i) { return of.open(paths[i], a->out_codec, a->codec_threads, i & 1 ? dev2 : dev1); });
    if (rc) return rc;
    for (uint32_t k = 0; k < r.n_touts; k++)
        for (int m = 0; m < (paired ? 2 : 1); m++)
            if ((rc = f.tx[m][k].open(m ? r.touts[k].out2 : r.touts[k].out1, a->out_codec, a->codec_threads, m ? dev2 : dev1))) return rc;
    if (want_k && (rc = f.ok.open(a->kraken_output))) return rc;
    if (r.calls && (rc = f.oc.open(r.calls))) return rc;
    if (r.ids && (rc = f.oi.open(r.ids))) return rc;
    if (r.hi_path && (rc = f.ohi.open(r.hi_path))) return rc;
    return NH_OK;
}

// per-taxon outputs: the bin of every node of the taxonomy -- its deepest selected ancestor-or-self, else `other`'s, else none
static int selector_bins(const Engine *e0, const RunRequest &r, std::vector<uint8_t> &bin_of) {
    const size_t nn = e0->external.size();
    bin_of.assign(std::max<size_t>(nn, 1), 0xFF);
    std::vector<int> own(nn, -1);
    int other = -1;
    for (int k = 0; k < (int)r.n_touts; k++) {
        if (r.touts[k].taxid == NH_TAXON_OTHER) {
            other = k;
            continue;
        }
        size_t at = 0;
        for (size_t i = 1; i < nn && !at; i++)
            if (e0->external[i] == r.touts[k].taxid) at = i;
        if (!at) return set_error(NH_EINVAL, "nh_run_taxa: taxid %llu is not in the database's taxonomy", (unsigned long long)r.touts[k].taxid);
        own[at] = k;
    }
    for (size_t i = 1; i < nn; i++) {  // (parents have smaller ids than their children: nh_open checked)
        const uint32_t p = e0->parent[i];
        bin_of[i] = own[i] >= 0 ? (uint8_t)own[i] : (i > 1 && p >= 1 && p < i) ? bin_of[p] : other >= 0 ? (uint8_t)other : (uint8_t)0xFF;
    }
    return NH_OK;
}

// What one device holds for the whole run, given back when the run's scope ends
struct RunBuffers {
    int device = -1;
    DevBuf<uint64_t> counters;  // the counters the classify kernels of this run add to (RunState::d_run_counters points here)
    DevBuf<uint8_t> bin_of;     // per-taxon outputs: the selectors' bins
    // host selection: host_of, and the pair of counters {host, spared} k_host_filter adds to
    DevBuf<uint8_t> host_of;
    DevBuf<unsigned long long> hcnt;
    DevBuf<unsigned long long> racc;  // read statistics: one block of four accumulators, zeroed with min_len all-ones
    // host bases only: {host, masked, closed} bases the mask builder and the closing add to; host cut: [2] closed, then CUT_COUNTS words
    DevBuf<unsigned long long> hbcnt;
    // minimizer data: one zeroed bitmap (a bit a cell) and one array of hit groups per node
    DevBuf<uint32_t> marks;
    DevBuf<unsigned long long> groups;
    RunBuffers() = default;
    ~RunBuffers() {  // (the members go back behind this, under their device)
        if (device >= 0) (void)dev_set(device);
    }
};

// (hipMemcpy / hipMemset block: the tables and the zeroes are in place before the slots' streams, which do not wait for the legacy
// stream, carry the first batch)
static int alloc_run_buffers(RunBuffers &b, const Engine *e, const std::vector<uint8_t> &bin_of, const std::vector<uint8_t> &host_of, bool rst,
                             size_t md_mark_bytes, size_t md_nodes, bool mdt, size_t hb_words) {
    b.device = e->device;
    const size_t nc = CNT_N + 12, nb = nc * sizeof(uint64_t);  // (+12: the words of the instrumented kernel variant)
    if (dev_set(e->device) != hipSuccess || b.counters.reserve(nc) != hipSuccess || hipMemset(b.counters, 0, nb) != hipSuccess)
        return set_error(NH_EDEVICE, "cannot allocate the run's counters on device %d", e->device);
    if (!bin_of.empty() && (b.bin_of.reserve(bin_of.size()) != hipSuccess ||
                            hipMemcpy(b.bin_of, bin_of.data(), bin_of.size(), hipMemcpyHostToDevice) != hipSuccess))
        return set_error(NH_EDEVICE, "cannot copy the selectors' bins to device %d", e->device);
    if (!host_of.empty() && (b.host_of.reserve(host_of.size()) != hipSuccess || b.hcnt.reserve(2) != hipSuccess ||
                             hipMemcpy(b.host_of, host_of.data(), host_of.size(), hipMemcpyHostToDevice) != hipSuccess ||
                             hipMemset(b.hcnt, 0, 16) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
        return set_error(NH_EDEVICE, "cannot copy the host selection's table to device %d", e->device);
    if (rst) {
        nh_read_class init[4];
        memset(init, 0, sizeof init);
        for (nh_read_class &c : init) c.min_len = ~0ull;
        if (b.racc.reserve(sizeof init / 8) != hipSuccess || hipMemcpy(b.racc, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess)
            return set_error(NH_EDEVICE, "cannot allocate the read statistics' accumulators on device %d", e->device);
    }
    if (hb_words && (dev_set(e->device) != hipSuccess || b.hbcnt.reserve(hb_words) != hipSuccess || hipMemset(b.hbcnt, 0, 8 * hb_words) != hipSuccess ||
                hipDeviceSynchronize() != hipSuccess))
        return set_error(NH_EDEVICE, "cannot allocate the host bases' counters on device %d", e->device);
    if (mdt) {
        const size_t mark_words = std::max<size_t>((md_mark_bytes + 3) / 4, 1), n_groups = std::max<size_t>(md_nodes, 1);
        if (b.marks.reserve(mark_words) != hipSuccess || b.groups.reserve(n_groups) != hipSuccess)
            return set_error(NH_EOOM, "minimizer data: cannot allocate the bitmap of %zu bytes and %zu counters on device %d", md_mark_bytes, md_nodes,
                             e->device);
        if (hipMemset(b.marks, 0, std::max<size_t>(md_mark_bytes, 4)) != hipSuccess ||
            hipMemset(b.groups, 0, std::max<size_t>(md_nodes, 1) * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return set_error(NH_EDEVICE, "minimizer data: cannot clear the bitmap on device %d", e->device);
    }
    return NH_OK;
}

// ---- after the writer threads are joined: what the devices counted over the whole run, fetched once.  (Every stream has been
// synchronised by the writer, or the run has failed: each step runs only while it has not, and fails it with its own words.)
// the bases k_qmask replaced
static void collect_qmask(std::vector<Slot> &slots, RunState &rs) {
    for (auto &s : slots)
        if (s.d_qcnt && rs.err_code == NH_OK) {
            unsigned long long c = 0;
            if (dev_set(s.e->device) == hipSuccess && hipMemcpy(&c, s.d_qcnt, 8, hipMemcpyDeviceToHost) == hipSuccess) rs.qmask_masked += c;
        }
}

// the bases k_rdust masked
static void collect_dust(std::vector<Slot> &slots, RunState &rs) {
    for (auto &s : slots)
        if (s.d_dcnt && rs.err_code == NH_OK) {
            unsigned long long c = 0;
            if (dev_set(s.e->device) == hipSuccess && hipMemcpy(&c, s.d_dcnt, 8, hipMemcpyDeviceToHost) == hipSuccess) rs.dust_masked += c;
            else rs.fail(NH_EDEVICE, "reading the read DUST's counter failed");
        }
}

// host selection: the devices' {host, spared} fragments summed into dev_host
static void collect_host_counts(const std::vector<RunBuffers> &dbuf, RunState &rs, uint64_t dev_host[2]) {
    for (size_t g = 0; g < dbuf.size() && rs.err_code == NH_OK; g++) {
        unsigned long long c[2] = {0, 0};
        if (dev_set(dbuf[g].device) != hipSuccess || hipMemcpy(c, dbuf[g].hcnt, 16, hipMemcpyDeviceToHost) != hipSuccess) {
            rs.fail(NH_EDEVICE, "reading the host filter's counters failed");
            break;
        }
        dev_host[0] += c[0], dev_host[1] += c[1];
    }
    // (the fragments the writer saw as host and as spared are the checker of what the kernel counted, as for the run's counters)
    if (rs.err_code == NH_OK && (dev_host[0] != rs.host_frags || dev_host[1] != rs.spared_frags)) {
        char msg[200];
        snprintf(msg, sizeof msg, "host filter: the devices counted %llu host / %llu spared fragments, the writer %llu / %llu", (unsigned long long)dev_host[0],
                 (unsigned long long)dev_host[1], (unsigned long long)rs.host_frags, (unsigned long long)rs.spared_frags);
        rs.fail(NH_EDEVICE, msg);
    }
}

// host bases only: the devices' {host, masked, closed} bases summed into the run's
static void collect_hostbases(const std::vector<RunBuffers> &dbuf, RunState &rs) {
    for (size_t g = 0; g < dbuf.size() && rs.err_code == NH_OK; g++) {
        unsigned long long c[3] = {0, 0, 0};
        if (dev_set(dbuf[g].device) != hipSuccess || hipMemcpy(c, dbuf[g].hbcnt, 24, hipMemcpyDeviceToHost) != hipSuccess) {
            rs.fail(NH_EDEVICE, "reading the host bases' counters failed");
            break;
        }
        for (int k = 0; k < 3; k++) rs.hb_bases[k] += c[k];
    }
    // (the bases of the fragments the writer saw as host are the checker of what the builder counted)
    if (rs.err_code == NH_OK && rs.hb_bases[0] != rs.hb_host_written) {
        char msg[200];
        snprintf(msg, sizeof msg, "host bases only: the devices counted %llu host bases, the writer %llu", (unsigned long long)rs.hb_bases[0],
                 (unsigned long long)rs.hb_host_written);
        rs.fail(NH_EDEVICE, msg);
    }
}

// host cut: the devices' closed bases and CUT_COUNTS counts summed into the run's, and the identities they must keep
static void collect_hostcut(const std::vector<RunBuffers> &dbuf, RunState &rs) {
    for (size_t g = 0; g < dbuf.size() && rs.err_code == NH_OK; g++) {
        unsigned long long c[3 + CUT_COUNTS] = {};
        if (dev_set(dbuf[g].device) != hipSuccess || hipMemcpy(c, dbuf[g].hbcnt, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) {
            rs.fail(NH_EDEVICE, "reading the host cut's counters failed");
            break;
        }
        rs.hb_bases[2] += c[2];
        for (int k = 0; k < CUT_COUNTS; k++) rs.cut_counts[k] += c[3 + k];
    }
    if (rs.err_code != NH_OK) return;
    const uint64_t *c = rs.cut_counts;
    char msg[240];
    // (the bases of the fragments the writer saw as host are the checker of what the builder counted)
    if (c[CUT_HOST_BASES] != rs.hb_host_written) {
        snprintf(msg, sizeof msg, "host cut: the devices counted %llu host bases, the writer %llu", (unsigned long long)c[CUT_HOST_BASES],
                 (unsigned long long)rs.hb_host_written);
        rs.fail(NH_EDEVICE, msg);
    } else if (c[CUT_HOST_BASES] != c[CUT_PIECE_BASES] + c[CUT_CUT_BASES] + c[CUT_SHORT_BASES]) {
        snprintf(msg, sizeof msg, "host cut: %llu host bases are not %llu in pieces + %llu cut + %llu in short runs", (unsigned long long)c[CUT_HOST_BASES],
                 (unsigned long long)c[CUT_PIECE_BASES], (unsigned long long)c[CUT_CUT_BASES], (unsigned long long)c[CUT_SHORT_BASES]);
        rs.fail(NH_EDEVICE, msg);
    }
}

// read statistics: the devices' accumulators, rows summed on the host into racc: [class][mate]
static void collect_rstats(const std::vector<RunBuffers> &dbuf, RunState &rs, std::vector<nh_read_class> &racc) {
    if (rs.err_code != NH_OK) return;
    racc.assign(4, nh_read_class{});
    for (nh_read_class &c : racc) c.min_len = ~0ull;
    for (size_t g = 0; g < dbuf.size() && rs.err_code == NH_OK; g++) {
        nh_read_class part[4];
        if (dev_set(dbuf[g].device) != hipSuccess || hipMemcpy(part, dbuf[g].racc, sizeof part, hipMemcpyDeviceToHost) != hipSuccess) {
            rs.fail(NH_EDEVICE, "reading the read statistics' accumulators failed");
            break;
        }
        for (int k = 0; k < 4; k++) {
            const uint64_t *src = (const uint64_t *)&part[k];
            uint64_t *dst = (uint64_t *)&racc[k];
            for (size_t w = 0; w < sizeof(nh_read_class) / 8; w++)
                if (w == 2) dst[w] = std::min(dst[w], src[w]);
                else if (w == 3) dst[w] = std::max(dst[w], src[w]);
                else dst[w] += src[w];
        }
    }
}

// minimizer data: the hit groups of the devices are added; their bitmaps are NOT counted one by one -- a minimizer hit on two
// devices is one -- but ORed on the host and the union counted on the first engine.  mdn: [3] minimizers_own, [5] distinct_own,
// [7] db_cells_own
static void collect_mdata(const std::vector<RunBuffers> &dbuf, RunState &rs, size_t md_mark_bytes, MdataNumbers &mdn, double *md_count_ms) {
    if (rs.err_code != NH_OK) return;
    const int G = (int)dbuf.size();
    Engine *e0 = rs.engines[0];
    const size_t md_nodes = e0->external.size();
    const size_t words = md_mark_bytes / 4;
    std::vector<unsigned long long> part(md_nodes), sum(md_nodes, 0);
    hipError_t he = hipSuccess;
    for (int g = 0; g < G && he == hipSuccess; g++) {
        he = dev_set(dbuf[g].device);
        if (he == hipSuccess) he = hipMemcpy(part.data(), dbuf[g].groups, md_nodes * 8, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < md_nodes; i++) sum[i] += part[i];
    }
    if (he == hipSuccess && G > 1) {
        std::vector<uint32_t> all(words, 0), one(words);
        for (int g = 0; g < G && he == hipSuccess; g++) {
            he = dev_set(dbuf[g].device);
            if (he == hipSuccess) he = hipMemcpy(one.data(), dbuf[g].marks, words * 4, hipMemcpyDeviceToHost);
            for (size_t i = 0; i < words; i++) all[i] |= one[i];
        }
        if (he == hipSuccess) he = dev_set(e0->device);
        if (he == hipSuccess) he = hipMemcpy(dbuf[0].marks, all.data(), words * 4, hipMemcpyHostToDevice);
    }
    mdn.v[3].assign(sum.begin(), sum.end());
    // two counts with the array of hit groups as their bins: the marked cells, then all cells
    EventPair cev;
    if (he == hipSuccess) he = dev_set(e0->device);
    if (he == hipSuccess && getenv("NOHUMAN_TRACE") && cev.create() != hipSuccess) he = hipErrorUnknown;
    for (int pass = 0; pass < 2 && he == hipSuccess; pass++) {
        he = hipMemsetAsync(dbuf[0].groups, 0, md_nodes * 8, e0->stream);
        if (he == hipSuccess && cev[0]) he = hipEventRecord(cev[0], e0->stream);
        if (he == hipSuccess) he = launch_mdata_count(e0, pass == 0 ? dbuf[0].marks : nullptr, dbuf[0].groups, e0->stream);
        if (he == hipSuccess && cev[1]) he = hipEventRecord(cev[1], e0->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e0->stream);
        if (he == hipSuccess) he = hipMemcpy(part.data(), dbuf[0].groups, md_nodes * 8, hipMemcpyDeviceToHost);
        mdn.v[pass == 0 ? 5 : 7].assign(part.begin(), part.end());
        if (he == hipSuccess && pass == 0) add_event_ms(cev, md_count_ms);
    }
    if (he != hipSuccess) rs.fail(NH_EDEVICE, std::string("minimizer data, counting the bitmap: ") + hipGetErrorString(he));
}

// The run's only exchange step: the counters the classify kernels kept in each
// device's HBM are summed by ONE all-reduce over RCCL, reduced where they lie.  The sums the writer kept
// on the host are the checker.  A collective that cannot run at G > 1 is reported on stderr (one WARN
// line; the host sums stand) and fails the run under NOHUMAN_RCCL=strict; NOHUMAN_RCCL=0 skips the
// collective, =1 also runs it for a single device.
static int reduce_run_counters(RunState &rs) {
    const std::vector<Engine *> &engines = rs.engines;
    const int G = (int)engines.size();
    std::vector<uint64_t> rows(4 * (size_t)G, 0);
    uint64_t dsum[4] = {0, 0, 0, 0};
    hipError_t he = hipSuccess;
    for (int g = 0; g < G && he == hipSuccess; g++) {
        he = dev_set(engines[g]->device);
        if (he == hipSuccess) he = hipMemcpy(&rows[4 * g], rs.d_run_counters[g], 32, hipMemcpyDeviceToHost);
        for (int i = 0; i < 4; i++) dsum[i] += rows[4 * g + i];
        if (he == hipSuccess) {  // the engine's running totals (nh_stats_get) include this run
            hipLaunchKernelGGL(k_add_counters, dim3(1), dim3(4), 0, engines[g]->stream,
                               (unsigned long long *)engines[g]->d_counters, (const unsigned long long *)rs.d_run_counters[g]);
            he = hipStreamSynchronize(engines[g]->stream);
        }
    }
    int crc = NH_OK;
    if (he != hipSuccess) crc = set_error(NH_EDEVICE, "reading the run's counters: %s", hipGetErrorString(he));
    else if (dsum[CNT_FRAGMENTS] != rs.total || dsum[CNT_CLASSIFIED] != rs.classified || dsum[CNT_BASES] != rs.total_bases)
        crc = set_error(NH_EDEVICE, "the devices counted %llu fragments / %llu classified / %llu bases, the writer %llu / %llu / %llu",
                        (unsigned long long)dsum[0], (unsigned long long)dsum[1], (unsigned long long)dsum[2],
                        (unsigned long long)rs.total, (unsigned long long)rs.classified, (unsigned long long)rs.total_bases);
    const char *env = getenv("NOHUMAN_RCCL");
    const bool strict = env && strcmp(env, "strict") == 0;
    const bool want = env ? env[0] != '0' : G > 1;
    if (!crc && want && (G > 1 || env)) {
        std::vector<int> ids;
        for (Engine *e : engines) ids.push_back(e->device);
        std::vector<const uint64_t *> src(rs.d_run_counters.begin(), rs.d_run_counters.end());
        std::string backend;
        const int arc = allreduce_counters(ids.data(), G, rows.data(), backend, src.data());
        if (arc == NH_OK) {
            for (int g = 0; g < G && !crc; g++)
                if (rows[4 * g] != rs.total || rows[4 * g + 1] != rs.classified || rows[4 * g + 2] != rs.total_bases)
                    crc = set_error(NH_EDEVICE, "count all-reduce disagrees with the host-side sum on device %d", ids[g]);
            if (getenv("NOHUMAN_TRACE")) fprintf(stderr, "[nohuman trace] counters reduced by %s\n", backend.c_str());
        } else if (strict) {
            crc = arc;
        } else {
            fprintf(stderr, "nohuman: WARN count all-reduce over %d devices did not run (%s); the counts were summed on the host\n",
                    G, g_last_error.c_str());
        }
    }
    return crc;
}

// ---- the run's shape ----------------------------------------------------------------------------------
// What kind of run a request asks for, computed once and const from then on: the constructor reads the request (check_request has
// passed it) and the environment -- the features' tables are checked with these flags before any output is created --,
// set_outputs() adds what the opened files decide.  Nothing else derives these values a second time.
namespace {  // (the pipeline's own types: this file's alone)
struct RunShape {
    bool mask, calls, ids, lists;
    uint32_t minq;
    // BAM output (a BAM in1 alone, neither masked nor with selectors): out1 and, a split run, human_out1 receive records of the
    // input selected on the device (nh_bamout.hip); none of the FASTQ record builders runs
    bool bamout;
    bool split_files;  // a split run: the human outputs are opened, flushed, closed
    bool split;        // ... and their records built as FASTQ text (nh_split.hip)
    int n_bout, K;     // BAM output: the builder's outputs; per-taxon outputs: the selectors
    bool taxa, qm, rst, mdt, hsel;
    bool dust;         // --dust-reads: k_rdust in front of the classifier
    bool cover;        // --host-intervals: k_cover_mark and the two builders behind the classifier
    bool hbo;          // --host-bases-only: k_cover_mark (one pass for both), the closing (gap > 0), the mask builder on the bitmap
    bool cut;          // --host-cut: the same mark pass and closing, the cut builder (nh_cut.hip) in the mask builder's place
    uint32_t gap, min_piece;
    bool close;        // the bitmap is closed behind the report (hbo or cut)
    bool mark;         // the batch's cover bitmap is made (cover, hbo or cut)
    bool idl;          // a builder prints mate 1's id: the id lengths go to the device (the read lists, the host intervals, the host cut)
    bool qtext;        // the classifier and the minimizer data's marks read the slot's masked text, not the batch's (qm or dust)
    bool want_rec;     // a kernel of the run reads the record table
    bool gzip_family;  // the codecs the GPU encodes
    int G, NS;         // devices, stream slots a device
    bool trace, trace_run;  // NOHUMAN_TRACE is set: events around the launches, the trace lines; it begins with 1: the run's own lines at its end
    // set_outputs() (outs_take_hbm: out1 / out2 are gzip-family encoders on the GPU that take device spans):
    int mates = 1;
    bool files2 = false;  // the second mate has files of its own: a paired run, but for BAM output (one BAM holds both mates)
    uint32_t flags = 0;
    bool outs_take_hbm = false, host_text_wanted = false, human_in_hbm = false, mask_in_hbm = false, bam_in_hbm = false, taxon_in_hbm = false;

    RunShape(const RunRequest &r, size_t n_engines) {
        const nh_run_args *a = r.a;
        mask = r.mask, calls = r.calls != nullptr, ids = r.ids != nullptr, lists = calls || ids, minq = r.minq;
        bamout = a->out_codec == NH_CODEC_BAM;
        split_files = r.hout1 != nullptr, split = split_files && !bamout, n_bout = split_files ? 2 : 1;
        K = (int)r.n_touts, taxa = K > 0;
        qm = minq > 0, rst = r.rs_path || r.rs_out, hsel = r.hf != nullptr;
        dust = r.dust, qtext = qm || dust;
        mdt = r.md && (r.md->in_report || r.md->table || r.md->taxa);
        cover = r.hi_path != nullptr;
        hbo = r.hbo, cut = r.cut, close = hbo || cut, gap = hbo ? r.hb->gap : cut ? r.hc->gap : 0, min_piece = cut ? r.hc->min_piece : 0;
        mark = cover || close, idl = lists || cover || cut;
        want_rec = split || mask || lists || qm || rst || taxa || cover;
        gzip_family = a->out_codec == NH_CODEC_GZIP || a->out_codec == NH_CODEC_BGZF || bamout;
        G = (int)n_engines;
        // stream slots a device: two keep the classifier busy; a third lets the copy of a batch's text back to the host (batches
        // born on the GPU, outputs written by the host) run while the writer is still busy with the batch before; a fourth is
        // held by the batch the flusher is writing
        NS = 4;
        if (const char *env = getenv("NOHUMAN_SLOTS")) NS = std::max(1, std::min(8, atoi(env)));
        const char *tr = getenv("NOHUMAN_TRACE");
        trace = tr != nullptr, trace_run = tr && tr[0] == '1';
    }
    void set_outputs(const nh_run_args *a, const RunState &rs, RunFiles &f) {
        auto takes = [](const OutFile &o) { return o.enc && o.enc->takes_device_spans(); };
        mates = rs.paired ? 2 : 1;
        files2 = rs.paired && !bamout;
        flags = rs.paired ? NH_FLAG_PAIRED : 0;
        outs_take_hbm = gzip_family && takes(f.o1) && (!files2 || takes(f.o2));
        // Batches of the reader on the GPU keep their text in HBM.  The host needs the bytes for plain outputs and the host's
        // codecs, for the ids of --output lines and for the suffix of classified-out headers; gzip outputs encoded on the GPU
        // take the kept records from HBM (a record that needs reformatting -- CRLF, "+id" -- makes the writer fetch its batch).
        // A masked run builds every output record on the device (the split side as well): only --output lines need the bytes.
        // BAM output takes nothing from the text at all: its records are the input's BAM bytes, which the reader keeps in HBM.
        host_text_wanted = bamout ? rs.want_k
                           : mask ? rs.want_k || G > 1
                                  : !outs_take_hbm || rs.want_k || a->keep_human != 0 || G > 1;  // (G > 1: a batch's slot and its file's encoder may sit on different GPUs)
        // split runs: the classified-out text is built in HBM; an encoder on the slot's GPU takes it from there, any other output
        // gets exactly the built bytes copied to the host (G > 1: a batch's slot and its file's encoder may sit on different GPUs)
        human_in_hbm = split && G == 1 && takes(f.h1) && (!rs.paired || takes(f.h2));
        // masked runs: the same for out1 / out2 -- one span a mate and batch, from HBM or copied to page-locked slot memory
        mask_in_hbm = mask && G == 1 && takes(f.o1) && (!rs.paired || takes(f.o2));
        // BAM output: the same for out1 / human_out1 -- one span an output and batch
        bam_in_hbm = bamout && G == 1 && takes(f.o1) && (!split_files || takes(f.h1));
        taxon_in_hbm = taxa && G == 1;
        for (int k = 0; k < K; k++)
            for (int m = 0; m < mates; m++) taxon_in_hbm = taxon_in_hbm && takes(f.tx[m][k]);
    }
};

// What the writer hands the flusher for one batch
struct FlushJob {
    Batch b;
    Spans s1, s2, sk, hs1, hs2;  // (hs1, hs2: a split run's classified records, one span a mate)
    Spans sc, si;                // (the batch's part of the calls table and of the human ids, one span each)
    Spans shi;                   // (... and of the host intervals)
    Spans ts[2][NH_MAX_TAXON_OUTS];  // (per-taxon outputs: a span a mate and selector with records in the batch)
    // the built spans that only exist in HBM (an address there, never read on the host): the flusher maps them for the file's encoder
    std::vector<std::pair<OutFile *, struct iovec>> dev;
    bool valid = false;  // (false: the run had failed when the batch arrived -- only its buffers go back)
};

// One active output builder of a run: which BuiltOut of the slot, how many words of totals come back with the results, where its
// kernel time is summed.  One pass in front of or behind the classifier: its pair of events, where its kernel time is summed.
struct Builder { BuiltOut Slot::*out; size_t total_words; double RunState::*ms; };
struct Pass { EventPair Slot::*ev; double RunState::*ms; };

// a launch on the slot's stream between a pair of events (NOHUMAN_TRACE; none without it); a failure fails the run under `name`
template <class F>
static void timed_launch(RunState &rs, hipStream_t stream, const EventPair &ev, const char *name, F launch) {
    if (ev[0]) (void)hipEventRecord(ev[0], stream);
    hipError_t he = launch();
    if (ev[1] && he == hipSuccess) he = hipEventRecord(ev[1], stream);
    if (he != hipSuccess) rs.fail(NH_EDEVICE, std::string(name) + ": " + hipGetErrorString(he));
}

// where a kernel finds the batch in the slot: the text, the sequences' lengths, the record table (CallsArgs takes no more) ...
template <class A>
static void batch_records(A &x, const Slot &s, const Batch &b) {
    x.text = (const char *)s.d_text, x.ntext = b.ntext();
    x.seq_len = (const uint32_t *)s.d_len;
    x.rec = (const uint32_t *)s.d_rec.p;
    x.mates = b.h2 ? 2 : 1;
}
// ... the sequences' starts and which mate is FASTQ (HumanOutArgs, TaxonOutArgs, MaskArgs, QmaskArgs, RstatsArgs)
template <class A>
static void batch_source(A &x, const Slot &s, const Batch &b) {
    batch_records(x, s, b);
    x.seq_off = (const uint64_t *)s.d_off;
    x.fastq[0] = b.h1->format == FMT_FASTQ, x.fastq[1] = b.h2 && b.h2->format == FMT_FASTQ;
}
// where a builder's kernels write: its n_out outputs, its scratch, the engine's error word
template <class A>
static void built_sink(A &x, const BuiltOut &o, int n_out, const Slot &s) {
    for (int i = 0; i < n_out; i++) x.out[i] = o.d_out[i], x.cap[i] = o.d_out[i].cap;
    x.blk = (uint64_t *)o.d_blk;
    x.error = s.e->d_error + LAUNCH_SLOTS;
}

// ---- the pipeline: readers -> main (pair, stage, launch) -> writer -> flusher ---------------------------
// The state the threads of one run share, and their bodies.  start() sets the readers, the writer and the flusher going, run()
// is the main thread's loop -- every batch through pick_slot, reserve, gather, stage_text, launch, queue_results --, shutdown()
// unblocks and joins them, also after an error.
struct Pipeline {
    const nh_run_args *const a;
    const RunShape &sh;
    RunState &rs;
    RunFiles &f;
    const std::vector<Engine *> &engines;
    std::vector<RunBuffers> &dbuf;
    const std::vector<uint8_t> &bin_of;
    size_t batch_frags = 0, batch_text = 0, mean_rec = 0;  // batch_limits()
    std::vector<Builder> builders;  // the run's active builders, in the order their totals are copied back
    std::vector<Pass> passes;
    std::vector<Slot> slots;
    BoundedQueue<std::unique_ptr<HalfBatch>> q1{3}, q2{3};
    BatchPool pool1, pool2;
    BoundedQueue<Batch> wq;
    BoundedQueue<std::unique_ptr<FlushJob>> fq{1};
    std::mutex slot_mu, w2_mu;  // (w2: the hand-shake between the flusher and its helper for the second mate's files)
    std::condition_variable slot_cv, w2_cv;
    int w2_state = 0, w2_rc = NH_OK;  // 0 idle, 1 flush requested, 2 done, -1 quit
    Spans *w2_spans = nullptr, *w2_hspans = nullptr, *w2_tspans = nullptr;
    std::string w2_err;
    StageClock clk;
    std::thread t1, t2, tw, tf, tw2;
    // the main loop: the half of each file in hand and how many of its records have gone out (a half is normally used whole: Batch)
    std::shared_ptr<HalfBatch> c1, c2;
    size_t p1 = 0, p2 = 0, cl1 = 0, cl2 = 0;  // (cl: the half's bytes of text, read once, when it arrives)
    uint64_t batch_no = 0, frags_out = 0;      // (frags_out: the fragments of the batches before this one)
    std::vector<uint64_t> home_turn;

    Pipeline(const RunShape &sh_, RunState &rs_, RunFiles &f_, std::vector<RunBuffers> &dbuf_, const std::vector<uint8_t> &bin_of_)
        : a(rs_.a), sh(sh_), rs(rs_), f(f_), engines(rs_.engines), dbuf(dbuf_), bin_of(bin_of_), wq((size_t)(sh_.NS * sh_.G)),
          home_turn((size_t)sh_.G, 0) {
        if (sh.split) builders.push_back({&Slot::human, 2, &RunState::human_kernel_ms});
        if (sh.bamout) builders.push_back({&Slot::bam, 2, &RunState::bam_kernel_ms});
        if (sh.taxa) builders.push_back({&Slot::taxon, 4 * (size_t)sh.K, &RunState::taxon_kernel_ms});
        if (sh.mask) builders.push_back({&Slot::mask, 4, &RunState::mask_kernel_ms});
        if (sh.lists) builders.push_back({&Slot::lists, 4, &RunState::list_kernel_ms});
        if (sh.mark) builders.push_back({&Slot::cover, 4, &RunState::cover_kernel_ms});
        if (sh.qm) passes.push_back({&Slot::qev, &RunState::qmask_kernel_ms});
        if (sh.dust) passes.push_back({&Slot::duev, &RunState::dust_kernel_ms});
        if (sh.rst) passes.push_back({&Slot::rev, &RunState::rstats_kernel_ms});
        if (sh.mdt) passes.push_back({&Slot::mev, &RunState::mdata_kernel_ms});
        if (sh.hsel) passes.push_back({&Slot::hev, &RunState::host_kernel_ms});
    }

    // fragments per batch: ~96 MB of sequence, at most 262144; both readers cut at the same record
    // count so that paired batches stay aligned (a byte budget only cuts single-end batches)
    void batch_limits() {
        batch_frags = estimate_batch_frags(a->in1, &mean_rec);
        if (const char *env = getenv("NOHUMAN_BATCH_FRAGS")) {  // tuning / test knob
            const long v = atol(env);
            if (v > 0) batch_frags = (size_t)v;
        }
        // byte budget of one reader's batch: single-end batches are cut by it; paired batches are cut by record
        // count (both readers at the same count), and their budget only keeps the text of the two halves together
        // below the 4 GB a batch's 32-bit sequence positions can address
        batch_text = rs.paired ? (size_t)0x7F000000u : (size_t)(512u << 20);
        if (const char *env = getenv("NOHUMAN_BATCH_TEXT")) {  // test knob: batches cut by text at small scale (paired: the halves then differ in length)
            const long v = atol(env);
            if (v > 0) batch_text = (size_t)v;
        }
    }

    // the stream and, under NOHUMAN_TRACE, the events of every slot
    int create_slots() {
        slots = std::vector<Slot>((size_t)sh.NS * sh.G);
        for (int i = 0; i < sh.NS * sh.G; i++) {
            Slot &s = slots[i];
            s.e = engines[i / sh.NS];
            bool ok = dev_set(s.e->device) == hipSuccess && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
            for (const Builder &bd : builders) ok = ok && (!sh.trace || (s.*bd.out).ev.create() == hipSuccess);
            for (const Pass &ps : passes) ok = ok && (!sh.trace || (s.*ps.ev).create() == hipSuccess);
            if (!ok) return set_error(NH_EDEVICE, "cannot create streams");
        }
        return NH_OK;
    }

    // the builders, a function each with three steps: RESERVE (main thread, before the record table is gathered), LAUNCH (main
    // thread, behind the classifier on the slot's stream), SPANS (writer thread: the totals that came back into spans of the
    // flusher's job).  *rc: the stage's error so far -- a reserve or a span is not made behind one -- and this step's
    enum BuildStep { RESERVE, LAUNCH, SPANS };
    // a span of built text for file `of`, kept in `sp`; in HBM: also noted for the flusher to map
    void add_built(FlushJob *j, OutFile &of, Spans &sp, char *at, size_t len, bool in_hbm) {
        sp.iov.push_back({(void *)at, len});
        sp.is_scratch.push_back(0);
        if (in_hbm) j->dev.push_back({&of, {(void *)at, len}});
    }
    // output i of a builder that makes one span an output: its total, added to *bytes, as a span of `of` kept in `sp`
    void one_span(FlushJob *j, BuiltOut &o, int i, bool in_hbm, OutFile &of, Spans &sp, uint64_t *bytes, int *rc, const char *what, const char *item) {
        const size_t tot = (size_t)o.h_total[i];
        *bytes += tot;
        if (tot) add_built(j, of, sp, built_span(o, i, tot, in_hbm, rs, rc, what, item), tot, in_hbm);
    }

    void start() {
        start_readers();
        if (sh.bamout) write_bam_header();
        if (sh.files2) tw2 = std::thread([this] { mate2_flusher_main(); });
        tf = std::thread([this] { flusher_main(); });
        tw = std::thread([this] { writer_main(); });
    }

    // sizes the pools' page-locked text buffers, chooses each input's reader and starts the reader threads
    void start_readers() {
        const int G = sh.G, mates = sh.mates;
        const bool host_text_wanted = sh.host_text_wanted;
        int prefill = 4 + 2 * G;
        if (mean_rec) {  // size the page-locked text buffers once: a batch of records plus one read chunk
            size_t want = batch_frags * mean_rec + batch_frags * mean_rec / 8 + (8u << 20);
            if (want > batch_text + (8u << 20)) want = batch_text + (8u << 20);
            // small inputs: no more (and no larger) buffers than the text they can hold, compressed 12:1 at most
            struct stat st1;
            if (stat(a->in1, &st1) == 0 && S_ISREG(st1.st_mode)) {
                const uint64_t est = (uint64_t)st1.st_size * 12 + (1u << 20);
                if (est < want) want = (size_t)est;
                const uint64_t nb = est / want + 1;
                if (nb < (uint64_t)prefill) prefill = (int)nb;
            }
            if (want < (1ull << 31)) pool1.first_reserve = pool2.first_reserve = want;
            if (sh.trace)
                fprintf(stderr, "[nohuman trace] batch: %zu fragments, text buffers of %zu bytes reserved at once, %d prefilled per file\n",
                        batch_frags, pool1.first_reserve, prefill);
        }
        int prefill1 = prefill, prefill2 = prefill;
        // which reader takes a gzip input: NOHUMAN_GZ_READER by name ("device", "host", "device-text"), else by the input
        // (device_reader_pays); paired files go the same way (the smaller file decides)
        bool dev_reader1 = false, dev_reader2 = false, split_readers = false;
        const char *how = getenv("NOHUMAN_GZ_READER");
        const bool off = how && (!strcmp(how, "host") || !strcmp(how, "device-text"));
        const bool named = how && !strcmp(how, "device");
        const bool by_host = a->keep_human == 0 && !sh.outs_take_hbm;
        // (a masked run whose outputs are written by the host: every byte leaves through it, as the kept reads of a normal run
        // do -- the same choice; with GPU gzip outputs nothing does and the reader on the GPU is taken, profiles/mask_e2e.txt)
        const bool text_to_host = host_text_wanted || (sh.mask && !sh.mask_in_hbm);
        dev_reader1 = !off && dev_gunzip_wants(a->in1) && (named || device_reader_pays(a->in1, mean_rec, text_to_host, by_host));
        const bool two_inputs = a->in2 != nullptr;  // (a paired BAM is a paired run from one file, one reader, one thread)
        dev_reader2 = two_inputs && !off && dev_gunzip_wants(a->in2) && (named || device_reader_pays(a->in2, mean_rec, text_to_host, by_host));
        if (two_inputs && !named && dev_reader1 != dev_reader2 && dev_gunzip_wants(a->in1) && dev_gunzip_wants(a->in2)) dev_reader1 = dev_reader2 = false;
        // "split": the two mate files on the two KINDS of reader at once -- file 1 inflated and indexed on the GPU, file 2 by all
        // the host's inflate workers (round 6: the GPU's codec kernels and the host's cores idle in turn otherwise)
        split_readers = two_inputs && how && !strcmp(how, "split") && dev_gunzip_wants(a->in1) && dev_gunzip_wants(a->in2);
        if (split_readers) dev_reader1 = true, dev_reader2 = false;
        if (bam_wants(a->in1)) {  // (its own reader, whatever NOHUMAN_GZ_READER says; its batches are born on the GPU as well)
            dev_reader1 = false;
            if (!host_text_wanted) pool1.first_reserve = 0, prefill1 = 0;
            if (!two_inputs) pool2.first_reserve = pool1.first_reserve, prefill2 = prefill1;  // (a paired BAM: mate 2's halves are of the same kind)
        }
        if (sh.trace)
            fprintf(stderr, "[nohuman trace] gzip reader: %s%s%s\n", dev_reader1 ? "GPU" : "host", two_inputs ? (dev_reader2 ? " / GPU" : " / host") : "",
                    how ? " (NOHUMAN_GZ_READER)" : "");
        // batches of the reader on the GPU carry no host text unless an output needs it: no page-locked buffers made ahead for them
        if (dev_reader1 && !host_text_wanted) pool1.first_reserve = 0, prefill1 = 0;
        if (dev_reader2 && !host_text_wanted) pool2.first_reserve = 0, prefill2 = 0;
        if (prefill1) pool1.start_prefill(prefill1);
        if (rs.paired && prefill2) pool2.start_prefill(prefill2);
        // gzip inputs are inflated by `threads` workers in all, shared between the files
        // (a paired BAM is one file: its inflate workers are not halved for a second file that does not exist)
        unsigned gz_threads = (a->threads ? a->threads : 1) / (two_inputs ? 2u : 1u);
        if (gz_threads < 1) gz_threads = 1;
        if (gz_threads > 16) gz_threads = 16;  // beyond that the record parser of the file is the limit
        unsigned gz_threads2 = gz_threads;
        if (split_readers) gz_threads2 = std::min(16u, std::max(1u, a->threads ? a->threads : 1u));  // (file 1's reader is on the GPU: every worker to file 2)
        // gzip inputs are read on the GPU (nh_gunzip.hip): file 1 on the first device, file 2 on the second where there is one
        // ... piece by piece over the run's devices (the compressed ranges are the shards): file 1 starts on the
        // first device, file 2 on the second, so the two files' pieces of the same moment sit on different GPUs
        std::vector<int> devs1, devs2;
        for (int g = 0; g < G; g++) {
            devs1.push_back(engines[(size_t)g]->device);
            devs2.push_back(engines[(size_t)((g + 1) % G)]->device);
        }
        if (getenv("NOHUMAN_GZ_SHARD") && getenv("NOHUMAN_GZ_SHARD")[0] == '0') devs1.resize(1), devs2.resize(1);  // (A / B: a file's reader on one device)
        if (const char *e = getenv("NOHUMAN_GZ_LANES")) {  // tuning knob: several lanes of the reader on ONE device (pieces decoded ahead there)
            const int n = atoi(e);
            while (G == 1 && (int)devs1.size() < n && n <= 4) devs1.push_back(devs1[0]), devs2.push_back(devs2[0]);
        }
        // The hybrid reader (round 6, nh_gunzip.hip): the odd cells of each input's (then alternating) piece grid inflated by host workers
        // beside the GPU's.  OFF unless asked for (NOHUMAN_GZ_HYBRID=n: n workers per file; 1: the run's threads less four, shared between
        // the files): built for the runs whose kept text is re-encoded on the GPU -- there the chip's codec kernels, inflate and deflate in
        // turn, are what the run waits for -- and measured there: 30.8 -> 24.7 Mreads/s on 40 M pairs (profiles/r06_hybrid.txt): a host
        // piece's in-order part (stitching, CRC, copy, upload: 0.2 s) holds the file's stream up five times a file, and pieces decoded
        // ahead lose the in-order reader's staged input.  Correct and covered; what would make it pay is written down there.
        unsigned hybrid_threads = 0;
        if (const char *e = getenv("NOHUMAN_GZ_HYBRID")) {
            const int v = atoi(e);
            const unsigned T = a->threads ? a->threads : 1;
            const unsigned want = v <= 0 ? 0u : v == 1 ? std::max(1u, (T > 4 ? T - 4 : 1u) / (unsigned)mates) : (unsigned)v;
            hybrid_threads = G == 1 ? std::min(16u, want) : 0u;  // (one device: the reader's lanes over several are untested with it)
            if (sh.trace && (dev_reader1 || dev_reader2))
                fprintf(stderr, "[nohuman trace] gzip reader: hybrid %s (%u host workers per file)\n", hybrid_threads ? "on" : "off", hybrid_threads);
        }
        t1 = std::thread(reader_main, a->in1, &q1, rs.paired && !two_inputs ? &q2 : nullptr, &rs, &pool1, &pool2, &clk, 0, batch_frags, batch_text, gz_threads,
                         devs1, dev_reader1, hybrid_threads);
        if (two_inputs)
            t2 = std::thread(reader_main, a->in2, &q2, nullptr, &rs, &pool2, nullptr, &clk, 1, batch_frags, batch_text, gz_threads2, devs2, dev_reader2, hybrid_threads);
    }

    // BAM output: the input's header, as the reader found it, is the first thing in every record output (a host span: the
    // encoder stages it), before the writer hands on the first batch's records
    void write_bam_header() {
        std::string hdr;
        {
            std::unique_lock<std::mutex> lk(rs.hdr_mu);
            rs.hdr_cv.wait(lk, [&] { return rs.hdr_set; });
            hdr.swap(rs.bam_header);
        }
        if (hdr.empty()) rs.fail(NH_EIO, std::string(a->in1) + ": no BAM header to copy (the file is not the BAM it was when the run was checked)");
        for (OutFile *of : {&f.o1, sh.split_files ? &f.h1 : (OutFile *)nullptr}) {
            if (!of || rs.failed()) continue;
            int hrc = of->enc->write(hdr.data(), hdr.size());
            if (!hrc) hrc = of->enc->settle();
            if (hrc) rs.fail(hrc, g_last_error);
        }
    }

    // the flusher's helper: the second mate's files, written while the flusher writes the first's
    void mate2_flusher_main() {
        for (;;) {
            std::unique_lock<std::mutex> lk(w2_mu);
            w2_cv.wait(lk, [&] { return w2_state == 1 || w2_state == -1; });
            if (w2_state == -1) return;
            Spans *sp2 = w2_spans, *hsp2 = w2_hspans, *tsp2 = w2_tspans;
            lk.unlock();
            int frc = f.o2.flush(*sp2);
            if (!frc && hsp2) frc = f.h2.flush(*hsp2);
            for (int k = 0; k < sh.K && !frc; k++)
                if (!tsp2[k].iov.empty()) frc = f.tx[1][k].flush(tsp2[k]);
            lk.lock();
            w2_rc = frc;
            if (frc) w2_err = g_last_error;
            w2_state = 2;
            w2_cv.notify_all();
        }
    }

    // The FLUSHER writes the spans of the batch before while the writer is on the next one -- a helper takes the second mate file, so
    // that both files are written at the same time -- and only then gives the batch's buffers and its stream slot back.  (One thread
    // did both in round 3: 35.5 GB of kept text leave through writev() at 12 GB/s, 2.9 s, and the 1.3 s of waiting and formatting
    // came on top, profiles/r04_e2e.txt.)
    void flusher_main() {
        std::unique_ptr<FlushJob> j;
        while (fq.pop(j)) {
            Slot &s = slots[j->b.slot];
            if (j->valid && !rs.failed()) {
                uint64_t c3 = StageClock::now();
                (void)dev_set(s.e->device);
                const Batch &b = j->b;
                // the batch's raw text is still in the slot's device buffer: an encoder on that GPU takes
                // the kept records from there instead of a second trip over PCIe
                // (a part that fetched its own host copy has its spans there: they are staged like any host memory)
                // (a masked run's spans are the built text: in HBM, mapped below, or in the slot's page-locked copy)
                if (f.o1.enc && !sh.mask && !sh.bamout) f.o1.enc->map_device(b.h1->text.data(), b.len1, s.d_text, s.e->device, b.h1->host_text_valid);
                if (sh.files2 && f.o2.enc && !sh.mask)
                    f.o2.enc->map_device(b.h2->text.data(), b.len2, (const char *)s.d_text + b.base2(), s.e->device, b.h2->host_text_valid);
                for (const auto &d : j->dev) d.first->enc->map_device(d.second.iov_base, d.second.iov_len, d.second.iov_base, s.e->device, false);
                if (sh.files2) {
                    std::lock_guard<std::mutex> lk(w2_mu);
                    w2_spans = &j->s2;
                    w2_hspans = sh.split ? &j->hs2 : nullptr;
                    w2_tspans = j->ts[1];
                    w2_state = 1;
                    w2_cv.notify_all();
                }
                int wrc = f.o1.flush(j->s1);
                if (!wrc && rs.want_k) wrc = f.ok.flush(j->sk);
                if (!wrc && sh.split_files) wrc = f.h1.flush(j->hs1);
                for (int k = 0; k < sh.K && !wrc; k++)
                    if (!j->ts[0][k].iov.empty()) wrc = f.tx[0][k].flush(j->ts[0][k]);
                if (!wrc && sh.calls) wrc = f.oc.flush(j->sc);
                if (!wrc && sh.ids) wrc = f.oi.flush(j->si);
                if (!wrc && sh.cover) wrc = f.ohi.flush(j->shi);
                if (sh.files2) {
                    std::unique_lock<std::mutex> lk(w2_mu);
                    w2_cv.wait(lk, [&] { return w2_state == 2; });
                    w2_state = 0;
                    if (!wrc && w2_rc) wrc = set_error(w2_rc, "%s", w2_err.c_str());
                }
                clk.ns[ST_WWRITE] += StageClock::now() - c3;
                if (wrc) rs.fail(wrc, g_last_error);
            }
            j->b.h1.reset();  // (the last part of a half gives it back to its pool: the deleter of next_batch's take)
            j->b.h2.reset();
            {
                std::lock_guard<std::mutex> lk(slot_mu);
                s.busy = false;
            }
            slot_cv.notify_all();
        }
    }

    // a batch whose text is only in HBM, and a kept record that must be rewritten (CRLF, "+id" line): fetch it
    // (into a buffer of this part: the half itself may be in use by other parts -- Batch)
    int fetch_text(Slot &s, Batch &b) {
        int wrc = NH_OK;
        auto need_fetch = [&](const HalfBatch &hb) {
            if (hb.host_text_valid || sh.mask || sh.bamout) return false;
            const size_t off = &hb == b.h1.get() ? b.off1 : b.off2;
            const nh_result *const hres = s.host_res();
            for (size_t i = 0; i < b.n; i++)
                if (!hb.recs[off + i].raw_end && (hres[i].call != 0) == (a->keep_human != 0)) return true;
            return false;
        };
        for (int m = 0; m < sh.mates && !wrc; m++) {
            const HalfBatch &hb = m ? *b.h2 : *b.h1;
            if (need_fetch(hb)) {
                const size_t L = m ? b.len2 : b.len1;
                std::unique_ptr<char[]> &dst = m ? b.fetch2 : b.fetch1;
                dst.reset(new (std::nothrow) char[L + 64]);
                if (!dst) wrc = set_error(NH_EOOM, "out of memory");
                if (!wrc && hipMemcpy(dst.get(), (const char *)s.d_text + (m ? b.base2() : 0), L, hipMemcpyDeviceToHost) != hipSuccess)
                    wrc = set_error(NH_EDEVICE, "fetching a batch's text from the device failed");
                rs.text_fetched += L;
            }
        }
        return wrc;
    }

    // read statistics: every length of the batch, by the class of its fragment (host or not) and its mate
    void note_lengths(const Slot &s, const Batch &b) {
        for (size_t i = 0; i < b.n; i++) {
            const int c = s.host_res()[i].call != 0;
            for (int m = 0; m < sh.mates; m++) {
                const uint64_t L = s.h_len[i * sh.mates + m];
                if (L >= (1u << 20)) {
                    rs.len_long[c][m][L]++;
                    continue;
                }
                std::vector<uint64_t> &h = rs.len_hist[c][m];
                if (L >= h.size()) h.resize(std::max<size_t>(L + 1, std::min<size_t>(2 * h.size(), 1u << 20)), 0);
                h[L]++;
            }
        }
    }

    // The WRITER consumes batches in order: it waits for the batch's stream, decides and formats (span lists, nothing is copied),
    // turns the builders' totals into spans and hands the job to the flusher.
    void writer_main() {
        Batch b;
        for (;;) {
            uint64_t c0 = StageClock::now();
            if (!wq.pop(b)) break;
            uint64_t c1 = StageClock::now();
            clk.ns[ST_WPOP] += c1 - c0;
            Slot &s = slots[b.slot];
            std::unique_ptr<FlushJob> j(new FlushJob());
            if (!rs.failed()) {
                (void)dev_set(s.e->device);
                hipError_t he = hipStreamSynchronize(s.stream);
                uint64_t c2 = StageClock::now();
                clk.ns[ST_WSYNC] += c2 - c1;
                int wrc = NH_OK;
                if (he != hipSuccess) wrc = set_error(NH_EDEVICE, "classify: %s", hipGetErrorString(he));
                // (the error bits came with the results on the slot's stream: a copy of their own here would queue behind
                // whatever else the device is running -- the gzip reader's kernels -- once a batch)
                if (!wrc && *s.h_flag) wrc = check_error_flag(s.e);
                if (!wrc) wrc = fetch_text(s, b);
                if (!wrc) {
                    format_batch(&rs, b, s, f.o1, f.o2, f.ok, !sh.mask && !sh.bamout);
                    for (const Builder &bd : builders) add_event_ms((s.*bd.out).ev, &(rs.*bd.ms));
                    for (const Pass &ps : passes) add_event_ms(s.*ps.ev, &(rs.*ps.ms));
                    if (sh.bamout) build_bam(SPANS, s, b, j.get(), &wrc);
                    if (sh.mask) build_mask(SPANS, s, b, j.get(), &wrc);
                    if (sh.split) build_human(SPANS, s, b, j.get(), &wrc);
                    if (sh.taxa) build_taxon(SPANS, s, b, j.get(), &wrc);
                    if (sh.rst) note_lengths(s, b);
                    if (sh.lists) build_lists(SPANS, s, b, j.get(), &wrc);
                    if (sh.cover) build_cover(SPANS, s, b, j.get(), &wrc);
                    clk.ns[ST_WFORMAT] += StageClock::now() - c2;
                    j->s1 = std::move(f.o1.sp), j->s2 = std::move(f.o2.sp), j->sk = std::move(f.ok.sp);
                    f.o1.sp.clear(), f.o2.sp.clear(), f.ok.sp.clear();
                    j->valid = true;
                }
                if (wrc) rs.fail(wrc, g_last_error);
            }
            j->b = std::move(b);
            fq.push(std::move(j));
        }
        fq.close();
    }

    // a split run's classified records (nh_split.hip): the text of both mates, one span a mate -- in HBM, or copied by the writer
    void build_human(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        const int mates = sh.mates;
        if (step == RESERVE) {  // a mate's classified-out text: its records less what normalisation drops, plus 36 bytes a suffix
            const size_t out_cap[2] = {b.len1 + b.n * 36 + 64, b.len2 + b.n * 36 + 64};
            if (!*rc) *rc = slot_reserve_rec(s, b.n * (size_t)mates);
            if (!*rc) *rc = built_reserve(s.human, 2 * human_out_blocks(b.n) + 2, out_cap, mates, "classified-out buffers");
        } else if (step == LAUNCH) {
            HumanOutArgs ha{};
            batch_source(ha, s, b);
            ha.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res);  // (the call of a host fragment is the true call: the suffix carries it)
            ha.ext = s.e->d_external, ha.n_ext = s.e->external.size();
            ha.n = b.n, ha.nblk = human_out_blocks(b.n);
            built_sink(ha, s.human, mates, s);
            ha.total = s.human.d_total = ha.blk + 2 * ha.nblk;
            timed_launch(rs, s.stream, s.human.ev, "classified-out builder", [&] { return launch_human_out(ha, s.stream); });
        } else {
            for (int m = 0; m < mates && !*rc; m++)
                one_span(j, s.human, m, sh.human_in_hbm, m ? f.h2 : f.h1, m ? j->hs2 : j->hs1, &rs.human_bytes, rc, "classified-out buffers", "classified records");
            for (size_t i = 0; i < b.n; i++) rs.human_records += s.host_res()[i].call != 0;
        }
    }

    // the per-taxon records (nh_split.hip, k_tout_*): the classified records of both mates sorted into the selectors' bins -- a mate's
    // buffer with the bins in it, in HBM or copied by the writer as far as the last bin reaches, and a span a bin that has bytes
    void build_taxon(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        const int mates = sh.mates, K = sh.K;
        if (step == RESERVE) {  // a mate's bins: the classified-out text at most, and the bins' alignment
            const size_t out_cap[2] = {b.len1 + b.n * 36 + 64 + 256 * (size_t)K, b.len2 + b.n * 36 + 64 + 256 * (size_t)K};
            if (!*rc) *rc = slot_reserve_rec(s, b.n * (size_t)mates);
            // (the scratch: block sums of every mate and bin, then start[2][K] and total[2][K]: TaxonOutArgs)
            if (!*rc) *rc = built_reserve(s.taxon, 2 * (size_t)K * human_out_blocks(b.n) + 4 * (size_t)K, out_cap, mates, "per-taxon buffers");
        } else if (step == LAUNCH) {
            TaxonOutArgs ta{};
            batch_source(ta, s, b);
            ta.res = (const nh_result *)s.d_res;
            ta.ext = s.e->d_external, ta.n_ext = s.e->external.size();
            ta.n = b.n, ta.nblk = human_out_blocks(b.n);
            built_sink(ta, s.taxon, mates, s);
            ta.bin_of = dbuf[(size_t)b.dev_index].bin_of, ta.K = K;
            ta.start = s.taxon.d_total = ta.blk + 2 * (uint64_t)K * ta.nblk;
            ta.total = ta.start + 2 * K;
            timed_launch(rs, s.stream, s.taxon.ev, "per-taxon builder", [&] { return launch_taxon_out(ta, s.stream); });
        } else {
            for (int m = 0; m < mates && !*rc; m++) {
                const uint64_t *start = s.taxon.h_total + m * K, *bytes = s.taxon.h_total + 2 * K + m * K;
                size_t end = 0;
                for (int k = 0; k < K; k++)
                    if (bytes[k]) end = (size_t)(start[k] + bytes[k]);
                if (!end) continue;
                if (end > s.taxon.d_out[m].cap) {
                    *rc = set_error(NH_EDEVICE, "per-taxon builder: a bin ends outside its buffer");
                    break;
                }
                char *at = built_span(s.taxon, m, end, sh.taxon_in_hbm, rs, rc, "per-taxon buffers", "per-taxon records");
                for (int k = 0; k < K; k++) {
                    if (!bytes[k]) continue;
                    rs.taxon_bytes += bytes[k];
                    add_built(j, f.tx[m][k], j->ts[m][k], at + start[k], (size_t)bytes[k], sh.taxon_in_hbm);
                }
            }
            for (size_t i = 0; i < b.n; i++) {
                const uint32_t call = s.h_res[i].call;
                const uint8_t bin = call && call < bin_of.size() ? bin_of[call] : 0xFF;
                if (bin < K) rs.taxon_frags[bin]++, rs.taxon_records++;
            }
        }
    }

    // a masked run's records (nh_mask.hip): every record of both mates, masked, one span a mate -- in HBM, or copied by the writer
    void build_mask(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        const int mates = sh.mates;
        if (sh.cut) return build_cut(step, s, b, j, rc);
        if (step == RESERVE) {  // a mate's masked text: its records less what normalisation drops, plus a final newline each
            const size_t out_cap[2] = {b.len1 + b.n + 64, b.len2 + b.n + 64};
            if (!*rc) *rc = slot_reserve_rec(s, b.n * (size_t)mates);
            // (the scratch: block offsets, totals and FAST counts, block flags: MaskArgs)
            if (!*rc) *rc = built_reserve(s.mask, 3 * mask_blocks(b.n) + 4, out_cap, mates, "masked-out buffers");
        } else if (step == LAUNCH) {
            MaskArgs ma{};
            batch_source(ma, s, b);
            ma.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res);
            ma.n = b.n, ma.nblk = mask_blocks(b.n);
            built_sink(ma, s.mask, mates, s);
            ma.total = s.mask.d_total = ma.blk + 2 * ma.nblk;
            ma.fast = (uint32_t *)(ma.total + 4);
            if (sh.hbo) ma.cover = s.d_cover, ma.hb = dbuf[(size_t)b.dev_index].hbcnt;  // (build_cover's, in front of this on the stream)
            timed_launch(rs, s.stream, s.mask.ev, "mask builder", [&] { return launch_mask(ma, s.stream); });
        } else {
            for (int m = 0; m < mates && !*rc; m++) {
                OutFile &of = m ? f.o2 : f.o1;  // (its span list is the batch's, empty in such a run: the writer moves it into the job)
                one_span(j, s.mask, m, sh.mask_in_hbm, of, of.sp, &rs.mask_bytes, rc, "masked-out buffers", "masked records");
            }
            rs.mask_records += b.n * (size_t)mates;
            rs.mask_nblk += mask_blocks(b.n) * (uint64_t)mates;
            for (int m = 0; m < mates; m++) rs.mask_fast += s.mask.h_total[2 + m];
            for (size_t i = 0; i < b.n; i++) rs.mask_masked += (s.host_res()[i].call != 0) * (uint64_t)mates;
            for (size_t i = 0; sh.hbo && i < b.n; i++)
                if (s.host_res()[i].call != 0) rs.hb_host_written += (uint64_t)b.h1->recs[b.off1 + i].slen + (b.h2 ? b.h2->recs[b.off2 + i].slen : 0);
        }
    }

    // a host-cut run's records (nh_cut.hip), in the mask builder's place and buffers: out1's text [0] and the item list it is made
    // from [1]; totals: bytes, items.  A sequence of L bases holds at most cut_max_pieces(L) pieces -- a piece is min_piece bases at
    // least and a covered run of k at least lies between two --, a piece's record is its bases and qualities, its header and at
    // most 22 bytes of coordinates and 5 of seams
    size_t cut_caps(const Batch &b, size_t *extra, size_t *max_item = nullptr) const {
        size_t pieces = 0, bytes = 0, longest = 0;
        for (size_t i = 0; i < b.n; i++) {
            const RecRef &r = b.h1->recs[b.off1 + i];
            const size_t p = (size_t)cut_max_pieces(r.slen, sh.min_piece);
            pieces += p, bytes += p * ((size_t)r.hlen + 29);
            longest = std::max(longest, (size_t)r.hlen + 29 + r.slen + r.qlen);
        }
        if (extra) *extra = bytes;
        if (max_item) *max_item = longest;
        return b.n + pieces;
    }
    void build_cut(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        if (step == RESERVE) {
            size_t extra = 0;
            const size_t cap_items = cut_caps(b, &extra);
            const size_t out_cap[2] = {b.len1 + b.n + 64 + extra, 12 * cap_items + 16};
            if (!*rc) *rc = slot_reserve_rec(s, b.n);
            if (!*rc) *rc = slot_reserve_idl(s, b.n);
            // (the scratch: the sequences' counts, the block offsets of both stages; then the totals: CutArgs)
            if (!*rc) *rc = built_reserve(s.mask, (size_t)cut_scratch_words(b.n, cap_items) + 4, out_cap, 2, "host-cut buffers");
        } else if (step == LAUNCH) {
            CutArgs ca{};
            ca.text = (const char *)s.d_text, ca.ntext = b.ntext();  // (the input's bases, never the masked copy)
            ca.seq_off = (const uint64_t *)s.d_off, ca.seq_len = (const uint32_t *)s.d_len, ca.rec = (const uint32_t *)s.d_rec.p;
            ca.idlen = (const uint32_t *)s.d_idl, ca.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res);
            ca.n = b.n, ca.fastq = b.h1->format == FMT_FASTQ;
            ca.cover = s.d_cover, ca.min_piece = sh.min_piece;  // (build_cover's, closed, in front of this on the stream)
            size_t longest = 0;
            ca.items = (uint32_t *)s.mask.d_out[1].p, ca.cap_items = cut_caps(b, nullptr, &longest), ca.max_item = longest;
            ca.out = s.mask.d_out[0], ca.cap = s.mask.d_out[0].cap;
            ca.scratch = (uint64_t *)s.mask.d_blk;
            ca.total = s.mask.d_total = ca.scratch + cut_scratch_words(b.n, ca.cap_items);
            ca.counts = dbuf[(size_t)b.dev_index].hbcnt + 3, ca.error = s.e->d_error + LAUNCH_SLOTS;
            timed_launch(rs, s.stream, s.mask.ev, "host-cut builder", [&] {
                const hipError_t he = hipMemsetAsync(ca.total, 0, 4 * sizeof(uint64_t), s.stream);  // (four words go back; the builder writes two)
                return he == hipSuccess ? launch_cut(ca, s.stream) : he;
            });
        } else {
            one_span(j, s.mask, 0, sh.mask_in_hbm, f.o1, f.o1.sp, &rs.mask_bytes, rc, "host-cut buffers", "cut records");
            rs.mask_records += b.n, rs.cut_items += s.mask.h_total[1];
            for (size_t i = 0; i < b.n; i++)
                if (s.host_res()[i].call != 0) rs.mask_masked++, rs.hb_host_written += b.h1->recs[b.off1 + i].slen;
        }
    }

    // BAM output (nh_bamout.hip): the selected records of the input's BAM bytes, compacted -- out1's [0] and, a split run, human_out1's
    // [1], one span an output, in HBM or copied by the writer
    void build_bam(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        const int n_bout = sh.n_bout;
        const size_t nrec = b.n * (size_t)sh.mates;  // (the builder's items are records: two a pair)
        if (step == RESERVE) {  // an output's records: the batch's BAM bytes at most
            const size_t out_cap[2] = {b.h1->bam_len + 64, b.h1->bam_len + 64};
            if (!*rc && (!b.h1->dev_bam || !b.h1->dev_bam_table || b.h1->dev_device != s.e->device))
                *rc = set_error(NH_EDEVICE, "BAM output: a batch without its BAM bytes on the device that classifies it");
            // (the scratch: block offsets of every output, totals: BamOutArgs)
            if (!*rc) *rc = built_reserve(s.bam, (size_t)n_bout * bam_out_blocks(nrec) + 2, out_cap, n_bout, "BAM-out buffers");
        } else if (step == LAUNCH) {
            BamOutArgs ba{};
            ba.bam = b.h1->dev_bam, ba.bam_len = b.h1->bam_len;
            // (a part of a half: a range of its table, two words a record -- of a paired BAM: two a pair, its records in file order)
            ba.table = b.h1->dev_bam_table + 2 * b.off1;
            ba.pairs = rs.paired;
            ba.n = nrec, ba.nblk = bam_out_blocks(nrec);
            ba.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res);
            ba.n_out = n_bout;
            ba.want[0] = sh.split_files ? 0 : a->keep_human != 0;  // out1: the non-host records, with keep_human the host records
            ba.want[1] = 1;                                         // human_out1: the host records
            built_sink(ba, s.bam, n_bout, s);
            ba.total = s.bam.d_total = ba.blk + (uint64_t)n_bout * ba.nblk;
            ba.err_fields = ba.err_total = 256;
            dev_check_ptr(ba.bam, s.e->device, "nh_run, a batch's BAM bytes");
            dev_check_ptr(ba.table, s.e->device, "nh_run, a batch's BAM table");
            timed_launch(rs, s.stream, s.bam.ev, "BAM-out builder", [&] { return launch_bam_out(ba, s.stream); });
        } else {
            for (int o = 0; o < n_bout && !*rc; o++) {
                const size_t tot = (size_t)s.bam.h_total[o];
                rs.bam_bytes[o] += tot;
                const bool want_host = sh.split_files ? o == 1 : a->keep_human != 0;
                for (size_t i = 0; i < b.n; i++) rs.bam_records[o] += (uint64_t)sh.mates * ((s.host_res()[i].call != 0) == want_host);
                if (!tot) continue;
                if (tot > s.bam.d_out[o].cap) {
                    *rc = set_error(NH_EDEVICE, "BAM-out builder: an output ends outside its buffer");
                    break;
                }
                char *at = built_span(s.bam, o, tot, sh.bam_in_hbm, rs, rc, "BAM-out buffers", "BAM records");
                // (out1's span list is the batch's, empty in such a run: the writer moves it into the job)
                add_built(j, o ? f.h1 : f.o1, o ? j->hs1 : f.o1.sp, at, tot, sh.bam_in_hbm);
            }
        }
    }

    // the read lists (nh_calls.hip): the calls table [0] and the human ids [1] -- exactly the built bytes, copied to the slot's
    // page-locked memory, one span a file
    void build_lists(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        if (step == RESERVE) {
            // a table line: "C\t", the id, then at most 1 + 20 + 1 + 21 + 1 + 3 * 11 bytes of numbers, separators and
            // the newline; an id line: the id and a newline
            uint64_t idsum = 0;
            for (size_t i = 0; i < b.n; i++) idsum += b.h1->recs[b.off1 + i].idlen;
            const size_t out_cap[2] = {sh.calls ? (size_t)idsum + b.n * 79 + 64 : 0, sh.ids ? (size_t)idsum + b.n + 64 : 0};
            if (!*rc) *rc = slot_reserve_rec(s, b.n * (size_t)sh.mates);
            if (!*rc) *rc = slot_reserve_idl(s, b.n);
            // (the scratch: block offsets and line counts of both outputs, totals: CallsArgs)
            if (!*rc) *rc = built_reserve(s.lists, 4 * calls_blocks(b.n) + 4, out_cap, 2, "read-list buffers");
        } else if (step == LAUNCH) {
            CallsArgs ca{};
            batch_records(ca, s, b);
            ca.idlen = (const uint32_t *)s.d_idl;
            ca.res = (const nh_result *)s.d_res;
            ca.res_ids = sh.hsel ? (const nh_result *)s.d_hres : nullptr;  // (the table keeps the true calls; the id list is the host fragments')
            ca.ext = s.e->d_external, ca.n_ext = s.e->external.size();
            ca.n = b.n, ca.nblk = calls_blocks(b.n);
            ca.want[0] = sh.calls, ca.want[1] = sh.ids;
            built_sink(ca, s.lists, 2, s);
            ca.total = s.lists.d_total = ca.blk + 4 * ca.nblk;
            timed_launch(rs, s.stream, s.lists.ev, "read-list builder", [&] { return launch_calls(ca, s.stream); });
        } else {
            for (int o = 0; o < 2 && !*rc; o++) {
                rs.list_lines[o] += s.lists.h_total[2 + o];
                one_span(j, s.lists, o, false, o ? f.oi : f.oc, o ? j->si : j->sc, &rs.list_bytes[o], rc, "read-list buffers", "read list");
            }
        }
    }

    // the host intervals (nh_cover.hip): the bitmap zeroed, the mark pass on the text the classifier read, the bitmap into records,
    // the records into BED lines -- exactly the built bytes, copied to the slot's page-locked memory, one span.  An interval holds
    // k = 35 bases at least and a base that is not covered lies between two of a sequence: (len + 1) / 36 of them at the most
    static size_t cover_max_intervals(size_t len) { return (len + 1) / 36; }
    size_t cover_max_records(const Batch &b, size_t *line_bytes) const {
        size_t nrec = 0, nbytes = 0;
        for (size_t i = 0; i < b.n; i++) {
            size_t m = cover_max_intervals(b.h1->recs[b.off1 + i].slen);
            if (b.h2) m += cover_max_intervals(b.h2->recs[b.off2 + i].slen);
            // a line: the id, then at most 1 + 10 + 1 + 10 + 2 + 1 + 20 + 1 bytes of numbers, separators and the newline
            nrec += m, nbytes += m * ((size_t)b.h1->recs[b.off1 + i].idlen + 46);
        }
        if (line_bytes) *line_bytes = nbytes;
        return nrec;
    }
    void build_cover(BuildStep step, Slot &s, const Batch &b, FlushJob *j, int *rc) {
        const int mates = sh.mates;
        const size_t nseq = b.n * (size_t)mates;
        const size_t pass_words = (size_t)std::max(cover_mark_scratch_words(nseq), cover_intervals_scratch_words(nseq));
        // (--host-bases-only without the report: the bitmap and the mark pass's scratch alone, no record, no line)
        if (step == RESERVE) {
            size_t nbytes = 0;
            const size_t nrec = sh.cover ? cover_max_records(b, &nbytes) : 0;
            const size_t out_cap[2] = {nbytes + 64, (nrec + 1) * 12};
            if (!*rc) *rc = slot_reserve_rec(s, nseq);
            if (!*rc && sh.cover) *rc = slot_reserve_idl(s, b.n);
            // (the scratch: the larger of the mark pass's and the interval builder's, the records' total, the line builder's block sums and totals)
            if (!*rc) *rc = built_reserve(s.cover, pass_words + 1 + 3 * (size_t)cover_line_blocks(nrec) + 4, out_cap, 2, "host-interval buffers");
            const size_t cw = (size_t)cover_words(b.ntext());
            if (!*rc && !have(s.d_cover, cw)) *rc = set_error(NH_EOOM, "cannot allocate the host intervals' bitmap (%zu words)", grow(cw));
        } else if (step == LAUNCH) {
            const uint64_t ntext = b.ntext();
            const size_t nrec = sh.cover ? cover_max_records(b, nullptr) : 0;
            int *const d_error = s.e->d_error + LAUNCH_SLOTS;
            uint64_t *const scratch = (uint64_t *)s.cover.d_blk;
            uint64_t *const n_ivl = scratch + pass_words;
            CoverArgs ca{};
            ca.text = (const char *)(sh.qtext ? s.d_qtext : s.d_text), ca.ntext = ntext;
            ca.seq_off = (const uint64_t *)s.d_off, ca.seq_len = (const uint32_t *)s.d_len, ca.n_seq = nseq;
            ca.host_of = sh.hsel ? dbuf[(size_t)b.dev_index].host_of : nullptr, ca.n_nodes = s.e->external.size();
            ca.cover = s.d_cover, ca.scratch = scratch, ca.error = d_error;
            CoverIvlArgs ia{};
            ia.cover = s.d_cover, ia.ntext = ntext, ia.seq_off = ca.seq_off, ia.seq_len = ca.seq_len, ia.n_seq = nseq;
            ia.rec = (uint32_t *)s.cover.d_out[1].p, ia.cap = nrec, ia.total = n_ivl, ia.scratch = scratch, ia.error = d_error;
            CoverLinesArgs la{};
            la.text = (const char *)s.d_text, la.ntext = ntext;
            la.rec = (const uint32_t *)s.d_rec.p, la.idlen = (const uint32_t *)s.d_idl, la.res = (const nh_result *)s.d_res;
            la.ext = s.e->d_external, la.n_ext = s.e->external.size(), la.n = b.n, la.mates = mates;
            la.ivl = ia.rec, la.n_ivl = n_ivl, la.cap_ivl = nrec;
            la.out = s.cover.d_out[0], la.cap = s.cover.d_out[0].cap;
            la.blk = n_ivl + 1, la.nblk = cover_line_blocks(nrec);
            la.total = s.cover.d_total = la.blk + 3 * la.nblk;
            la.error = d_error;
            CoverCloseArgs cl{};
            cl.cover = s.d_cover, cl.ntext = ntext, cl.seq_off = ca.seq_off, cl.seq_len = ca.seq_len, cl.n_seq = nseq;
            cl.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res), cl.mates = mates;  // (the host fragments alone: closed_bases counts what is masked)
            cl.gap = sh.gap, cl.closed = sh.close ? dbuf[(size_t)b.dev_index].hbcnt + 2 : nullptr, cl.error = d_error;
            timed_launch(rs, s.stream, s.cover.ev, "host intervals", [&] {
                hipError_t he = hipMemsetAsync(s.d_cover, 0, (size_t)cover_words(ntext) * 4, s.stream);
                if (he == hipSuccess) he = launch_cover_mark(s.e, ca, s.stream);
                if (he == hipSuccess && sh.cover) he = launch_cover_intervals(ia, s.stream);
                if (he == hipSuccess && sh.cover) he = launch_cover_lines(la, s.stream);
                if (he == hipSuccess && !sh.cover) he = hipMemsetAsync(la.total, 0, 4 * sizeof(uint64_t), s.stream);  // (the totals go back all the same)
                if (he == hipSuccess && sh.close) he = launch_cover_close(cl, s.stream);  // (behind the report: the BED is the coverage before the closing)
                return he;
            });
        } else {
            rs.cover_ivls += s.cover.h_total[1], rs.cover_frags += s.cover.h_total[2], rs.cover_bases += s.cover.h_total[3];
            one_span(j, s.cover, 0, false, f.ohi, j->shi, &rs.cover_bytes, rc, "host-interval buffers", "host intervals");
        }
    }

    // main: pair halves, stage, launch
    void run() {
        for (bool last = false; !last && !rs.failed();) {
            Batch b;
            const uint64_t m0 = StageClock::now();
            if (!next_batch(b, &last) || (b.n > 0 && !submit(b, m0))) break;
        }
    }

    // the next batch of the two files' halves; false: an input has ended (or the run was shut down)
    bool next_batch(Batch &b, bool *last) {
        auto take = [](BoundedQueue<std::unique_ptr<HalfBatch>> &q, BatchPool *pool, std::shared_ptr<HalfBatch> &c, size_t &pos, size_t &len) {
            std::unique_ptr<HalfBatch> u;
            if (!q.pop(u)) return false;
            c = std::shared_ptr<HalfBatch>(u.release(), [pool](HalfBatch *h) { pool->put(std::unique_ptr<HalfBatch>(h)); });
            pos = 0;
            len = c->text.size();
            return true;
        };
        if (!c1 && !take(q1, &pool1, c1, p1, cl1)) return false;
        if (rs.paired && !c2 && !take(q2, &pool2, c2, p2, cl2)) return false;
        // kraken2 reads the files in lockstep and stops at the shorter one.  Both readers cut batches at the same record
        // counts, so the halves normally pair up whole; where they do not (see Batch) the shorter one decides and the rest of
        // the longer one pairs with the other file's next half -- no read is dropped, no run stopped
        b.h1 = c1, b.off1 = p1, b.len1 = cl1;
        b.n = c1->recs.size() - p1;
        if (rs.paired) {
            b.h2 = c2, b.off2 = p2, b.len2 = cl2;
            b.n = std::min(b.n, c2->recs.size() - p2);
            p2 += b.n;
        }
        p1 += b.n;
        // a half that is used up is let go of HERE, not when the next one arrives: a reader on the GPU may need its buffer to
        // produce that next one (a piece smaller than a batch hands out nothing until the piece behind it is decoded)
        const bool done1 = p1 == c1->recs.size(), done2 = rs.paired && p2 == c2->recs.size();
        *last = (done1 && c1->eof) || (done2 && c2->eof);
        if (done1) c1.reset();
        if (done2) c2.reset();
        return true;
    }

    // one batch through the stages; false: the run has failed in a way that ends the loop (the batch still goes to the writer,
    // which gives its buffers back)
    bool submit(Batch &b, uint64_t m0) {
        const uint64_t m1 = StageClock::now();
        clk.ns[ST_MPOP] += m1 - m0;
        Slot &s = pick_slot(b);
        const uint64_t m2 = StageClock::now();
        clk.ns[ST_MSLOT] += m2 - m1;
        int rc;
        if (b.ntext() >= (1ull << 32))
            rc = set_error(NH_EINVAL, "a batch of more than 4 GB of record text (its offsets are 32-bit): paired records of several kilobases each are not supported");
        else rc = reserve(s, b);
        if (rc) {
            rs.fail(rc, g_last_error);
            wq.push(std::move(b));
            return false;
        }
        dev_check_ptr(s.d_text, s.e->device, "nh_run, a slot's text buffer");
        const uint64_t nbases = gather(s, b);
        // H2D, classify, D2H: all asynchronous on the slot's stream
        const uint64_t m3 = StageClock::now();
        clk.ns[ST_MGATHER] += m3 - m2;
        const bool staged = stage_text(s, b);
        launch(s, b, nbases, staged);
        queue_results(s, b);
        batch_no++;
        frags_out += b.n;
        wq.push(std::move(b));
        clk.ns[ST_MLAUNCH] += StageClock::now() - m3;
        return true;
    }

    // the slot: in turn over all devices' slots -- but a batch born on a GPU (the gzip reader there) is classified
    // on THAT device, in that device's slots in turn, unless they are all busy and another device has a free one
    // (then its text crosses xGMI once); the writer takes the batches in the order they are pushed, whatever the slot
    Slot &pick_slot(Batch &b) {
        const int G = sh.G, NS = sh.NS;
        int si = (int)(batch_no % (uint64_t)(NS * G));
        {
            int home = -1;
            if (G > 1 && b.h1->dev_text)
                for (int g = 0; g < G; g++)
                    if (engines[(size_t)g]->device == b.h1->dev_device) {
                        home = g;
                        break;
                    }
            std::unique_lock<std::mutex> lk(slot_mu);
            if (home >= 0) {
                si = home * NS + (int)(home_turn[(size_t)home]++ % (uint64_t)NS);
                if (slots[(size_t)si].busy && !sh.bamout)  // (BAM output: the builder reads the batch's BAM bytes where they lie)
                    for (int i = 0; i < NS * G; i++)
                        if (!slots[(size_t)i].busy) {
                            si = i;
                            break;
                        }
            }
            slot_cv.wait(lk, [&] { return !slots[(size_t)si].busy; });
            slots[(size_t)si].busy = true;
        }
        b.slot = si;
        b.dev_index = si / NS;
        return slots[(size_t)si];
    }

    // the slot's buffers for this batch, every active feature's; then the refusal of a record the quality passes cannot read
    int reserve(Slot &s, const Batch &b) {
        uint64_t ntaxa = 0;
        for (size_t i = 0; rs.want_k && i < b.n; i++) ntaxa += b.kmer_taxa(i, s.e->info.k);
        int rc = slot_reserve(s, b.ntext(), b.n, ntaxa + 1);
        for (const Builder &bd : builders)  // (the totals that come back with the results: queue_results copies total_words of them)
            if (!rc && (s.*bd.out).h_total.reserve(bd.total_words) != hipSuccess) rc = set_error(NH_EOOM, "cannot allocate batch buffers");
        if (sh.split) build_human(RESERVE, s, b, nullptr, &rc);
        if (sh.taxa) build_taxon(RESERVE, s, b, nullptr, &rc);
        if (sh.mask) build_mask(RESERVE, s, b, nullptr, &rc);
        if (sh.bamout) build_bam(RESERVE, s, b, nullptr, &rc);
        if (sh.lists) build_lists(RESERVE, s, b, nullptr, &rc);
        if (sh.mark) build_cover(RESERVE, s, b, nullptr, &rc);
        if (!rc && sh.qm) rc = slot_reserve_qmask(s, b.ntext(), b.n * (size_t)sh.mates);
        if (!rc && sh.dust) rc = slot_reserve_dust(s, b.ntext(), b.n * (size_t)sh.mates);
        if (!rc && sh.rst) rc = slot_reserve_rec(s, b.n * (size_t)sh.mates);
        if (!rc && sh.hsel) rc = slot_reserve_pair(s.h_hres, s.d_hres, b.n, "host-filtered results");
        if (!rc && (sh.qm || sh.rst || sh.cut)) rc = check_quality_lengths(b);
        return rc;
    }

    // kraken2 ends a run at a FASTQ record whose quality line is not as long as its sequence when it masks by quality;
    // the read statistics count a base per quality as well
    int check_quality_lengths(const Batch &b) {
        for (size_t i = 0; i < b.n; i++)
            for (int m = 0; m < sh.mates; m++) {
                const HalfBatch &hb = m ? *b.h2 : *b.h1;
                const RecRef &rr = hb.recs[(m ? b.off2 : b.off1) + i];
                if (hb.format == FMT_FASTQ && rr.qlen != rr.slen)
                    return set_error(NH_EIO, "%s, read %llu: sequence length (%u) != quality string length (%u), which %s", m && a->in2 ? a->in2 : a->in1,
                                     (unsigned long long)(frags_out + i + 1), rr.slen, rr.qlen,
                                     sh.qm ? "--minimum-base-quality cannot mask" : sh.rst ? "--read-stats cannot count" : "--host-cut cannot slice");
            }
        return NH_OK;
    }

    // (start, length) of every sequence inside the raw text -- text of file 1 at byte 0 of the device buffer, text of file 2
    // behind it --, the record table, the id lengths, where each fragment's k-mer taxa go; returns the batch's bases
    uint64_t gather(Slot &s, const Batch &b) {
        const int mates = sh.mates;
        const size_t base2 = b.base2();
        uint64_t nbases = 0, toff = 0;
        for (size_t i = 0; i < b.n; i++) {
            const RecRef &r1 = b.h1->recs[b.off1 + i];
            s.h_off[i * mates] = r1.s;
            s.h_len[i * mates] = r1.slen;
            nbases += r1.slen;
            if (sh.idl) s.h_idl[i] = r1.idlen;
            if (sh.want_rec) {
                uint32_t *hr = s.h_rec[i * mates];
                hr[0] = r1.h, hr[1] = r1.hlen, hr[2] = r1.q, hr[3] = r1.qlen;
                if (rs.paired) {
                    const RecRef &r2 = b.h2->recs[b.off2 + i];
                    hr[4] = (uint32_t)(base2 + r2.h), hr[5] = r2.hlen, hr[6] = (uint32_t)(base2 + r2.q), hr[7] = r2.qlen;
                }
            }
            if (rs.want_k) s.h_taxa_off[i] = toff, toff += b.kmer_taxa(i, s.e->info.k);
            if (rs.paired) {
                const RecRef &r2 = b.h2->recs[b.off2 + i];
                s.h_off[i * mates + 1] = base2 + r2.s;
                s.h_len[i * mates + 1] = r2.slen;
                nbases += r2.slen;
            }
        }
        if (rs.want_k) s.h_taxa_off[b.n] = toff;
        s.n_taxa = toff;
        return nbases;
    }

    // the batch's text and its tables onto the slot's stream; false: a copy failed (and failed the run)
    bool stage_text(Slot &s, Batch &b) {
        const int mates = sh.mates;
        hipError_t he = dev_set(s.e->device);
        // test knob of the checker itself: the launch goes out under the run's FIRST device whatever slot carries it
        static const bool brk = getenv("NOHUMAN_DEBUG_DEVICE_BREAK") != nullptr;
        if (brk) he = dev_set(engines[0]->device);
        // the batch's text: from the host as it was read, or -- a batch of the reader on the GPU -- from HBM to HBM (from
        // another device's memory: over xGMI); the bytes then go to the host only if an output written there needs them
        auto half = [&](HalfBatch &hb, size_t at, size_t len) -> hipError_t {
            if (!len) return hipSuccess;
            if (!hb.dev_text) return hipMemcpyAsync((char *)s.d_text + at, hb.text.data(), len, hipMemcpyHostToDevice, s.stream);
            hipError_t e2 = dev_copy_between((char *)s.d_text + at, s.e->device, hb.dev_text, hb.dev_device, len, s.stream);
            if (e2 == hipSuccess && sh.host_text_wanted && !hb.host_text_valid) {  // (a half used in parts is fetched by its first)
                hb.text.clear();  // (a batch born on the GPU comes with a token buffer: the real one only where it is needed)
                if (!hb.text.reserve(len + 64)) return hipErrorOutOfMemory;
                hb.text.set_size(len);
                e2 = hipMemcpyAsync(hb.text.data(), (char *)s.d_text + at, len, hipMemcpyDeviceToHost, s.stream);
                rs.text_fetched += len;
                hb.host_text_valid = true;  // (once the stream has been synchronised: the writer does that first)
            }
            return e2;
        };
        if (he == hipSuccess) he = half(*b.h1, 0, b.len1);
        if (he == hipSuccess && rs.paired) he = half(*b.h2, b.base2(), b.len2);
        if (he == hipSuccess) he = hipMemcpyAsync(s.d_off, s.h_off, b.n * mates * 8, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess) he = hipMemcpyAsync(s.d_len, s.h_len, b.n * mates * 4, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess && rs.want_k) he = hipMemcpyAsync(s.d_taxa_off, s.h_taxa_off, (b.n + 1) * 8, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess && sh.want_rec) he = hipMemcpyAsync(s.d_rec, s.h_rec, b.n * mates * 16, hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess && sh.idl) he = hipMemcpyAsync(s.d_idl, s.h_idl, b.n * 4, hipMemcpyHostToDevice, s.stream);
        if (he != hipSuccess) rs.fail(NH_EDEVICE, std::string("H2D: ") + hipGetErrorString(he));
        return he == hipSuccess;
    }

    // the batch's launches on the slot's stream, in this order: the quality mask, the read DUST (on a copy of the text where no
    // quality mask has written the sequences), the classifier, the host filter, the read
    // statistics, the minimizer data's marks, then the builders -- lists, host intervals (the cover bitmap, its closing), split, BAM out, per-taxon, mask.  Each goes out only
    // while the run has not failed.
    void launch(Slot &s, const Batch &b, uint64_t nbases, bool staged) {
        const int mates = sh.mates;
        const uint64_t ntext = b.ntext();
        RunBuffers &db = dbuf[(size_t)b.dev_index];
        int *const d_error = s.e->d_error + LAUNCH_SLOTS;
        if (staged && sh.qm) {  // the sequences the classifier reads: a copy with 'N' where the quality is below minq
            dev_check_ptr(s.d_qtext, s.e->device, "nh_run, a slot's quality-masked text");
            QmaskArgs qa{};
            batch_source(qa, s, b);
            qa.n = b.n * (uint64_t)mates;
            qa.thresh = sh.minq + 33;
            qa.out = (char *)s.d_qtext, qa.masked = s.d_qcnt, qa.error = d_error;
            timed_launch(rs, s.stream, s.qev, "quality mask", [&] { return launch_qmask(qa, s.stream); });
        }
        if (staged && sh.dust && !rs.failed()) {  // ... and 'N' over the low-complexity stretches of every sequence: the union of the masks
            dev_check_ptr(s.d_qtext, s.e->device, "nh_run, a slot's DUST-masked text");
            if (!sh.qm && hipMemcpyAsync(s.d_qtext, s.d_text, ntext, hipMemcpyDeviceToDevice, s.stream) != hipSuccess)
                rs.fail(NH_EDEVICE, "read DUST: the copy of the batch's text failed");
            ReadDustArgs da{};
            da.text = (const char *)s.d_text, da.ntext = ntext;  // (DUST reads the input's bases, not the quality-masked ones)
            da.seq_off = (const uint64_t *)s.d_off, da.seq_len = (const uint32_t *)s.d_len, da.n = b.n * (uint64_t)mates;
            da.out = (char *)s.d_qtext, da.masked = s.d_dcnt, da.error = d_error;
            if (!rs.failed()) timed_launch(rs, s.stream, s.duev, "read DUST", [&] { return launch_read_dust(da, s.d_dscr, s.dust_grid, s.stream); });
        }
        if (!rs.failed()) {
            const int rc = classify_device(s.e, sh.qtext ? s.d_qtext : s.d_text, s.d_off, b.n, sh.flags | (nbases / b.n > 2000 ? NH_FLAG_LONG : 0u),
                                           a->confidence, s.d_res, rs.want_k ? s.d_taxa : nullptr, rs.want_k ? s.d_taxa_off : nullptr,
                                           rs.d_run_counters[(size_t)b.dev_index], s.stream, s.d_len, ntext);
            if (rc) rs.fail(rc, g_last_error);
        }
        // the results that decide host-ness from here on: the classifier's, or -- a host selection -- their copy with call = 0
        // where the fragment is not host, made right behind the classifier on the same stream
        if (!rs.failed() && sh.hsel)
            timed_launch(rs, s.stream, s.hev, "host filter",
                         [&] { return launch_host_filter(s.d_res, s.d_hres, b.n, db.host_of, s.e->external.size(), db.hcnt, d_error, s.stream); });
        if (!rs.failed() && sh.rst) {  // the read statistics, counted behind the classifier on the same stream: the INPUT's bases
            RstatsArgs ta{};
            batch_source(ta, s, b);
            ta.n = b.n * (uint64_t)mates;
            ta.res = (const nh_result *)(sh.hsel ? s.d_hres : s.d_res);
            ta.acc = db.racc, ta.error = d_error;
            timed_launch(rs, s.stream, s.rev, "read statistics", [&] { return launch_rstats(ta, s.e->n_cu, 0, s.stream); });
        }
        if (!rs.failed() && sh.mdt)  // minimizer data, marked behind the classifier on the same stream: the text the classifier read
            timed_launch(rs, s.stream, s.mev, "minimizer data", [&] {
                return launch_mdata_mark(s.e, sh.qtext ? s.d_qtext : s.d_text, ntext, s.d_off, s.d_len, b.n, mates, db.marks, db.groups, s.stream);
            });
        int none = NH_OK;  // (a launch fails the run itself)
        if (!rs.failed() && sh.lists) build_lists(LAUNCH, s, b, nullptr, &none);
        if (!rs.failed() && sh.mark) build_cover(LAUNCH, s, b, nullptr, &none);
        if (!rs.failed() && sh.split) build_human(LAUNCH, s, b, nullptr, &none);
        if (!rs.failed() && sh.bamout) build_bam(LAUNCH, s, b, nullptr, &none);
        if (!rs.failed() && sh.taxa) build_taxon(LAUNCH, s, b, nullptr, &none);
        if (!rs.failed() && sh.mask) build_mask(LAUNCH, s, b, nullptr, &none);
    }

    // the copies of the batch's results back to the host, behind its launches on the slot's stream
    void queue_results(Slot &s, const Batch &b) {
        if (rs.failed()) return;
        hipError_t he = hipMemcpyAsync(s.h_res, s.d_res, b.n * sizeof(nh_result), hipMemcpyDeviceToHost, s.stream);
        if (he == hipSuccess && sh.hsel) he = hipMemcpyAsync(s.h_hres, s.d_hres, b.n * sizeof(nh_result), hipMemcpyDeviceToHost, s.stream);
        if (he == hipSuccess) he = hipMemcpyAsync(s.h_flag, s.e->d_error + LAUNCH_SLOTS, sizeof(int), hipMemcpyDeviceToHost, s.stream);
        if (he == hipSuccess && rs.want_k && s.n_taxa) he = hipMemcpyAsync(s.h_taxa, s.d_taxa, s.n_taxa * 4, hipMemcpyDeviceToHost, s.stream);
        for (const Builder &bd : builders) {
            BuiltOut &o = s.*bd.out;
            if (he == hipSuccess) he = hipMemcpyAsync(o.h_total, o.d_total, bd.total_words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
        }
        if (he != hipSuccess) rs.fail(NH_EDEVICE, std::string("D2H: ") + hipGetErrorString(he));
    }

    // shuts the pipeline down (also on errors): unblocks the readers, drains the writer, joins every thread
    void shutdown() {
        c1.reset(), c2.reset();  // (a reader on the GPU waits in close() for every batch it handed out)
        pool1.stop(), pool2.stop();
        q1.close(), q2.close(), wq.close();
        {   // what the readers had queued is dropped (a batch born on the GPU gives its text buffer back: its reader waits for that)
            std::unique_ptr<HalfBatch> drop;
            while (q1.pop(drop)) drop.reset();
            while (q2.pop(drop)) drop.reset();
        }
        t1.join();
        if (t2.joinable()) t2.join();
        tw.join(), tf.join();
        if (tw2.joinable()) {
            {
                std::lock_guard<std::mutex> lk(w2_mu);
                w2_state = -1;
            }
            w2_cv.notify_all();
            tw2.join();
        }
    }
};
}  // namespace

// ---- after the pipeline -------------------------------------------------------------------------------
// NOHUMAN_TRACE=1: where the wall time went, and a line a feature of the run
static void print_run_trace(const RunShape &sh, RunState &rs, const StageClock &clk, double wall, const std::vector<nh_read_class> &racc,
                            const MdataNumbers &mdn, double md_count_ms, const uint64_t dev_host[2]) {
    static const char *names[] = {"read1", "read2", "rpush1", "rpush2", "main.pop", "main.slot", "main.gather",
                                  "main.launch", "wr.pop", "wr.sync", "wr.format", "wr.write"};
    const unsigned long long fetched = rs.text_fetched.load();
    fprintf(stderr, "[nohuman trace] wall %.3fs |", wall);
    for (int i = 0; i < 12; i++) fprintf(stderr, " %s %.3f", names[i], (double)clk.ns[i].load() * 1e-9);
    fprintf(stderr, "\n");
    if (sh.split)
        fprintf(stderr, "[nohuman trace] human-out: %llu records, %llu bytes built on device; %llu fetched to host; builder kernels %.3f ms (%.1f GB/s of text)\n",
                (unsigned long long)rs.human_records, (unsigned long long)rs.human_bytes, fetched,
                rs.human_kernel_ms, rs.human_kernel_ms > 0 ? (double)rs.human_bytes / (rs.human_kernel_ms * 1e6) : 0.0);
    if (sh.bamout)
        fprintf(stderr, "[nohuman trace] bam-out: %llu + %llu records, %llu + %llu bytes selected on device; %llu fetched to host; builder kernels %.3f ms (%.1f GB/s of records)\n",
                (unsigned long long)rs.bam_records[0], (unsigned long long)rs.bam_records[1], (unsigned long long)rs.bam_bytes[0],
                (unsigned long long)rs.bam_bytes[1], fetched, rs.bam_kernel_ms,
                rs.bam_kernel_ms > 0 ? (double)(rs.bam_bytes[0] + rs.bam_bytes[1]) / (rs.bam_kernel_ms * 1e6) : 0.0);
    if (sh.mask)
        fprintf(stderr, "[nohuman trace] mask: %llu records masked, %llu written, %llu bytes built on device; %llu fetched to host; builder kernels %.3f ms (%.1f GB/s of text); %llu of %llu blocks copied whole\n",
                (unsigned long long)rs.mask_masked, (unsigned long long)rs.mask_records, (unsigned long long)rs.mask_bytes,
                fetched, rs.mask_kernel_ms, rs.mask_kernel_ms > 0 ? (double)rs.mask_bytes / (rs.mask_kernel_ms * 1e6) : 0.0,
                (unsigned long long)rs.mask_fast, (unsigned long long)rs.mask_nblk);
    if (sh.taxa)
        fprintf(stderr, "[nohuman trace] taxon-out: %llu records, %llu bytes built on device; %llu fetched to host; kernel %.3f ms\n",
                (unsigned long long)rs.taxon_records, (unsigned long long)rs.taxon_bytes, fetched, rs.taxon_kernel_ms);
    if (sh.lists)
        fprintf(stderr, "[nohuman trace] calls: %llu lines, %llu bytes; ids: %llu lines, %llu bytes built on device; %llu fetched to host; builder kernels %.3f ms\n",
                (unsigned long long)rs.list_lines[0], (unsigned long long)rs.list_bytes[0], (unsigned long long)rs.list_lines[1],
                (unsigned long long)rs.list_bytes[1], fetched, rs.list_kernel_ms);
    if (sh.cover)
        fprintf(stderr, "[nohuman trace] host-intervals: %llu intervals in %llu fragments, %llu bases covered, %llu bytes built on device; kernels %.3f ms\n",
                (unsigned long long)rs.cover_ivls, (unsigned long long)rs.cover_frags, (unsigned long long)rs.cover_bases,
                (unsigned long long)rs.cover_bytes, rs.cover_kernel_ms);
    if (sh.hbo)
        fprintf(stderr, "[nohuman trace] host-bases-only: %llu of %llu host bases masked, %llu by closing; gap %u, cover kernels %.3f ms, mask builder kernels %.3f ms\n",
                (unsigned long long)rs.hb_bases[1], (unsigned long long)rs.hb_bases[0], (unsigned long long)rs.hb_bases[2], sh.gap, rs.cover_kernel_ms,
                rs.mask_kernel_ms);
    if (sh.cut)
        fprintf(stderr, "[nohuman trace] host-cut: %llu host bases: %llu in %llu pieces, %llu cut (%llu by closing), %llu in short runs; %llu reads dropped; %llu items; gap %u, min piece %u, cover kernels %.3f ms, cut builder kernels %.3f ms\n",
                (unsigned long long)rs.cut_counts[CUT_HOST_BASES], (unsigned long long)rs.cut_counts[CUT_PIECE_BASES], (unsigned long long)rs.cut_counts[CUT_PIECES],
                (unsigned long long)rs.cut_counts[CUT_CUT_BASES], (unsigned long long)rs.hb_bases[2], (unsigned long long)rs.cut_counts[CUT_SHORT_BASES],
                (unsigned long long)rs.cut_counts[CUT_DROPPED], (unsigned long long)rs.cut_items, sh.gap, sh.min_piece, rs.cover_kernel_ms, rs.mask_kernel_ms);
    if (sh.qm)
        fprintf(stderr, "[nohuman trace] qmask: Q %u, %llu of %llu bases masked, kernel %.3f ms\n", sh.minq,
                (unsigned long long)rs.qmask_masked, (unsigned long long)rs.total_bases, rs.qmask_kernel_ms);
    if (sh.dust)
        fprintf(stderr, "[nohuman trace] dust-reads: %llu of %llu bases masked, kernel %.3f ms\n", (unsigned long long)rs.dust_masked,
                (unsigned long long)rs.total_bases, rs.dust_kernel_ms);
    if (sh.rst && racc.size() == 4)
        fprintf(stderr, "[nohuman trace] rstats: %llu bases, kernel %.3f ms\n",
                (unsigned long long)(racc[0].bases + racc[1].bases + racc[2].bases + racc[3].bases), rs.rstats_kernel_ms);
    if (sh.mdt && rs.err_code == NH_OK) {
        unsigned long long groups = 0, distinct = 0;
        for (uint64_t v : mdn.v[3]) groups += v;
        for (uint64_t v : mdn.v[5]) distinct += v;
        fprintf(stderr, "[nohuman trace] minimizer data: %llu hit groups on %llu distinct minimizers, k_mdata_mark %.3f ms, k_mdata_count %.3f ms\n", groups,
                distinct, rs.mdata_kernel_ms, md_count_ms);
    }
    if (sh.hsel && rs.err_code == NH_OK)
        fprintf(stderr, "[nohuman trace] host-filter: %llu host, %llu spared fragments; kernel %.3f ms\n", (unsigned long long)dev_host[0],
                (unsigned long long)dev_host[1], rs.host_kernel_ms);
    if (g_pageable_batches.load())
        fprintf(stderr, "[nohuman trace] %d batch buffers could not be page-locked (pageable memory used)\n", g_pageable_batches.load());
}

// closes the outputs: the record files side by side (the last chunks of two GPU encoders, their buffers' release), then the
// selectors' files, the -k file and the read lists one after the other
static int close_run_files(RunFiles &f, const RunShape &sh, const RunState &rs) {
    int rc = record_files_side_by_side(f, sh.files2, sh.split_files, [](OutFile &of, int) { return of.close(); });
    if (rc) return rc;
    for (int k = 0; k < sh.K; k++)
        for (int m = 0; m < sh.mates; m++)
            if ((rc = f.tx[m][k].close())) return rc;
    if (rs.want_k && (rc = f.ok.close())) return rc;
    if (sh.calls && (rc = f.oc.close())) return rc;
    if (sh.ids && (rc = f.oi.close())) return rc;
    if (sh.cover && (rc = f.ohi.close())) return rc;
    return NH_OK;
}

// read statistics: the devices' sums and the writer's lengths into the run's nh_read_stats -- median and N50 from every length --,
// checked against each other, written to the table and to the caller's struct
static int finish_read_stats(const RunRequest &r, const RunState &rs, int mates, const std::vector<nh_read_class> &racc) {
    nh_read_stats out;
    memset(&out, 0, sizeof out);
    out.mates = mates;
    uint64_t dev_reads = 0, dev_bases = 0, host_reads = 0, host_bases = 0;
    for (int m = 0; m < mates; m++) {
        std::vector<std::pair<uint64_t, uint64_t>> lens[3];  // (length, reads) ascending: input, non-human, human
        for (int c = 0; c < 2; c++) {
            nh_read_class &k = out.cls[c][m];
            k = racc[(size_t)(2 * c + m)];
            if (!k.reads) k.min_len = 0;
            dev_reads += k.reads, dev_bases += k.bases;
            const std::vector<uint64_t> &h = rs.len_hist[c][m];
            for (size_t L = 0; L < h.size(); L++)
                if (h[L]) lens[1 + c].push_back({L, h[L]});
            for (const auto &p : rs.len_long[c][m]) lens[1 + c].push_back(p);
            for (const auto &p : lens[1 + c]) host_reads += p.second, host_bases += p.first * p.second;
        }
        // the input: the union of the two classes (both ascending)
        std::map<uint64_t, uint64_t> all;
        for (int c = 1; c < 3; c++)
            for (const auto &p : lens[c]) all[p.first] += p.second;
        lens[0].assign(all.begin(), all.end());
        for (int set = 0; set < 3; set++) length_summary(lens[set], &out.median_len[set][m], &out.n50[set][m]);
    }
    // (the lengths the writer kept are the checker of what the devices counted, as for the run's counters)
    if (dev_reads != host_reads || dev_bases != host_bases || dev_reads != rs.total * (uint64_t)mates)
        return set_error(NH_EDEVICE, "read statistics: the devices counted %llu reads / %llu bases, the writer %llu / %llu",
                         (unsigned long long)dev_reads, (unsigned long long)dev_bases, (unsigned long long)host_reads,
                         (unsigned long long)host_bases);
    if (r.rs_path)
        if (const int rc = nh_read_stats_write(&out, r.rs_path)) return rc;
    if (r.rs_out) *r.rs_out = out;
    return NH_OK;
}

// minimizer data: the clade sums, checked against the classifier's own count of hit groups, fragment by fragment
static int finish_mdata(const TaxoView &view, const RunState &rs, MdataNumbers &mdn) {
    mdn.v[1] = rs.call_counts;
    mdata_clades(view, mdn);
    uint64_t groups = 0;
    for (uint64_t i = 1; i < view.n; i++) groups += mdn.v[3][i];
    if (groups != rs.hit_groups)
        return set_error(NH_EDEVICE, "minimizer data: the pass counted %llu hit groups, the classifier %llu", (unsigned long long)groups,
                         (unsigned long long)rs.hit_groups);
    return NH_OK;
}
// ... and handed out: the table, the caller's array
static int report_mdata(const TaxoView &view, const MdataNumbers &mdn, nh_minimizer_data *md) {
    if (md->table)
        if (const int rc = write_mdata_table(view, mdn, md->table)) return rc;
    md->n_taxa = view.n > 1 ? (uint32_t)(view.n - 1) : 0;
    for (uint64_t i = 1; md->taxa && i < view.n && i - 1 < md->taxa_cap; i++) {
        nh_taxon_minimizers &o = md->taxa[i - 1];
        o.taxid = view.field(i, 5);
        o.reads_clade = mdn.v[0][i], o.reads_own = mdn.v[1][i], o.minimizers_clade = mdn.v[2][i], o.minimizers_own = mdn.v[3][i];
        o.distinct_clade = mdn.v[4][i], o.distinct_own = mdn.v[5][i], o.db_cells_clade = mdn.v[6][i], o.db_cells_own = mdn.v[7][i];
    }
    return NH_OK;
}

// what run_engines refuses before it touches a device or a file: the arguments, unreadable inputs, an output that is an input
static int check_run_files(const RunRequest &r, const RunState &rs) {
    const nh_run_args *a = r.a;
    if (rs.paired && !a->out2 && a->out_codec != NH_CODEC_BAM) return set_error(NH_EINVAL, "nh_run: paired input needs out2");
    if (!(a->confidence >= 0.0 && a->confidence <= 1.0)) return set_error(NH_EINVAL, "Confidence score must be in the closed interval [0, 1]");
    for (const char *p : {a->in1, a->in2}) {  // fail on unreadable inputs before creating outputs
        if (!p) continue;
        FILE *f = fopen(p, "rb");
        if (!f) return set_error(NH_EIO, "cannot open %s", p);
        fclose(f);
    }
    // outputs are created with O_TRUNC before the first input byte is read: an output that IS an input
    // (same device and inode) would be emptied -- refuse (the CLI host stages its outputs and renames).  Only an output that is
    // there, as a regular file, is looked at; for a plain nh_run this is the only such check.
    const std::vector<RunFile> files = request_files(r, F_COVER);
    size_t inputs = 0;
    while (inputs < files.size() && files[inputs].kind == F_INPUT) inputs++;
    for (size_t c = inputs; c < files.size(); c++) {
        struct stat so;
        if (!files[c].path[0] || stat(files[c].path, &so) != 0 || !S_ISREG(so.st_mode)) continue;
        if (const int rc = check_collision(files, c, inputs)) return rc;
    }
    if (a->out_codec < NH_CODEC_NONE || a->out_codec > NH_CODEC_BAM) return set_error(NH_EINVAL, "nh_run: unknown out_codec %d", a->out_codec);
    return NH_OK;
}

int run_engines(const std::vector<Engine *> &engines, const RunRequest &r, nh_stats *stats) {
    const nh_run_args *a = r.a;
    if (!a || !a->in1 || !a->out1) return set_error(NH_EINVAL, "nh_run: in1 and out1 are required");
    if (const int brc = check_bam_inputs(a)) return brc;
    if (engines.empty()) return set_error(NH_EINVAL, "nh_run: no engine");
    RunShape sh(r, engines.size());
    // the features' tables, and what they ask of the database (it is open: before any input is read or any output created)
    int rc;
    std::vector<uint8_t> bin_of, host_of;  // per node of the taxonomy: the selector's bin, host or not
    if (sh.taxa && (rc = selector_bins(engines[0], r, bin_of))) return rc;
    for (size_t g = 0; sh.mdt && g < engines.size(); g++)
        if ((rc = mdata_check_db(engines[g]))) return rc;
    if (sh.hsel) {
        if ((rc = host_table(engines[0], r.hf, host_of))) return rc;
        r.hf->host_fragments = r.hf->spared_fragments = 0;
    }
    for (size_t g = 0; sh.mark && g < engines.size(); g++)
        if ((rc = cover_check_db(engines[g]))) return rc;
    if (r.rd) r.rd->masked_bases = 0;
    if (sh.cover) r.hi->fragments = r.hi->intervals = r.hi->covered_bases = 0;
    if (sh.hbo) r.hb->host_bases = r.hb->masked_bases = r.hb->closed_bases = 0;
    if (sh.cut) r.hc->host_bases = r.hc->pieces = r.hc->piece_bases = r.hc->cut_bases = r.hc->short_bases = r.hc->dropped_reads = r.hc->closed_bases = 0;
    if (sh.split || sh.lists || sh.taxa || sh.cover)
        for (Engine *e : engines)
            if ((rc = ensure_device_external(e))) return rc;
    RunState rs;
    rs.a = a, rs.engines = engines;
    rs.paired = r.paired;
    rs.want_k = a->kraken_output && a->kraken_output[0] && strcmp(a->kraken_output, "/dev/null") != 0;
    rs.call_counts.assign(engines[0]->external.size(), 0);
    rs.dev_counts.assign(4 * engines.size(), 0);
    if ((rc = check_run_files(r, rs))) return rc;
    RunFiles files;
    if ((rc = open_run_files(files, r, engines, rs.paired && !sh.bamout, rs.want_k))) return rc;
    std::vector<RunBuffers> dbuf((size_t)sh.G);  // per device, for the run
    Pipeline p(sh, rs, files, dbuf, bin_of);
    p.batch_limits();
    sh.set_outputs(a, rs, files);
    auto t0 = std::chrono::steady_clock::now();

    const size_t md_mark_bytes = sh.mdt ? (size_t)mdata_mark_words(engines[0]) * 4 : 0;
    MdataNumbers mdn;  // [3] minimizers_own, [5] distinct_own, [7] db_cells_own, filled at the end of the run
    double md_count_ms = 0;
    std::vector<nh_read_class> racc;  // read statistics: the devices' blocks summed: [class][mate]
    rs.d_run_counters.assign((size_t)sh.G, nullptr);
    for (int g = 0; g < sh.G; g++) {
        if ((rc = alloc_run_buffers(dbuf[g], engines[g], bin_of, host_of, sh.rst, md_mark_bytes, engines[0]->external.size(), sh.mdt, sh.hbo ? 3 : sh.cut ? 3 + CUT_COUNTS : 0))) return rc;
        rs.d_run_counters[g] = dbuf[g].counters;
    }
    if ((rc = p.create_slots())) return rc;
    p.start();
    p.run();
    p.shutdown();

    collect_qmask(p.slots, rs);
    if (sh.dust) collect_dust(p.slots, rs);
    uint64_t dev_host[2] = {0, 0};  // host selection: the devices' {host, spared} fragments summed
    if (sh.hsel) collect_host_counts(dbuf, rs, dev_host);
    if (sh.rst) collect_rstats(dbuf, rs, racc);
    if (sh.hbo) collect_hostbases(dbuf, rs);
    if (sh.cut) collect_hostcut(dbuf, rs);
    if (sh.mdt) collect_mdata(dbuf, rs, md_mark_bytes, mdn, &md_count_ms);
    p.slots.clear();  // (every slot's buffers, events and stream go back here, each under its device)
    if (sh.trace_run)
        print_run_trace(sh, rs, p.clk, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), racc, mdn, md_count_ms, dev_host);
    if (rs.err_code != NH_OK) return set_error(rs.err_code, "%s", rs.err_msg.c_str());
    if (dev_debug()) {  // NOHUMAN_DEBUG_DEVICE: a launch, copy or allocation under the wrong device fails the run that met it
        const std::string v = dev_violation(true);
        if (!v.empty()) return set_error(NH_EDEVICE, "device discipline: %s", v.c_str());
    }
    rc = reduce_run_counters(rs);
    dbuf.clear();  // (the run's device buffers go back before the reports are written)
    if (rc) return rc;

    const TaxoView mdview = taxo_view(engines[0]);
    if (sh.mdt && (rc = finish_mdata(mdview, rs, mdn))) return rc;
    const std::vector<uint64_t> md_report[2] = {mdn.v[2], mdn.v[4]};
    if (a->report && a->report[0] &&
        (rc = write_report(engines[0], a->report, rs.call_counts, rs.total, rs.total - rs.classified, sh.mdt && r.md->in_report ? md_report : nullptr)))
        return rc;
    if ((rc = close_run_files(files, sh, rs))) return rc;
    if (sh.rst && (rc = finish_read_stats(r, rs, sh.mates, racc))) return rc;
    for (int k = 0; k < sh.K; k++) r.touts[k].fragments = rs.taxon_frags[k];
    if (sh.hsel) r.hf->host_fragments = rs.host_frags, r.hf->spared_fragments = rs.spared_frags;
    if (sh.dust) r.rd->masked_bases = rs.dust_masked;
    if (sh.cover) r.hi->fragments = rs.cover_frags, r.hi->intervals = rs.cover_ivls, r.hi->covered_bases = rs.cover_bases;
    if (sh.hbo) r.hb->host_bases = rs.hb_bases[0], r.hb->masked_bases = rs.hb_bases[1], r.hb->closed_bases = rs.hb_bases[2];
    if (sh.cut) {
        const uint64_t *c = rs.cut_counts;
        r.hc->host_bases = c[CUT_HOST_BASES], r.hc->pieces = c[CUT_PIECES], r.hc->piece_bases = c[CUT_PIECE_BASES], r.hc->cut_bases = c[CUT_CUT_BASES];
        r.hc->short_bases = c[CUT_SHORT_BASES], r.hc->dropped_reads = c[CUT_DROPPED], r.hc->closed_bases = rs.hb_bases[2];
    }
    if (sh.mdt && (rc = report_mdata(mdview, mdn, r.md))) return rc;
    if (stats) {
        nh_stats st;
        memset(&st, 0, sizeof st);
        st.total_sequences = rs.total, st.classified = rs.classified, st.unclassified = rs.total - rs.classified;
        st.total_bases = rs.total_bases;
        st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *stats = st;
    }
    return NH_OK;
}

int run_engine(Engine *e, const RunRequest &r, nh_stats *stats) {
    std::vector<Engine *> v{e};
    return run_engines(v, r, stats);
}

}  // namespace nh

extern "C" {

// an engine entry: the request's own checks (before any device is touched), then the run on the caller's engine
static int run_on_engine(nh_engine *e, const nh::RunRequest &r, nh_stats *stats) {
    if (const int rc = nh::check_request(r)) return rc;
    if (!e) return nh::set_error(NH_EINVAL, "null engine");
    return nh::run_engine((nh::Engine *)e, r, stats);
}

int nh_run_engine(nh_engine *e, const nh_run_args *args, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::RUN, args, nullptr), stats);
}

int nh_run_engine_split(nh_engine *e, const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::SPLIT, args, nullptr, human_out1, human_out2), stats);
}

int nh_run_engine_mask(nh_engine *e, const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::MASK, args, nullptr, human_out1, human_out2), stats);
}

int nh_run_engine_ex(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::EX, args, extras), stats);
}

int nh_run_engine_minq(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality), stats);
}

int nh_run_engine_rstats(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                         const char *read_stats_path, nh_read_stats *out, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, out), stats);
}

int nh_run_engine_taxa(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs),
                         stats);
}

int nh_run_engine_mdata(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                        const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                        nh_stats *stats) {
    return run_on_engine(e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md),
                         stats);
}

// (without a selection -- hf NULL, or no taxid in it -- the request is nh_run_engine_mdata's: make_request drops such an hf)
int nh_run_engine_host(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                       nh_host_filter *hf, nh_stats *stats) {
    return run_on_engine(
        e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf), stats);
}

// (rd NULL, or its enable 0: the request is nh_run_engine_host's)
int nh_run_engine_dust(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                       nh_host_filter *hf, nh_read_dust *rd, nh_stats *stats) {
    return run_on_engine(
        e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd),
        stats);
}

// (hi NULL, or its path NULL: the request is nh_run_engine_dust's)
int nh_run_engine_intervals(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                            const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                            nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_stats *stats) {
    return run_on_engine(
        e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi),
        stats);
}

// (hb NULL, or its enable 0: the request is nh_run_engine_intervals')
int nh_run_engine_hostbases(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                            const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                            nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb, nh_stats *stats) {
    return run_on_engine(
        e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi, hb),
        stats);
}

// (hc NULL, or its enable 0: the request is nh_run_engine_hostbases')
int nh_run_engine_hostcut(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                          const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md,
                          nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb, nh_host_cut *hc, nh_stats *stats) {
    return run_on_engine(
        e, nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi, hb, hc),
        stats);
}

int nh_fastx_scan(const char *path, uint64_t *n_records, uint64_t *n_bases, uint64_t *digest) {
    if (!path || !n_records || !n_bases || !digest) return nh::set_error(NH_EINVAL, "null argument");
    nh::BlockReader r;
    std::string err;
    if (r.open(path, err) != 0) return nh::set_error(NH_EIO, "%s", err.c_str());
    uint64_t n = 0, nb = 0, h = 0xcbf29ce484222325ull;
    auto mix = [&](const char *p, size_t len) {
        for (size_t i = 0; i < len; i++) h = (h ^ (unsigned char)p[i]) * 0x100000001b3ull;
        h = (h ^ 0) * 0x100000001b3ull;
    };
    size_t scan_batch = 4096;
    if (const char *env = getenv("NOHUMAN_SCAN_BATCH")) {  // test knob
        const long v = atol(env);
        if (v > 0) scan_batch = (size_t)v;
    }
    nh::HalfBatch hb;
    for (;;) {
        r.next_batch(hb, scan_batch, 64u << 20);
        if (!hb.error.empty()) return nh::set_error(NH_EIO, "%s", hb.error.c_str());
        for (const nh::RecRef &x : hb.recs) {
            n++;
            nb += x.slen;
            mix(hb.text.data() + x.h, x.hlen);
            mix(hb.text.data() + x.s, x.slen);
            mix(hb.text.data() + x.q, x.qlen);
        }
        if (hb.eof) break;
    }
    *n_records = n;
    *n_bases = nb;
    *digest = h;
    return NH_OK;
}

// Test hook (not part of the ABI in include/nohuman_engine.h, like nh_debug_sched): one reader driven alone -- no engine, no
// classification, no outputs -- and what it handed out, record by record.  reader 0: the host's BlockReader; 1: DevFastqReader
// on `device`; 2: BamReader on `device` (the batches' bytes are copied back from HalfBatch::dev_text; every batch is released); 3 and 4: the
// paired BamReader's halves of mate 1 and of mate 2 (both halves of every batch are made and released, one is reported).  next_batch() is called
// until the reader reports the end of the input, hands the file over to the host reader (reported, not followed) or fails.
//   recs     NH_DUMP_REC_WORDS words a record, in input order: hlen, idlen, slen, qlen, canonical (raw_end != 0), raw length
//            (raw_end - h), index of its batch, digest of header / sequence / qualities (mixed like nh_fastx_scan, from the
//            start value for every record), digest of text[h, raw_end) for a canonical record (else 0)
//   batches  two words a batch: records, bytes of text
//   pieces   reader 1: where each piece's body begins in the inflated stream
//   end      0: end of the input, 1: handover (msg: handover_reason()), 2: error (msg: its text)
// NH_EINVAL when one of the tables is too small (n_recs / n_batches / n_pieces say what it takes).
enum { NH_DUMP_REC_WORDS = 9 };
int nh_debug_reader_dump(const char *path, int reader, int device, uint64_t batch_recs, uint64_t max_text, uint64_t *recs, uint64_t rec_cap,
                         uint64_t *n_recs, uint64_t *batches, uint64_t batch_cap, uint64_t *n_batches, uint64_t *pieces, uint64_t piece_cap,
                         uint64_t *n_pieces, int *end, char *msg, uint64_t msg_cap) {
    if (!path || !recs || !n_recs || !batches || !n_batches || !pieces || !n_pieces || !end || !msg || !msg_cap || !batch_recs || reader < 0 || reader > 4)
        return nh::set_error(NH_EINVAL, "nh_debug_reader_dump: bad argument");
    auto fnv = [](const uint8_t *p, size_t len, uint64_t h) {
        for (size_t i = 0; i < len; i++) h = (h ^ p[i]) * 0x100000001b3ull;
        return h * 0x100000001b3ull;
    };
    uint64_t nr = 0, nb = 0;
    std::vector<uint8_t> host;  // a device batch's bytes
    std::string text;           // msg
    bool short_text = false;
    auto take = [&](nh::HalfBatch &hb) -> bool {  // false: the batch's bytes could not be had
        const uint8_t *t = (const uint8_t *)hb.text.data();
        const size_t len = hb.text.size();
        if (hb.dev_text) {
            host.resize(len + 1);
            if (len && hipMemcpy(host.data(), hb.dev_text, len, hipMemcpyDeviceToHost) != hipSuccess) return false;
            t = host.data();
        }
        if (nb < batch_cap) {
            batches[2 * nb] = hb.recs.size();
            batches[2 * nb + 1] = len;
        }
        for (const nh::RecRef &x : hb.recs) {
            if ((size_t)x.h + x.hlen > len || (size_t)x.s + x.slen > len || (size_t)x.q + x.qlen > len || x.raw_end > len || (x.raw_end && x.raw_end < x.h))
                short_text = true;  // (an offset beyond the batch's text: reported, never read)
            else if (nr < rec_cap) {
                uint64_t *o = recs + NH_DUMP_REC_WORDS * nr;
                o[0] = x.hlen, o[1] = x.idlen, o[2] = x.slen, o[3] = x.qlen, o[4] = x.raw_end != 0, o[5] = x.raw_end ? x.raw_end - x.h : 0, o[6] = nb;
                o[7] = fnv(t + x.q, x.qlen, fnv(t + x.s, x.slen, fnv(t + x.h, x.hlen, 0xcbf29ce484222325ull)));
                o[8] = x.raw_end ? fnv(t + x.h, x.raw_end - x.h, 0xcbf29ce484222325ull) : 0;
            }
            nr++;
        }
        nb++;
        return true;
    };
    *end = 0;
    *n_pieces = 0;
    std::string err;
    nh::HalfBatch hb;
    if (reader == 0) {
        nh::BlockReader r;
        if (r.open(path, err) != 0) return nh::set_error(NH_EIO, "%s", err.c_str());
        for (;;) {
            r.next_batch(hb, (size_t)batch_recs, max_text ? (size_t)max_text : (size_t)3u << 30);
            if (!hb.error.empty()) {
                *end = 2;
                text = hb.error;
                break;
            }
            if (!hb.recs.empty() || !hb.eof) (void)take(hb);
            if (hb.eof) break;
        }
    } else if (reader == 3 || reader == 4) {
        nh::BamReader br;
        nh::HalfBatch other;
        if (!nh::bam_paired(path)) return nh::set_error(NH_EINVAL, "nh_debug_reader_dump: %s is no paired BAM file", path);
        if (br.open(path, &device, 1, err, 1) != 0) return nh::set_error(NH_EIO, "%s", err.c_str());
        nh::HalfBatch &mine = hb, &h1 = reader == 3 ? hb : other, &h2 = reader == 3 ? other : hb;
        for (;;) {
            br.next_batch(h1, h2, (size_t)batch_recs, (size_t)max_text);
            if (!mine.error.empty()) {
                *end = 2;
                text = mine.error;
                break;
            }
            const bool same = h1.recs.size() == h2.recs.size() && h1.eof == h2.eof;
            if (!same || ((!mine.recs.empty() || !mine.eof) && !take(mine))) {
                h1.reset();
                h2.reset();
                br.close();
                return nh::set_error(NH_EDEVICE, same ? "nh_debug_reader_dump: a batch's text could not be copied back"
                                                      : "nh_debug_reader_dump: the two halves of a paired batch differ in their records");
            }
            const bool eof = mine.eof;
            h1.reset();  // (the set is free when BOTH halves have been released: close() waits for that)
            h2.reset();
            if (eof) break;
        }
        h1.reset();
        h2.reset();
        br.close();
    } else if (reader == 2) {
        nh::BamReader br;
        if (!nh::bam_wants(path)) return nh::set_error(NH_EINVAL, "nh_debug_reader_dump: %s is no BAM file", path);
        if (br.open(path, &device, 1, err, 1) != 0) return nh::set_error(NH_EIO, "%s", err.c_str());
        for (;;) {
            br.next_batch(hb, (size_t)batch_recs, (size_t)max_text);
            if (!hb.error.empty()) {
                *end = 2;
                text = hb.error;
                break;
            }
            if ((!hb.recs.empty() || !hb.eof) && !take(hb)) {
                hb.reset();
                br.close();
                return nh::set_error(NH_EDEVICE, "nh_debug_reader_dump: a batch's text could not be copied back");
            }
            const bool eof = hb.eof;
            hb.reset();  // (releases the batch: the reader's close() waits for every batch it handed out)
            if (eof) break;
        }
        hb.reset();
        br.close();
    } else {
        nh::DevFastqReader dr;
        const int orc = dr.open(path, device, err);
        if (orc != 0) return nh::set_error(NH_EIO, "nh_debug_reader_dump: the reader on the GPU does not take the file (%s)", err.c_str());
        for (;;) {
            const int rc = dr.next_batch(hb, (size_t)batch_recs, (size_t)max_text);
            if (rc == 1) {
                *end = 1;
                text = dr.handover_reason();
                break;
            }
            if (!hb.error.empty()) {
                *end = 2;
                text = hb.error;
                break;
            }
            if ((!hb.recs.empty() || !hb.eof) && !take(hb)) {
                hb.reset();
                dr.close();
                return nh::set_error(NH_EDEVICE, "nh_debug_reader_dump: a batch's text could not be copied back");
            }
            const bool eof = hb.eof;
            hb.reset();  // (releases the batch: the reader's close() waits for every batch it handed out)
            if (eof) break;
        }
        hb.reset();
        dr.close();  // (joins the decode stage: the list of pieces is final)
        const std::vector<uint64_t> ps = dr.piece_starts();
        *n_pieces = ps.size();
        for (size_t i = 0; i < ps.size() && i < piece_cap; i++) pieces[i] = ps[i];
    }
    *n_recs = nr;
    *n_batches = nb;
    snprintf(msg, (size_t)msg_cap, "%s", text.c_str());
    if (short_text) return nh::set_error(NH_EIO, "nh_debug_reader_dump: a record's offsets lie beyond its batch's text");
    if (nr > rec_cap || nb > batch_cap || *n_pieces > piece_cap || text.size() >= msg_cap)
        return nh::set_error(NH_EINVAL, "nh_debug_reader_dump: a table is too small");
    return NH_OK;
}

// Whole run on one or several devices: the database is loaded into every device's HBM, batches go
// round-robin, outputs stay in input order, the counts are summed on the host.
static int run_devices(const nh::RunRequest &r, nh_stats *stats) {
    const nh_run_args *args = r.a;
    if (!args || !args->db_dir) return nh::set_error(NH_EINVAL, "nh_run: db_dir is required");
    if (const int brc = nh::check_bam_inputs(args)) return brc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return nh::set_error(NH_EDEVICE, "no HIP device available");
    ndev = nh::dev_count();
    std::vector<int> devs;
    if (args->device_ids && args->n_devices > 0)
        devs.assign(args->device_ids, args->device_ids + args->n_devices);
    else
        for (int i = 0; i < (args->n_devices > 0 ? args->n_devices : ndev); i++) devs.push_back(i);
    // one replica of the database per device, loaded at the same time (each device has its own PCIe
    // link; the file comes from the page cache after the first reader)
    const bool trace = getenv("NOHUMAN_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    std::vector<nh::Engine *> opened(devs.size(), nullptr);
    std::vector<int> rcs(devs.size(), NH_OK);
    std::vector<std::string> errs(devs.size());
    {
        std::vector<std::thread> loaders;
        for (size_t i = 0; i < devs.size(); i++)
            loaders.emplace_back([&, i] {
                rcs[i] = nh::open_dir(args->db_dir, devs[i], &opened[i]);
                if (rcs[i]) errs[i] = nh::g_last_error;  // thread-local: carry it over
            });
        for (auto &t : loaders) t.join();
    }
    std::vector<nh::Engine *> engines;
    int rc = NH_OK;
    for (size_t i = 0; i < devs.size(); i++) {
        if (opened[i]) engines.push_back(opened[i]);
        if (rcs[i] && !rc) rc = nh::set_error(rcs[i], "%s", errs[i].c_str());
    }
    const double t_load = since(t_begin);
    const auto t_run = std::chrono::steady_clock::now();
    if (!rc) rc = nh::run_engines(engines, r, stats);
    const double s_run = since(t_run);
    std::string keep = nh::g_last_error;
    const auto t_close = std::chrono::steady_clock::now();
    for (nh::Engine *e : engines) nh::destroy(e);
    if (trace)
        fprintf(stderr, "[nohuman trace] nh_run: database into HBM %.3f s, the run %.3f s, closing (HBM and page-locked buffers given back) %.3f s\n", t_load,
                s_run, since(t_close));
    if (rc) nh::g_last_error = keep;
    return rc;
}

// a standalone entry: the request's own checks (before any device is touched), then the run on the devices it names
static int run_standalone(const nh::RunRequest &r, nh_stats *stats) {
    if (const int rc = nh::check_request(r)) return rc;
    return run_devices(r, stats);
}

int nh_run(const nh_run_args *args, nh_stats *stats) { return run_standalone(nh::make_request(nh::RunRequest::RUN, args, nullptr), stats); }

int nh_run_split(const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::SPLIT, args, nullptr, human_out1, human_out2), stats);
}

int nh_run_mask(const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::MASK, args, nullptr, human_out1, human_out2), stats);
}

int nh_run_ex(const nh_run_args *args, const nh_run_extras *extras, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::EX, args, extras), stats);
}

int nh_run_minq(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality), stats);
}

int nh_run_rstats(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                  nh_read_stats *out, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, out), stats);
}

int nh_run_taxa(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs),
                          stats);
}

int nh_run_mdata(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                 nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_stats *stats) {
    return run_standalone(nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md),
                          stats);
}

// (without a selection -- hf NULL, or no taxid in it -- the request is nh_run_mdata's: make_request drops such an hf)
int nh_run_host(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf, nh_stats *stats) {
    return run_standalone(
        nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf), stats);
}

// (rd NULL, or its enable 0: the request is nh_run_host's)
int nh_run_dust(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd,
                nh_stats *stats) {
    return run_standalone(
        nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd),
        stats);
}

// (hi NULL, or its path NULL: the request is nh_run_dust's)
int nh_run_intervals(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                     nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd,
                     nh_host_intervals *hi, nh_stats *stats) {
    return run_standalone(
        nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi),
        stats);
}

// (hb NULL, or its enable 0: the request is nh_run_intervals')
int nh_run_hostbases(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                     nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd,
                     nh_host_intervals *hi, nh_host_bases *hb, nh_stats *stats) {
    return run_standalone(
        nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi, hb),
        stats);
}

// (hc NULL, or its enable 0: the request is nh_run_hostbases')
int nh_run_hostcut(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                   nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd,
                   nh_host_intervals *hi, nh_host_bases *hb, nh_host_cut *hc, nh_stats *stats) {
    return run_standalone(
        nh::make_request(nh::RunRequest::RUN, args, extras, nullptr, nullptr, min_base_quality, read_stats_path, read_stats, outs, n_outs, md, hf, rd, hi, hb, hc),
        stats);
}

}  // extern "C"
