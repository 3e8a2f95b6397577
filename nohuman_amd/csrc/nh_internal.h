// nh_internal.h -- host-side engine state shared by nh_engine.hip and nh_run.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "nh_device.h"
#include "nohuman_engine.h"

namespace nh {
constexpr unsigned LAUNCH_SLOTS = 16;  // launches of one engine that may be in flight at once
constexpr uint64_t DEFER_WORDS = 1u << 15;  // 1 Mi chunks per launch (24 M pairs); larger launches skip the short-read kernel
// kraken2's default masks: what the builder writes, and what the passes that scan at the default geometry ask of a database
constexpr uint64_t TOGGLE_MASK = 0xe37e28c4271b5a2dull;
constexpr uint64_t SPACED_MASK = 0x3FFFFFFFF3333333ull;  // "1" x 17 + "01" x 7, two bits a base

// blocks of `kernel` (`threads` a block, no dynamic LDS) that a CU holds, `fallback` where the runtime does not say: a launcher
// asks once and keeps the answer in a static
template <class Kernel>
int blocks_per_cu(Kernel kernel, int threads, int fallback) {
    int v = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, threads, 0) == hipSuccess && v > 0 ? v : fallback;
}
}

namespace nh {

struct Staging {  // grow-only device buffers behind nh_classify_batch (host-buffer entry)
    void *d_bases = nullptr, *d_offsets = nullptr, *d_results = nullptr, *d_taxa = nullptr,
         *d_taxa_off = nullptr;
    size_t cap_bases = 0, cap_offsets = 0, cap_results = 0, cap_taxa = 0, cap_taxa_off = 0;
};

// Tuning / test knobs of a launch, read from the environment ONCE, when the engine is opened (round 6; rounds 1-5 called
// getenv at every launch): NOHUMAN_FRAG_CHUNK (fragments a wave claims at a time), NOHUMAN_SEG_CAP (segments a long-read
// launch may cut), NOHUMAN_SCHED (claim map: "off" or c1,c2,p1,p2).  nh_debug_reload_knobs (a test hook like
// nh_debug_sched, not part of the ABI) reads them again for the sweeps of tools/.
struct LaunchKnobs {
    uint32_t frag_chunk = 0;  // 0: the default for the launch's shape
    uint64_t seg_cap = 0;     // 0: 8 segments per read, 2^16 .. 2^20
    SchedKnobs sched;
};
LaunchKnobs read_launch_knobs();
SchedKnobs parse_sched_knobs(const char *env);  // NOHUMAN_SCHED's grammar (nh_kernels.hip, beside make_sched)

// What nh_open* found when it read every cell of the table once (k_validate_table): a cell's value indexes the taxonomy
// in every kernel, so a value >= node_count (a hash.k2d beside another database's taxo.k2d) is refused with NH_EDB
// instead of faulting on the GPU; so is a table whose non-empty cells are not the `size` its header states.
struct TableCheck {
    uint64_t non_empty = 0, max_value = 0;
    double seconds = 0;
};

struct Engine {
    int device = -1;
    int n_cu = 0;
    int grid_blocks = 0;
    nh_db_info info{};
    nh_options options{};
    DevDB dev{};
    void *d_table_raw = nullptr;    // one allocation: n_copies staggered copies of the table (DevDB::copy_stride)
    uint32_t *d_table = nullptr;    // copy 0, 128-byte aligned
    uint32_t n_copies = 1;
    uint64_t copy_stride = 0;       // cells
    uint64_t table_cells_alloc = 0; // cells of one copy incl. padding
    uint32_t *d_parent = nullptr;
    uint64_t *d_counters = nullptr;
    int *d_error = nullptr;
    unsigned long long *d_work = nullptr;  // work counters of k_classify: WORK_WORDS per launch slot (nh_device.h)
    unsigned long long *d_cshard = nullptr; // counter rows the waves of a launch add to, COUNTER_SHARDS per launch slot
    uint32_t *d_defer = nullptr;           // per launch slot DEFER_WORDS words: chunks the short-read kernel left behind
    // long-read item buffers per launch slot (SplitBufs, nh_device.h), allocated when a slot first carries a
    // launch of long single-end reads and grown when a larger one comes
    SplitBufs split[LAUNCH_SLOTS] = {};
    uint64_t split_single_cap[LAUNCH_SLOTS] = {};
    bool split_fresh[LAUNCH_SLOTS] = {};  // buffers allocated, header not yet cleared (the first launch does it)
    std::mutex split_mu;
    std::atomic<unsigned> launch_seq{0};
    // A launch slot is used by one launch at a time: the launch that takes a slot waits (on the device, hipStreamWaitEvent)
    // for the event the slot's previous launch recorded behind its k_finish_launch.  With at most LAUNCH_SLOTS launches
    // in flight -- what every caller in this repo does -- the event has long fired; more than that are ORDERED, not
    // undefined (rounds 1-5 documented "not supported" and nothing detected it).  slot_mu orders the hosts' enqueues.
    hipEvent_t slot_ev[LAUNCH_SLOTS] = {};
    bool slot_used[LAUNCH_SLOTS] = {};
    std::mutex slot_mu[LAUNCH_SLOTS];
    LaunchKnobs knobs;
    TableCheck check;
    hipStream_t stream = nullptr;
    std::vector<uint32_t> parent;
    std::vector<uint64_t> external;
    uint64_t *d_external = nullptr;  // `external` in HBM (the classified-out builder, nh_split.hip): made by a run that needs it
    std::vector<uint8_t> taxo_image, opts_image;
    Staging st;
    std::mutex mu;
    std::mutex db_mu;  // options / DevDB parameter block (set from one thread, read by launches on others)
    double seconds = 0;
};

extern thread_local std::string g_last_error;
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

hipError_t launch_classify(const DevDB &db, const LaunchIO &io, double confidence, const LaunchSlot &sl,
                           uint32_t frag_chunk, int grid_blocks, hipStream_t stream, const SchedKnobs &sched_knobs);
Sched make_sched(uint64_t n_frag, uint32_t c0, int mates, uint64_t waves, const SchedKnobs &kn);
hipError_t launch_validate_table(const uint32_t *table, uint64_t n_cells, uint32_t vmask, unsigned long long *d_out2,
                                 hipStream_t stream);
int classify_blocks_per_cu();
hipError_t launch_insert_sequences(const DevDB &db, const void *d_bases, const void *d_seq_off,
                                   uint64_t n_seq, uint32_t value, unsigned long long *d_inserted,
                                   int grid_blocks, hipStream_t stream);
hipError_t launch_synth_insert(uint32_t *table, uint64_t capacity, uint64_t cap_magic,
                               uint32_t value_bits, uint32_t value, uint64_t n_keys, uint64_t seed,
                               uint64_t key_mask, unsigned long long *d_size, hipStream_t stream);

int check_device(int device);  // NH_OK, or NH_EDEVICE with a message: no HIP device, `device` out of range, not a gfx950
int open_dir(const char *db_dir, int device, Engine **out);
int open_images(const void *opts, size_t opts_len, const void *taxo, size_t taxo_len,
                const void *hash, size_t hash_len, int device, Engine **out);
int open_synthetic(uint64_t capacity, uint64_t n_keys, uint32_t depth, uint64_t seed, int device,
                   Engine **out);
void destroy(Engine *e);
void finish_devdb_public(Engine *e);
DevDB devdb_now(Engine *e);  // the parameter block of a launch made now, taken under db_mu: options may be set from another thread
int refresh_table_copies(Engine *e);  // after the cells of copy 0 changed (load, inserts): device-wide sync + re-copy
int resolve_db_dir(const char *db_dir, std::string &resolved);
int classify_device(Engine *e, const void *d_bases, const void *d_seq_off, uint64_t n_frag,
                    uint32_t flags, double confidence, void *d_results, void *d_kmer_taxa,
                    const void *d_kmer_taxa_off, void *d_counters, hipStream_t stream,
                    const void *d_seq_len = nullptr, uint64_t bases_end = 0);
int classify_host(Engine *e, const uint8_t *bases, const uint64_t *seq_offsets, uint64_t n_frag,
                  uint32_t flags, double confidence, nh_result *results, uint32_t *kmer_taxa,
                  uint64_t *kmer_taxa_offsets, uint64_t kmer_taxa_cap);
int check_error_flag(Engine *e);
// The classified-out records of one batch built in HBM (nh_split.hip; nh_run_split's human outputs): both mates' text as
// the classifier sees it, out[m] receives mate m's records of the fragments with call != 0, total[m] their bytes.
struct HumanOutArgs {
    const char *text;         // the batch's text (d_text), ntext bytes
    uint64_t ntext;
    const uint64_t *seq_off;  // n * mates sequence starts (absolute), as classified
    const uint32_t *seq_len;  // n * mates sequence lengths
    const uint32_t *rec;      // n * mates {header start (absolute), header length, qualities start (absolute), length}
    const nh_result *res;     // n results
    const uint64_t *ext;      // internal -> external taxon id, n_ext entries
    uint64_t n_ext, n, nblk;  // nblk = human_out_blocks(n)
    int mates;
    int fastq[2];             // per mate: FASTQ (else FASTA)
    char *out[2];
    uint64_t cap[2];          // bytes of out[m]
    uint64_t *blk;            // 2 * nblk words of scratch
    uint64_t *total;          // 2 words
    int *error;               // the engine's sticky error word (bit 4: a record outside its text or buffer)
};
uint64_t human_out_blocks(uint64_t n);
hipError_t launch_human_out(const HumanOutArgs &a, hipStream_t stream);
// The same records sorted into K bins by the taxon of the call (nh_split.hip, k_tout_*; nh_run_taxa's per-taxon outputs): out[m]
// is mate m's ONE buffer, bin k of it the region [start[m * K + k], + total[m * K + k]), every start a multiple of 256; a fragment
// whose call has bin_of 0xFF is written nowhere.  Records in input order inside each bin.
struct TaxonOutArgs : HumanOutArgs {  // blk: 2 * K * nblk words of scratch; total: 2 * K words
    const uint8_t *bin_of;    // n_ext bytes: internal taxon id -> bin, 0xFF = none
    int K;                    // bins, 1 .. NH_MAX_TAXON_OUTS
    uint64_t *start;          // 2 * K words; error: bit 64 (a record outside its text or buffer, a bin index >= K)
};
hipError_t launch_taxon_out(const TaxonOutArgs &a, hipStream_t stream);
// The masked records of one batch built in HBM (nh_mask.hip; nh_run_mask's outputs): out[m] receives mate m's record of every
// fragment, in order, the sequence of a classified fragment as 'N'; total[m] their bytes.
struct MaskArgs {
    const char *text;         // the batch's text (d_text), ntext bytes
    uint64_t ntext;
    const uint64_t *seq_off;  // n * mates sequence starts (absolute), as classified
    const uint32_t *seq_len;  // n * mates sequence lengths
    const uint32_t *rec;      // n * mates {header start (absolute), header length, qualities start (absolute), length}
    const nh_result *res;     // n results
    uint64_t n, nblk;         // nblk = mask_blocks(n)
    int mates;
    int fastq[2];             // per mate: FASTQ (else FASTA)
    char *out[2];
    uint64_t cap[2];          // bytes of out[m]
    uint64_t *blk;            // 2 * nblk words of scratch
    uint32_t *fast;           // 2 * nblk words of scratch
    uint64_t *total;          // 4 words: [m] the bytes of mate m's output, [2 + m] how many of its blocks are FAST
    int *error;               // the engine's sticky error word (bit 8: a record outside its text or buffer)
    // --host-bases-only (NULL: the whole sequence of a classified fragment is 'N', as ever): the batch's cover bitmap after the
    // closing, one bit a byte of the text (nh_cover.hip) -- a classified fragment's base is 'N' where its bit is set and the text's
    // own byte elsewhere; hb: two counters the waves add to, the sequence bases of the classified fragments and those written as 'N'
    const uint32_t *cover;
    unsigned long long *hb;
};
uint64_t mask_blocks(uint64_t n);
hipError_t launch_mask(const MaskArgs &a, hipStream_t stream);
// The read lists of one batch built in HBM (nh_calls.hip; nh_run_ex's calls table and human ids): out[0] receives a table line
// for every fragment, out[1] the id of every fragment with call != 0; total[o] their bytes, total[2 + o] their lines.
struct CallsArgs {
    const char *text;         // the batch's text (d_text), ntext bytes
    uint64_t ntext;
    const uint32_t *seq_len;  // n * mates sequence lengths, as classified
    const uint32_t *rec;      // n * mates {header start (absolute), header length, qualities start (absolute), length}
    const uint32_t *idlen;    // n: the length of mate 1's id (RecRef::idlen)
    const nh_result *res;     // n results
    const nh_result *res_ids; // NULL (= res), or the n results whose call != 0 decides the id list (a host selection: nh_host.hip)
    const uint64_t *ext;      // internal -> external taxon id, n_ext entries
    uint64_t n_ext, n, nblk;  // nblk = calls_blocks(n)
    int mates;
    int want[2];              // per output: asked for (an output that is not builds nothing: total 0)
    char *out[2];
    uint64_t cap[2];          // bytes of out[o]
    uint64_t *blk;            // 4 * nblk words of scratch
    uint64_t *total;          // 4 words
    int *error;               // the engine's sticky error word (bit 16: a record outside its text or buffer)
};
uint64_t calls_blocks(uint64_t n);
hipError_t launch_calls(const CallsArgs &a, hipStream_t stream);
// Where the sequences of one batch and their quality lines lie (nh_qseq.h): what the kernels that walk both take.
struct QSeqSrc {
    const char *text;         // the batch's text (d_text), ntext bytes, readable for 8 more
    uint64_t ntext;
    const uint64_t *seq_off;  // n sequence starts (absolute), as classified
    const uint32_t *seq_len;  // n sequence lengths
    const uint64_t *qual_off; // rec == NULL: n quality starts (absolute); all-ones: the sequence has no qualities
    const uint32_t *rec;      // or the run's record table: n * {header start, header length, qualities start (absolute), length}
    uint64_t n;               // sequences (a paired run: 2 a fragment, mate m at odd / even entries)
    int mates;                // rec: 1 or 2
    int fastq[2];             // rec: per mate, FASTQ (else FASTA: no qualities)
};
// The quality-masked bases of one batch (nh_qmask.hip; kraken2's --minimum-base-quality): out, a buffer with the layout of the
// text, receives for every sequence its bases with 'N' where the quality byte is below thresh (a sequence without qualities is
// copied); no other byte of out is written.  The classifier is then launched in place on out with the same seq_off / seq_len.
struct QmaskArgs : QSeqSrc {
    uint32_t thresh;          // Q + 33: a quality byte below it masks its base
    char *out;                // ntext + 8 bytes
    unsigned long long *masked;  // NULL or one counter the waves add their masked bases to
    int *error;               // the engine's sticky error word (bit 32: a quality line not as long as its sequence, a range outside the text)
};
hipError_t launch_qmask(const QmaskArgs &a, hipStream_t stream);
// The read statistics of one batch (nh_rstats.hip; nh_run_rstats): every sequence adds its counts to acc[2 * class + mate], class
// 1 where its fragment's call is not 0 (res[i / mates]), mate i % mates.  A record that fails the checks of the quality mask is
// not counted and sets the same error bit.
struct RstatsArgs : QSeqSrc {
    const nh_result *res;     // n / mates results
    unsigned long long *acc;  // 4 nh_read_class the workgroups add to (min_len: atomic minimum)
    int *error;               // the engine's sticky error word (bit 32, as the quality mask)
};
// max_workgroups 0: as many as an n_cu-CU device holds at once
hipError_t launch_rstats(const RstatsArgs &a, int n_cu, uint32_t max_workgroups, hipStream_t stream);
// median and N50 of a set of read lengths given as (length, reads) in ascending order of length (nh_rstats.hip, host)
void length_summary(const std::vector<std::pair<uint64_t, uint64_t>> &lens, uint64_t *median, uint64_t *n50);
// Minimizer data (nh_mdata.hip; nh_run_mdata): k_mdata_mark behind the classifier sets, for every hit group of the batch, the bit of
// the cell where the key was found in d_marks (mdata_mark_words() uint32) and adds the group to d_groups[value] (node_count
// uint64); k_mdata_count adds the marked cells (d_marks NULL: all cells) per value to d_counts (node_count uint64).
int mdata_check_db(const Engine *e);  // NH_OK, NH_EDB (a geometry the pass does not support: the field named) or NH_EINVAL (linear_probing 0)
uint64_t mdata_mark_words(const Engine *e);
hipError_t launch_mdata_mark(Engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens, uint64_t n_frag,
                             int mates, void *d_marks, void *d_groups, hipStream_t stream);
hipError_t launch_mdata_count(Engine *e, const void *d_marks, void *d_counts, hipStream_t stream);
// The host selection (nh_host.hip; nh_run_host): the selection's own checks (NH_EINVAL, no device needed); host_of, one byte per
// node of the engine's taxonomy, 1 where the deepest listed ancestor-or-self is a host taxid (NH_EINVAL: a taxid the taxonomy does
// not hold); k_host_filter: out[i] = in[i] with call = 0 where host_of[call] is 0 (out == in allowed), counts (NULL or two words:
// host, spared) added to, error: the engine's sticky error word (bit 128: a call >= n_nodes, written as 0, never an index).
bool host_filter_given(const nh_host_filter *hf);  // not NULL and a taxid listed (or a struct too small to say: refused by the check)
int check_host_filter(const nh_host_filter *hf);
int host_table(const Engine *e, const nh_host_filter *hf, std::vector<uint8_t> &host_of);
hipError_t launch_host_filter(const void *d_in, void *d_out, uint64_t n, const uint8_t *d_host_of, uint64_t n_nodes, unsigned long long *d_counts,
                              int *d_error, hipStream_t stream);
// Host intervals (nh_cover.hip; nh_run_intervals): k_cover_mark behind the classifier ORs the bases that host k-mers cover into
// `cover`, one bit a byte of the text (cover_words() uint32, zeroed by the caller); k_cover_ivl_* turn the bitmap into records
// {seq, start, end}; k_cover_line_* the records into BED lines.  The engine's sticky error word: NH_ERR_COVER, a sequence (or a
// record's header) outside the text, skipped; NH_ERR_COVER_CAP, a list or a text above its capacity, total 0 and nothing written.
constexpr int NH_ERR_COVER = 1024, NH_ERR_COVER_CAP = 2048;
struct CoverArgs {
    const char *text;         // the text the classifier read, ntext bytes, 4-byte aligned
    uint64_t ntext;
    const uint64_t *seq_off;  // n_seq sequence starts (absolute)
    const uint32_t *seq_len;  // n_seq sequence lengths
    uint64_t n_seq;
    const uint8_t *host_of;   // NULL (every non-zero value is host), or n_nodes bytes: host_table()'s
    uint64_t n_nodes;
    uint32_t *cover;          // cover_words(ntext) words, ORed into
    uint64_t *scratch;        // cover_mark_scratch_words(n_seq) words
    int *error;
};
struct CoverIvlArgs {
    const uint32_t *cover;    // cover_words(ntext) words
    uint64_t ntext;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    uint64_t n_seq;
    uint32_t *rec;            // cap records of three words: sequence, start, end
    uint64_t cap;
    uint64_t *total;          // one word: the records written
    uint64_t *scratch;        // cover_intervals_scratch_words(n_seq) words
    int *error;
    uint32_t *cnt;            // (the launcher's: where in the scratch the counts and the block sums lie)
    uint64_t *blk, nblk;
};
struct CoverLinesArgs {
    const char *text;         // the batch's text (the ids), ntext bytes
    uint64_t ntext;
    const uint32_t *rec;      // n * mates {header start (absolute), header length, ...}: the run's record table
    const uint32_t *idlen;    // n: the length of mate 1's id
    const nh_result *res;     // n results (the true calls)
    const uint64_t *ext;      // internal -> external taxon id, n_ext entries
    uint64_t n_ext, n;        // n: fragments
    int mates;
    const uint32_t *ivl;      // the records, *n_ivl of them (a number above cap_ivl: none)
    const uint64_t *n_ivl;
    uint64_t cap_ivl;
    char *out;                // cap bytes
    uint64_t cap;
    uint64_t *blk;            // 3 * nblk words of scratch, nblk = cover_line_blocks(cap_ivl)
    uint64_t nblk;
    uint64_t *total;          // 4 words: bytes, lines, fragments with a line, covered bases
    int *error;
};
struct CoverCloseArgs {       // --host-bases-only's gap closing: an uncovered run of at most gap bases between two covered ones of a sequence
    uint32_t *cover;          // cover_words(ntext) words, ORed into
    uint64_t ntext;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    uint64_t n_seq;
    uint32_t gap;
    const nh_result *res;     // NULL (every sequence), or the results of the n_seq / mates fragments: a fragment whose call is 0 is left alone
    int mates;
    unsigned long long *closed;  // NULL or one counter the waves add the bases they set to
    int *error;
};
int cover_check_db(const Engine *e);  // NH_OK, or NH_EINVAL: a geometry or a probing the pass does not support, named
uint64_t cover_words(uint64_t ntext);
uint64_t cover_mark_scratch_words(uint64_t n_seq);
uint64_t cover_intervals_scratch_words(uint64_t n_seq);
uint64_t cover_line_blocks(uint64_t cap_ivl);
hipError_t launch_cover_mark(Engine *e, const CoverArgs &c, hipStream_t stream);
hipError_t launch_cover_intervals(const CoverIvlArgs &a, hipStream_t stream);
hipError_t launch_cover_lines(const CoverLinesArgs &a, hipStream_t stream);
hipError_t launch_cover_close(const CoverCloseArgs &a, hipStream_t stream);
// Host cut (nh_cut.hip; nh_run_hostcut): a single-end masked run whose host fragments are written as PIECES -- the
// maximal runs of at least min_piece bases that the closed cover bitmap does not cover, each a record of its own, "<id>:<a>-<b>" --
// and every other fragment whole.  k_cut_item_* turn the bitmap and the calls into the items {seq, a, b} (a whole record: 0, slen),
// k_cut_* the items into text.  The engine's sticky error word: NH_ERR_CUT, a record whose fields leave the text or whose id is
// longer than its header (nothing of it is written); NH_ERR_CUT_QLEN, a FASTQ host record whose quality line is not as long as its
// sequence (nothing of it is written); NH_ERR_CUT_CAP, a list or a text above its capacity, total 0 and nothing written.
constexpr int NH_ERR_CUT = 4096, NH_ERR_CUT_CAP = 8192, NH_ERR_CUT_QLEN = 16384;
enum { CUT_HOST_BASES, CUT_PIECES, CUT_PIECE_BASES, CUT_CUT_BASES, CUT_SHORT_BASES, CUT_DROPPED, CUT_COUNTS };
struct CutArgs {
    const char *text;         // the batch's text (d_text: the INPUT's bases), ntext bytes
    uint64_t ntext;
    const uint64_t *seq_off;  // n sequence starts (absolute), as classified
    const uint32_t *seq_len;  // n sequence lengths
    const uint32_t *rec;      // n {header start (absolute), header length, qualities start (absolute), length}
    const uint32_t *idlen;    // n: the length of the id (RecRef::idlen)
    const nh_result *res;     // n results: call != 0 is a host fragment
    uint64_t n;
    int fastq;
    const uint32_t *cover;    // cover_words(ntext) words: the closed coverage, one bit a byte of the text
    uint32_t min_piece;       // >= 1
    uint32_t *items;          // cap_items items of three words: sequence, a, b
    uint64_t cap_items;
    uint64_t max_item;        // bytes of the longest item's output there can be: the write kernel's spans
    char *out;                // cap bytes
    uint64_t cap;
    uint64_t *scratch;        // cut_scratch_words(n, cap_items) words
    uint64_t *total;          // two words: the bytes written, the items
    unsigned long long *counts;  // NULL or CUT_COUNTS counters the waves add to
    int *error;
};
uint64_t cut_scratch_words(uint64_t n, uint64_t cap_items);
uint64_t cut_max_pieces(uint64_t slen, uint32_t min_piece);  // P(L) = (L + k) / (M + k), 0 where L < M
hipError_t launch_cut(const CutArgs &a, hipStream_t stream);
// buffers kept between the runs of a process (nh_run.hip: page-locked batch text; nh_gunzip.hip: the gzip reader's HBM and
// staging): emptied when an engine is closed
void run_cache_trim();
void dev_cache_trim();
// ---- devices.  Every device id in this library (nh_open's `device`, nh_run_args.device_ids, Engine::device, a batch's
// dev_device ...) is a LOGICAL device; dev_set() is the only way a thread selects one.  By default logical == HIP ordinal.
// NOHUMAN_FAKE_DEVICES=N (test mode for a box with one GPU): N logical devices, all on HIP device 0 -- the run's engines,
// reader lanes, encoders, streams and buffers then have N distinct owners, copies between them take the peer route, and
// NOHUMAN_DEBUG_DEVICE=1 checks the discipline a real multi-GPU node enforces by failing: dev_check() that the calling
// thread's current logical device is the owner's at every launch / copy / allocation site, dev_check_ptr() that a buffer
// was allocated under its owner (this library's allocations are registered; hipPointerGetAttributes has the last word on
// the physical device).  The first violation is kept (dev_violation()) and fails the run that meets it.
int dev_count();                 // logical devices (<= 0: none / HIP error)
int dev_phys(int ldev);          // HIP ordinal behind a logical device
hipError_t dev_set(int ldev);    // hipSetDevice(dev_phys(ldev)) and the thread's logical device
int dev_current();               // the thread's logical device (-1: none selected yet)
bool dev_debug();
void dev_check(int owner, const char *where);
void dev_check_ptr(const void *p, int owner, const char *where);
std::string dev_violation(bool clear = false);
// n bytes from device memory of src_ldev to device memory of dst_ldev on `stream` (a stream of dst_ldev, the calling
// thread's current device): the same logical device: an ordinary device-to-device copy; otherwise hipMemcpyPeerAsync --
// peer access between the two HIP devices is enabled the first time where hipDeviceCanAccessPeer allows it (without it the
// runtime stages the copy itself) -- or, under NOHUMAN_NO_PEER=1, through a page-locked host buffer (D2H, H2D; synchronous).
hipError_t dev_copy_between(void *dst, int dst_ldev, const void *src, int src_ldev, size_t n, hipStream_t stream);
// Every allocation of the run path goes through these two: when the device (or the page-locked pool) is full, what the
// process keeps between runs is given back first and the allocation tried once more -- idle buffers never fail a run.
hipError_t dev_malloc(void **p, size_t bytes);
hipError_t host_malloc(void **p, size_t bytes, unsigned flags = hipHostMallocDefault);
template <class T>
inline hipError_t dev_malloc(T **p, size_t bytes) {
    return dev_malloc((void **)p, bytes);
}
template <class T>
inline hipError_t host_malloc(T **p, size_t bytes, unsigned flags = hipHostMallocDefault) {
    return host_malloc((void **)p, bytes, flags);
}
// A block of device memory (PINNED: of page-locked host memory) with one owner: `cap` elements at `p`, freed exactly once.  The
// destructor frees under the device the thread has selected -- whoever holds buffers of a device (a slot, a run's RunBuffers,
// the build's Builder) selects it in its own destructor, which runs before its members'; a local's owner has it selected.
template <class T, bool PINNED>
struct Buf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) reset(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
        return *this;
    }
    ~Buf() { reset(); }
    void reset() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
    // room for `need` elements: nothing to do where there is; else the block is freed FIRST -- the peak is one block, no content
    // is kept -- and `new_cap` elements are allocated (the caller's growth policy).  A failure leaves the buffer empty.
    hipError_t reserve(size_t need, size_t new_cap) {
        if (need <= cap) return hipSuccess;
        reset();
        const hipError_t he = PINNED ? host_malloc(&p, new_cap * sizeof(T)) : dev_malloc(&p, new_cap * sizeof(T));
        if (he == hipSuccess) cap = new_cap;
        else p = nullptr;
        return he;
    }
    hipError_t reserve(size_t n) { return reserve(n, n); }  // exactly n: a buffer that does not grow
    operator T *() const { return p; }
};
template <class T>
using DevBuf = Buf<T, false>;
template <class T>
using PinBuf = Buf<T, true>;
// The events around stretches of a stream, a pair as a rule (NOHUMAN_TRACE, the build's kernel times): made on request under the
// owner's device, destroyed with their owner; without create() all are null and nobody records them.
template <int N>
struct Events {
    hipEvent_t ev[N] = {};
    Events() = default;
    Events(Events &&o) noexcept { std::swap(ev, o.ev); }
    Events &operator=(Events &&o) noexcept {
        std::swap(ev, o.ev);
        return *this;
    }
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {
        hipError_t he = hipSuccess;
        for (hipEvent_t &e : ev)
            if (he == hipSuccess && !e) he = hipEventCreate(&e);
        return he;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
};
using EventPair = Events<2>;
// the path's only collective: rows[g] = counters of device ids[g] -> every row = the sum (RCCL, nh_collective.hip)
// (d_src[g] != NULL: the four counters lie in device ids[g]'s memory and are reduced from there)
int allreduce_counters(const int *ids, int n_dev, uint64_t *rows, std::string &backend,
                       const uint64_t *const *d_src = nullptr);
uint64_t kmer_taxa_entries(const Engine *e, const uint64_t *seq_offsets, uint64_t n_frag, int mates,
                           uint64_t *offsets_out);

}  // namespace nh
