/*
 * nohuman_engine.h -- C ABI of libnohuman_engine.so, the MI355X (gfx950) in-process replacement
 * for the `kraken2` subprocess that nohuman spawns.
 *
 * What it replaces in the reference (file:line under /root/reference):
 *   - the process boundary  CommandRunner::run -> Command::new("kraken2").args(..).output()
 *     (src/lib.rs:22-48) called once, blocking, from main() (src/main.rs:270);
 *   - the information carried by the argv built at src/main.rs:210-267
 *     (--threads, --db, --output, --confidence, --report, --paired,
 *      --classified-out | --unclassified-out, input paths);
 *   - the three integers scraped from kraken2's stderr by parse_kraken_stderr
 *     (src/lib.rs:61-97), which the engine returns directly in nh_stats;
 *   - the dependency check CommandRunner::is_executable (src/lib.rs:50-57) -> nh_probe;
 *   - the database directory contract validate_db_directory (src/lib.rs:119-141) -> nh_open.
 *
 * Conventions: every function returns 0 on success or a negative nh_status; nothing throws or
 * aborts across the ABI; the caller owns every buffer it passes; the engine handle is opaque and
 * only created/destroyed by nh_open... / nh_close; nh_last_error() is a thread-local string valid
 * until the next call on that thread.  There is NO CPU fallback: without a usable gfx950 device
 * nh_open / nh_probe fail with NH_EDEVICE.
 */
#ifndef NOHUMAN_ENGINE_H
#define NOHUMAN_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NH_ABI_VERSION 5

typedef enum {
    NH_OK = 0,
    NH_EINVAL = -1,   /* bad argument */
    NH_EIO = -2,      /* file could not be read / written */
    NH_EDB = -3,      /* malformed or unsupported database (e.g. protein DB) */
    NH_EDEVICE = -4,  /* no usable gfx950 device, HIP error */
    NH_EOOM = -5,     /* host or device allocation failed */
    NH_ECAPACITY = -6 /* an internal per-fragment capacity was exceeded (reported, never silent) */
} nh_status;

typedef struct nh_engine nh_engine;

/* One record per fragment (read or read pair).  16 bytes; the "result record" of the roofline
 * formula in BASELINE.md section 4.  Replaces the C/U column, the taxid column and the hit list
 * totals of kraken2's per-read output line. */
typedef struct {
    uint32_t call;        /* internal taxon id of the call; 0 = unclassified (kept by nohuman) */
    uint32_t total_kmers; /* k-mers of both mates, ambiguous ones included (confidence denominator) */
    uint32_t clade_hits;  /* k-mer hits in the clade rooted at `call` (confidence numerator) */
    uint32_t hit_groups;  /* kraken2 minimizer_hit_groups */
} nh_result;

/* per-k-mer taxa list markers (the "A:n" and "|:|" items of kraken2's hit list) */
#define NH_TAXON_AMBIGUOUS 0xFFFFFFFFu
#define NH_TAXON_MATE_BORDER 0xFFFFFFFEu

/* Replaces the three summary lines of kraken2's stderr (src/lib.rs:67-89). */
typedef struct {
    uint64_t total_sequences; /* fragments processed */
    uint64_t classified;      /* "sequences classified" == human for nohuman */
    uint64_t unclassified;
    uint64_t total_bases;
    uint64_t table_lookups;   /* D of the roofline formula, summed */
    double seconds;           /* classify wall time, database load excluded (as kraken2's timer) */
} nh_stats;

typedef struct {
    uint64_t k, l, spaced_seed_mask, toggle_mask, minimum_acceptable_hash_value;
    int32_t revcom_version, dna_db;
    uint64_t capacity, size, key_bits, value_bits;
    uint64_t node_count;
    int32_t device;
    int32_t reserved;
} nh_db_info;

/* Behaviour switches; defaults reproduce kraken2 as nohuman invokes it (src/main.rs:215-224:
 * no --minimum-hit-groups, no --quick, no quality masking).  kraken2's --minimum-base-quality is not a field here (the struct
 * keeps its size): it is an argument of nh_run_minq / nh_quality_mask_device below. */
typedef struct {
    uint32_t minimum_hit_groups; /* default 2 */
    int32_t linear_probing;      /* default 1 (kraken2 builds with -DLINEAR_PROBING) */
    int32_t reset_per_mate;      /* default 1 (last minimizer/taxon reset for each mate) */
    /* ABI 4 (ABI 2: `reserved`, 0; ABI 3: 0 / 1): which k-mers next to an ambiguous base count as ambiguous ("A:n" in the
     * hit list, no look-up) -- the two recollections of kraken2's scanner, switchable until a binary has been diffed
     * (BASELINE.md section 2).  ZERO MEANS "THE ENGINE'S DEFAULT": a caller that fills the struct
     * from scratch and leaves the former `reserved` word 0 keeps the pinned default instead of silently selecting a rule:
     *   NH_AMBIGUITY_ENGINE_DEFAULT (0)  whatever NH_AMBIGUITY_DEFAULT names (nh_options_get reports the rule in force);
     *   NH_AMBIGUITY_LAST_LMER (1)  the bool* flag of MinimizerScanner::NextMinimizer: an ambiguous byte among the
     *                               k-mer's last l bases; an isolated N costs l = 31 k-mers, the next three are
     *                               looked up with windows of 1, 2, 3 l-mers;
     *   NH_AMBIGUITY_QUEUE (2)      mmscanner.h is_ambiguous() = (queue_pos_ < k_ - l_) || !!last_ambig_, what
     *                               classify.cc / build_db.cc ask: also ambiguous until k - l l-mers have been queued
     *                               behind the base, i.e. an ambiguous byte among the last k - 1 bases; an isolated N
     *                               costs k - 1 = 34 k-mers.  The default. */
    int32_t ambiguity_rule;
} nh_options;
#define NH_AMBIGUITY_ENGINE_DEFAULT 0
#define NH_AMBIGUITY_LAST_LMER 1
#define NH_AMBIGUITY_QUEUE 2
#define NH_AMBIGUITY_DEFAULT NH_AMBIGUITY_QUEUE

/* flags of nh_classify_* */
#define NH_FLAG_PAIRED 1u /* sequences 2f and 2f+1 are the mates of fragment f (--paired) */
#define NH_FLAG_LONG 2u   /* scheduling hint: fragments are long (kilobases); hand them out one by one */

const char *nh_last_error(void);
int nh_abi_version(void);

/* 0 if a gfx950 device is usable; msg receives a one-line description either way.
 * Replaces CommandRunner::is_executable (src/lib.rs:50-57), used by `nohuman --check`. */
int nh_probe(char *msg, size_t msg_len);
int nh_device_count(int *count);

/* Load <db_dir>/{hash,opts,taxo}.k2d -- or <db_dir>/db/... (src/lib.rs:119-141) -- into the HBM
 * of `device`.  Replaces kraken2's "Loading database information..." phase.
 * The CONTENT is checked too (ABI 5), because the kernels index the taxonomy with the cells' values and nohuman can have
 * several database versions installed side by side (src/download.rs:178-222): every cell is read once on the device
 * (about a millisecond per 5 GB); a value >= taxo.k2d's node count, a count of non-empty cells that is not the header's
 * `size`, or a taxonomy whose parent ids do not lie below their children fail with NH_EDB -- never with a GPU fault. */
int nh_open(const char *db_dir, int device, nh_engine **out);
/* Same from in-memory images of the three files (borrowed for the duration of the call). */
int nh_open_images(const void *opts, size_t opts_len, const void *taxo, size_t taxo_len,
                   const void *hash, size_t hash_len, int device, nh_engine **out);
/* Bench/test support: a database whose hash table is generated directly in HBM (n_keys pseudo-
 * random minimizers inserted with kraken2's CompareAndSet linear-probing rule; every value is the
 * deepest node of a `depth`-node chain taxonomy).  Stands in for HPRC.r2, which cannot be
 * downloaded on the build or GPU boxes. */
int nh_open_synthetic(uint64_t capacity, uint64_t n_keys, uint32_t depth, uint64_t seed, int device,
                      nh_engine **out);
/* Bench/test support: inserts every minimizer of the given device-resident sequences into the
 * table with internal taxon id `value` (kraken2 build semantics: CompareAndSet, linear probing), so
 * that reads drawn from them hit.  Default k=35/l=31 geometry only. */
int nh_synthetic_add_sequences(nh_engine *e, const void *d_bases, const void *d_seq_offsets,
                               uint64_t n_seq, uint32_t value, void *stream);
int nh_close(nh_engine *e);

int nh_db_info_get(const nh_engine *e, nh_db_info *info);
/* What the content check of nh_open* measured (ABI 5). */
typedef struct {
    uint64_t non_empty_cells; /* cells whose value field is not 0; == nh_db_info.size of a database that opened */
    uint64_t max_value;       /* largest value field in the table; < nh_db_info.node_count */
    double load_factor;       /* non_empty_cells / capacity */
    double seconds;           /* what the pass cost */
} nh_db_check;
int nh_db_check_get(const nh_engine *e, nh_db_check *c);
/* The defaults of a freshly opened engine can be overridden per process by NOHUMAN_OPT_AMBIGUITY_RULE,
 * NOHUMAN_OPT_LINEAR_PROBING, NOHUMAN_OPT_RESET_PER_MATE, NOHUMAN_OPT_MIN_HIT_GROUPS (integers): how
 * scripts/parity_vs_kraken2.sh walks the switch lattice through nh_run and the CLI host. */
int nh_options_get(const nh_engine *e, nh_options *o);
int nh_options_set(nh_engine *e, const nh_options *o);
/* internal taxon id -> external (NCBI) id, as printed in kraken2's output / "kraken:taxid|N" */
int nh_taxon_external(const nh_engine *e, uint32_t internal, uint64_t *external);
/* copies of the database images back to the host (tests and the bench's CPU-baseline leg) */
int nh_table_download(const nh_engine *e, uint32_t *cells, uint64_t n_cells);
int nh_taxonomy_image(const nh_engine *e, void *buf, size_t cap, size_t *len);
int nh_opts_image(const nh_engine *e, void *buf, size_t cap, size_t *len);

/*
 * Classify one batch held in HOST memory; blocking.  Replaces kraken2's per-block loop
 * (classify.cc ProcessFiles/ClassifySequence) for the reads of one batch.
 *   bases        concatenated sequence bytes exactly as in the FASTQ/FASTA sequence lines
 *   seq_offsets  n_seq+1 offsets into bases; n_seq = n_frag * (paired ? 2 : 1)
 *   confidence   the f64 value kraken2 would parse from --confidence (src/main.rs:213)
 *   results      n_frag records
 *   kmer_taxa / kmer_taxa_offsets (both NULL or both set): per-k-mer internal taxon ids with the
 *                two markers above -- the material of the `-k` hit list.
 *                kmer_taxa_offsets[f] = sum over fragments < f of (k-mers of both mates + paired);
 *                the caller sizes kmer_taxa with nh_kmer_taxa_entries.
 * NH_ECAPACITY: a fragment (both mates together) hit more than 2048 distinct taxa.  The whole call fails, here and in every
 * nh_run*: `results` and `kmer_taxa` are not to be read.  The error is cleared with the call that reports it, so the engine
 * classifies the next batch as if nothing had happened.
 */
int nh_classify_batch(nh_engine *e, const uint8_t *bases, const uint64_t *seq_offsets,
                      uint64_t n_frag, uint32_t flags, double confidence, nh_result *results,
                      uint32_t *kmer_taxa, uint64_t *kmer_taxa_offsets, uint64_t kmer_taxa_cap);
uint64_t nh_kmer_taxa_entries(const nh_engine *e, const uint64_t *seq_offsets, uint64_t n_frag,
                              uint32_t flags);

/*
 * Same with every buffer already resident in the engine device's HBM; asynchronous on `stream`
 * (a hipStream_t, NULL = the default stream).  d_bases must be 4-byte aligned and readable for
 * 8 bytes past the last base.  d_kmer_taxa / d_kmer_taxa_offsets may be NULL.  d_counters (may be
 * NULL) points at 4 uint64 accumulators {fragments, classified, bases, table_lookups} that the
 * kernel adds to.  This is the entry the roofline number of bench.py is measured on.
 * Thread-safe per engine: any number of host threads may call it on one engine, each on its own stream.  The engine has
 * 16 launch slots; a launch that finds its slot still taken by the launch sixteen before it waits for that one ON THE
 * DEVICE (an event wait queued on `stream`), so more than 16 launches in flight are ordered, never mixed.
 */
int nh_classify_batch_device(nh_engine *e, const void *d_bases, const void *d_seq_offsets,
                             uint64_t n_frag, uint32_t flags, double confidence, void *d_results,
                             void *d_kmer_taxa, const void *d_kmer_taxa_offsets, void *d_counters,
                             void *stream);

/*
 * The same launch with the sequences classified IN PLACE inside a device-resident buffer of record text
 * (what nh_run does with the FASTQ / FASTA text of a batch, copied to the device as read -- no pass that
 * gathers the sequence lines): sequence i is d_text[d_seq_starts[i], +d_seq_lens[i]) (uint64 / uint32,
 * n_frag * (paired ? 2 : 1) entries each; pairs: entries 2f and 2f+1; the first sequence must be the
 * one at the lowest address and all of a launch must lie within 4 GB).  Whatever surrounds a sequence
 * (header, '+' line, qualities, newlines) is never interpreted.  d_text must be 4-byte aligned and readable
 * for 8 bytes past text_len.
 */
int nh_classify_records_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts,
                               const void *d_seq_lens, uint64_t n_frag, uint32_t flags, double confidence,
                               void *d_results, void *d_kmer_taxa, const void *d_kmer_taxa_offsets,
                               void *d_counters, void *stream);

/* running totals over every nh_classify_batch* call on this engine since open / reset */
int nh_stats_get(nh_engine *e, nh_stats *s);
int nh_stats_reset(nh_engine *e);

/* container of the kept reads (CompressionFormat, /root/reference/src/compression.rs:12-20) */
typedef enum nh_codec {
    NH_CODEC_NONE = 0,
    NH_CODEC_BZIP2 = 1,
    NH_CODEC_GZIP = 2,
    NH_CODEC_XZ = 3,
    NH_CODEC_ZSTD = 4, /* through the system's libzstd.so.1 (level 3, frame checksum, `threads` workers) */
    /* gzip in bgzip's blocked container (BGZF): a series of gzip members of 65280 bytes of text each (the last data member
     * 1 to 65280), every one with its compressed size in a 'B' 'C' extra field and its own CRC-32 / ISIZE, closed by the
     * 28-byte EOF member; an empty text is the EOF member alone.  Any gzip reader takes it; htslib tools seek in it, and
     * this library's GPU reader finds its chunks by the headers.  Encoded like NH_CODEC_GZIP: on the GPU where nh_run has one
     * (NOHUMAN_GZIP=host: zlib level 6 on `threads` workers), accepted wherever a codec is.  No .gzi index is written. */
    NH_CODEC_BGZF = 5,
    /* BAM output (nh_run* only; "BAM output" below): every record output of the run is a BAM file -- the input's header and the
     * selected records of the input, byte for byte, in NH_CODEC_BGZF's framing.  in1 must be a BAM file. */
    NH_CODEC_BAM = 6
} nh_codec;

/*
 * Whole-run entry: the information of the argv at src/main.rs:210-267, outputs written
 * UNCOMPRESSED (out_codec 0) to the given paths exactly where kraken2 would write kraken_out.fq /
 * kraken_out_1.fq + kraken_out_2.fq (src/main.rs:252-256,308-309,333), so nohuman's compress stage
 * (src/main.rs:342-368) is untouched -- or, with out_codec set, already in their final container.
 */
typedef struct {
    const char *db_dir;        /* --db */
    const char *in1;           /* first input (plain or gzip FASTQ/FASTA) */
    const char *in2;           /* second input or NULL (--paired when set) */
    const char *out1;          /* kraken_out.fq / kraken_out_1.fq */
    const char *out2;          /* kraken_out_2.fq or NULL */
    const char *kraken_output; /* --output; NULL or "/dev/null" = none */
    const char *report;        /* --report; NULL = none */
    double confidence;         /* --confidence */
    uint32_t threads;          /* --threads: host reader/writer workers */
    int32_t keep_human;        /* 0: --unclassified-out (default), 1: --classified-out (-H) */
    int32_t n_devices;         /* 0 = all visible devices */
    const int32_t *device_ids; /* NULL = 0..n_devices-1 */
    /* ABI 2 -- SURVEY.md 8f-4: the kept reads can leave the engine already compressed, written straight to
     * their final paths by a streaming encoder, which removes the temporary uncompressed files and the
     * second pass of the reference's compress stage (src/compression.rs:182-268, src/main.rs:342-368).
     * 0 (NH_CODEC_NONE) keeps the kraken2 behaviour: plain text at out1 / out2. */
    int32_t out_codec;         /* nh_codec of out1 / out2 */
    uint32_t codec_threads;    /* encoder workers per output file (0 = 1) */
} nh_run_args;

int nh_run(const nh_run_args *args, nh_stats *stats);
/* Host-side check of the sequence reader nh_run uses (kraken2 record semantics, SURVEY.md A.6;
 * plain / gzip / bzip2, FASTA / FASTQ): number of records, total bases, and an FNV-1a-64 digest
 * over every record's header line, sequence and qualities (each followed by one 0 byte).
 * Needs no GPU. */
int nh_fastx_scan(const char *path, uint64_t *n_records, uint64_t *n_bases, uint64_t *digest);
/*
 * BAM input.  in1 of every nh_run* may be a BAM file -- unaligned (ONT, PacBio HiFi, uBAM) or aligned, single-end or collated
 * pairs (below): a file whose
 * first gzip member carries the BGZF extra field and whose inflated stream begins "BAM\1"; anything else is read as before.  Its
 * records are transcoded on the GPU to the canonical FASTQ `samtools fastq` would write (as far as that is recalled: DESIGN.md
 * 6.16) and everything behind the reader runs on that text: "@name\nSEQ\n+\nQUAL\n", bases from "=ACMGRSVTWYHKDBN", qualities
 * + 33 (absent qualities, first byte 0xFF: every quality '"'), reverse-strand records (flag 0x10) reverse-complemented with their
 * qualities reversed, no tags in the header (the tags survive only in BAM output, NH_CODEC_BAM below).  Secondary and supplementary records (0x100, 0x800) and records without bases are
 * skipped.  A BAM in1 with an in2, or a BAM in2, is NH_EINVAL before any device is touched.
 *
 * Paired BAM.  A file is paired iff its first kept record has flag 0x1 (a file without a kept record is single-end).  In a
 * single-end file a later 0x1 record fails the run with NH_EIO, as every malformed record does, with the record's ordinal and
 * name in the message.  In a paired file the kept records are taken two at a time, in file order, skipped records in between
 * stepped over: both have 0x1, exactly one has 0x40 and the other 0x80, their names are equal byte for byte; the 0x40 record is
 * mate 1 whichever comes first (`samtools collate` promises no order).  Anything else -- a kept record without 0x1, with both
 * or neither of 0x40 / 0x80, two records of one mate, two names (the file is not collated), a last record without a partner, a
 * record whose mate is empty and therefore skipped -- is NH_EIO with the record's ordinal and name.  Each mate is transcoded as
 * a single-end record is and its name written as it is, without "/1" or "/2" (`samtools fastq -n -1 -2`, as far as recalled).
 * The run is, in every output, the run on the two FASTQ files the mates transcode to: it is a paired run with in2 NULL, and
 * wants out2, human_out2 and the selectors' out2 as one with in2 does (NH_EINVAL without them), except with NH_CODEC_BAM, where
 * one BAM holds both mates and out2 / human_out2 are NH_EINVAL.  nh_bam_paired: 1 for a paired BAM file, 0 for anything else.
 *
 * nh_bam_scan: the host side alone, no device -- the counts of a BAM file and nh_fastx_scan's digest of the FASTQ it transcodes
 * to (a paired file: of its kept records in file order; the counts cover all kept records).  NH_EINVAL: a null argument, a
 * struct_size below the struct's, a file that is no BAM; NH_EIO: a malformed one.
 * nh_bam_scan_pairs: the same pass, and what a paired file has besides -- the pairs, each mate's bases and nh_fastx_scan's digest
 * of each mate's FASTQ (a single-end file: paired 0, no pairs, the digests of empty files).
 */
typedef struct nh_bam_info {
    uint32_t struct_size;          /* sizeof(nh_bam_info), set by the caller */
    uint32_t reserved;
    uint64_t records;              /* all records of the file */
    uint64_t reads;                /* records kept */
    uint64_t bases;                /* bases of the kept records */
    uint64_t skipped_secondary;    /* flag 0x100 or 0x800 */
    uint64_t skipped_empty;        /* l_seq == 0 */
    uint64_t reverse_complemented; /* kept records with flag 0x10 */
    uint64_t missing_qualities;    /* kept records whose qualities are absent */
    uint64_t digest;
} nh_bam_info;
int nh_bam_scan(const char *path, uint32_t threads, nh_bam_info *info);
typedef struct nh_bam_pair_info {
    uint32_t struct_size;          /* sizeof(nh_bam_pair_info), set by the caller */
    uint32_t paired;               /* 1: the first kept record has flag 0x1 */
    uint64_t pairs;
    uint64_t bases1, bases2;       /* bases of the mates 1 (flag 0x40), of the mates 2 */
    uint64_t digest1, digest2;     /* nh_fastx_scan's digest of mate 1's FASTQ, of mate 2's */
} nh_bam_pair_info;
int nh_bam_scan_pairs(const char *path, uint32_t threads, nh_bam_info *info, nh_bam_pair_info *pairs);
int nh_bam_paired(const char *path);
/* The kernel alone, asynchronous on `stream`, on the engine's device.  d_bam: bam_len BAM bytes (4-byte aligned, readable up to
 * bam_len rounded up to a multiple of 4); d_table: two uint64 a record -- the offset of its block_size field in d_bam and the
 * offset of its '@' in d_text, the latter ascending; d_text: text_cap bytes (4-byte aligned) of which [0, text_len) is the text.
 * error_bits: one int in device memory, zeroed by the caller.  A record whose fields, as its own fixed part states them, do not
 * lie inside d_bam sets bit 1 there, one whose text does not lie inside [0, text_len) bit 2; nothing of such a record is written
 * and the others are.  NOHUMAN_BAM_SPAN: the bytes of text one wave writes of a long record (a test and tuning knob). */
int nh_bam_to_fastq_device(nh_engine *e, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_records,
                           void *d_text, uint64_t text_cap, uint64_t text_len, int *error_bits, void *stream);
/*
 * BAM output.  With out_codec = NH_CODEC_BAM and a BAM in1, single-end or paired, out1 (and human_out1 of a split run) is a BAM file: the input's
 * header copied byte for byte (magic, l_text, text, n_ref, references; no @PG line is added), then the selected records of the
 * input in input order, each copied byte for byte with its block_size field -- tags (MM / ML, mv, RG ...), CIGAR, flags and a
 * reverse-strand record's orientation untouched -- framed as BGZF and closed by bgzip's EOF member.  Which records are selected
 * is the FASTQ outputs' rule: out1 gets the non-host records (with keep_human the host records), human_out1 the host records; a
 * host selection (nh_host_filter) is followed as the FASTQ outputs follow it.  No record selected: the header and the EOF
 * member, still a valid BAM.  The records the reader skips -- secondary, supplementary, without bases -- are never classified
 * and are written NOWHERE (nh_bam_scan counts them).  No call is added to a record: it is in `calls` and kraken_output.  Every
 * other output (kraken_output, report, calls, human_ids, read statistics, minimizer data, nh_stats) is byte for byte what the
 * same run with a FASTQ codec writes.  The records are selected and compacted on the GPU from the BAM bytes the reader holds
 * there (nh_bamout.hip) and encoded by NH_CODEC_BGZF's encoders.  A paired BAM: the two records of a pair are selected
 * together, by the pair's call, and written in the order they have in the file.
 * NH_EINVAL, before any device is touched and with nothing created: NH_CODEC_BAM with an in1 that is not a BAM file, with in2,
 * with out2 or human_out2 beside a paired BAM, in a masked run, with per-taxon outputs (the last two: not built yet).  nh_compress_file* refuse it: a FASTQ file cannot be
 * made a BAM.
 *
 * nh_bam_select_device: the select-and-compact kernels alone, on the engine's device and `stream`.  d_bam / bam_len as for
 * nh_bam_to_fastq_device; d_table: the reader's table, two uint64 a record, of which the first -- the offset of the record's
 * block_size field in d_bam -- is used; d_results: n_records nh_result; want: 0 selects the records with call == 0, 1 those with
 * call != 0.  d_out (out_cap bytes, 4-byte aligned) receives the selected records, 4 + block_size bytes each, contiguous and in
 * table order; *d_total (device memory) their bytes.  error_bits: one int in device memory, zeroed by the caller: a record whose
 * block_size field or whose bytes [offset, offset + 4 + block_size) do not lie inside [0, bam_len) sets bit 1 and is not
 * written (the others are); a total above out_cap sets bit 4, nothing is written and *d_total is 0.  The call waits for
 * `stream` (its scratch is the call's own).  NOHUMAN_BAM_SPAN: the bytes one wave copies of a long record (test / tuning knob).
 *
 * nh_bam_select_pairs_device: the same on pairs.  d_table: the paired reader's, two uint64 a PAIR -- the offsets of its two
 * records' block_size fields, in file order; d_results: n_pairs nh_result, one a pair.  Both records of a selected pair are
 * written, in table order.  A record outside the BAM bytes sets bit 1 and is written nowhere, and neither is its mate.
 */
int nh_bam_select_device(nh_engine *e, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_records,
                         const void *d_results, int want, void *d_out, uint64_t out_cap, uint64_t *d_total, int *error_bits,
                         void *stream);
int nh_bam_select_pairs_device(nh_engine *e, const void *d_bam, uint64_t bam_len, const void *d_table, uint64_t n_pairs,
                               const void *d_results, int want, void *d_out, uint64_t out_cap, uint64_t *d_total, int *error_bits,
                               void *stream);
/* Output compression stage: replaces CompressionFormat::compress
 * (/root/reference/src/compression.rs:182-200, called from src/main.rs:342-368).  Compresses file
 * `in` to file `out`; gzip runs block-parallel on `threads` workers like the reference's gzp
 * encoder (compression.rs:214-233) and produces one ordinary gzip member at level 6; bzip2 and xz
 * go through libbz2.so.1 / liblzma.so.5 (one thread / `threads` workers, preset 6, CRC64), zstd through
 * libzstd.so.1; NH_CODEC_BGZF is zlib level 6 per 65280-byte member on `threads` workers; NH_CODEC_NONE copies; NH_CODEC_BAM is NH_EINVAL (a FASTQ file cannot be made a BAM).  Parity target is the decompressed content and
 * the container magic (compression.rs:282-288).  Needs no GPU. */
int nh_compress_file(const char *in, const char *out, int codec, uint32_t threads);
/* The gzip case of that stage on the GPU (nohuman_amd/csrc/nh_deflate.hip; replaces gzip_compress,
 * /root/reference/src/compression.rs:214-233): n bytes at `in` (host memory) become ONE ordinary gzip member in
 * file `out` -- 64 KiB regions of the text, a wave each, dynamic Huffman blocks, regions joined by empty stored
 * blocks the way gzp / pigz join theirs.  It is what nh_run's writer feeds when out_codec is NH_CODEC_GZIP
 * (NOHUMAN_GZIP=host selects the host encoder above).  stats (may be NULL): [0] bytes of the file, [1] microseconds
 * of kernel time (HIP events).  Parity target as above: the decompressed content. */
int nh_gzip_gpu_file(int32_t device, const void *in, uint64_t n, const char *out, uint64_t *stats);
/* The same through the encoder's BGZF mode (NH_CODEC_BGZF): a member per 65280-byte region, framed on the GPU, then the EOF
 * member.  Arguments and stats as nh_gzip_gpu_file. */
int nh_bgzf_gpu_file(int32_t device, const void *in, uint64_t n, const char *out, uint64_t *stats);
/* Test / tool support for that encoder: its HOST MODEL (nohuman_amd/csrc/nh_deflate_model.h -- the kernel's own lane-level functions,
 * nh_deflate_core.h, the 64 lanes run by a loop, with the host side's chunks, price pilot, price hand-over and framing).  Writes to
 * `out` the file nh_gzip_gpu_file (bgzf = 0) or nh_bgzf_gpu_file (bgzf = 1) writes for the same text when the encoder runs with
 * NOHUMAN_GZIP_WAYS = ways (4, 6, 8), NOHUMAN_GZIP_REGION = region_bytes (rounded as the encoder rounds it; BGZF: 65280 whatever it
 * says), chunks of chunk_bytes (the encoder's: NOHUMAN_GZIP_CHUNK_MB << 20, 128 MiB by default; here anything from one region up, BGZF:
 * cut down to whole regions) and NOHUMAN_GZIP_PRICES = prices (-1: unset, the pilot chooses).  The regions of a chunk run on `threads`
 * threads (0: up to 16); the bytes do not depend on that.  region_sizes (may be NULL): region_sizes_cap entries that receive the bytes
 * of every region's deflate stream, in order.  stats12 (may be NULL): {file bytes, regions, price set chosen, dynamic blocks, stored
 * blocks, blocks with a literal/length or distance code repaired to 15 bits, blocks with the code-length code repaired to 7 bits,
 * longest match, longest distance, matches extended beyond the scan cap, tokens, matches}.  Needs no GPU. */
typedef struct nh_gzip_model_opts {
    uint32_t ways;
    uint32_t region_bytes;
    uint64_t chunk_bytes;
    int32_t prices;
    int32_t bgzf;
    uint32_t threads;
    uint32_t reserved;
    uint32_t *region_sizes;
    uint64_t region_sizes_cap;
} nh_gzip_model_opts;
int nh_gzip_model_file(const void *in, uint64_t n, const char *out, const nh_gzip_model_opts *opts, uint64_t *stats12);
/* nh_compress_file for a host that keeps the reference's two stages (kraken2-style temporary file, then compress,
 * src/main.rs:342-368) but has the GPU at hand: NH_CODEC_GZIP and NH_CODEC_BGZF are encoded on `device` as above, the other codecs as in
 * nh_compress_file. */
int nh_compress_file_device(const char *in, const char *out, int codec, uint32_t threads, int32_t device);
/* Test / tool support for the multi-threaded gzip input decoder nh_run reads .gz inputs with
 * (kraken2's wrapper pipes them through `gzip -dc`): decompress `in` to
 * `out` on `threads` workers, cutting the compressed file every chunk_bytes (0 = default).
 * stats3 (optional) receives {chunks accepted, chunks rejected, bytes decoded in order by the
 * consumer}.  Needs no GPU. */
int nh_gunzip_file(const char *in, const char *out, uint32_t threads, uint64_t chunk_bytes, uint64_t *stats3);
/* The gzip READER on the GPU (nohuman_amd/csrc/nh_gunzip.hip; what nh_run reads .gz inputs with: replaces the `gzip -dc`
 * pipe of kraken2's wrapper): decompress `in` to `out` on `device` -- block search, decode to
 * 16-bit symbols with markers, the chunks' windows by a prefix scan, marker replacement and the members' CRC-32 on the
 * device (BGZF files: the chunks' starts from the members' headers, no search); seg_bytes / stretch_bytes = compressed
 * bytes per piece / per chunk (0 = defaults).  stats8 (optional):
 * {pieces, chunks, chunks decoded again after a false block start, pieces the host decoder took over, members, text
 * bytes, gzip bytes, kernel microseconds (NOHUMAN_TRACE only)}.  Test / tool support like nh_gunzip_file. */
int nh_gunzip_device_file(const char *in, const char *out, int32_t device, uint64_t seg_bytes, uint64_t stretch_bytes,
                          uint64_t *stats8);
/* Bytes of idle buffers the process keeps between runs for the gzip reader on `device` (page_locked != 0: its
 * page-locked staging, all devices): bounded by bytes, oldest evicted first, given back before any allocation of the
 * run path fails, emptied by nh_close.  Diagnostic / test support. */
uint64_t nh_cache_bytes(int32_t device, int32_t page_locked);
/* The one collective of the path: `counters` holds n_devices rows of 4 uint64
 * {fragments, classified, bases, table_lookups}, row g being the totals of device_ids[g] (NULL =
 * 0..n_devices-1); on return every row is the sum over the devices -- one ncclAllReduce(4 x uint64, sum)
 * over RCCL / xGMI, single process, ncclCommInitAll.  nh_run calls it at the end of a multi-device run
 * (and checks it against the host-side sum, which stays the fallback when RCCL cannot be loaded).
 * `backend` (optional) receives a one-line description of what ran.  Replaces nothing in the
 * reference (kraken2 sums its thread-local counters with atomics); it is the multi-GPU form of the
 * three integers of src/lib.rs:61-97. */
int nh_allreduce_counters(const int32_t *device_ids, int32_t n_devices, uint64_t *counters, char *backend,
                          size_t backend_len);
/* nh_run on an already opened engine (single device) */
int nh_run_engine(nh_engine *e, const nh_run_args *args, nh_stats *stats);
/*
 * Split run: nh_run that also writes the classified (human) records, in the same pass.  out1 / out2 of `args` receive
 * exactly what nh_run writes with keep_human = 0, human_out1 / human_out2 exactly what it writes with keep_human = 1
 * (" kraken:taxid|<id>" suffix included); kraken_output / report / stats exactly as one nh_run.  One codec
 * (args->out_codec) for all outputs.  The classified-out text is built in the GPU's memory.  NH_EINVAL, before any device
 * is touched: human_out1 NULL; keep_human not 0; human_out2 given without in2 or missing with in2; a human output that
 * names an input, out1, out2, kraken_output, report or the other human output.
 */
int nh_run_split(const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats);
int nh_run_engine_split(nh_engine *e, const nh_run_args *args, const char *human_out1, const char *human_out2,
                        nh_stats *stats);
/*
 * Masked run: nh_run with keep_human = 0 in which no fragment is dropped.  out1 / out2 receive every record, in input
 * order: an unclassified fragment's exactly as nh_run writes it, a classified fragment's (both mates) in the same form with
 * every base of its sequence replaced by 'N' (length and qualities unchanged, no " kraken:taxid|" suffix).  kraken_output /
 * report / stats exactly as one nh_run.  human_out1 (and, paired, human_out2) given: the classified records also go there
 * exactly as nh_run_split writes them; NULL: no human outputs.  The masked text is built in the GPU's memory.  NH_EINVAL,
 * before any device is touched: keep_human not 0; a human output that fails nh_run_split's checks; an output that names an
 * input.
 */
int nh_run_mask(const nh_run_args *args, const char *human_out1, const char *human_out2, nh_stats *stats);
int nh_run_engine_mask(nh_engine *e, const nh_run_args *args, const char *human_out1, const char *human_out2,
                       nh_stats *stats);
/*
 * Extended run: one entry for everything a run can write beside out1 / out2.  With calls and human_ids NULL it is exactly the
 * entry its other fields select (mask: nh_run_mask; a human output: nh_run_split; neither: nh_run).  The two read lists are plain
 * text whatever out_codec is, one line per fragment, in input order, no header line, built in the GPU's memory behind the
 * classifier in the same pass -- without the per-k-mer taxon lists and without the batches' text on the host that
 * kraken_output costs -- and mean the same in a normal, a keep_human, a split and a masked run:
 *   calls      a line for EVERY fragment:
 *                <C|U> \t <id> \t <taxid> \t <len>  or  <len1>|<len2> \t <total_kmers> \t <clade_hits> \t <hit_groups> \n
 *              columns 1-4 are byte for byte columns 1-4 of the fragment's kraken_output line (<id>: mate 1's header from the
 *              byte behind '@' / '>' to the first space, tab or '\r'; a paired run drops a trailing "/1" or "/2" from an id
 *              longer than two bytes; <taxid>: the external id of the call, 0 for U), columns 5-7 the fragment's nh_result as
 *              the classifier left it.  clade_hits / total_kmers is the confidence that nh_run_args.confidence thresholds:
 *              a threshold can be chosen from this table without running again.
 *   human_ids  <id> \n for every classified fragment, the same id; a run without human reads writes an empty file.
 * NH_EINVAL, before any device is touched: struct_size smaller than the struct; every check of nh_run_split / nh_run_mask for
 * the fields they share; calls or human_ids that names an input (the same path, or the same device and inode), out1, out2,
 * kraken_output, report, a human output, or each other.
 */
typedef struct {
    uint32_t struct_size;      /* sizeof(nh_run_extras) of the caller */
    int32_t mask;              /* 1: as nh_run_mask */
    const char *human_out1, *human_out2; /* as nh_run_split / nh_run_mask */
    const char *calls;         /* calls table, NULL = none */
    const char *human_ids;     /* ids of the classified fragments, NULL = none */
} nh_run_extras;
int nh_run_ex(const nh_run_args *args, const nh_run_extras *extras, nh_stats *stats);
int nh_run_engine_ex(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, nh_stats *stats);

/*
 * kraken2's --minimum-base-quality (classify.cc MaskLowQualityBases; a recollection like the rest of SURVEY.md A.5, parity
 * UNPINNED): with a threshold Q > 0 a base of a FASTQ record whose quality byte satisfies  qual - 33 < Q  (Phred+33 only, the
 * byte read as unsigned) is classified as an ambiguous base, in both mates; FASTA records have no qualities and are never
 * masked.  Only classification changes: nh_result, the hit list of kraken_output (masked stretches show as "A:n"), the calls
 * table, the report and the three totals; total_kmers, the lengths of kraken_output / calls and total_bases do not.
 * ONE DELIBERATE DEVIATION: kraken2 masks the sequence object itself and (as far as it is recalled) then writes the masked
 * 'x' bases into --unclassified-out; here EVERY OUTPUT RECORD KEEPS THE INPUT'S BASES -- kept, human, masked and split outputs
 * alike -- because a decontamination tool must not alter the reads it returns.  The mask byte the classifier sees is 'N'
 * (kraken2: 'x'; the scanner cannot tell them apart).
 *
 * nh_quality_mask_device: the pass itself, asynchronous on `stream`, on the engine's device.  Sequence i is
 * d_text[d_seq_starts[i], +d_seq_lens[i]) (uint64 / uint32, the arrays of nh_classify_records_device), its qualities start at
 * d_qual_starts[i] (uint64; all-ones: no qualities, the sequence is copied unmasked).  d_out[d_seq_starts[i], +d_seq_lens[i])
 * receives the masked bases; no other byte of d_out is written, so nh_classify_records_device can be launched on d_out with the
 * same starts and lengths.  A record whose quality line is not exactly as long as its sequence (a '\n' among the bytes, or a
 * byte above ' ' behind them) or whose ranges leave the text is not written at all and sets a sticky error bit (value 32) that
 * fails the engine's next blocking call or run.  Q = 0 masks nothing (bytes below '!' excepted).
 */
/* out must be 4-byte aligned and text_len + 8 bytes long; d_masked (may be NULL): one uint64 the kernel adds to */
int nh_quality_mask_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts,
                           const void *d_seq_lens, const void *d_qual_starts, uint64_t n_seq,
                           uint32_t min_base_quality, void *d_out, void *d_masked, void *stream);
/* nh_run_ex with kraken2's --minimum-base-quality; extras may be NULL (plain nh_run); 0 = exactly nh_run_ex.  Above 93 (the
 * highest printable quality is '~'): NH_EINVAL before any device is touched.  A FASTQ record whose quality line is not as long
 * as its sequence ends a kraken2 run; here, with Q > 0, it fails the run with NH_EIO and a message that names both lengths. */
int nh_run_minq(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, nh_stats *stats);
int nh_run_engine_minq(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras,
                       uint32_t min_base_quality, nh_stats *stats);

/*
 * Read statistics (--read-stats): the QC summary a user would otherwise get from a second pass over the input and the output
 * (seqkit stats -a, NanoPlot), counted in the run itself, on the device, for three sets of reads -- all the reads read
 * ("input"), the non-human ones and the human ones -- per mate.  The sets follow the CALLS, whatever the run writes: their
 * naming does not depend on keep_human, mask or the human outputs.  The bases are the input's, also in a run with a minimum
 * base quality (the class counts then follow the masked calls) and in a masked run.
 * THE DEFINITIONS ARE THIS PROJECT'S OWN, NOT seqkit's: the median is the lower nearest-rank element (0-based index
 * ceil(n/2) - 1 of the ascending lengths; seqkit averages the two middle ones); N50 is the largest L such that the reads of
 * length >= L hold at least half of the set's bases (2 * sum >= bases); gc counts G, C, g, c over ALL bases of the set (not over
 * A, C, G, T only); other counts the bytes not in ACGTacgt; qhist[q] counts the bases whose quality byte, read as unsigned, less
 * 33, clamped to 0 .. 93, is q, over the records that have qualities (FASTQ).  A read of length 0 is a read.  All of it is
 * integer sums, minima and maxima: bit-exact, whatever the batches, devices or order.
 */
#define NH_RS_QBINS 94
typedef struct {
    uint64_t reads, bases, min_len, max_len, gc, other, qual_reads, qual_bases, qhist[NH_RS_QBINS];
} nh_read_class;
typedef struct {
    nh_read_class cls[2][2];   /* [0 non-human | 1 human][mate]; a class without reads: all 0 (min_len too) */
    uint64_t median_len[3][2]; /* [0 input | 1 non-human | 2 human][mate]; 0 for an empty set */
    uint64_t n50[3][2];
    int32_t mates, reserved;
} nh_read_stats;
/* The counting pass itself, asynchronous on `stream`, on the engine's device: the arrays of nh_quality_mask_device (n_frag
 * fragments; with NH_FLAG_PAIRED in flags sequences 2f and 2f + 1 are the mates of fragment f) and the classifier's results:
 * sequence i goes to class d_results[i / mates].call != 0, mate i % mates.  d_acc: four nh_read_class in HBM, [class][mate], that
 * the kernel ADDS to (two launches accumulate); the caller zeroes them and sets the four min_len words to all-ones.  d_text must
 * be 4-byte aligned, readable for text_len + 8 bytes, text_len below 4 GiB, the sequences of a launch disjoint.  A record whose
 * quality line is not as long as its sequence or whose ranges leave the text is not counted and sets the sticky error bit of
 * nh_quality_mask_device (value 32).  max_workgroups: 0, or a cap on the grid (each workgroup loops over its share of the
 * sequences and adds its totals to d_acc once). */
int nh_read_stats_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                         const void *d_qual_starts, const void *d_results, uint64_t n_frag, uint32_t flags, void *d_acc,
                         uint32_t max_workgroups, void *stream);
/* nh_run_minq with read statistics: read_stats_path (may be NULL) receives the table -- plain text whatever out_codec is, a header
 * line and a row per set (input, nonhuman, human) and mate, tab-separated:
 *   set mate reads bases min_len mean_len median_len max_len N50 gc_pct other_bases q20_pct q30_pct mean_qual
 * integers as integers, ratios as %.2f ("NA" where the denominator is 0), mean_qual = -10 log10(sum qhist[q] 10^(-q/10) /
 * qual_bases) -- and `out` (may be NULL) the numbers.  Both NULL: exactly nh_run_minq.  extras may be NULL.  A path that names an
 * input or another output of the run (the same path, or the same device and inode): NH_EINVAL before any device is touched.
 * With statistics on, a FASTQ record whose quality line is not as long as its sequence fails the run with NH_EIO, as with
 * min_base_quality > 0.  The table is written when the run has succeeded. */
int nh_run_rstats(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                  nh_read_stats *out, nh_stats *stats);
int nh_run_engine_rstats(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                         const char *read_stats_path, nh_read_stats *out, nh_stats *stats);
/* the table of nh_run_rstats from the numbers; host only, no device needed */
int nh_read_stats_write(const nh_read_stats *stats, const char *path);

/*
 * Per-taxon outputs (--taxon-out): nh_run_rstats that also sorts the classified records by clade, in the same pass.  Up to
 * NH_MAX_TAXON_OUTS selectors, each a taxid of the database's taxonomy or NH_TAXON_OTHER, each with a file per mate.  A classified
 * fragment goes to exactly one selector: the deepest selected taxon that is its call or an ancestor of its call; where none is, to
 * NH_TAXON_OTHER if that was given, else to no per-taxon file.  Unclassified fragments go to none.  The record written is byte for
 * byte the one nh_run writes with keep_human = 1 (" kraken:taxid|<id>" suffix, normalised), in input order within each file, in the
 * run's out_codec; a selector without reads gets an empty file of that codec.  `fragments` receives the selector's fragments.
 * Every other output and the stats are exactly those of nh_run_rstats with the same arguments; n_outs == 0 IS nh_run_rstats.
 * The records are sorted in the GPU's memory (nh_split.hip, k_tout_*): one more copy of the classified text per batch in HBM,
 * whatever the number of selectors.  Taxid 1 (the root) is a selector like any other: everything not selected deeper.
 * NH_EINVAL, before any device is touched and with no file created: n_outs above NH_MAX_TAXON_OUTS; outs NULL with n_outs > 0; a
 * taxid given twice; out1 NULL or empty; out2 given without in2 or missing with in2; keep_human set; a path that names an input (the
 * same path, or the same device and inode), out1, out2, a human output, kraken_output, report, calls, human_ids, the read statistics
 * table or another per-taxon file; every check of nh_run_rstats.  A taxid that the opened database's taxonomy does not hold:
 * NH_EINVAL with the taxid in the message, once the database is open, before any input is read or any output created.
 */
#define NH_MAX_TAXON_OUTS 8
#define NH_TAXON_OTHER 0u /* selector: classified, in no other selector's clade */
typedef struct {
    uint64_t taxid;          /* external (NCBI) id, or NH_TAXON_OTHER */
    const char *out1, *out2; /* out2: the second mate's file, NULL for single-end input */
    uint64_t fragments;      /* out: fragments written to this selector */
} nh_taxon_out;
int nh_run_taxa(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_stats *stats);
int nh_run_engine_taxa(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_stats *stats);

/*
 * Minimizer data (--report-minimizer-data, --minimizer-table; nohuman_amd/csrc/nh_mdata.hip): per taxon, how many
 * minimizer hits the reads of a run produced and how many DISTINCT database minimizers they were -- kraken2's
 * --report-minimizer-data, the KrakenUniq idea: many reads on few distinct minimizers is the signature of a false positive.
 * DEFINITIONS.  A HIT GROUP is what the classifier counts in nh_result.hit_groups: a run start of the scanner whose look-up found a
 * cell with a non-zero value.  A run start is a minimizer that differs from the fragment's previous non-ambiguous minimizer; the
 * previous minimizer survives ambiguous stretches and is reset at mate 2 exactly when nh_options.reset_per_mate is set.  For every
 * hit group, over ALL fragments of the run and both mates, classified or not, let t be the value found and c the index of the cell
 * where the key matched.  Per taxonomy node t:
 *   minimizers_own[t]  hit groups with value t (kraken2's n_kmers)
 *   distinct_own[t]    distinct cells c among them (kraken2: a HyperLogLog estimate of the distinct minimizers; here exact)
 *   db_cells_own[t]    cells of the table whose value is t (kraken2-inspect's number)
 *   *_clade[t]         the sum over t's subtree, reads_* as the report has them
 * Every database minimizer lives in exactly one cell, so one bit per cell counts exactly: the numbers do not depend on batches,
 * streams or devices, and clades sum.  Two minimizers that the compact hash cannot tell apart (one compacted key inside one probe
 * run) are one entry of the database and count once, as the classifier treats them.  With a minimum base quality the pass reads
 * the masked sequences the classifier reads.  Always: sum_t minimizers_own[t] == sum over the fragments of hit_groups;
 * distinct_own[t] <= min(minimizers_own[t], db_cells_own[t]); sum_t db_cells_own[t] == nh_db_info.size.
 * The pass is one of its own behind the classifier, launched only when asked for; it costs capacity / 8 bytes of device memory a
 * device.  It supports the default geometry (k = 35, l = 31, the default spaced-seed and toggle masks, revcom_version 1,
 * minimum_acceptable_hash_value 0) and linear probing: any other database is NH_EDB with the field in the message, linear_probing
 * = 0 in the engine's options NH_EINVAL -- once the database is open, before any input is read or any output created.
 */
typedef struct {            /* 72 bytes */
    uint64_t taxid;         /* external id */
    uint64_t reads_clade, reads_own, minimizers_clade, minimizers_own, distinct_clade, distinct_own, db_cells_clade, db_cells_own;
} nh_taxon_minimizers;
typedef struct {            /* 32 bytes */
    uint32_t struct_size;   /* sizeof(nh_minimizer_data) of the caller */
    int32_t in_report;      /* not 0: args->report gets kraken2's two extra columns (below) */
    const char *table;      /* the project's own table (below), NULL = none */
    nh_taxon_minimizers *taxa; /* NULL, or receives one entry a node in internal-id order from the root (at most taxa_cap) */
    uint32_t taxa_cap, n_taxa; /* n_taxa: out, nodes of the taxonomy without the sentinel */
} nh_minimizer_data;
/* nh_run_taxa with minimizer data; any kind of run.  md NULL, or md with in_report 0, table NULL and taxa NULL: exactly nh_run_taxa,
 * nothing allocated or launched.
 * in_report: columns 4 and 5 of the report become minimizers_clade and distinct_clade --
 *   pct <TAB> reads_clade <TAB> reads_own <TAB> minimizers_clade <TAB> distinct_clade <TAB> rank <TAB> taxid <TAB> name
 * -- the `unclassified` line carries 0 and 0, the lines and their order are those of the report without it (a clade without reads is
 * not printed).  A recollection of kraken2's reports.cc, unpinned like the rest (PINDAY.md).
 * table: plain text, a header line, then a row for every node with reads_clade > 0 or minimizers_clade > 0 in internal-id order,
 * tab-separated:  taxid name reads_clade reads_own minimizers_clade minimizers_own distinct_clade distinct_own db_cells_clade
 * db_cells_own coverage_pct,  coverage_pct = 100 distinct_clade / db_cells_clade as %.4f, "NA" where the denominator is 0.  Written
 * when the run has succeeded.
 * NH_EINVAL before any device is touched, nothing created: struct_size too small; in_report without args->report; table empty;
 * table naming an input or any other output of the run (the same path, or the same device and inode); taxa with taxa_cap 0; every
 * check of nh_run_taxa.  NH_EOOM (the bytes in the message) where the bitmap cannot be allocated. */
int nh_run_mdata(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                 nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_stats *stats);
int nh_run_engine_mdata(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                        const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                        nh_minimizer_data *md, nh_stats *stats);
/* The two passes themselves, asynchronous on `stream`, on the engine's device.  bytes: of the bitmap, 4 ceil(capacity / 32). */
int nh_minimizer_marks_bytes(const nh_engine *e, uint64_t *bytes);
/* The sequences are addressed as in nh_classify_records_device (d_text 4-byte aligned and readable for text_len + 8 bytes; with
 * NH_FLAG_PAIRED sequences 2f and 2f + 1 are the mates of fragment f).  Every hit group sets the bit of its cell in d_marks (bit
 * c & 31 of word c / 32; bits at and above the capacity are never set) and adds 1 to d_groups[value] (node_count uint64).  The
 * kernels ADD: the caller zeroes d_marks and d_groups; two launches accumulate. */
int nh_minimizer_mark_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts,
                             const void *d_seq_lens, uint64_t n_frag, uint32_t flags, void *d_marks, void *d_groups, void *stream);
/* d_counts[value] (node_count uint64, zeroed by the caller) grows by the marked cells of that value; d_marks NULL: by all its cells. */
int nh_minimizer_count_device(nh_engine *e, const void *d_marks, void *d_counts, void *stream);

/*
 * Host selection (--host-taxid, --keep-taxid; nohuman_amd/csrc/nh_host.hip): which classified fragments count as
 * HOST.  Without a selection every classified fragment does (call != 0) -- right while a database holds one taxon, wrong for a
 * database of several (a manifest build with a spike-in or a decoy, a standard kraken2 database).  With one, there are two lists
 * of external taxids, host and keep, and a classified fragment is a host fragment iff the DEEPEST listed taxon that is its call or
 * an ancestor of its call is a host taxid (the rule of the per-taxon outputs above).  No listed ancestor: not host.  An unclassified
 * fragment is never host.  A classified fragment that is not host is SPARED: every output treats it exactly as it treats an
 * unclassified fragment.  host {1} is the behaviour without a selection.
 * What follows the selection: out1 / out2 (the non-host fragments; keep_human: the host fragments, the suffix carrying the true
 * call; a spared record is written as an unclassified one is, raw where the input allows, no " kraken:taxid" suffix), the human
 * outputs, the mask (N over host fragments only), human_ids, the classes of the read statistics.  What does NOT: nh_result, the
 * calls table, kraken_output, the report, nh_stats, the per-taxon outputs and the minimizer data report the true calls, byte for
 * byte as the same run without a selection writes them.
 * The pass is one kernel behind the classifier (k_host_filter: a second array of results with call = 0 where the fragment is not
 * host), launched only when a selection is given; without one nothing is allocated or launched.
 */
#define NH_MAX_HOST_TAXA 16            /* host + keep together */
typedef struct {
    uint32_t struct_size;              /* sizeof(nh_host_filter) of the caller */
    uint32_t n_host, n_keep, reserved;
    const uint64_t *host_taxids, *keep_taxids;   /* external ids */
    uint64_t host_fragments, spared_fragments;   /* out: host_fragments + spared_fragments == nh_stats.classified */
} nh_host_filter;
/* nh_run_mdata with a host selection; any kind of run (keep_human and per-taxon outputs included).  hf NULL, or n_host == 0 and
 * n_keep == 0: exactly nh_run_mdata.  NH_EINVAL before any device is touched, nothing created: struct_size too small; n_keep > 0
 * with n_host == 0; more than NH_MAX_HOST_TAXA taxids together; a NULL list with a non-zero count; taxid 0; a taxid given twice,
 * within or across the lists; every check of nh_run_mdata.  A taxid that the opened database's taxonomy does not hold: NH_EINVAL
 * with the taxid in the message, once the database is open, before any input is read or any output created. */
int nh_run_host(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf,
                nh_stats *stats);
int nh_run_engine_host(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                       nh_minimizer_data *md, nh_host_filter *hf, nh_stats *stats);
/* The host-node table of a selection from a taxo.k2d image; host only, no device needed: host_of[i] = 1 where node i (internal id)
 * is host, else 0; entry 0 is 0.  *n_nodes receives the taxonomy's node count (sentinel included); cap: entries of host_of.
 * NH_EINVAL: the selection's own errors (above), a taxid the taxonomy does not hold, cap below the node count.  NH_EDB: an image
 * that is not a taxonomy, is truncated, or whose parents do not lie below their children. */
int nh_host_table_image(const void *taxo, size_t taxo_len, const nh_host_filter *hf, uint8_t *host_of, uint64_t cap, uint64_t *n_nodes);
/* The pass itself, asynchronous on `stream`, on the engine's device: d_res_out[i] = d_res_in[i] with call = 0 where
 * d_host_of[call] is 0 (n nh_result each; d_res_out == d_res_in is allowed; d_host_of: n_nodes bytes).  d_counts (may be NULL): two
 * uint64 {host, spared} the kernel ADDS to.  A call >= n_nodes is never used as an index: it becomes 0, is counted nowhere, and
 * sets a sticky error bit (value 128) that fails the engine's next blocking call or run with NH_EDEVICE.  n == 0 launches nothing. */
int nh_host_filter_device(nh_engine *e, const void *d_res_in, void *d_res_out, uint64_t n, const void *d_host_of, uint64_t n_nodes,
                          void *d_counts, void *stream);

/*
 * Database builder (--build-db; nohuman_amd/csrc/nh_build.hip): FASTA in, a kraken2 database directory out (hash.k2d, opts.k2d,
 * taxo.k2d), built on the GPU.  What kraken2-build does for ONE taxon at the default geometry, and nothing more: k = 35, l = 31,
 * the default spaced-seed and toggle masks, revcom_version 1, dna_db 1, minimum_acceptable_hash_value 0, linear probing -- the
 * geometry of the HPRC databases and the one the classifier's fast path is built for.  Low-complexity masking (kraken2-build's
 * dustmasker / k2mask step) is off unless mask_low_complexity is set: then every batch of text is masked on the device before its
 * minimizers are taken (symmetric DUST, window 64, threshold 2.0: see nh_dust_mask below), a masked base is an N to the scanner,
 * and masked_bases counts every input base that was masked, once (one more batch of device memory is held).  A k-mer is
 * skipped exactly when the classifier's scanner calls it ambiguous under the rule in force (NH_AMBIGUITY_DEFAULT,
 * NOHUMAN_OPT_AMBIGUITY_RULE honoured); bases are read as the classifier reads them, lowercase included.
 * taxo.k2d: node 0 the null sentinel, node 1 "root" (external id 1), node 2 the taxon (external `taxid`, child of 1); every
 * inserted value is 2, value_bits 2, key_bits 30.
 * The text goes to the device in batches of bounded size, every sequence cut into pieces of piece_kmers k-mers that overlap by
 * k - 1 bases, a wave per piece.  Two passes over the input: COUNT the distinct minimizers exactly in a device set of 64-bit keys
 * (it grows by doubling and stays at most half full: 16 bytes of HBM per distinct minimizer at the least, 48 at the most while it
 * grows), which gives capacity = ceil(distinct_minimizers / load_factor); INSERT into a zeroed table (CompareAndSet, linear
 * probing, 64-bit cell indices).  Which key sits in which cell of a probe run depends on the order of arrival, as in kraken2's
 * threaded build; the set of occupied cells and the sorted cells do not.  The three files are written under temporary names in
 * out_dir and renamed into place when all three are complete; any failure removes them and leaves out_dir as it was.
 * NH_EINVAL before any device is touched: struct_size too small; n_fasta 0 or a NULL path; out_dir NULL; load_factor outside
 * (0, 0.95]; taxid 1; a database already in out_dir without `force`; an input that lies in out_dir under one of the three names.
 * NH_EIO: an input that cannot be read.  NH_EDB: no k-mer at all in the input.  NH_EOOM: the counting set or the table cannot be
 * allocated (the message names `capacity` as the way round the set).  NH_ECAPACITY: a given `capacity` that the minimizers fill.
 * FASTQ inputs are accepted (their sequences are read).  One device; no multi-GPU build.
 *
 * Several taxa (taxa_file; nh_build.hip, nh_taxa.h): a manifest with one taxon a line,
 *     taxid <TAB> parent taxid <TAB> name [<TAB> FASTA path]...
 * `#` lines and empty lines skipped, CRLF tolerated; a line without a path is an inner node, a node with children may carry
 * sequences too; parent 1 is the root, which is implicit and never a line; relative paths resolve against the manifest's
 * directory; every rank is "no rank".  Internal ids: 0 the null sentinel, 1 the root, then breadth first with the children of a
 * node in ascending taxid.  At most 4095 taxa, 4096 nodes with the root.  value_bits is the smallest b >= 1 with 2^b >= nodes + 1
 * (the sentinel takes a value: 12 bits up to 4094 taxa, 13 at 4095), key_bits = 32 - value_bits.  A minimizer found in two
 * taxa is stored as their lowest common ancestor (kraken2-build's CompareAndSet with taxonomy.LowestCommonAncestor), merged on the
 * device with compare-and-swap; the files are read in internal-id order.  taxon_stats receives, per node, what its own files
 * held and the cells of the finished table that hold it (counted on the device); stats->taxa the nodes without the sentinel.
 * NH_EINVAL before any device is touched, out_dir as it was, every message with the file and the line: a line with fewer than
 * three fields; a taxid that is not a number, is 0 or 1, or appears twice; an empty name; a parent that is neither 1 nor a line; a
 * cycle; no FASTA in the whole file; one FASTA given twice (by real path); more than 4095 taxa; the manifest or a listed FASTA
 * being one of out_dir's three files; taxa_file together with fasta / n_fasta, a non-zero taxid or a taxon_name.  NH_EIO: a
 * manifest or a listed FASTA that cannot be read.  A build without taxa_file writes its three files as it always did.
 */
typedef struct {
    uint64_t taxid;              /* external id of the node (1 for the root) */
    uint64_t sequences, bases, kmers; /* of the node's own FASTA files (not of its descendants) */
    uint64_t cells;              /* cells of the finished table that hold this node; the sum over all nodes is `size` */
} nh_build_taxon_stats;
typedef struct {
    uint32_t struct_size;        /* sizeof(nh_build_args) of the caller */
    uint32_t n_fasta;
    const char *const *fasta;    /* plain or gzip FASTA, wrapped lines allowed, any number of records */
    const char *out_dir;         /* receives hash.k2d, opts.k2d, taxo.k2d (created if missing) */
    uint64_t taxid;              /* external id of the one taxon; 0 = 9606 */
    const char *taxon_name;      /* NULL = "Homo sapiens" when taxid is 9606, else "taxon<taxid>" */
    double load_factor;          /* 0 = 0.7 (kraken2-build's default, a recollection: unpinned like SURVEY.md A) */
    uint64_t capacity;           /* 0 = ceil(distinct_minimizers / load_factor); else used as given, counting pass skipped */
    uint64_t piece_kmers;        /* 0 = default (1984, 16 tiles); k-mers per piece (tests set it small) */
    int32_t device;
    uint32_t threads;            /* host reader workers (gzip inputs) */
    int32_t force;               /* 0: refuse an out_dir that already holds any of the three files */
    int32_t reserved0;           /* (the tail padding of the first layout: never read) */
    /* ---- behind NH_BUILD_ARGS_SIZE_V1 */
    int32_t mask_low_complexity; /* not 0: mask low-complexity sequence before the minimizers are taken */
    int32_t reserved1;
    /* ---- behind NH_BUILD_ARGS_SIZE_V2 */
    const char *taxa_file;       /* not NULL: the taxa manifest of a build of several taxa (below); excludes fasta / n_fasta,
                                  * taxid and taxon_name */
    nh_build_taxon_stats *taxon_stats; /* NULL, or receives one entry a node in internal-id order, starting at the root */
    uint32_t taxon_stats_cap;    /* entries of taxon_stats: at most that many are written */
    uint32_t reserved2;
} nh_build_args;
typedef struct {
    uint64_t sequences, bases, kmers, ambiguous_kmers, distinct_minimizers, capacity, size;
    double seconds_read, seconds_count, seconds_insert, seconds_write;
    /* ---- behind NH_BUILD_STATS_SIZE_V1 */
    uint64_t masked_bases;       /* input bases turned into N by the masking (as the inserting pass counted them) */
    double seconds_mask;         /* the masking kernel alone, both passes (a part of seconds_count + seconds_insert) */
    /* ---- behind NH_BUILD_STATS_SIZE_V2 */
    uint64_t taxa;               /* nodes of the taxonomy without the sentinel: 2 for a build of one taxon */
} nh_build_stats;
/* Both structs have grown at their ends, twice, and the library tells the caller's layout by nh_build_args.struct_size alone:
 *   struct_size <  NH_BUILD_ARGS_SIZE_V1 (80)     NH_EINVAL
 *   struct_size <  NH_BUILD_ARGS_SIZE_V2 (88)     the first layout: fields through `force` are read, no masking, and only the first
 *                                                 NH_BUILD_STATS_SIZE_V1 (88) bytes of *stats are written -- a caller compiled
 *                                                 against the first header passes a buffer of that size
 *   struct_size <  sizeof(nh_build_args) now      the second layout: mask_low_complexity is read too, and the first
 *                                                 NH_BUILD_STATS_SIZE_V2 (104) bytes of *stats are written
 *   struct_size >= sizeof(nh_build_args) now      taxa_file and taxon_stats are read and the whole nh_build_stats is written */
#define NH_BUILD_ARGS_SIZE_V1 80u
#define NH_BUILD_STATS_SIZE_V1 88u
#define NH_BUILD_ARGS_SIZE_V2 88u
#define NH_BUILD_STATS_SIZE_V2 104u
int nh_build_db(const nh_build_args *args, nh_build_stats *stats);
/* Every check nh_build_db makes before it touches a device, and no more: the same return code and message, nothing created, no
 * device needed.  With the present layout and a taxa_file, stats->taxa and the taxid of every taxon_stats entry (the internal-id
 * order of the manifest's nodes) are written as well; stats may be NULL. */
int nh_build_check(const nh_build_args *args, nh_build_stats *stats);

/*
 * Extension of an existing database (--build-db OUT --extend-db BASE; nh_build.hip, nh_extend.hip): the taxa of
 * `b` (a taxa_file, or the one-taxon form fasta / taxid / taxon_name) are added to the database in x->base_dir and the result is
 * written to b->out_dir.  Only the three .k2d files of the base are needed, not the sequences it was made from: the table is
 * loaded, re-keyed in place for the merged taxonomy and the new minimizers are inserted into its free cells.
 * The 64-bit hash of a stored minimizer is not in hash.k2d, so the capacity cannot change: b->capacity must be 0, and
 * b->load_factor is the highest load the RESULT may have (0 = 0.95).  out_dir, force, mask_low_complexity, piece_kmers, device,
 * threads and taxon_stats mean what they mean to nh_build_db.
 * Taxonomy: a manifest line's parent may be 1, another line or an external id of the base; a line whose taxid the base holds adds
 * its FASTA files to that node (its parent field must name the base's parent; the base's name stays); the one-taxon form is a
 * child of the root or the existing node of that taxid.  The merged tree is numbered as nh_build_db numbers any tree, value_bits
 * is the larger of the base's and what the merged nodes need, names are written in internal-id order and the rank strings of the
 * base are kept ("no rank" for added nodes).  opts.k2d is the base's, byte for byte.  Extending a database made by nh_build_db
 * gives the taxo.k2d and opts.k2d of a build of all taxa in one go, and the same table (occupied cells, sorted cell words).
 * Where the value field widens by d bits every stored key loses its low d bits.  Two cells of one probe run whose keys become
 * equal that way both receive the lowest common ancestor of their values; the later one can no longer be reached by a look-up
 * and cannot be deleted: shadowed_cells counts such cells, which stay in the table and in `size`.
 * NH_EINVAL before any device is touched, out_dir as it was: what nh_build_db refuses; base_dir NULL or without one of the three
 * files; out_dir the same directory as base_dir; capacity not 0; a parent that is neither 1, a line nor in the base; an existing
 * taxid under another parent; more than 4096 merged nodes.  NH_EDB: a base file with a bad magic or truncated; key_bits +
 * value_bits not 32; capacity 2^33 or more; an opts.k2d of another geometry than nh_build_db's; a base taxonomy with one
 * external id twice; on the device, a cell whose value is no node of the base or a count of non-empty cells other than the
 * header's size.  NH_ECAPACITY, nothing written: the table fills, or size / capacity of the result exceeds the ceiling.
 * The base directory is never opened for writing.
 */
typedef struct {
    uint32_t struct_size;      /* sizeof(nh_extend_args) of the caller */
    uint32_t base_cells_cap;   /* entries of base_cells */
    const char *base_dir;      /* the database to extend: read, never written */
    uint64_t *base_cells;      /* NULL, or per node of the NEW taxonomy in internal-id order from the root: cells of the
                                * base table that held it before anything was added (0 for an added node) */
} nh_extend_args;
typedef struct {
    uint32_t struct_size, reserved; /* struct_size: sizeof(nh_extend_stats) of the caller */
    uint64_t base_size, base_nodes, base_value_bits; /* base_nodes: nodes of the base's taxonomy, the sentinel included */
    uint64_t nodes_added, cells_added;  /* cells_added = size - base_size */
    uint64_t shadowed_cells;            /* cells that are not the first of their key in their probe run (above) */
    double load;                        /* size / capacity of the result */
    double seconds_load, seconds_rekey; /* base table to the device; the re-key passes alone (events) */
} nh_extend_stats;
int nh_extend_db(const nh_build_args *b, const nh_extend_args *x, nh_build_stats *bs, nh_extend_stats *xs);
/* Every check nh_extend_db makes before it touches a device: the same codes and messages, nothing created.  bs->taxa, the taxid
 * of every taxon_stats entry (the new internal-id order) and xs->base_nodes, nodes_added and base_value_bits are written. */
int nh_extend_check(const nh_build_args *b, const nh_extend_args *x, nh_build_stats *bs, nh_extend_stats *xs);

/*
 * A build that leaves out the minimizers other sequences carry too (--build-db OUT --exclude FILE; nh_build.hip):
 * with H the distinct minimizers of the host inputs of `b` (of the masked sequences where mask_low_complexity is set) and X those of
 * the files of `x` -- read by the same parser, plain or gzip, FASTA or FASTQ, any number of records, scanned under the same
 * ambiguity rule and never masked -- the database written is the one nh_build_db would make of a host whose minimizer set is
 * H \ X.  Nothing of the exclusion input is stored, so it may be of any size, and the result is an ordinary database that needs no
 * flag where it is used.  Exclusion works on the 62-bit minimizers; the table keeps 30-bit keys (fewer with many taxa), so a
 * look-up of an excluded minimizer still finds a kept one of the same key on its probe path, as in any kraken2 table.
 * The counting pass runs even where b->capacity is given (the exclusion pass flags what it finds in that pass's set; a given
 * capacity is then used as it is, NH_ECAPACITY as ever), bs->distinct_minimizers is |H|, bs->capacity is
 * ceil(|H \ X| / load_factor) unless given, xs->excluded_minimizers is |H and X|, exact whatever the order, batching or repetition
 * of the exclusion input, and kept_minimizers = distinct_minimizers - excluded_minimizers.  With a taxa_file H is the union over
 * the taxa: a minimizer in X is stored under no taxon.  x == NULL or x->n_fasta == 0 is nh_build_db(b, bs), to the byte.
 * NH_EINVAL before any device is touched, nothing created: what nh_build_db refuses; a struct_size below nh_exclude_args' or
 * nh_exclude_stats'; a NULL path; an exclusion file that is one of out_dir's three files, that is also a host input or a FASTA of
 * the manifest (by real path), or that is given twice.  NH_EIO, out_dir as it was: an exclusion file that cannot be read or
 * parsed (the message names it).  NH_EDB, nothing written: H \ X is empty.  Not available to nh_extend_db, which has no counting set.
 */
typedef struct {
    uint32_t struct_size;      /* sizeof(nh_exclude_args) of the caller */
    uint32_t n_fasta;
    const char *const *fasta;  /* the exclusion files */
} nh_exclude_args;
typedef struct {
    uint32_t struct_size, reserved;  /* struct_size: sizeof(nh_exclude_stats) of the caller */
    uint64_t sequences, bases, kmers, ambiguous_kmers; /* of the exclusion input */
    uint64_t lookups;                /* run-start minimizers of the exclusion input looked up in the set */
    uint64_t excluded_minimizers, kept_minimizers;
    double seconds_read, seconds_exclude; /* reading the exclusion files; the pass on the device (copies, kernels, waits) */
} nh_exclude_stats;
int nh_build_db_exclude(const nh_build_args *b, const nh_exclude_args *x, nh_build_stats *bs, nh_exclude_stats *xs);
/* Every check nh_build_db_exclude makes before it touches a device: the same codes and messages, nothing created.  With x == NULL
 * or x->n_fasta == 0 it is nh_build_check(b, bs). */
int nh_exclude_check(const nh_build_args *b, const nh_exclude_args *x, nh_build_stats *bs, nh_exclude_stats *xs);

/*
 * Low-complexity masking of a host buffer in place, by the kernel and the launch code the builder uses (nh_dust.hip): symmetric
 * DUST (Morgulis et al. 2006) at dustmasker's defaults, window 64 bases and score threshold 2.0, neither an option.  Each segment
 * [seg_start[i], +seg_len[i]) of text is one sequence: it is split into maximal runs of ACGTacgt (case carries no meaning; any
 * other byte ends a run and is never touched), t_i is the triplet of bases i, i+1, i+2 of a run, the triplet interval
 * [i, i+d] scores r / d with r = sum over the 64 triplets of n (n - 1) / 2, an interval is perfect when d <= 61, 10 r > 20 d and
 * no sub-interval scores higher, and the bases of every perfect interval become N.  No triplet spans two runs or two
 * segments.  Integer arithmetic throughout.  Bytes outside the segments are not touched; segments should not overlap (a base in two of them is masked by
 * either and counted twice).  *masked_bases (may be NULL) receives the number of bases turned.
 * NH_EINVAL, before any device is touched and with the buffer unchanged: text NULL; a NULL list with n_seg > 0; a segment that
 * leaves [0, n_bytes).  With no base in any segment the call succeeds without a device.
 * Device memory: the whole buffer twice (the text as given, which the kernel reads, and the copy it masks) and 24 bytes for
 * every 900 bases of a segment; NH_EOOM when that cannot be allocated -- a genome larger than that is masked a part at a time,
 * its sequences as the segments of each part.
 */
int nh_dust_mask(int32_t device, char *text, uint64_t n_bytes, const uint64_t *seg_start, const uint64_t *seg_len, uint64_t n_seg,
                 uint64_t *masked_bases);

/*
 * Reads classified with their low-complexity stretches masked (--dust-reads; nh_dust.hip).  A table that holds the
 * minimizers of poly-A tails or of (AC)n / (CAG)n microsatellites -- any database built without masking, of which the user may
 * only have the three .k2d files -- calls a microbial read that carries such a stretch host.  With the pass enabled EVERY
 * sequence of every batch, both mates, FASTA as well as FASTQ, is masked by the symmetric DUST of nh_dust_mask above, each sequence
 * ON ITS OWN (one segment: no triplet spans two sequences), window 64 and threshold 2.0 fixed, and the classifier and the minimizer
 * data's marks read the masked copy, in which a masked base is 'N', an ambiguous base to the scanner.
 * Only classification changes: nh_result, the hit list of kraken_output (a masked stretch shows as "A:n"), the calls table, the
 * report, the three totals, and what follows from the calls; total_kmers, the lengths and total_bases do not.
 * THE DEVIATION OF nh_run_minq, FOR THE SAME REASON: EVERY RECORD WRITTEN KEEPS THE INPUT'S BASES, in every output -- a
 * decontamination tool does not alter the reads it returns.  With a minimum base quality as well the classifier sees the union of
 * the two masks; DUST is computed on the input's bases, not on the quality-masked ones.  Not enabled: nothing is allocated, copied
 * or launched, and every output is byte for byte that of nh_run_host.
 *
 * nh_run_dust / nh_run_engine_dust: nh_run_host with the pass.  rd NULL or rd->enable == 0: exactly nh_run_host.  A struct_size
 * smaller than the struct: NH_EINVAL before any device is touched, nothing created.  masked_bases receives the bases masked over
 * the whole run, all devices summed (0 where the run fails after its arguments and its database were accepted; untouched before).
 *
 * nh_dust_reads_device: the pass itself on the engine's device, on `stream`.  Sequence i is d_text[d_seq_starts[i],
 * +d_seq_lens[i]) (uint64 / uint32, the arrays of nh_classify_records_device, in any order).  d_out (text_len bytes) ALREADY HOLDS
 * the sequences at the same offsets -- a copy of the text, or nh_quality_mask_device's output; every masked base becomes 'N' there
 * and no other byte of it is written; d_text is only read.  d_masked (may be NULL): one uint64 the kernel adds to.  The entry
 * allocates its scratch (8 bytes a sequence), waits for the stream and frees it.  n_seq == 0 launches nothing.  A sequence that
 * leaves [0, text_len) is skipped -- nothing of it is read or written, the others are masked -- and sets a sticky error bit
 * (value 512) that fails the engine's next blocking call or run with NH_EDEVICE.
 */
typedef struct {
    uint32_t struct_size;   /* sizeof(nh_read_dust) of the caller */
    uint32_t enable;        /* not 0: mask */
    uint64_t masked_bases;  /* out */
} nh_read_dust;
int nh_run_dust(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf,
                nh_read_dust *rd, nh_stats *stats);
int nh_run_engine_dust(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                       const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                       nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd, nh_stats *stats);
int nh_dust_reads_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                         uint64_t n_seq, void *d_out, void *d_masked, void *stream);

/*
 * Host intervals (--host-intervals; nh_cover.hip): WHERE in each read the host k-mers lie, as BED.  Every other
 * answer of a run is about a whole read; a 40 kb read that is half viral and half human, or a microbial read with one 300-base
 * stretch of human-like minimizers, is host as a whole.  This report alters nothing -- a decontamination tool does not alter the
 * reads it returns -- and lets `bedtools maskfasta`, `seqkit subseq --bed` or a trimmer act on it.
 *
 * HOST K-MERS.  Every sequence of the batch, both mates, FASTA as FASTQ, in the copy the classifier reads (with a minimum base
 * quality or the read DUST: the masked copy, so the intervals agree with the calls).  k-mer i (0-based, bases [i, i + k)) is a
 * host k-mer when it is not ambiguous under the ambiguity rule in force, its minimizer is looked up (a minimizer below
 * minimum_acceptable_hash_value is not, as in the classifier), the look-up finds a non-zero value v and -- a run with a host
 * selection (nh_host_filter) -- the one-byte-a-node table of that selection says v is host; without a selection every non-zero
 * value is host.
 * INTERVALS.  A base is covered when a host k-mer contains it; a sequence's intervals are its maximal runs of covered bases,
 * 0-based and half-open.  Host k-mers i < j with j <= i + k share an interval; an interval never crosses a sequence's end.  An
 * ambiguous base p splits a host stretch into [.., p) and [p + 1, ..) where no unambiguous k-mer contains it.  Under the default
 * ambiguity rule (1, kraken2's: an N costs the k - 1 k-mers that hold it in their last k - 1 bases) the k-mer that BEGINS with
 * the N is looked up like any other, so ONE N INSIDE A HOST STRETCH USUALLY STAYS COVERED and two in a row leave the first
 * uncovered; under rule 0 it takes k - l + 1.  The intervals are what the classifier's own hit list (kraken_output's fifth
 * column) says, k-mer for k-mer.  They do not depend on reset_per_mate, on the confidence, on minimum_hit_groups or on the call.
 * THE FILE is plain text, never compressed, without a header line: one line an interval,
 *     <id> \t <start> \t <end> \t <mate: 1|2> \t <external taxid of the fragment's call, 0 if unclassified> \n
 * in input order: fragment, then mate, then start.  <id> is exactly the calls table's id (a paired run drops a trailing /1 or /2).
 * A fragment without a covered base has no line, classified or not; an unclassified read with one hit group has one.  The taxid
 * is the true call, as in the calls table, not the host-filtered one.  BAM INPUT: THE COORDINATES ARE THOSE OF THE FASTQ TEXT THE
 * READER TRANSCODES TO, SO A REVERSE-STRAND RECORD IS COUNTED ON ITS REVERSE COMPLEMENT (the read as the sequencer gave it).
 * Every other output and the three totals are byte for byte what the same run writes without the file; without it nothing is
 * allocated or launched.  The pass supports the default geometry (k 35, l 31, the default masks, revcom_version 1) and linear
 * probing only: another database is refused with NH_EINVAL, the reason named, once it is open and before any input is read or any
 * output created.
 *
 * nh_run_intervals / nh_run_engine_intervals: nh_run_dust with the report.  hi NULL or hi->path NULL: exactly nh_run_dust.  A
 * struct_size smaller than the struct, an empty path, a path that names an input or any other output of the run (a per-taxon file
 * and the read statistics' table included): NH_EINVAL before any device is touched, nothing created.  fragments (those with a
 * line), intervals and covered_bases are summed over the run's devices (0 where the run fails after its arguments were accepted).
 *
 * nh_host_cover_device: the mark pass on the engine's device, on `stream`.  Sequence i is d_text[d_seq_starts[i], +d_seq_lens[i])
 * (uint64 / uint32, the arrays of nh_classify_records_device, in any order); d_text is 4-byte aligned and only read, no byte
 * behind the dword of its last byte.  d_host_of: NULL, or n_nodes bytes (nh_host_table_image).  d_cover, ceil(text_len / 32)
 * uint32 zeroed by the caller, gets bit (p & 31) of word p / 32 set for every covered byte p of the text; a word without a new
 * bit is not written.  A sequence that leaves [0, text_len) is skipped -- nothing of it is read or written -- and sets a sticky
 * error bit (value 1024) that fails the engine's next blocking call or run with NH_EDEVICE.
 * nh_cover_intervals_device: the bitmap into records {uint32 seq, start, end}, in the order of the sequence table, then by start,
 * every interval clipped to its sequence (two sequences back to back give two records).  *d_total (uint64) receives the records;
 * more than cap_records: bit 2048 is set in *error_bits (an int32 of the caller's in device memory), the total is 0 and nothing is
 * written; a sequence outside the text has no record and sets bit 1024 there.
 * Both entries allocate their scratch (8 and 4 bytes a sequence), wait for the stream and free it; n_seq == 0 launches nothing.
 */
typedef struct {
    uint32_t struct_size;    /* sizeof(nh_host_intervals) of the caller */
    uint32_t reserved;       /* 0 */
    const char *path;        /* the BED file; NULL: no report */
    uint64_t fragments;      /* out: fragments with an interval */
    uint64_t intervals;      /* out */
    uint64_t covered_bases;  /* out */
} nh_host_intervals;
int nh_run_intervals(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                     nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf,
                     nh_read_dust *rd, nh_host_intervals *hi, nh_stats *stats);
int nh_run_engine_intervals(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                            const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                            nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_stats *stats);
int nh_host_cover_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                         uint64_t n_seq, const void *d_host_of, uint64_t n_nodes, void *d_cover, void *stream);
int nh_cover_intervals_device(nh_engine *e, const void *d_cover, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                              uint64_t n_seq, void *d_intervals, uint64_t cap_records, void *d_total, void *error_bits, void *stream);

/*
 * Host bases only (--host-bases-only, --host-gap; nh_cover.hip and nh_mask.hip; tests/hitmask_model.py is the
 * specification): a masked run that writes 'N' only over the bases that host k-mers cover.  A masked run blanks a 40 kb bacterial
 * read with one 300-base human-like stretch whole; this one removes the stretch and keeps the rest of the read, in the pass that
 * already holds the text and the answer in HBM.
 *
 * COVERAGE is the host intervals' (above), bit for bit: the same mark pass, on the copy the classifier read, with the host
 * selection where the run has one.  CLOSING, gap = G: a maximal run of uncovered bases [a, b) of one sequence with a covered base
 * on each side in that sequence (a > 0, b < its length) and b - a <= G becomes covered; mates are closed separately, a run that
 * touches an end of its sequence never is, G = 0 changes nothing.  An uncovered run shorter than k between two host k-mers holds
 * no whole k-mer of its own, so nothing says it is not host: --host-gap 34 (k - 1) is the recommendation for noisy long reads.
 * OUTPUT: the run is a masked run -- extras->mask is required --, every record in input order in the forms of nh_run_mask.  A
 * HOST FRAGMENT is one whose call, after the host selection, is not 0: exactly the fragments a masked run blanks.  Byte p of each
 * mate's sequence of a host fragment is 'N' where the closed coverage is set and the INPUT's own byte elsewhere (its case kept;
 * never the quality- or DUST-masked copy); every other byte of every record is the masked run's.  Every other output, the three
 * totals and a host intervals' file of the same run (the coverage BEFORE the closing) are byte for byte those of the masked run
 * without it; not enabled, nothing is allocated or launched.
 *
 * nh_run_hostbases / nh_run_engine_hostbases: nh_run_intervals with the struct.  hb NULL or hb->enable 0: exactly
 * nh_run_intervals.  A struct_size smaller than the struct, enable without extras->mask, gap above NH_HOST_GAP_MAX (a design cap:
 * closing is for leftovers of k-mer size between error-broken stretches, not for deleting sequence): NH_EINVAL before any device is
 * touched, nothing created.  The database must be one the mark pass supports (see above): NH_EINVAL, the reason named, once it is
 * open.  host_bases (the sequence bases of host fragments, both mates), masked_bases (those written as 'N', whatever letter was
 * there) and closed_bases (the masked ones that only the closing set) are exact, summed over the run's devices, and 0 where the
 * run fails after its arguments were accepted.
 *
 * nh_cover_close_device: the closing on a bitmap laid out as nh_host_cover_device leaves it, on the engine's device, on `stream`.
 * d_closed_bases: NULL, or a uint64 in device memory the kernel adds the bases it sets to.  It waits for the stream; n_seq == 0
 * or gap == 0 launches nothing; a gap above NH_HOST_GAP_MAX is NH_EINVAL; a sequence that leaves [0, text_len) is skipped and
 * sets the sticky error bit 1024, as in nh_host_cover_device.
 */
#define NH_HOST_GAP_MAX 4096
typedef struct {
    uint32_t struct_size;   /* sizeof(nh_host_bases) of the caller */
    uint32_t enable;        /* 0: no such run */
    uint32_t gap;           /* 0 .. NH_HOST_GAP_MAX */
    uint32_t reserved;      /* 0 */
    uint64_t host_bases;    /* out */
    uint64_t masked_bases;  /* out */
    uint64_t closed_bases;  /* out */
} nh_host_bases;
int nh_run_hostbases(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                     nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf,
                     nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb, nh_stats *stats);
int nh_run_engine_hostbases(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                            const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                            nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb,
                            nh_stats *stats);
int nh_cover_close_device(nh_engine *e, void *d_cover, uint64_t text_len, const void *d_seq_starts, const void *d_seq_lens,
                          uint64_t n_seq, uint32_t gap, void *d_closed_bases, void *stream);

/*
 * Host cut (--host-cut, --host-min-piece; nh_cut.hip; tests/hostcut_model.py is the specification): a masked run
 * that CUTS the host stretches out of a host fragment and writes what is left as records of their own, where --host-bases-only
 * writes 'N' over them.  A run of 300 'N' in the middle of a 40 kb read breaks assemblers, polishers and mappers; a ligation chimera
 * should leave the run as its non-host half, not as that half with a tail of 'N'.
 *
 * COVERAGE and CLOSING are host bases only's (above), bit for bit: the mark pass on the copy the classifier read, with the host
 * selection where the run has one, closed with gap = G over the sequences of host fragments.  PIECES: the maximal runs [a, b) of
 * bases of a host fragment's sequence that the closed coverage does not cover, with b - a >= min_piece (runs that touch an end of
 * the sequence included).  A piece's RECORD: the header's first 1 + idlen bytes (the id as the read lists print it, with '@' / '>'),
 * ":<a>-<b>" in decimal (0-based, half-open: the BED's coordinates), the rest of the header, "\n", the INPUT's own bases [a, b) (their
 * case kept; never the quality- or DUST-masked copy) and, FASTQ, "\n+\n" and the qualities [a, b), "\n".  Pieces are written in
 * input order, by fragment, then by a.  A host fragment without a piece writes nothing; one without a covered base writes one piece,
 * "<id>:0-<len>".  Every other fragment is written whole, as nh_run_mask writes an unclassified record.  Every other output of the
 * run (-k, the report, the read lists, human_out1 -- the host records whole --, per-taxon outputs, the read statistics, the minimizer
 * data, the three totals, a host intervals' file: the coverage BEFORE the closing) is byte for byte the masked run's; not enabled,
 * nothing is allocated or launched.  SINGLE-END ONLY: the pieces of two mates cannot stay in step.  A FASTQ record whose quality
 * line is not as long as its sequence ends the run (NH_EIO), as with a minimum base quality: a piece's qualities are a slice.
 *
 * nh_run_hostcut / nh_run_engine_hostcut: nh_run_hostbases with the struct.  hc NULL or hc->enable 0: exactly nh_run_hostbases.  A
 * struct_size smaller than the struct, enable without extras->mask, enable together with an enabled nh_host_bases, gap above
 * NH_HOST_GAP_MAX, min_piece 0 or above 2^31 - 1, a second input or a paired BAM as in1: NH_EINVAL before any device is touched,
 * nothing created.  The database must be one the mark pass supports: NH_EINVAL, the reason named, once it is open.  The counts are
 * exact, summed over the run's devices, and 0 where the run fails after its arguments were accepted: host_bases (the sequence bases
 * of host fragments) = piece_bases (written in `pieces` pieces) + cut_bases (the closed coverage inside host sequences) + short_bases
 * (uncovered, in runs shorter than min_piece); dropped_reads (host fragments without a piece); closed_bases (as in nh_host_bases).
 *
 * nh_host_cut_device: the item list and the text builder on caller-owned device buffers, on the engine's device, on `stream`; it
 * waits for the stream.  d_text (4-byte aligned, text_len < 2^32 bytes, only read, no byte behind the dword of its last byte),
 * d_records (n x {uint32 header start, header length, qualities start, qualities length}, 16-byte aligned), d_seq_starts (uint64),
 * d_seq_lens, d_idlen (uint32), d_results (nh_result: call != 0 is a host fragment), fastq (0: FASTA records, no qualities),
 * d_cover (ceil(text_len / 32) uint32, laid out as nh_host_cover_device leaves it; a bit outside a sequence changes nothing),
 * min_piece (1 .. 2^31 - 1).  d_out receives the text, at most cap bytes, *d_total (uint64) its length; d_counts: NULL, or six
 * uint64 in device memory that are ADDED to: host_bases, pieces, piece_bases, cut_bases, short_bases, dropped_reads.  *error_bits
 * (an int32 of the caller's in device memory) gets bit 4096 for a sequence or a record's field outside the text or an id longer than
 * its header, bit 16384 for a FASTQ host record whose quality line is not as long as its sequence (nothing of such a record is
 * written), bit 8192 for a text above cap: total 0 and nothing written.
 */
typedef struct {
    uint32_t struct_size;    /* sizeof(nh_host_cut) of the caller */
    uint32_t enable;         /* 0: no such run */
    uint32_t gap;            /* 0 .. NH_HOST_GAP_MAX */
    uint32_t min_piece;      /* 1 .. 2^31 - 1; the CLI's default is 35 = k */
    uint64_t host_bases;     /* out */
    uint64_t pieces;         /* out */
    uint64_t piece_bases;    /* out */
    uint64_t cut_bases;      /* out */
    uint64_t short_bases;    /* out */
    uint64_t dropped_reads;  /* out */
    uint64_t closed_bases;   /* out */
} nh_host_cut;
int nh_run_hostcut(const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality, const char *read_stats_path,
                   nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs, nh_minimizer_data *md, nh_host_filter *hf,
                   nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb, nh_host_cut *hc, nh_stats *stats);
int nh_run_engine_hostcut(nh_engine *e, const nh_run_args *args, const nh_run_extras *extras, uint32_t min_base_quality,
                          const char *read_stats_path, nh_read_stats *read_stats, nh_taxon_out *outs, uint32_t n_outs,
                          nh_minimizer_data *md, nh_host_filter *hf, nh_read_dust *rd, nh_host_intervals *hi, nh_host_bases *hb,
                          nh_host_cut *hc, nh_stats *stats);
int nh_host_cut_device(nh_engine *e, const void *d_text, uint64_t text_len, const void *d_records, const void *d_seq_starts,
                       const void *d_seq_lens, const void *d_idlen, const void *d_results, uint64_t n, int fastq, const void *d_cover,
                       uint32_t min_piece, void *d_out, uint64_t cap, void *d_total, void *d_counts, void *error_bits, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NOHUMAN_ENGINE_H */
