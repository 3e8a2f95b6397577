// nohuman_cli.cpp -- C++ host with the observable behaviour of the reference's `nohuman` binary
// (the reference host is Rust, which cannot be built in this image): same
// flags, log lines, output naming and temp-dir contract, with the kraken2 subprocess replaced by
// nh_run() from libnohuman_engine.so.
//
// Mirrors, file:line under /root/reference:
//   flags                      src/main.rs:21-104         (clap Args)
//   logger format / level      src/main.rs:110-121        ([<UTC>Z LEVEL ] message on stderr)
//   early exits                src/main.rs:123-195        (--list-db-versions, --download, --check)
//   database resolution        src/main.rs:388-434, src/download.rs:178-232, src/lib.rs:119-141
//   output codec decision      src/main.rs:238-245, src/compression.rs:107-118,271-296
//   temp dir + kraken_out[#]   src/main.rs:248-265
//   default output names       src/main.rs:273-338        (incl. the `.zstd` extension quirk)
//   compress stage             src/main.rs:342-368, src/compression.rs:182-268
//   summary line               src/lib.rs:38-45
// Not rebuilt (network provisioning, out of scope): --download / --list-db-versions report so.
#include <dirent.h>
#include <errno.h>
#include <pwd.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "nohuman_engine.h"

static bool g_verbose = false;

static void logmsg(const char *level, const char *fmt, ...) {
    if (!g_verbose && strcmp(level, "DEBUG") == 0) return;
    char ts[32];
    time_t t = time(nullptr);
    struct tm tmv;
    gmtime_r(&t, &tmv);
    strftime(ts, sizeof ts, "%Y-%m-%dT%H:%M:%SZ", &tmv);
    fprintf(stderr, "[%s %-5s] ", ts, level);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
#define INFO(...) logmsg("INFO", __VA_ARGS__)
#define DEBUG(...) logmsg("DEBUG", __VA_ARGS__)
#define WARN(...) logmsg("WARN", __VA_ARGS__)
#define ERROR(...) logmsg("ERROR", __VA_ARGS__)

[[noreturn]] static void die(const char *fmt, ...) {  // anyhow's "Error: ..." on stderr, exit 1
    fprintf(stderr, "Error: ");
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    exit(1);
}

// ---- path helpers with std::path semantics -----------------------------------------------------------
static bool exists(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
static bool is_dir(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
static std::string parent_of(const std::string &p) {
    size_t s = p.find_last_of('/');
    if (s == std::string::npos) return "";
    return s == 0 ? "/" : p.substr(0, s);
}
static std::string file_name(const std::string &p) {
    size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}
static std::string join(const std::string &dir, const std::string &name) {
    if (dir.empty()) return name;
    return dir.back() == '/' ? dir + name : dir + "/" + name;
}
// Path::extension: text after the last '.' of the file name, none for ".hidden" or no dot
static std::string extension(const std::string &p) {
    std::string f = file_name(p);
    size_t d = f.find_last_of('.');
    if (d == std::string::npos || d == 0) return "";
    return f.substr(d + 1);
}
static std::string file_stem(const std::string &p) {
    std::string f = file_name(p);
    size_t d = f.find_last_of('.');
    if (d == std::string::npos || d == 0) return f;
    return f.substr(0, d);
}
static std::string quoted(const std::string &p) { return "\"" + p + "\""; }  // {:?} of a path

// ---- CompressionFormat (src/compression.rs) ----------------------------------------------------------
enum Codec { C_NONE, C_BZ2, C_GZ, C_XZ, C_ZST };
static const char *codec_ext(Codec c) {
    switch (c) {
        case C_BZ2: return "bz2";
        case C_GZ: return "gz";
        case C_XZ: return "xz";
        case C_ZST: return "zst";
        default: return "";
    }
}
static bool codec_from_str(const std::string &s, Codec &c) {  // FromStr, case-insensitive single letter
    if (s.size() != 1) return false;
    switch (s[0]) {
        case 'b': case 'B': c = C_BZ2; return true;
        case 'g': case 'G': c = C_GZ; return true;
        case 'x': case 'X': c = C_XZ; return true;
        case 'z': case 'Z': c = C_ZST; return true;
        case 'u': case 'U': c = C_NONE; return true;
        default: return false;
    }
}
static Codec codec_from_path(const std::string &p) {
    std::string e = extension(p);
    if (e == "bz2") return C_BZ2;
    if (e == "gz") return C_GZ;
    if (e == "xz") return C_XZ;
    if (e == "zst" || e == "zstd") return C_ZST;
    return C_NONE;
}
static Codec codec_from_magic(const std::string &p) {
    unsigned char m[5] = {0, 0, 0, 0, 0};
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) die("Failed to open %s", quoted(p).c_str());
    size_t got = fread(m, 1, 5, f);
    fclose(f);
    if (got != 5) die("Failed to read the first five bytes of the file");
    if (m[0] == 0x1f && m[1] == 0x8b) return C_GZ;
    if (m[0] == 0x42 && m[1] == 0x5a) return C_BZ2;
    if (m[0] == 0x28 && m[1] == 0xb5 && m[2] == 0x2f && m[3] == 0xfd) return C_ZST;
    if (m[0] == 0xfd && m[1] == 0x37 && m[2] == 0x7a && m[3] == 0x58 && m[4] == 0x5a) return C_XZ;
    return C_NONE;
}
// Is the file a BAM: a first gzip member with the BGZF extra field that inflates to a stream beginning "BAM\1" (the library's test)
static bool is_bam_file(const std::string &p) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    std::vector<unsigned char> m(65536 + 64);
    const size_t got = fread(m.data(), 1, m.size(), f);
    fclose(f);
    if (got < 18 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return false;
    const size_t xlen = m[10] | (size_t)m[11] << 8;
    if (12 + xlen > got) return false;
    bool bc = false;
    for (size_t at = 12; at + 4 <= 12 + xlen;) {
        const size_t slen = m[at + 2] | (size_t)m[at + 3] << 8;
        if (m[at] == 'B' && m[at + 1] == 'C' && slen == 2) bc = true;
        at += 4 + slen;
    }
    if (!bc) return false;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    unsigned char magic[4] = {0, 0, 0, 0};
    z.next_in = m.data() + 12 + xlen;
    z.avail_in = (uInt)(got - 12 - xlen);
    z.next_out = magic;
    z.avail_out = 4;
    (void)inflate(&z, Z_SYNC_FLUSH);
    const bool four = z.avail_out == 0;
    inflateEnd(&z);
    return four && memcmp(magic, "BAM\1", 4) == 0;
}

// Is the run paired: two inputs, or one input that is a paired BAM (its first kept record has flag 0x1: the library's test).
// Asked once, when the arguments have been read (Args::paired); every question of the kind reads the answer there.
static bool paired_input(const std::vector<std::string> &input) {
    return input.size() == 1 ? nh_bam_paired(input[0].c_str()) != 0 : input.size() == 2;
}
static std::string add_extension(Codec c, const std::string &p) {
    if (c == C_NONE) return p;
    return p + "." + codec_ext(c);  // "a.fq" -> "a.fq.gz", "a" -> "a.gz"
}

// compress stage (src/compression.rs:182-268): content parity, not byte-identical streams
// ---- database discovery (src/download.rs:178-232, src/lib.rs:119-141) --------------------------------
static bool validate_db_directory(const std::string &p, std::string &actual) {
    const char *req[3] = {"hash.k2d", "opts.k2d", "taxo.k2d"};
    for (const std::string &d : {p, join(p, "db")}) {
        bool ok = is_dir(d);
        for (const char *r : req) ok = ok && exists(join(d, r));
        if (ok) {
            actual = d;
            return true;
        }
    }
    return false;
}
struct Installed {
    std::string version, path, added;
};
static bool read_metadata(const std::string &dir, Installed &m) {  // nohuman-db.toml: version, added
    FILE *f = fopen(join(dir, "nohuman-db.toml").c_str(), "r");
    if (!f) return false;
    char line[1024];
    bool v = false, a = false;
    while (fgets(line, sizeof line, f)) {
        char key[64], val[512];
        if (sscanf(line, " %63[A-Za-z_] = \"%511[^\"]\"", key, val) == 2) {
            if (!strcmp(key, "version")) { m.version = val; v = true; }
            if (!strcmp(key, "added")) { m.added = val; a = true; }
        }
    }
    fclose(f);
    return v && a;
}
static std::string date_key(const std::string &s) {  // invalid dates sort as the legacy date
    int y, mo, d;
    if (s.size() == 10 && sscanf(s.c_str(), "%4d-%2d-%2d", &y, &mo, &d) == 3) return s;
    return "1970-01-01";
}
static std::vector<Installed> installed_databases(const std::string &root) {
    std::vector<Installed> out;
    if (DIR *d = opendir(root.c_str())) {
        while (struct dirent *e = readdir(d)) {
            if (!strcmp(e->d_name, ".") || !strcmp(e->d_name, "..")) continue;
            std::string p = join(root, e->d_name), actual;
            Installed m;
            if (!is_dir(p) || !read_metadata(p, m)) continue;
            if (validate_db_directory(p, actual)) {
                m.path = p;
                out.push_back(m);
            } else {
                DEBUG("Skipping %s because the required Kraken files were not found", quoted(p).c_str());
            }
        }
        closedir(d);
    }
    std::string actual;
    Installed tmp;
    if (validate_db_directory(root, actual) && !read_metadata(root, tmp))
        out.push_back({"legacy", root, "1970-01-01"});
    return out;
}

struct Args {
    bool paired = false;  // the run classifies pairs: two inputs, or a paired BAM (paired_input, once the inputs are known)
    std::vector<std::string> input;
    std::string out1, out2, database, db_version, kraken_output, kraken_report;
    std::string human_out1, human_out2;  // split run: the human reads in the same pass (nh_run_split)
    bool has_human_out1 = false, has_human_out2 = false;
    bool bgzf = false;  // gzip outputs in bgzip's blocked form (NH_CODEC_BGZF)
    bool bam_out = false;  // a BAM input's kept records as BAM, tags intact (NH_CODEC_BAM)
    bool mask = false;  // masked run: every read written, the human ones' bases as N (nh_run_mask)
    std::string calls, human_ids;  // read lists (nh_run_ex): a table line per read; the ids of the human reads
    unsigned min_base_quality = 0;  // kraken2's --minimum-base-quality (nh_run_minq); 0: off
    bool dust_reads = false;        // classify every read with its low-complexity stretches as ambiguous bases (nh_run_dust)
    std::string read_stats;         // the read statistics table (nh_run_rstats)
    std::string host_intervals;     // the BED file of the bases that host k-mers cover (nh_run_intervals)
    bool host_bases_only = false;   // a masked run that writes N over the bases that host k-mers cover alone (nh_run_hostbases)
    unsigned host_gap = 0;          // ... and over the uncovered runs of at most so many bases between two of them
    bool has_host_gap = false;
    bool host_cut = false;          // a masked run that cuts the host stretches out and writes the rest of a human read as pieces (nh_run_hostcut)
    unsigned host_min_piece = 35;   // ... of at least so many bases (k: a shorter piece holds no k-mer)
    bool has_host_min_piece = false;
    bool report_minimizer_data = false;  // kraken2's flag: two more columns in the report (nh_run_mdata)
    std::string minimizer_table;         // the minimizer table (nh_run_mdata)
    // per-taxon outputs (nh_run_taxa): the selectors in the order given -- taxid (0: `other`), the path as given ('#' in it: the mate)
    std::vector<std::pair<unsigned long long, std::string>> taxon_out;
    // the host selection (nh_run_host): the clades whose reads count as host, and the clades inside them that do not
    std::vector<unsigned long long> host_taxids, keep_taxids;
    bool has_out1 = false, has_out2 = false, check = false, download = false, list = false, human = false;
    bool has_type = false;
    Codec type = C_NONE;
    // --build-db: make a database from FASTA instead of running on reads (nh_build_db)
    std::string extend_db;  // --extend-db: the database that --build-db adds its taxa to (nh_extend_db)
    bool has_extend_db = false;
    std::string build_db, taxon_name, taxa;  // taxa: the manifest of a build of several taxa (nh_build_args.taxa_file)
    bool has_taxa = false, has_taxid = false;
    bool has_build_db = false, has_taxon_name = false, has_build_opt = false, force = false, mask_low_complexity = false;
    std::vector<std::string> reference;
    std::vector<std::string> exclude;  // --exclude: files whose minimizers --build-db leaves out of the database (nh_build_db_exclude)
    unsigned long long taxid = 0, capacity = 0;
    double load_factor = 0;
    unsigned threads = 1;
    float confidence = 0.0f;
    std::string conf_text = "0.0";
};

static void usage(FILE *f) {
    fputs("Usage: nohuman [OPTIONS] [INPUT]...\n\n"
          "Arguments:\n  [INPUT]...  Input file(s) to remove human reads from (FASTA or FASTQ, plain, gzip or bzip2; or one BAM file of single-end reads or of collated pairs: mates adjacent, as `samtools collate` leaves them)\n\n"
          "Options:\n"
          "  -o, --out1 <OUTPUT_1>        First output file\n"
          "  -O, --out2 <OUTPUT_2>        Second output file\n"
          "  -c, --check                  Check that all required dependencies are available and exit\n"
          "  -d, --download               Download the database\n"
          "  -D, --db <PATH>              Path to the database [env: NOHUMAN_DB=] [default: ~/.nohuman/db]\n"
          "      --db-version <VERSION>   Name of the database version to use\n"
          "      --list-db-versions       List available database versions and exit\n"
          "  -F, --output-type <FORMAT>   Output compression format. u: uncompressed; b: Bzip2; g: Gzip; x: Xz (Lzma); z: Zstd\n"
          "      --bgzf                   Write gzip outputs as BGZF (blocked gzip, as bgzip writes it); needs the output format g\n"
          "      --bam-out                Write the kept records of a BAM input as BAM: the input's header (no @PG line is added) and records copied byte for byte, "
          "tags (MM/ML, mv, RG ...) intact, BGZF framed [default output: <stem>.nohuman.bam]. Secondary, supplementary and empty records are written nowhere; the call "
          "is not added to a record (see --calls, -k). A paired BAM's two mates go to the one file, in the order they have in the input. Not with another output format or container, a masked run, per-taxon outputs, two inputs, "
          "-O / --human-out2 or an input that is not a BAM\n"
          "  -t, --threads <INT>          Number of threads to use [default: 1]\n"
          "  -H, --human                  Output human reads instead of removing them\n"
          "      --human-out1 <PATH>      Also write the human reads, in the same run, to this file (as -H would)\n"
          "      --human-out2 <PATH>      Second human output file (required with two inputs)\n"
          // (one line for both flags whose names start with --mask: the help keeps a single line that mentions "--mask")
          "      --mask                   Replace the bases of human reads with N instead of removing them (every read is written, in input order). "
          "With --build-db: --mask-low-complexity masks low-complexity sequence of the genome (symmetric DUST, window 64, level 20) before its "
          "minimizers are taken [recommended for real genomes]\n"
          "  -C, --conf <[0, 1]>          Kraken2 minimum confidence score [default: 0.0]\n"
          "      --minimum-base-quality <INT>  Kraken2 minimum base quality: classify FASTQ bases with a lower Phred+33 quality as ambiguous (0-93; the reads written keep their bases) [default: 0]\n"
          "      --dust-reads             Classify every read with its low-complexity stretches (poly-A, microsatellites: symmetric DUST, window 64, level 20) "
          "as ambiguous bases, so that a database built without low-complexity filtering does not call them human (the reads written keep their bases)\n"
          "      --host-intervals <FILE>  Write where in each read the host k-mers lie, as BED without a header: one line 'id, start, end, mate (1|2), taxid of the read's call' for every "
          "maximal run of bases covered by k-mers whose minimizer is in the database (with --host-taxid: in the host clades), 0-based and half-open, in input order. Plain text, never "
          "compressed; no other output changes. With --minimum-base-quality / --dust-reads the masked bases are not covered. For BAM input the coordinates are those of the FASTQ "
          "record the read is transcoded to: a reverse-strand record is counted on its reverse complement\n"
          // (the help keeps a single line that mentions the masked run's own flag: these two say "a masked run")
          "      --host-bases-only        Make the run a masked run that writes N only over the bases of a human read that host k-mers cover (the intervals of --host-intervals) and keeps "
          "the rest of the read: every read is written, in input order. Not with -H\n"
          "      --host-gap <INT>         With --host-bases-only: also write N over an uncovered run of at most INT bases that lies between two covered bases of the same read "
          "(each mate on its own; never a run that touches an end of the read). 34 (k - 1) is recommended for noisy long reads, whose sequencing errors break a host stretch "
          "into pieces with leftovers too short to hold a k-mer (0-4096) [default: 0]\n"
          "      --host-cut               Make the run a masked run that cuts the bases that host k-mers cover out of a human read and writes what is left as records of their own, "
          "named '<id>:<start>-<end>' (0-based, half-open: the coordinates of --host-intervals), in input order; a human read with nothing left is not written, every other read is "
          "written whole. --host-gap closes gaps as with --host-bases-only. Single-end input only. Not with -H or --host-bases-only\n"
          "      --host-min-piece <INT>   With --host-cut: the shortest piece that is written, in bases; shorter leftovers are dropped. The default is k: a shorter piece holds no "
          "k-mer (1-2147483647) [default: 35]\n"
          "  -k, --kraken-output <FILE>   Write the Kraken2 read classification output to a file\n"
          "  -r, --kraken-report <FILE>   Write the Kraken2 report with aggregate counts/clade to file\n"
          "      --report-minimizer-data  Report, per clade, the minimizer hits of the reads and how many distinct minimizers they were, as columns 4 and 5 of the Kraken2 report "
          "(many reads on few distinct minimizers mark a false positive; counted exactly on the GPU); needs --kraken-report\n"
          "      --minimizer-table <FILE> Write a table with, per taxon: reads, minimizer hits, distinct minimizers and cells of the database, own and clade, and the coverage in percent\n"
          "      --calls <FILE>           Write a table with one line per read: C/U, id, taxid, length(s), k-mers, clade hits (hits / k-mers is the confidence -C thresholds), hit groups\n"
          "      --read-stats <FILE>      Write a QC table of all, non-human and human reads per mate: reads, bases, min/mean/median/max length, N50, GC %, other bases, Q20 %, Q30 %, mean quality (counted on the GPU in the same pass)\n"
          "      --human-ids <FILE>       Write the ids of the human reads, one per line\n"
          "      --taxon-out <TAXID|other>:<PATH>  Also write the classified reads of this taxon's clade to PATH, in the same run (as -H would write them); "
          "may be given up to 8 times: a read goes to the deepest selected taxon that is its call or an ancestor of it, `other` takes the "
          "classified reads in no selected clade. With two inputs PATH must contain '#', which becomes _1 / _2\n"
          "      --host-taxid <TAXID>     Count only the reads classified into this taxon's clade as host (removed, written by -H / --human-out1, masked, listed by "
          "--human-ids); may be given more than once, 16 times together with --keep-taxid. Without it every classified read is host, which is "
          "--host-taxid 1. A classified read outside the host clades is kept and written as an unclassified one; -k, -r, --calls and --taxon-out report the true calls\n"
          "      --keep-taxid <TAXID>     Do not count the reads of this taxon's clade as host although a --host-taxid clade contains it (the deepest of the "
          "listed taxa above a read's call decides); needs --host-taxid\n"
          "      --build-db <DIR>         Build a database (hash.k2d, opts.k2d, taxo.k2d) in DIR from the --reference files, on the GPU, and exit\n"
          "      --reference <FILE>       FASTA file (plain or gzip) of the host genome for --build-db; may be given more than once\n"
          "      --taxid <INT>            Taxonomy id of the host for --build-db [default: 9606]\n"
          "      --taxon-name <NAME>      Name of the host in the database's taxonomy for --build-db\n"
          "      --taxa <FILE>            Build a database of several taxa from a manifest, one taxon per line, tab-separated: taxid, parent taxid (1 is the root), name, "
          "FASTA files; a minimizer shared by two taxa is stored as their lowest common ancestor\n"
          "      --extend-db <DIR>        With a database build: add the taxa given to the existing database in DIR (its three .k2d files are enough, not the "
          "genomes it was made from) and write the result to the build's directory; the table keeps its size, a load factor given is the highest load "
          "the result may have [default: 0.95], a fixed number of cells cannot be asked for\n"
          "      --exclude <FILE>         With a database build from genomes alone: leave out every minimizer that the sequences of FILE (FASTA or FASTQ, plain or "
          "gzip; bacterial and viral genomes, say) carry too; nothing of FILE is stored; may be given more than once\n"
          "      --load-factor <FLOAT>    Load factor of the hash table for --build-db, in (0, 0.95] [default: 0.7]\n"
          "      --capacity <INT>         Cells of the hash table for --build-db; skips the counting pass [default: distinct minimizers / load factor]\n"
          "      --force                  Let --build-db replace a database that DIR already holds\n"
          "  -v, --verbose                Set the logging level to verbose\n"
          "  -h, --help                   Print help\n"
          "  -V, --version                Print version\n",
          f);
}

// the file of mate m (0, 1) of a --taxon-out path: every '#' becomes _1 / _2 (kraken2's convention for its paired outputs)
static std::string taxon_out_path(const std::string &path, int m) {
    std::string out;
    for (char c : path) {
        if (c == '#') out += m ? "_2" : "_1";
        else out += c;
    }
    return out;
}

[[noreturn]] static void arg_error(const char *fmt, ...) {  // clap: message, exit code 2
    fprintf(stderr, "error: ");
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fprintf(stderr, "\n\nFor more information, try '--help'.\n");
    exit(2);
}

static Args parse_args(int argc, char **argv) {
    Args a;
    const char *home = getenv("HOME");
    if (!home) {
        struct passwd *pw = getpwuid(getuid());
        home = pw ? pw->pw_dir : "";
    }
    a.database = join(join(home, ".nohuman"), "db");
    if (const char *env = getenv("NOHUMAN_DB")) a.database = env;
    auto value = [&](int &i, const std::string &flag) -> std::string {
        if (i + 1 >= argc) arg_error("a value is required for '%s' but none was supplied", flag.c_str());
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        std::string s = argv[i], v;
        size_t eq = s.find('=');
        bool inline_val = s.rfind("--", 0) == 0 && eq != std::string::npos;
        if (inline_val) {
            v = s.substr(eq + 1);
            s = s.substr(0, eq);
        }
        auto val = [&]() { return inline_val ? v : value(i, s); };
        if (s == "-o" || s == "--out1") { a.out1 = val(); a.has_out1 = true; }
        else if (s == "-O" || s == "--out2") { a.out2 = val(); a.has_out2 = true; }
        else if (s == "-c" || s == "--check") a.check = true;
        else if (s == "-d" || s == "--download") a.download = true;
        else if (s == "-D" || s == "--db") a.database = val();
        else if (s == "--db-version") a.db_version = val();
        else if (s == "--list-db-versions") a.list = true;
        else if (s == "-F" || s == "--output-type") {
            std::string t = val();
            if (!codec_from_str(t, a.type)) arg_error("invalid value '%s' for '--output-type <FORMAT>': %s is not a valid output format", t.c_str(), t.c_str());
            a.has_type = true;
        } else if (s == "-t" || s == "--threads") {
            std::string t = val();
            char *end;
            long n = strtol(t.c_str(), &end, 10);
            if (*end || t.empty() || n <= 0) arg_error("invalid value '%s' for '--threads <INT>': number would be zero for non-zero type", t.c_str());
            a.threads = (unsigned)n;
        } else if (s == "-H" || s == "--human") a.human = true;
        else if (s == "--human-out1") { a.human_out1 = val(); a.has_human_out1 = true; }
        else if (s == "--human-out2") { a.human_out2 = val(); a.has_human_out2 = true; }
        else if (s == "--mask") a.mask = true;
        else if (s == "--bgzf") a.bgzf = true;
        else if (s == "--bam-out") a.bam_out = true;
        else if (s == "-C" || s == "--conf") {
            std::string t = val();
            char *end;
            float c = strtof(t.c_str(), &end);
            if (*end || t.empty()) arg_error("invalid value '%s' for '--conf <[0, 1]>': Confidence score must be a number", t.c_str());
            if (!(c >= 0.0f && c <= 1.0f)) arg_error("invalid value '%s' for '--conf <[0, 1]>': Confidence score must be in the closed interval [0, 1]", t.c_str());
            a.confidence = c;
        } else if (s == "--minimum-base-quality") {
            std::string t = val();
            char *end;
            errno = 0;
            long n = strtol(t.c_str(), &end, 10);
            if (*end || t.empty() || t[0] == ' ' || t[0] == '\t')
                arg_error("invalid value '%s' for '--minimum-base-quality <INT>': invalid digit found in string", t.c_str());
            if (errno || n < 0 || n > 93) arg_error("invalid value '%s' for '--minimum-base-quality <INT>': %s is not in 0..=93", t.c_str(), t.c_str());
            a.min_base_quality = (unsigned)n;
        } else if (s == "-k" || s == "--kraken-output") a.kraken_output = val();
        else if (s == "-r" || s == "--kraken-report") a.kraken_report = val();
        else if (s == "--calls") a.calls = val();
        else if (s == "--human-ids") a.human_ids = val();
        else if (s == "--read-stats") a.read_stats = val();
        else if (s == "--host-intervals") a.host_intervals = val();
        else if (s == "--host-bases-only") a.host_bases_only = true;
        else if (s == "--host-gap") {
            std::string t = val();
            char *end;
            errno = 0;
            long n = strtol(t.c_str(), &end, 10);
            if (*end || t.empty() || t[0] == ' ' || t[0] == '\t') arg_error("invalid value '%s' for '--host-gap <INT>': invalid digit found in string", t.c_str());
            if (errno || n < 0 || n > NH_HOST_GAP_MAX) arg_error("invalid value '%s' for '--host-gap <INT>': %s is not in 0..=%d", t.c_str(), t.c_str(), NH_HOST_GAP_MAX);
            a.host_gap = (unsigned)n, a.has_host_gap = true;
        }
        else if (s == "--host-cut") a.host_cut = true;
        else if (s == "--host-min-piece") {
            std::string t = val();
            char *end;
            errno = 0;
            long long n = strtoll(t.c_str(), &end, 10);
            if (*end || t.empty() || t[0] == ' ' || t[0] == '\t') arg_error("invalid value '%s' for '--host-min-piece <INT>': invalid digit found in string", t.c_str());
            if (errno || n < 1 || n > 2147483647ll) arg_error("invalid value '%s' for '--host-min-piece <INT>': %s is not in 1..=2147483647", t.c_str(), t.c_str());
            a.host_min_piece = (unsigned)n, a.has_host_min_piece = true;
        }
        else if (s == "--report-minimizer-data") a.report_minimizer_data = true;
        else if (s == "--minimizer-table") a.minimizer_table = val();
        else if (s == "--taxon-out") {
            const std::string t = val();
            const size_t colon = t.find(':');
            if (colon == std::string::npos || colon + 1 == t.size())
                arg_error("invalid value '%s' for '--taxon-out <TAXID|other>:<PATH>': a selector, a ':' and a path are expected", t.c_str());
            const std::string sel = t.substr(0, colon);
            unsigned long long id = 0;
            if (sel != "other") {
                char *end;
                errno = 0;
                id = strtoull(sel.c_str(), &end, 10);
                if (*end || sel.empty() || sel[0] < '0' || sel[0] > '9' || errno || id == 0)
                    arg_error("invalid value '%s' for '--taxon-out <TAXID|other>:<PATH>': %s is neither a taxid nor `other`", t.c_str(), quoted(sel).c_str());
            }
            for (const auto &o : a.taxon_out)
                if (o.first == id) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' selects %s more than once", sel.c_str());
            if (a.taxon_out.size() == NH_MAX_TAXON_OUTS) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' cannot be used more than %d times", NH_MAX_TAXON_OUTS);
            a.taxon_out.push_back({id, t.substr(colon + 1)});
        }
        else if (s == "--host-taxid" || s == "--keep-taxid") {
            const std::string t = val();
            char *end;
            errno = 0;
            const unsigned long long id = strtoull(t.c_str(), &end, 10);
            if (*end || t.empty() || t[0] < '0' || t[0] > '9' || errno)
                arg_error("invalid value '%s' for '%s <TAXID>': invalid digit found in string", t.c_str(), s.c_str());
            if (id == 0) arg_error("invalid value '%s' for '%s <TAXID>': 0 is not a taxon", t.c_str(), s.c_str());
            for (const std::vector<unsigned long long> *l : {&a.host_taxids, &a.keep_taxids})
                for (unsigned long long o : *l)
                    if (o == id) arg_error("the arguments '--host-taxid <TAXID>' and '--keep-taxid <TAXID>' name taxon %llu more than once", id);
            if (a.host_taxids.size() + a.keep_taxids.size() == NH_MAX_HOST_TAXA)
                arg_error("the arguments '--host-taxid <TAXID>' and '--keep-taxid <TAXID>' cannot be used more than %d times together", NH_MAX_HOST_TAXA);
            (s == "--host-taxid" ? a.host_taxids : a.keep_taxids).push_back(id);
        }
        else if (s == "--build-db") { a.build_db = val(); a.has_build_db = true; }
        else if (s == "--extend-db") { a.extend_db = val(); a.has_extend_db = true; }
        else if (s == "--reference") a.reference.push_back(val());
        else if (s == "--exclude") a.exclude.push_back(val());
        else if (s == "--taxid" || s == "--capacity") {
            std::string t = val();
            char *end;
            errno = 0;
            unsigned long long n = strtoull(t.c_str(), &end, 10);
            if (*end || t.empty() || t[0] == '-' || errno || (s == "--taxid" && n == 0) || (s == "--capacity" && n == 0))
                arg_error("invalid value '%s' for '%s <INT>': a positive integer is expected", t.c_str(), s.c_str());
            (s == "--taxid" ? a.taxid : a.capacity) = n;
            if (s == "--taxid") a.has_taxid = true;
            a.has_build_opt = true;
        } else if (s == "--taxon-name") { a.taxon_name = val(); a.has_taxon_name = a.has_build_opt = true; }
        else if (s == "--load-factor") {
            std::string t = val();
            char *end;
            double f = strtod(t.c_str(), &end);
            if (*end || t.empty() || !(f > 0 && f <= 0.95)) arg_error("invalid value '%s' for '--load-factor <FLOAT>': a number in (0, 0.95] is expected", t.c_str());
            a.load_factor = f;
            a.has_build_opt = true;
        } else if (s == "--force") a.force = a.has_build_opt = true;
        else if (s == "--mask-low-complexity") a.mask_low_complexity = true;
        else if (s == "--dust-reads") a.dust_reads = true;
        else if (s == "--taxa") { a.taxa = val(); a.has_taxa = true; }
        else if (s == "-v" || s == "--verbose") g_verbose = true;
        else if (s == "-h" || s == "--help") { usage(stdout); exit(0); }
        else if (s == "-V" || s == "--version") { puts("nohuman 0.5.1 (MI355X engine)"); exit(0); }
        else if (s.size() > 1 && s[0] == '-') arg_error("unexpected argument '%s' found", s.c_str());
        else {
            if (!exists(s)) arg_error("invalid value '%s' for '[INPUT]...': %s does not exist", s.c_str(), quoted(s).c_str());
            a.input.push_back(s);
        }
    }
    a.paired = paired_input(a.input);
    if (a.has_build_db) {  // builds and exits: nothing of a run may come with it
        if (a.has_taxa) {
            const char *with = !a.reference.empty() ? "--reference <FILE>" : a.has_taxid ? "--taxid <INT>" : a.has_taxon_name ? "--taxon-name <NAME>" : nullptr;
            if (with) arg_error("the argument '--taxa <FILE>' cannot be used with '%s': the manifest gives the taxids, the names and the FASTA files", with);
            if (!exists(a.taxa)) arg_error("invalid value '%s' for '--taxa <FILE>': %s does not exist", a.taxa.c_str(), quoted(a.taxa).c_str());
        } else if (a.reference.empty())
            arg_error("the following required arguments were not provided:\n  --reference <FILE> (with '--build-db <DIR>')");
        if (!a.input.empty()) arg_error("the argument '--build-db <DIR>' cannot be used with read inputs ('%s'): the genome is given with '--reference <FILE>'", a.input[0].c_str());
        const char *out_flag = a.has_out1 ? "--out1" : a.has_out2 ? "--out2" : a.has_human_out1 ? "--human-out1" : a.has_human_out2 ? "--human-out2"
                             : !a.kraken_output.empty() ? "--kraken-output" : !a.kraken_report.empty() ? "--kraken-report" : !a.calls.empty() ? "--calls"
                             : !a.human_ids.empty() ? "--human-ids" : !a.read_stats.empty() ? "--read-stats" : a.report_minimizer_data ? "--report-minimizer-data"
                             : !a.minimizer_table.empty() ? "--minimizer-table" : a.has_type ? "--output-type"
                             : a.bgzf ? "--bgzf" : a.bam_out ? "--bam-out" : a.mask ? "--mask" : a.human ? "--human" : !a.taxon_out.empty() ? "--taxon-out"
                             : !a.host_taxids.empty() ? "--host-taxid" : !a.keep_taxids.empty() ? "--keep-taxid" : a.dust_reads ? "--dust-reads"
                             : !a.host_intervals.empty() ? "--host-intervals" : a.host_bases_only ? "--host-bases-only" : a.has_host_gap ? "--host-gap"
                             : a.host_cut ? "--host-cut" : a.has_host_min_piece ? "--host-min-piece" : nullptr;
        if (out_flag) arg_error("the argument '--build-db <DIR>' cannot be used with '%s'", out_flag);
        if (a.has_extend_db) {
            if (a.capacity) arg_error("the argument '--extend-db <DIR>' cannot be used with '--capacity <INT>': an extension keeps the capacity of its base");
            if (!exists(a.extend_db)) arg_error("invalid value '%s' for '--extend-db <DIR>': %s does not exist", a.extend_db.c_str(), quoted(a.extend_db).c_str());
        }
        if (!a.exclude.empty() && a.has_extend_db)
            arg_error("the argument '--exclude <FILE>' cannot be used with '--extend-db <DIR>': an extension has no counting pass whose set the "
                      "exclusion could be held against");
        for (const std::string &r : a.reference)
            if (!exists(r)) arg_error("invalid value '%s' for '--reference <FILE>': %s does not exist", r.c_str(), quoted(r).c_str());
        for (const std::string &r : a.exclude)
            if (!exists(r)) arg_error("invalid value '%s' for '--exclude <FILE>': %s does not exist", r.c_str(), quoted(r).c_str());
        return a;
    }
    if (a.mask_low_complexity) arg_error("the argument '--mask-low-complexity' needs '--build-db <DIR>': it masks the genome a database is built from, not reads");
    if (!a.reference.empty()) arg_error("the argument '--reference <FILE>' needs '--build-db <DIR>'");
    if (a.has_taxa) arg_error("the argument '--taxa <FILE>' needs '--build-db <DIR>'");
    if (!a.exclude.empty()) arg_error("the argument '--exclude <FILE>' needs '--build-db <DIR>': it names sequences whose minimizers a database build leaves out");
    if (a.has_extend_db) arg_error("the argument '--extend-db <DIR>' needs '--build-db <DIR>': it names the database that the build adds its taxa to");
    if (a.has_build_opt) arg_error("the arguments '--taxid', '--taxon-name', '--load-factor', '--capacity' and '--force' need '--build-db <DIR>'");
    if (a.input.empty() && !a.check && !a.download && !a.list)
        arg_error("the following required arguments were not provided:\n  <INPUT>...");
    if (a.mask && a.human) arg_error("the argument '--mask' cannot be used with '--human'");
    if (a.host_bases_only && a.human) arg_error("the argument '--host-bases-only' cannot be used with '--human'");
    if (a.host_cut && a.human) arg_error("the argument '--host-cut' cannot be used with '--human'");
    if (a.host_cut && a.host_bases_only) arg_error("the argument '--host-cut' cannot be used with '--host-bases-only': a host stretch is cut out or written as N, not both");
    if (a.host_cut && a.input.size() > 1) arg_error("the argument '--host-cut' cannot be used with two inputs: the pieces of two mates cannot stay in step");
    if (a.has_host_min_piece && !a.host_cut) arg_error("the argument '--host-min-piece <INT>' needs '--host-cut': it is the shortest piece that run writes");
    if (a.has_host_gap && !a.host_bases_only && !a.host_cut) arg_error("the argument '--host-gap <INT>' needs '--host-bases-only': it closes the gaps between the bases that run masks");
    if (a.host_bases_only || a.host_cut) a.mask = true;  // (a masked run in everything else)
    // BAM output (--bam-out): the kept records of ONE BAM input, copied; its container is BGZF, whatever -F or the names say
    if (a.bam_out) {
        if (a.has_type) arg_error("the argument '--bam-out' cannot be used with '--output-type <FORMAT>': a BAM file is its own container");
        if (a.bgzf) arg_error("the argument '--bam-out' cannot be used with '--bgzf': a BAM file is BGZF framed already");
        if (a.mask) arg_error("the argument '--bam-out' cannot be used with '--mask'");
        if (!a.taxon_out.empty()) arg_error("the argument '--bam-out' cannot be used with '--taxon-out <TAXID|other>:<PATH>'");
        if (a.input.size() > 1) arg_error("the argument '--bam-out' cannot be used with two inputs: a BAM holds both mates of a pair, and is given alone");
        if (a.has_out2) arg_error("the argument '--bam-out' cannot be used with '--out2 <OUT2>': one BAM file holds both mates");
        if (a.has_human_out2) arg_error("the argument '--bam-out' cannot be used with '--human-out2 <PATH>': one BAM file holds both mates");
        if (a.input.size() == 1 && !is_bam_file(a.input[0]))
            arg_error("the argument '--bam-out' needs a BAM input: %s is not a BAM file", quoted(a.input[0]).c_str());
    }
    if (!a.keep_taxids.empty() && a.host_taxids.empty())
        arg_error("the argument '--keep-taxid <TAXID>' needs '--host-taxid <TAXID>': it keeps a clade inside a host clade");
    // split run (--human-out1 / --human-out2): the non-human reads to -o / -O, the human ones to these, in one pass
    if (a.has_human_out1 || a.has_human_out2) {
        const bool paired = a.paired && !a.bam_out;  // (the second mate has files of its own)
        if (a.human) arg_error("the argument '--human' cannot be used with '--human-out1 <PATH>'");
        if (!a.has_human_out1) arg_error("the following required arguments were not provided:\n  --human-out1 <PATH>");
        if (a.has_human_out2 && !paired) arg_error("the argument '--human-out2 <PATH>' needs two inputs, or a paired BAM");
        if (paired && !a.has_human_out2)
            arg_error("the following required arguments were not provided:\n  --human-out2 <PATH> (two inputs, or a paired BAM)");
        for (const std::string *h : {&a.human_out1, &a.human_out2}) {
            if (h == &a.human_out2 && !a.has_human_out2) continue;
            const char *flag = h == &a.human_out1 ? "--human-out1" : "--human-out2";
            if ((a.has_out1 && *h == a.out1) || (a.has_out2 && *h == a.out2))
                arg_error("the argument '%s <PATH>' names the same file as '--out1' / '--out2': %s", flag, h->c_str());
        }
        if (a.has_human_out2 && a.human_out1 == a.human_out2)
            arg_error("the arguments '--human-out1 <PATH>' and '--human-out2 <PATH>' name the same file: %s", a.human_out1.c_str());
    }
    // per-taxon outputs (--taxon-out): a file per selector and mate, written in the same pass
    if (!a.taxon_out.empty()) {
        const bool paired = a.paired;
        if (a.human) arg_error("the argument '--human' cannot be used with '--taxon-out <TAXID|other>:<PATH>'");
        std::vector<std::string> mine;
        for (const auto &o : a.taxon_out) {
            const bool hash = o.second.find('#') != std::string::npos;
            if (paired && !hash) arg_error("invalid value '%s' for '--taxon-out <TAXID|other>:<PATH>': with two inputs, or a paired BAM, the path needs a '#' (it becomes _1 / _2)", o.second.c_str());
            if (!paired && hash) arg_error("invalid value '%s' for '--taxon-out <TAXID|other>:<PATH>': a '#' in the path needs two inputs, or a paired BAM", o.second.c_str());
            for (int m = 0; m < (paired ? 2 : 1); m++) {
                const std::string p = taxon_out_path(o.second, m);
                const char *other = (a.has_out1 && p == a.out1) ? "--out1" : (a.has_out2 && p == a.out2) ? "--out2"
                                  : (a.has_human_out1 && p == a.human_out1) ? "--human-out1" : (a.has_human_out2 && p == a.human_out2) ? "--human-out2"
                                  : p == a.kraken_output ? "--kraken-output" : p == a.kraken_report ? "--kraken-report" : p == a.calls ? "--calls"
                                  : p == a.human_ids ? "--human-ids" : p == a.read_stats ? "--read-stats"
                                  : p == a.minimizer_table ? "--minimizer-table" : nullptr;
                if (other) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' names the same file as '%s': %s", other, p.c_str());
                for (const std::string &q : mine)
                    if (p == q) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' names the same file twice: %s", p.c_str());
                for (const std::string &in : a.input)
                    if (p == in) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' names the input %s", p.c_str());
                mine.push_back(p);
            }
        }
    }
    if (!a.calls.empty() && a.calls == a.human_ids)
        arg_error("the arguments '--calls <FILE>' and '--human-ids <FILE>' name the same file: %s", a.calls.c_str());
    for (const std::string *o : {&a.calls, &a.human_ids})
        if (!a.read_stats.empty() && a.read_stats == *o)
            arg_error("the argument '--read-stats <FILE>' names the same file as '%s <FILE>': %s", o == &a.calls ? "--calls" : "--human-ids",
                      a.read_stats.c_str());
    if (a.report_minimizer_data && a.kraken_report.empty())
        arg_error("the argument '--report-minimizer-data' needs '--kraken-report <FILE>': its two columns go into the report");
    if (!a.minimizer_table.empty()) {
        const std::string &p = a.minimizer_table;
        const char *other = (a.has_out1 && p == a.out1) ? "--out1" : (a.has_out2 && p == a.out2) ? "--out2"
                          : (a.has_human_out1 && p == a.human_out1) ? "--human-out1" : (a.has_human_out2 && p == a.human_out2) ? "--human-out2"
                          : p == a.kraken_output ? "--kraken-output" : p == a.kraken_report ? "--kraken-report" : p == a.calls ? "--calls"
                          : p == a.human_ids ? "--human-ids" : p == a.read_stats ? "--read-stats" : nullptr;
        if (other) arg_error("the argument '--minimizer-table <FILE>' names the same file as '%s': %s", other, p.c_str());
        for (const std::string &in : a.input)
            if (p == in) arg_error("the argument '--minimizer-table <FILE>' names the input %s", p.c_str());
    }
    if (!a.host_intervals.empty()) {
        const std::string &p = a.host_intervals;
        const char *other = (a.has_out1 && p == a.out1) ? "--out1" : (a.has_out2 && p == a.out2) ? "--out2"
                          : (a.has_human_out1 && p == a.human_out1) ? "--human-out1" : (a.has_human_out2 && p == a.human_out2) ? "--human-out2"
                          : p == a.kraken_output ? "--kraken-output" : p == a.kraken_report ? "--kraken-report" : p == a.calls ? "--calls"
                          : p == a.human_ids ? "--human-ids" : p == a.read_stats ? "--read-stats" : p == a.minimizer_table ? "--minimizer-table" : nullptr;
        if (other) arg_error("the argument '--host-intervals <FILE>' names the same file as '%s': %s", other, p.c_str());
        for (const std::string &in : a.input)
            if (p == in) arg_error("the argument '--host-intervals <FILE>' names the input %s", p.c_str());
    }
    return a;
}

// f32 Display as Rust prints it (shortest round-trip decimal), then what kraken2 would parse (f64)
static double confidence_as_kraken2_sees_it(float c, std::string &text) {
    char buf[64];
    for (int prec = 1; prec < 12; prec++) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)c);
        if (strtof(buf, nullptr) == c) break;
    }
    text = buf;
    return strtod(buf, nullptr);
}

// --bam-out: "<stem>.nohuman.bam" beside the input (the stem without a trailing ".bam")
static std::string default_bam_out_name(const std::string &in) {
    return join(parent_of(in), (extension(in) == "bam" ? file_stem(in) : file_name(in)) + ".nohuman.bam");
}

// a paired BAM's two FASTQ outputs: "<stem>.nohuman_1.fq[.ext]" and "<stem>.nohuman_2.fq[.ext]" beside the input
static std::string default_pair_out_name(const std::string &in, Codec out_codec, int mate) {
    const std::string stem = extension(in) == "bam" ? file_stem(in) : file_name(in);
    return add_extension(out_codec, join(parent_of(in), stem + (mate ? ".nohuman_2.fq" : ".nohuman_1.fq")));
}

static std::string default_out_name(const std::string &in, Codec out_codec);
// the default name of mate m's record output: beside its own input; a paired BAM is the input of both
static std::string default_mate_out_name(const std::vector<std::string> &input, bool paired, Codec out_codec, int mate) {
    if (input.size() == 1 && paired) return default_pair_out_name(input[0], out_codec, mate);
    return default_out_name(input[mate && input.size() > 1 ? 1 : 0], out_codec);
}

static std::string default_out_name(const std::string &in, Codec out_codec) {
    // src/main.rs:274-290: strip a trailing compression extension only when it equals the codec's
    // canonical extension (so ".zstd" is not stripped), then "<stem>.nohuman.fq[.ext]" beside the input
    std::string ext = codec_ext(codec_from_path(in));
    std::string stem;
    if (extension(in) == ext) {
        std::string no_ext = in.substr(0, in.size() - (extension(in).empty() ? 0 : extension(in).size() + 1));
        stem = file_stem(no_ext);
    } else {
        stem = file_stem(in);
    }
    return add_extension(out_codec, join(parent_of(in), stem + ".nohuman.fq"));
}

// the names of a database's nodes from the root on, read from its taxo.k2d ("K2TAXDAT", node count, bytes of names and of ranks,
// 56-byte nodes with the name's offset as their fourth word, the names)
static std::vector<std::string> node_names(const std::string &db_dir) {
    std::vector<std::string> out;
    FILE *f = fopen(join(db_dir, "taxo.k2d").c_str(), "rb");
    if (!f) return out;
    std::string img;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) img.append(buf, n);
    fclose(f);
    uint64_t hdr[3];
    if (img.size() < 32 || memcmp(img.data(), "K2TAXDAT", 8) != 0) return out;
    memcpy(hdr, img.data() + 8, 24);
    if (hdr[0] > (1u << 20) || hdr[1] > img.size() || 32 + hdr[0] * 56 + hdr[1] > img.size()) return out;
    const char *names = img.data() + 32 + hdr[0] * 56;
    for (uint64_t i = 1; i < hdr[0]; i++) {
        uint64_t off;
        memcpy(&off, img.data() + 32 + i * 56 + 24, 8);
        out.push_back(off < hdr[1] ? std::string(names + off, strnlen(names + off, hdr[1] - off)) : std::string("?"));
    }
    return out;
}

// the name of the node with this external id in a database's taxo.k2d (the id is the node's sixth word); "?" when it has none
static std::string taxon_name_of(const std::string &db_dir, unsigned long long taxid) {
    FILE *f = fopen(join(db_dir, "taxo.k2d").c_str(), "rb");
    if (!f) return "?";
    std::string img;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) img.append(buf, n);
    fclose(f);
    uint64_t hdr[3];
    if (img.size() < 32 || memcmp(img.data(), "K2TAXDAT", 8) != 0) return "?";
    memcpy(hdr, img.data() + 8, 24);
    if (hdr[0] > (1u << 20) || hdr[1] > img.size() || 32 + hdr[0] * 56 + hdr[1] > img.size()) return "?";
    const char *names = img.data() + 32 + hdr[0] * 56;
    for (uint64_t i = 1; i < hdr[0]; i++) {
        uint64_t off, ext;
        memcpy(&off, img.data() + 32 + i * 56 + 24, 8);
        memcpy(&ext, img.data() + 32 + i * 56 + 40, 8);
        if (ext == taxid) return off < hdr[1] ? std::string(names + off, strnlen(names + off, hdr[1] - off)) : std::string("?");
    }
    return "?";
}

static void fill_build_args(const Args &args, std::vector<const char *> &refs, nh_build_args &ba) {
    for (const std::string &r : args.reference) refs.push_back(r.c_str());
    memset(&ba, 0, sizeof ba);
    ba.struct_size = (uint32_t)sizeof ba;
    ba.n_fasta = (uint32_t)refs.size();
    ba.fasta = refs.empty() ? nullptr : refs.data();
    ba.out_dir = args.build_db.c_str();
    ba.taxid = args.taxid;
    ba.taxon_name = args.has_taxon_name ? args.taxon_name.c_str() : nullptr;
    ba.load_factor = args.load_factor;
    ba.capacity = args.capacity;
    ba.threads = args.threads;
    ba.force = args.force ? 1 : 0;
    ba.mask_low_complexity = args.mask_low_complexity ? 1 : 0;
    ba.taxa_file = args.has_taxa ? args.taxa.c_str() : nullptr;
    if (const char *dv = getenv("NOHUMAN_DEVICES")) ba.device = (int32_t)strtol(dv, nullptr, 10);  // (one device: the first listed)
}

// --exclude: the list as nh_build_db_exclude takes it (empty: the call is nh_build_db)
static void fill_exclude_args(const Args &args, std::vector<const char *> &files, nh_exclude_args &xa) {
    for (const std::string &f : args.exclude) files.push_back(f.c_str());
    memset(&xa, 0, sizeof xa);
    xa.struct_size = (uint32_t)sizeof xa;
    xa.n_fasta = (uint32_t)files.size();
    xa.fasta = files.empty() ? nullptr : files.data();
}

int main(int argc, char **argv) {
    Args args = parse_args(argc, argv);
    if (args.has_build_db && args.has_extend_db) {  // the base, the taxa and how they fit together: checked before any device is asked for
        std::vector<const char *> refs;
        nh_build_args ba;
        fill_build_args(args, refs, ba);
        nh_extend_args xa;
        memset(&xa, 0, sizeof xa);
        xa.struct_size = (uint32_t)sizeof xa;
        xa.base_dir = args.extend_db.c_str();
        const int rc = nh_extend_check(&ba, &xa, nullptr, nullptr);
        if (rc == NH_EINVAL) arg_error("invalid value '%s' for '--extend-db <DIR>': %s", args.extend_db.c_str(), nh_last_error());
        if (rc != 0) die("Failed to extend the database\n\nCaused by:\n    %s", nh_last_error());
    } else if (args.has_build_db && !args.exclude.empty()) {  // the exclusion list against the inputs and the output, and the manifest if there is one
        std::vector<const char *> refs, files;
        nh_build_args ba;
        nh_exclude_args xa;
        fill_build_args(args, refs, ba);
        fill_exclude_args(args, files, xa);
        const int rc = nh_exclude_check(&ba, &xa, nullptr, nullptr);
        if (rc == NH_EINVAL && strstr(nh_last_error(), "nh_build_db_exclude:"))
            arg_error("invalid value '%s' for '--exclude <FILE>': %s", args.exclude[0].c_str(), nh_last_error());
        if (rc == NH_EINVAL && args.has_taxa) arg_error("invalid value '%s' for '--taxa <FILE>': %s", args.taxa.c_str(), nh_last_error());
        if (rc == NH_EINVAL) arg_error("%s", nh_last_error());
        if (rc != 0) die("Failed to build the database\n\nCaused by:\n    %s", nh_last_error());
    } else if (args.has_build_db && args.has_taxa) {  // what the manifest says wrongly is an argument error too: read before any device is asked for
        std::vector<const char *> refs;
        nh_build_args ba;
        fill_build_args(args, refs, ba);
        const int rc = nh_build_check(&ba, nullptr);
        if (rc == NH_EINVAL) arg_error("invalid value '%s' for '--taxa <FILE>': %s", args.taxa.c_str(), nh_last_error());
        if (rc != 0) die("Failed to build the database\n\nCaused by:\n    %s", nh_last_error());
    }
    if (args.bgzf && !args.input.empty()) {  // BGZF is a form of gzip: any other resolved output format is an argument error
        const Codec c = args.has_type ? args.type : args.has_out1 ? codec_from_path(args.out1) : codec_from_magic(args.input[0]);
        if (c != C_GZ)
            arg_error("the argument '--bgzf' needs the output format g (Gzip), but the output format is %s",
                      c == C_NONE ? "u (uncompressed)" : c == C_BZ2 ? "b (Bzip2)" : c == C_XZ ? "x (Xz)" : "z (Zstd)");
    }
    if (args.has_human_out1 && !args.input.empty()) {  // a human output equal to a DEFAULT output name: an argument error as well
        const Codec c = args.has_type ? args.type : args.has_out1 ? codec_from_path(args.out1) : codec_from_magic(args.input[0]);
        const bool two = args.paired && !args.bam_out;
        const std::string o1 = args.has_out1 ? args.out1 : args.bam_out ? default_bam_out_name(args.input[0]) : default_mate_out_name(args.input, args.paired, c, 0);
        const std::string o2 = two ? (args.has_out2 ? args.out2 : default_mate_out_name(args.input, args.paired, c, 1)) : "";
        for (const std::string *h : {&args.human_out1, &args.human_out2})
            if (!h->empty() && (*h == o1 || *h == o2))
                arg_error("the argument '%s <PATH>' names the same file as the output %s", h == &args.human_out1 ? "--human-out1" : "--human-out2",
                          h->c_str());
    }
    if (!args.taxon_out.empty() && !args.input.empty()) {  // and a per-taxon file equal to a DEFAULT output name
        const Codec c = args.has_type ? args.type : args.has_out1 ? codec_from_path(args.out1) : codec_from_magic(args.input[0]);
        const bool two = args.paired;
        const std::string o1 = args.has_out1 ? args.out1 : default_mate_out_name(args.input, args.paired, c, 0);
        const std::string o2 = two ? (args.has_out2 ? args.out2 : default_mate_out_name(args.input, args.paired, c, 1)) : "";
        for (const auto &o : args.taxon_out)
            for (int m = 0; m < (two ? 2 : 1); m++) {
                const std::string p = taxon_out_path(o.second, m);
                if (p == o1 || p == o2) arg_error("the argument '--taxon-out <TAXID|other>:<PATH>' names the same file as the output %s", p.c_str());
            }
    }
    if (args.list) die("Failed to download database manifest: network access is not available in this build");
    if (args.download) {
        INFO("Downloading database...");
        die("Failed to download database: network access is not available in this build");
    }
    // dependency check: the engine library + a gfx950 device take the place of `kraken2` on PATH
    char probe[256];
    if (nh_probe(probe, sizeof probe) != 0) {
        DEBUG("kraken2 is not executable");
        ERROR("The following dependencies are missing:");
        ERROR("kraken2 (in-process engine: %s)", probe);
        die("Missing dependencies");
    }
    DEBUG("kraken2 is executable (in-process engine: %s)", probe);
    if (args.check) {
        INFO("All dependencies are available");
        return 0;
    }
    if (args.has_build_db && args.has_extend_db) {
        INFO("Extending database %s into %s...", quoted(args.extend_db).c_str(), quoted(args.build_db).c_str());
        std::vector<const char *> refs;
        nh_build_args ba;
        fill_build_args(args, refs, ba);
        std::vector<nh_build_taxon_stats> per_taxon(4096);
        std::vector<uint64_t> base_cells(4096, 0);
        ba.taxon_stats = per_taxon.data();
        ba.taxon_stats_cap = (uint32_t)per_taxon.size();
        nh_extend_args xa;
        memset(&xa, 0, sizeof xa);
        xa.struct_size = (uint32_t)sizeof xa;
        xa.base_dir = args.extend_db.c_str();
        xa.base_cells = base_cells.data();
        xa.base_cells_cap = (uint32_t)base_cells.size();
        nh_build_stats bs;
        nh_extend_stats xs;
        memset(&xs, 0, sizeof xs);
        xs.struct_size = (uint32_t)sizeof xs;
        if (nh_extend_db(&ba, &xa, &bs, &xs) != 0) die("Failed to extend the database\n\nCaused by:\n    %s", nh_last_error());
        INFO("Base database: size %llu, capacity %llu, load %.4f, %llu nodes, %llu value bits", (unsigned long long)xs.base_size, (unsigned long long)bs.capacity,
             bs.capacity ? (double)xs.base_size / (double)bs.capacity : 0.0, (unsigned long long)(xs.base_nodes - 1), (unsigned long long)xs.base_value_bits);
        INFO("Database extended: %llu nodes added, %llu sequences, %llu bases, %llu cells added, %llu shadowed cells, size %llu, load %.4f; load %.2f s, "
             "re-key %.4f s, read %.2f s, insert %.2f s, write %.2f s",
             (unsigned long long)xs.nodes_added, (unsigned long long)bs.sequences, (unsigned long long)bs.bases, (unsigned long long)xs.cells_added,
             (unsigned long long)xs.shadowed_cells, (unsigned long long)bs.size, xs.load, xs.seconds_load, xs.seconds_rekey, bs.seconds_read, bs.seconds_insert,
             bs.seconds_write);
        if (args.mask_low_complexity)
            INFO("%llu low-complexity bases masked (%.2f %% of the bases), mask %.2f s", (unsigned long long)bs.masked_bases,
                 bs.bases ? 100.0 * (double)bs.masked_bases / (double)bs.bases : 0.0, bs.seconds_mask);
        const std::vector<std::string> taxon_names = node_names(args.build_db);
        for (uint64_t i = 0; i < bs.taxa && i < per_taxon.size(); i++)  // (how many minimizers of the base an added taxon moved up the tree)
            if (per_taxon[i].cells != base_cells[i])
                DEBUG("  %s (taxid %llu): %llu cells before, %llu after", taxon_names.size() > i ? taxon_names[i].c_str() : "?",
                      (unsigned long long)per_taxon[i].taxid, (unsigned long long)base_cells[i], (unsigned long long)per_taxon[i].cells);
        INFO("Database written to: %s", quoted(args.build_db).c_str());
        INFO("Done.");
        return 0;
    }
    if (args.has_build_db) {
        INFO("Building database in %s...", quoted(args.build_db).c_str());
        std::vector<const char *> refs;
        nh_build_args ba;
        fill_build_args(args, refs, ba);
        std::vector<nh_build_taxon_stats> per_taxon(4096);
        ba.taxon_stats = per_taxon.data();
        ba.taxon_stats_cap = (uint32_t)per_taxon.size();
        nh_build_stats bs;
        std::vector<const char *> x_files;
        nh_exclude_args xa;
        fill_exclude_args(args, x_files, xa);
        nh_exclude_stats xs;
        memset(&xs, 0, sizeof xs);
        xs.struct_size = (uint32_t)sizeof xs;
        if (nh_build_db_exclude(&ba, &xa, &bs, &xs) != 0) die("Failed to build the database\n\nCaused by:\n    %s", nh_last_error());
        if (!args.exclude.empty())
            INFO("Exclusion: %llu sequences, %llu bases; %llu of %llu distinct minimizers excluded, %llu kept; read %.2f s, exclude %.2f s",
                 (unsigned long long)xs.sequences, (unsigned long long)xs.bases, (unsigned long long)xs.excluded_minimizers,
                 (unsigned long long)bs.distinct_minimizers, (unsigned long long)xs.kept_minimizers, xs.seconds_read, xs.seconds_exclude);
        char masked[128] = "";
        if (args.mask_low_complexity)
            snprintf(masked, sizeof masked, "; %llu low-complexity bases masked (%.2f %% of the bases), mask %.2f s", (unsigned long long)bs.masked_bases,
                     bs.bases ? 100.0 * (double)bs.masked_bases / (double)bs.bases : 0.0, bs.seconds_mask);
        INFO("Database built: %llu sequences, %llu bases, %llu distinct minimizers, capacity %llu, size %llu, load %.4f; read %.2f s, count %.2f s, "
             "insert %.2f s, write %.2f s%s",
             (unsigned long long)bs.sequences, (unsigned long long)bs.bases, (unsigned long long)bs.distinct_minimizers,
             (unsigned long long)bs.capacity, (unsigned long long)bs.size, bs.capacity ? (double)bs.size / (double)bs.capacity : 0.0, bs.seconds_read,
             bs.seconds_count, bs.seconds_insert, bs.seconds_write, masked);
        const std::vector<std::string> taxon_names = args.has_taxa ? node_names(args.build_db) : std::vector<std::string>();
        if (args.has_taxa)
            for (uint64_t i = 0; i < bs.taxa && i < per_taxon.size(); i++) {
                const nh_build_taxon_stats &t = per_taxon[i];
                INFO("  %s (taxid %llu): %llu sequences, %llu bases, %llu cells", taxon_names.size() > i ? taxon_names[i].c_str() : "?",
                     (unsigned long long)t.taxid, (unsigned long long)t.sequences, (unsigned long long)t.bases, (unsigned long long)t.cells);
            }
        INFO("Database written to: %s", quoted(args.build_db).c_str());
        INFO("Done.");
        return 0;
    }
    if (args.input.empty()) die("No input files provided");
    if (args.input.size() > 2) die("Only one or two input files are allowed");

    // resolve_database (src/main.rs:393-434)
    std::string db_path, db_ver;
    if (!args.db_version.empty()) {
        if (args.db_version == "all")
            die("Cannot run with `--db-version all`. Use `--download --db-version all` to download every database.");
        bool found = false;
        for (const Installed &i : installed_databases(args.database))
            if (i.version == args.db_version) {
                if (!validate_db_directory(i.path, db_path))
                    die("Required files (hash.k2d, opts.k2d, taxo.k2d) not found in %s or its 'db' subdirectory", quoted(i.path).c_str());
                db_ver = i.version;
                found = true;
                break;
            }
        if (!found)
            die("Database version '%s' is not installed under %s. Run `nohuman --download --db-version %s` to download it.",
                args.db_version.c_str(), quoted(args.database).c_str(), args.db_version.c_str());
    } else if (!validate_db_directory(args.database, db_path)) {
        std::vector<Installed> inst = installed_databases(args.database);
        const Installed *best = nullptr;
        for (const Installed &i : inst)
            if (!best || date_key(i.added) >= date_key(best->added)) best = &i;
        if (!best)
            die("Database does not exist at %s. Run `nohuman --download` to fetch one.", quoted(args.database).c_str());
        if (!validate_db_directory(best->path, db_path))
            die("Required files (hash.k2d, opts.k2d, taxo.k2d) not found in %s or its 'db' subdirectory", quoted(best->path).c_str());
        db_ver = best->version;
    }
    if (!db_ver.empty())
        INFO("Using database version %s at %s", db_ver.c_str(), quoted(db_path).c_str());
    else
        INFO("Using database at %s", quoted(db_path).c_str());

    // paired: the run classifies pairs; two: the second mate has files of its own (not with --bam-out: one BAM holds both mates)
    const bool paired = args.paired, two = paired && !args.bam_out;
    Codec out_codec = args.has_type ? args.type : args.has_out1 ? codec_from_path(args.out1) : codec_from_magic(args.input[0]);

    // The reference lets kraken2 write kraken_out*.fq into a temporary directory "nohuman*" in the current
    // directory (src/main.rs:248-257) and compresses them to the output paths afterwards
    // (src/main.rs:342-368).  Here the engine's writer feeds the kept records straight into the output
    // encoder: no temporary file, one pass.
    std::string out1 = args.has_out1 ? args.out1 : args.bam_out ? default_bam_out_name(args.input[0]) : default_mate_out_name(args.input, args.paired, out_codec, 0);
    std::string out2 = two ? (args.has_out2 ? args.out2 : default_mate_out_name(args.input, args.paired, out_codec, 1)) : "";
    const int codec = args.bam_out ? NH_CODEC_BAM : out_codec == C_GZ ? (args.bgzf ? NH_CODEC_BGZF : NH_CODEC_GZIP) : out_codec == C_BZ2 ? NH_CODEC_BZIP2 : out_codec == C_XZ ? NH_CODEC_XZ
                    : out_codec == C_ZST ? NH_CODEC_ZSTD : NH_CODEC_NONE;
    INFO(args.mask ? "Masking human reads..." : args.human ? "Keeping human reads..." : "Removing human reads...");

    std::string conf_text;
    const double conf64 = confidence_as_kraken2_sees_it(args.confidence, conf_text);
    DEBUG("Running kraken2...");
    DEBUG("With arguments: [\"--threads\", \"%u\", \"--db\", %s, \"--output\", %s, \"--confidence\", \"%s\"%s%s]",
          args.threads, quoted(db_path).c_str(),
          quoted(args.kraken_output.empty() ? "/dev/null" : args.kraken_output).c_str(), conf_text.c_str(),
          paired ? ", \"--paired\"" : "", args.human ? ", \"--classified-out\", ..." : ", \"--unclassified-out\", ...");
    nh_run_args ra;
    memset(&ra, 0, sizeof ra);
    ra.db_dir = db_path.c_str();
    ra.in1 = args.input[0].c_str();
    ra.in2 = args.input.size() == 2 ? args.input[1].c_str() : nullptr;
    // The engine writes to "<out>.partial" and the finished file is renamed over the output path: a run
    // that fails -- before or after it created anything -- leaves a file already at the output path
    // untouched, and `-o` equal to an input path works as in the reference (the input is replaced after
    // it has been read: src/main.rs:342-368 compresses the temporary kraken_out*.fq to the output path
    // last).  Outputs that exist and are not regular files (/dev/stdout, a fifo) are written directly.
    auto staged = [](const std::string &out) {
        struct stat sb;
        if (stat(out.c_str(), &sb) == 0 && !S_ISREG(sb.st_mode)) return out;
        return out + ".partial";
    };
    const std::string part1 = staged(out1), part2 = two ? staged(out2) : "";
    const bool split = args.has_human_out1;
    const std::string hpart1 = split ? staged(args.human_out1) : "", hpart2 = split && two ? staged(args.human_out2) : "";
    // the staged files of this run (final path, the one written): removed when the run fails
    // (renamed in this order: the human outputs first, so that a rename that fails part-way never leaves the non-human outputs --
    // what the next step of a pipeline looks for -- in place without their human counterparts)
    std::vector<std::pair<std::string, std::string>> staged_files;
    if (split) staged_files.push_back({args.human_out1, hpart1});
    if (split && two) staged_files.push_back({args.human_out2, hpart2});
    const bool lists = !args.calls.empty() || !args.human_ids.empty();
    const std::string cpart = args.calls.empty() ? "" : staged(args.calls), ipart = args.human_ids.empty() ? "" : staged(args.human_ids);
    if (!args.calls.empty()) staged_files.push_back({args.calls, cpart});
    if (!args.human_ids.empty()) staged_files.push_back({args.human_ids, ipart});
    const std::string spart = args.read_stats.empty() ? "" : staged(args.read_stats);
    if (!args.read_stats.empty()) staged_files.push_back({args.read_stats, spart});
    const std::string bpart = args.host_intervals.empty() ? "" : staged(args.host_intervals);
    if (!args.host_intervals.empty()) staged_files.push_back({args.host_intervals, bpart});
    const std::string mpart = args.minimizer_table.empty() ? "" : staged(args.minimizer_table);
    if (!args.minimizer_table.empty()) staged_files.push_back({args.minimizer_table, mpart});
    // the per-taxon files: staged and renamed like the human outputs
    std::vector<std::string> tfinal, tpart;  // [2 * selector + mate]
    for (const auto &o : args.taxon_out)
        for (int m = 0; m < 2; m++) {
            tfinal.push_back(m && !paired ? "" : taxon_out_path(o.second, m));
            tpart.push_back(m && !paired ? "" : staged(tfinal.back()));
            if (!tfinal.back().empty()) staged_files.push_back({tfinal.back(), tpart.back()});
        }
    std::vector<nh_taxon_out> touts(args.taxon_out.size());
    for (size_t k = 0; k < touts.size(); k++) {
        touts[k].taxid = args.taxon_out[k].first ? args.taxon_out[k].first : NH_TAXON_OTHER;
        touts[k].out1 = tpart[2 * k].c_str();
        touts[k].out2 = paired ? tpart[2 * k + 1].c_str() : nullptr;
        touts[k].fragments = 0;
    }
    staged_files.push_back({out1, part1});
    if (two) staged_files.push_back({out2, part2});
    auto unlink_staged = [&] {
        for (const auto &f : staged_files)
            if (f.second != f.first) unlink(f.second.c_str());
    };
    ra.out1 = part1.c_str();
    ra.out2 = two ? part2.c_str() : nullptr;
    ra.out_codec = codec;
    ra.codec_threads = two ? (args.threads / 2 ? args.threads / 2 : 1) : args.threads;  // src/main.rs:342-346
    ra.kraken_output = args.kraken_output.empty() ? "/dev/null" : args.kraken_output.c_str();
    ra.report = args.kraken_report.empty() ? nullptr : args.kraken_report.c_str();
    ra.confidence = conf64;
    ra.threads = args.threads;
    ra.keep_human = args.human ? 1 : 0;
    ra.n_devices = 0;  // all visible devices, database replicated (env NOHUMAN_DEVICES narrows it)
    std::vector<int32_t> devs;
    if (const char *dv = getenv("NOHUMAN_DEVICES")) {
        for (const char *p = dv; *p;) {
            devs.push_back((int32_t)strtol(p, (char **)&p, 10));
            while (*p == ',' || *p == ' ') p++;
        }
        ra.n_devices = (int32_t)devs.size();
        ra.device_ids = devs.data();
    }
    nh_stats st;
    const char *hp1 = split ? hpart1.c_str() : nullptr, *hp2 = split && two ? hpart2.c_str() : nullptr;
    nh_run_extras rx;
    memset(&rx, 0, sizeof rx);
    rx.struct_size = (uint32_t)sizeof rx;
    rx.mask = args.mask ? 1 : 0;
    rx.human_out1 = hp1, rx.human_out2 = hp2;
    rx.calls = args.calls.empty() ? nullptr : cpart.c_str();
    rx.human_ids = args.human_ids.empty() ? nullptr : ipart.c_str();
    nh_minimizer_data md;
    memset(&md, 0, sizeof md);
    md.struct_size = (uint32_t)sizeof md;
    md.in_report = args.report_minimizer_data ? 1 : 0;
    md.table = args.minimizer_table.empty() ? nullptr : mpart.c_str();
    nh_host_filter hf;
    memset(&hf, 0, sizeof hf);
    hf.struct_size = (uint32_t)sizeof hf;
    hf.n_host = (uint32_t)args.host_taxids.size(), hf.n_keep = (uint32_t)args.keep_taxids.size();
    std::vector<uint64_t> host_ids(args.host_taxids.begin(), args.host_taxids.end()), keep_ids(args.keep_taxids.begin(), args.keep_taxids.end());
    hf.host_taxids = host_ids.empty() ? nullptr : host_ids.data();
    hf.keep_taxids = keep_ids.empty() ? nullptr : keep_ids.data();
    const bool hsel = hf.n_host != 0;
    if (hsel) {  // the host selection by name, before the run
        auto named = [&](const std::vector<unsigned long long> &ids) {
            std::string out;
            for (unsigned long long id : ids) {
                char b[32];
                snprintf(b, sizeof b, "%llu (", id);
                out += (out.empty() ? "" : ", ") + std::string(b) + taxon_name_of(db_path, id) + ")";
            }
            return out;
        };
        if (args.keep_taxids.empty()) INFO("Host clades: %s", named(args.host_taxids).c_str());
        else INFO("Host clades: %s; kept clades: %s", named(args.host_taxids).c_str(), named(args.keep_taxids).c_str());
    }
    nh_read_dust rd;
    memset(&rd, 0, sizeof rd);
    rd.struct_size = (uint32_t)sizeof rd;
    rd.enable = args.dust_reads ? 1 : 0;
    nh_host_intervals hi;
    memset(&hi, 0, sizeof hi);
    hi.struct_size = (uint32_t)sizeof hi;
    hi.path = args.host_intervals.empty() ? nullptr : bpart.c_str();
    nh_host_bases hbs;
    memset(&hbs, 0, sizeof hbs);
    hbs.struct_size = (uint32_t)sizeof hbs;
    hbs.enable = args.host_bases_only ? 1 : 0, hbs.gap = args.host_gap;
    nh_host_cut hcs;
    memset(&hcs, 0, sizeof hcs);
    hcs.struct_size = (uint32_t)sizeof hcs;
    hcs.enable = args.host_cut ? 1 : 0, hcs.gap = args.host_gap, hcs.min_piece = args.host_min_piece;
    const int run_rc = hcs.enable ? nh_run_hostcut(&ra, &rx, args.min_base_quality, args.read_stats.empty() ? nullptr : spart.c_str(), nullptr,
                                                   touts.empty() ? nullptr : touts.data(), (uint32_t)touts.size(), md.in_report || md.table ? &md : nullptr,
                                                   hsel ? &hf : nullptr, &rd, hi.path ? &hi : nullptr, nullptr, &hcs, &st)
                       : hbs.enable ? nh_run_hostbases(&ra, &rx, args.min_base_quality, args.read_stats.empty() ? nullptr : spart.c_str(), nullptr,
                                                     touts.empty() ? nullptr : touts.data(), (uint32_t)touts.size(), md.in_report || md.table ? &md : nullptr,
                                                     hsel ? &hf : nullptr, &rd, hi.path ? &hi : nullptr, &hbs, &st)
                       : hi.path ? nh_run_intervals(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality,
                                                  args.read_stats.empty() ? nullptr : spart.c_str(), nullptr, touts.empty() ? nullptr : touts.data(),
                                                  (uint32_t)touts.size(), md.in_report || md.table ? &md : nullptr, hsel ? &hf : nullptr, &rd, &hi, &st)
                       : args.dust_reads ? nh_run_dust(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality,
                                                     args.read_stats.empty() ? nullptr : spart.c_str(), nullptr, touts.empty() ? nullptr : touts.data(),
                                                     (uint32_t)touts.size(), md.in_report || md.table ? &md : nullptr, hsel ? &hf : nullptr, &rd, &st)
                       : hsel ? nh_run_host(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality,
                                          args.read_stats.empty() ? nullptr : spart.c_str(), nullptr, touts.empty() ? nullptr : touts.data(),
                                          (uint32_t)touts.size(), md.in_report || md.table ? &md : nullptr, &hf, &st)
                       : md.in_report || md.table ? nh_run_mdata(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality,
                                                               args.read_stats.empty() ? nullptr : spart.c_str(), nullptr,
                                                               touts.empty() ? nullptr : touts.data(), (uint32_t)touts.size(), &md, &st)
                       : !touts.empty() ? nh_run_taxa(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality,
                                                    args.read_stats.empty() ? nullptr : spart.c_str(), nullptr, touts.data(), (uint32_t)touts.size(), &st)
                       : !args.read_stats.empty() ? nh_run_rstats(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality, spart.c_str(), nullptr, &st)
                       : args.min_base_quality ? nh_run_minq(&ra, lists || args.mask || split ? &rx : nullptr, args.min_base_quality, &st)
                       : lists     ? nh_run_ex(&ra, &rx, &st)
                       : args.mask ? nh_run_mask(&ra, hp1, hp2, &st)
                       : split     ? nh_run_split(&ra, hp1, hp2, &st)
                                   : nh_run(&ra, &st);
    if (run_rc != 0) {
        std::string msg = nh_last_error();
        // nothing half-written stays behind, and nothing this run did not create is touched
        unlink_staged();
        die("Failed to run kraken2\n\nCaused by:\n    kraken2 failed with stderr %s", msg.c_str());
    }
    for (const auto &f : staged_files)
        if (f.second != f.first && rename(f.second.c_str(), f.first.c_str()) != 0) {
            const std::string why = strerror(errno);
            unlink_staged();
            die("Failed to move the output into place: %s", why.c_str());
        }
    // src/lib.rs:38-45 (0/0 prints NaN there as well)
    auto pct = [&](uint64_t a) -> std::string {
        if (st.total_sequences == 0) return "NaN";
        char b[32];
        snprintf(b, sizeof b, "%.2f", (double)a / (double)st.total_sequences * 100.0);
        return b;
    };
    INFO("%llu / %llu (%s%%) sequences classified as human; %llu (%s%%) as non-human",
         (unsigned long long)st.classified, (unsigned long long)st.total_sequences, pct(st.classified).c_str(),
         (unsigned long long)st.unclassified, pct(st.unclassified).c_str());
    if (hsel)
        INFO("%llu host sequences removed; %llu classified sequences outside the host clades kept", (unsigned long long)hf.host_fragments,
             (unsigned long long)hf.spared_fragments);
    if (args.dust_reads)
        DEBUG("%llu low-complexity bases of the reads masked for classification (%.2f %% of the bases)", (unsigned long long)rd.masked_bases,
              st.total_bases ? 100.0 * (double)rd.masked_bases / (double)st.total_bases : 0.0);
    if (hi.path)
        DEBUG("Host intervals: %llu intervals in %llu reads, %llu bases covered by host k-mers (%.2f %% of the bases)", (unsigned long long)hi.intervals,
              (unsigned long long)hi.fragments, (unsigned long long)hi.covered_bases,
              st.total_bases ? 100.0 * (double)hi.covered_bases / (double)st.total_bases : 0.0);
    if (hbs.enable)
        DEBUG("Host bases only: %llu of %llu bases of the human reads written as N, %llu of them by closing gaps of at most %u bases",
              (unsigned long long)hbs.masked_bases, (unsigned long long)hbs.host_bases, (unsigned long long)hbs.closed_bases, hbs.gap);
    if (hcs.enable)
        DEBUG("Host cut: %llu bases of the human reads: %llu written in %llu pieces of at least %u bases, %llu cut out (%llu of them by closing gaps of at most %u bases), "
              "%llu in shorter leftovers; %llu human reads left nothing",
              (unsigned long long)hcs.host_bases, (unsigned long long)hcs.piece_bases, (unsigned long long)hcs.pieces, hcs.min_piece, (unsigned long long)hcs.cut_bases,
              (unsigned long long)hcs.closed_bases, hcs.gap, (unsigned long long)hcs.short_bases, (unsigned long long)hcs.dropped_reads);
    if (g_verbose) {  // a BAM input: what the reader made of its records (the host side of the reader once more: nh_bam_scan)
        nh_bam_info bi;
        nh_bam_pair_info bp;
        memset(&bi, 0, sizeof bi);
        memset(&bp, 0, sizeof bp);
        bi.struct_size = (uint32_t)sizeof bi;
        bp.struct_size = (uint32_t)sizeof bp;
        if (nh_bam_scan_pairs(args.input[0].c_str(), args.threads, &bi, &bp) == 0) {
            DEBUG("BAM input: %llu records, %llu kept, %llu secondary or supplementary and %llu without bases skipped, %llu reverse-complemented",
                  (unsigned long long)bi.records, (unsigned long long)bi.reads, (unsigned long long)bi.skipped_secondary,
                  (unsigned long long)bi.skipped_empty, (unsigned long long)bi.reverse_complemented);
            if (bp.paired)
                DEBUG("BAM input: paired, %llu pairs, %llu bases in the first mates and %llu in the second", (unsigned long long)bp.pairs,
                      (unsigned long long)bp.bases1, (unsigned long long)bp.bases2);
        }
    }
    INFO("Kraken2 finished. Organising output...");

    if (two && args.threads / 2 > 1) {  // the reference announces both files before its two compress threads run
        INFO("Writing output file to: %s", quoted(out1).c_str());
        INFO("Writing output file to: %s", quoted(out2).c_str());
    } else {
        INFO("Output file written to: %s", quoted(out1).c_str());
        if (two) INFO("Output file written to: %s", quoted(out2).c_str());
    }
    if (split) {
        INFO("Human reads written to: %s", quoted(args.human_out1).c_str());
        if (two) INFO("Human reads written to: %s", quoted(args.human_out2).c_str());
    }
    for (size_t k = 0; k < touts.size(); k++) {
        const unsigned long long id = args.taxon_out[k].first;
        const std::string files = paired ? quoted(tfinal[2 * k]) + " " + quoted(tfinal[2 * k + 1]) : quoted(tfinal[2 * k]);
        if (id) INFO("Taxon %llu (%s): %llu reads written to: %s", id, taxon_name_of(db_path, id).c_str(), (unsigned long long)touts[k].fragments, files.c_str());
        else INFO("Taxon other (classified, in no selected clade): %llu reads written to: %s", (unsigned long long)touts[k].fragments, files.c_str());
    }
    if (!args.kraken_output.empty() && args.kraken_output != "/dev/null")
        INFO("Kraken output file written to: %s", quoted(args.kraken_output).c_str());
    if (!args.calls.empty()) INFO("Calls table written to: %s", quoted(args.calls).c_str());
    if (!args.human_ids.empty()) INFO("Human read ids written to: %s", quoted(args.human_ids).c_str());
    if (!args.read_stats.empty()) INFO("Read statistics written to: %s", quoted(args.read_stats).c_str());
    if (!args.host_intervals.empty()) INFO("Host intervals written to: %s", quoted(args.host_intervals).c_str());
    if (!args.minimizer_table.empty()) INFO("Minimizer table written to: %s", quoted(args.minimizer_table).c_str());
    if (!args.kraken_report.empty()) INFO("Kraken report file written to: %s", quoted(args.kraken_report).c_str());
    INFO("Done.");
    return 0;
}
