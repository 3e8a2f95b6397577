// bam_scan_main.cpp -- the BAM reader's host side as a program of its own, for sanitizer builds: nh_bam.cpp with NH_BAM_HOST_ONLY
// (the record chain, its validation, the scalar transcoder, the scan) reading through zlib.  tools/README.md has the command.
//   bam_scan_main FILE...   per file: "ok <counts> <digest> header <bytes> <FNV-1a of the header BamStream kept>", "refused <message>"
//                           or "not a BAM"; exit 0 unless a file cannot be read
#include <stdio.h>
#include <stdlib.h>
#include <zlib.h>

#include "nh_bam.h"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        if (!nh::bam_wants(argv[i])) {
            printf("%s: not a BAM\n", argv[i]);
            continue;
        }
        gzFile g = gzopen(argv[i], "rb");
        if (!g) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 1;
        }
        nh::BamStream s;
        s.open([&](uint8_t *b, size_t n) { return (long)gzread(g, b, (unsigned)n); }, argv[i]);
        nh::BamCounts c;
        uint64_t digest = 0;
        std::string err;
        if (nh::bam_scan_stream(s, &c, &digest, err) != 0) printf("refused %s\n", err.c_str());
        else {
            // (the header's bytes as BAM output copies them: kept while read_header() walks, and compacts, the window)
            uint64_t h = 0xcbf29ce484222325ull;
            for (unsigned char ch : s.header_bytes()) h = (h ^ ch) * 0x100000001b3ull;
            printf("ok %llu %llu %llu %llu %llu %llu %llu %016llx header %zu %016llx\n", (unsigned long long)c.records, (unsigned long long)c.reads,
                   (unsigned long long)c.bases, (unsigned long long)c.skipped_secondary, (unsigned long long)c.skipped_empty,
                   (unsigned long long)c.reverse_complemented, (unsigned long long)c.missing_qualities, (unsigned long long)digest,
                   s.header_bytes().size(), (unsigned long long)h);
        }
        gzclose(g);
    }
    return 0;
}
