"""A plain Python model of the two read lists of a run (nohuman_amd/csrc/nh_calls.hip; nh_run_ex's `calls` and `human_ids`),
and the corpora the tests of those lists run on.  Test helper: pure Python / numpy, it never imports the engine.

  record_id     the id of a record as the lists and the -k line print it
  expected      the exact bytes of both files from the parsed records and the per-fragment results
  k_columns     columns 1-4 of the -k line of a fragment, built by the rules of nh_run.hip's format_batch
  buffer_caps   the bound the host puts on a batch's two texts before the launch
  reads_corpus / edge_corpus / carry_corpus   the inputs of tests/test_gpu_calls.py
"""
import numpy as np

from tests import synth
from tests.builder_model import parse_record

ID_END = b" \t\r"
# a table line without its id: "C\t", "\t" taxid (20 digits of a uint64), "\t" len1|len2 (10 + 1 + 10), "\t", and three uint32
# (10 digits) each followed by a tab or the newline
TAIL_MAX = 2 + 1 + 20 + 1 + 21 + 1 + 3 * 11
BLOCK = 256  # fragments of one builder block (CB_FRAGS)


def raw_id(header):
    """mate 1's header from the byte behind '@' / '>' up to the first space, tab or '\\r', or its end (RecRef::idlen)"""
    i = header[1:]
    for k, c in enumerate(i):
        if c in ID_END:
            return i[:k]
    return i


def record_id(header, paired):
    """... and, in a paired run, without a trailing /1 or /2 when it is longer than two bytes (kraken2 TrimPairInfo)"""
    i = raw_id(header)
    if paired and len(i) > 2 and i[-2:] in (b"/1", b"/2"):
        i = i[:-2]
    return i


def k_columns(header, paired, call, ext_ids, lens):
    """columns 1-4 of the fragment's -k line: C/U, id, external taxon id (0: unclassified), len or len1|len2"""
    ext = int(ext_ids[call]) if call else 0
    return b"\t".join([b"C" if call else b"U", record_id(header, paired), b"%d" % ext, b"|".join(b"%d" % n for n in lens)])


def expected(records, results, ext_ids):
    """records: per mate the list of Rec (tests/builder_model.py); results: per fragment (call, total_kmers, clade_hits,
    hit_groups); ext_ids: internal -> external taxon id.  -> (calls table, human ids), the files' bytes"""
    paired = len(records) == 2
    table, ids = [], []
    for f, r1 in enumerate(records[0]):
        call, total, clade, groups = (int(x) for x in tuple(results[f])[:4])
        lens = [r1.slen] + ([records[1][f].slen] if paired else [])
        table.append(k_columns(r1.header, paired, call, ext_ids, lens) + b"\t%d\t%d\t%d\n" % (total, clade, groups))
        if call:
            ids.append(record_id(r1.header, paired) + b"\n")
    return b"".join(table), b"".join(ids)


def buffer_caps(records):
    """bytes the host reserves for a batch's table and ids before the launch (nh_run.hip): the ids as the reader found them
    (nothing trimmed yet) and the widest line around each"""
    n = len(records[0])
    idsum = sum(len(raw_id(r.header)) for r in records[0])
    return idsum + n * TAIL_MAX + 64, idsum + n + 64


def line_starts(text):
    """the offset of every line of a file"""
    out, p = [], 0
    while p < len(text):
        out.append(p)
        p = text.index(b"\n", p) + 1
    return out


# ---- corpora ---------------------------------------------------------------------------------------------------------------
def _fastq(header, seq, eol=b"\n"):
    return b"@" + header + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol


def _fasta(header, seq, eol=b"\n"):
    return b">" + header + eol + seq + eol


def _human(rng, genomes, n):
    """n bases copied from a toy genome: classified at confidence 0 when n is a few k-mers or more"""
    g = genomes[111]
    st = int(rng.integers(0, len(g) - n + 1))
    return g[st:st + n]


def _build(items, fasta=False):
    """items: per mate a list of (header, sequence, end of line) -> (texts, records)"""
    texts, records = [], []
    for mate in items:
        raws = [(_fasta if fasta else _fastq)(h, s, eol) for h, s, eol in mate]
        texts.append(b"".join(raws))
        records.append([parse_record(r, not fasta) for r in raws])
    return texts, records


def reads_corpus(genomes, n, paired, seed=11, length=100, frac_random=None):
    """n fragments of synth.sample_reads, ids r0, r1 ... (paired: r0/1 and r0/2); a pair stays unclassified only when both
    mates are random reads, so a paired corpus draws more of them"""
    rng = np.random.default_rng(seed)
    if frac_random is None:
        frac_random = 0.65 if paired else 0.4
    reads = synth.sample_reads(rng, genomes, n, length=length, paired=paired, frac_random=frac_random, len_jitter=min(20, length // 3))
    if not paired:
        return _build([[(b"r%d" % i, s, b"\n") for i, s in enumerate(reads)]])
    return _build([[(b"r%d/%d" % (i, m + 1), s[m], b"\n") for i, s in enumerate(reads)] for m in (0, 1)])


EDGE_IDS = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"L" * 300, b"x/1", b"y/2", b"z/3", b"/1", b"longer-name/1", b"longer-name/2"]
EDGE_LENGTHS = [9, 10, 99, 100, 999, 1000]


def edge_corpus(genomes, paired, fasta=False, seed=23):
    """the ids and numbers at which a line can go wrong: EDGE_IDS, each once on a human and once on a random read; headers
    with a tab, with a comment behind a space, with CRLF line ends; a record with an empty sequence; reads of EDGE_LENGTHS
    (human and random); and 40 plain reads around them.  Mate 2 of a paired corpus: reads of 50 +- 10 bases."""
    rng = np.random.default_rng(seed)
    m1 = []
    for i in EDGE_IDS:
        m1.append((i, _human(rng, genomes, 120), b"\n"))
        m1.append((i, synth.random_seq(rng, 120), b"\n"))
    m1.append((b"tab1\tdescription", _human(rng, genomes, 120), b"\n"))
    m1.append((b"tab2/1\tdescription", synth.random_seq(rng, 77), b"\n"))
    m1.append((b"com1 a comment/1", _human(rng, genomes, 101), b"\n"))
    m1.append((b"com2/2 1:N:0:ACGT", synth.random_seq(rng, 83), b"\n"))
    eol = b"\n" if fasta else b"\r\n"  # (the FASTA variant keeps to one-line records with plain line ends)
    m1.append((b"crlf1", _human(rng, genomes, 130), eol))
    m1.append((b"crlf2/1 comment", synth.random_seq(rng, 90), eol))
    m1.append((b"crlf3/2", _human(rng, genomes, 111), eol))
    if not fasta:
        m1.append((b"empty", b"", b"\n"))
    for n in EDGE_LENGTHS:
        m1.append((b"h%d" % n, _human(rng, genomes, n), b"\n"))
        m1.append((b"u%d" % n, synth.random_seq(rng, n), b"\n"))
    for k, s in enumerate(synth.sample_reads(rng, genomes, 40, length=150, frac_random=0.5, len_jitter=30)):
        m1.append((b"plain.%d" % k, s, b"\n"))
    order = rng.permutation(len(m1))
    m1 = [m1[int(j)] for j in order]
    items = [m1]
    if paired:
        items.append([(h, synth.random_seq(rng, int(rng.integers(40, 61))), eol) for h, _s, eol in m1])
    return _build(items, fasta)


CARRY_UNIT, CARRY_REPS, CARRY_BATCH_FRAGS = 600, 111, 70000


def carry_corpus(genomes, seed=31):
    """more fragments in one batch than 256 builder blocks hold (256 * 256 = 65536): a unit of 600 short single-end reads
    111 times over, every read under an id of its own.  -> (text, records, unit's records, repetitions)"""
    rng = np.random.default_rng(seed)
    reads = synth.sample_reads(rng, genomes, CARRY_UNIT, length=60, frac_random=0.4, len_jitter=8)
    raws, recs = [], []
    for rep in range(CARRY_REPS):
        for i, s in enumerate(reads):
            raw = _fastq(b"s%d" % (rep * CARRY_UNIT + i), s)
            raws.append(raw)
            recs.append(parse_record(raw, True))
    return b"".join(raws), [recs], recs[:CARRY_UNIT], CARRY_REPS


def fragments(records):
    """the sequences as the classifier gets them: bytes (single-end) or (bytes, bytes) per fragment"""
    if len(records) == 1:
        return [r.seq for r in records[0]]
    return [(a.seq, b.seq) for a, b in zip(*records)]
