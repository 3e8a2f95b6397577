"""A plain Python model of a run with a minimum base quality (kraken2's --minimum-base-quality; nh_run_minq,
nohuman_amd/csrc/nh_qmask.hip), and the corpora its tests run on.  Test helper: pure Python / numpy plus the CPU oracle; it
never imports the engine.

The model masks the parsed records in Python, gives the masked sequences to the oracle, and builds every file of the run from
the oracle's answer -- the records themselves from the ORIGINAL bases (tests/builder_model.py, tests/calls_model.py): only
classification may change.

  mask_seq          one sequence under a threshold: N where quality - 33 < Q
  classify          the oracle on the masked sequences of parsed records -> (results, per-k-mer taxa, offsets)
  expected          every file of a run, and its stats
  e2e_corpus / ont_corpus   the inputs of tests/test_gpu_minq_run.py; tests/test_qmask_model.py asserts what they contain
"""
import numpy as np

from tests import builder_model as bm
from tests import calls_model as cm
from tests import synth

AMBIG, BORDER = 0xFFFFFFFF, 0xFFFFFFFE
Q_E2E = 20


def mask_seq(seq, qual, q):
    """the bases the classifier sees: N where the Phred+33 quality byte, less 33, is below q (q = 0: nothing)"""
    assert len(seq) == len(qual)
    if q <= 0:
        return bytes(seq)
    s = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    ql = np.frombuffer(bytes(qual), dtype=np.uint8).astype(np.int64)
    s[ql - 33 < q] = 0x4E
    return s.tobytes()


def masked_fragments(records, q):
    """the sequences of every fragment as oracle.pack_reads() takes them; a FASTA record has no qualities and stays"""
    seqs = [[mask_seq(r.seq, r.qual, q) if r.fastq else r.seq for r in recs] for recs in records]
    if len(seqs) == 2:
        return list(zip(*seqs))
    return seqs[0]


def masked_bases(records, q):
    return sum(int((np.frombuffer(r.qual, dtype=np.uint8).astype(np.int64) - 33 < q).sum()) for recs in records for r in recs if r.fastq) if q > 0 else 0


def classify(db, records, q, conf=0.0):
    from oracle import oracle as orc
    paired = len(records) == 2
    bases, offs = orc.pack_reads(masked_fragments(records, q), paired)
    res, _lookups, taxa, toff = db.classify(bases, offs, paired, conf, want_taxa=True)
    return res, taxa, toff


def hitlist(taxa, ext_ids):
    """kraken2 AddHitlistString (nh_run.hip append_hitlist)"""
    if len(taxa) == 0:
        return b"0:0"
    out, i, n = [], 0, len(taxa)
    while i < n:
        t = int(taxa[i])
        j = i
        while j < n and int(taxa[j]) == t:
            j += 1
        if t == BORDER:
            out += [b"|:|"] * (j - i)
        elif t == AMBIG:
            out.append(b"A:%d" % (j - i))
        else:
            out.append(b"%d:%d" % (int(ext_ids[t]), j - i))
        i = j
    return b" ".join(out)


def k_lines(records, res, taxa, toff, ext_ids):
    """the lines of the -k file"""
    paired = len(records) == 2
    out = []
    for f, r1 in enumerate(records[0]):
        lens = [r1.slen] + ([records[1][f].slen] if paired else [])
        out.append(cm.k_columns(r1.header, paired, int(res["call"][f]), ext_ids, lens) + b"\t" +
                   hitlist(taxa[int(toff[f]):int(toff[f + 1])], ext_ids))
    return out


def report(calls):
    """the -r file of a run on the toy database (every rank "no rank", names taxon<id>): nh_run.hip write_report"""
    from oracle import minidb
    tax = minidb.Taxonomy(synth.TOY_EDGES)
    n = tax.node_count
    own = [0] * n
    for c in calls:
        if c:
            own[int(c)] += 1
    clade = own[:]
    for i in range(n - 1, 1, -1):
        clade[tax.parent[i]] += clade[i]
    total = len(calls)
    uncl = sum(1 for c in calls if not c)
    kids = {i: [j for j in range(1, n) if tax.parent[j] == i] for i in range(n)}
    lines = []
    if uncl:
        lines.append("%6.2f\t%d\t%d\tU\t0\tunclassified" % (100.0 * uncl / total, uncl, uncl))

    def dfs(i, depth, rank_depth):
        if clade[i] == 0:
            return
        rank_depth += 1
        lines.append("%6.2f\t%d\t%d\t%s\t%d\t%s%s" % (100.0 * clade[i] / total, clade[i], own[i], "R" + (str(rank_depth) if rank_depth else ""),
                                                     tax.external[i], "  " * depth, "taxon%d" % tax.external[i]))
        for j in sorted(kids[i], key=lambda j: -clade[j]):
            dfs(j, depth + 1, rank_depth)

    if total:
        dfs(1, 0, -1)
    return "".join(ln + "\n" for ln in lines).encode()


def expected(db, records, q, conf=0.0):
    """every file a run with threshold q may write, from the records and the oracle: dict with
    normal / keep / masked (per mate: out1 / out2 of a normal, a -H and a masked run; the human side of a split run is keep),
    k (the -k file), report, calls, ids, stats (total, classified, unclassified, bases), res, masked_bases"""
    res, taxa, toff = classify(db, records, q, conf)
    ext = db.external_ids
    calls = res["call"]
    table, ids = cm.expected(records, res, ext)
    ncls = int((calls != 0).sum())
    return dict(normal=bm.expected_outputs(records, calls, ext, "normal"), keep=bm.expected_outputs(records, calls, ext, "keep"),
                masked=bm.expected_outputs(records, calls, ext, "masked"),
                k=b"".join(ln + b"\n" for ln in k_lines(records, res, taxa, toff, ext)), report=report(calls), calls=table, ids=ids,
                stats=(len(calls), ncls, len(calls) - ncls, sum(r.slen for recs in records for r in recs)),
                res=res, masked_bases=masked_bases(records, q))


# ---- corpora ---------------------------------------------------------------------------------------------------------------
def _fastq(header, seq, qual):
    return b"@" + header + b"\n" + seq + b"\n+\n" + qual + b"\n"


def _qual(rng, n, lo, hi):
    """n Phred+33 quality bytes with scores in lo .. hi"""
    return (rng.integers(lo, hi + 1, size=n) + 33).astype(np.uint8).tobytes()


def _with_stretch(rng, n, a, b, q=Q_E2E):
    """scores of q .. 40 but for [a, b): 2 .. q - 1"""
    ql = bytearray(_qual(rng, n, q, 40))
    ql[a:b] = _qual(rng, b - a, 2, q - 1)
    return bytes(ql)


def e2e_corpus(genomes, paired, n=400, seed=71, q=Q_E2E):
    """n fragments of four kinds in turn: a human read of good qualities; a human read all of whose bases are below q (its
    call flips to U); a human read of 150 bases with a stretch of 10 .. 50 low qualities in it (it stays C with fewer clade
    hits and shows an A: run); a random read with qualities on both sides of q, exactly q and q - 1 among them.  Mate 2 of a
    paired corpus: a random read of 60 +- 10 bases with qualities of 2 .. 40 -- it never carries a call."""
    rng = np.random.default_rng(seed)
    g = genomes[111]

    def human(ln):
        st = int(rng.integers(0, len(g) - ln + 1))
        return g[st:st + ln]

    items = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            s = human(int(rng.integers(100, 151)))
            ql = _qual(rng, len(s), q, 40)
        elif kind == 1:
            s = human(int(rng.integers(100, 151)))
            ql = _qual(rng, len(s), 2, q - 1)
        elif kind == 2:
            s = human(150)
            a = int(rng.integers(40, 70))
            ql = _with_stretch(rng, 150, a, a + int(rng.integers(10, 51)), q)
        else:
            s = synth.random_seq(rng, int(rng.integers(90, 161)))
            ql = bytearray(_qual(rng, len(s), 2, 40))
            ql[0], ql[1] = 33 + q, 33 + q - 1
            ql = bytes(ql)
        items.append((b"f%d.k%d" % (i, kind), s, ql))
    texts, records = [], []
    mates = [items]
    if paired:
        mates = [[(h + b"/1", s, ql) for h, s, ql in items],
                 [(h + b"/2", s2, _qual(rng, len(s2), 2, 40)) for h, _s, _q in items
                  for s2 in [synth.random_seq(rng, int(rng.integers(50, 71)))]]]
    for mate in mates:
        raws = [_fastq(h, s, ql) for h, s, ql in mate]
        texts.append(b"".join(raws))
        records.append([bm.parse_record(r, True) for r in raws])
    return texts, records


SEG_KMERS = 32 * 124  # k-mers of a segment of a long read that is cut (nh_device.h), at k = 35


def ont_corpus(genomes, seed=73, q=Q_E2E):
    """ONT-like single-end reads: three of 12 .. 20 kilobases stitched from the toy genomes and random sequence (long enough
    to be cut into segments), each with low-quality stretches of 300 bases that lie across the first two cuts and a few short
    ones elsewhere, and two short reads"""
    rng = np.random.default_rng(seed)
    allg = b"".join(genomes[k] for k in sorted(genomes))
    items = []
    for i, ln in enumerate((12_000, 20_000, 150, 16_001, 40)):
        parts, have = [], 0
        while have < ln:
            if rng.random() < 0.6:
                st = int(rng.integers(0, len(allg) - 900))
                p = allg[st:st + int(rng.integers(150, 900))]
            else:
                p = synth.random_seq(rng, int(rng.integers(100, 1500)))
            parts.append(p)
            have += len(p)
        s = synth.mutate(rng, b"".join(parts)[:ln], 0.02, 0.0, 0.0)
        ql = bytearray(_qual(rng, ln, q, 40))
        for cut in (SEG_KMERS, 2 * SEG_KMERS):
            if cut + 200 < ln:
                ql[cut - 150:cut + 150] = _qual(rng, 300, 2, q - 1)
        for _ in range(ln // 2000):
            a = int(rng.integers(0, ln - 30))
            ql[a:a + 25] = _qual(rng, 25, 2, q - 1)
        items.append((b"ont%d" % i, s, bytes(ql)))
    raws = [_fastq(h, s, ql) for h, s, ql in items]
    return [b"".join(raws)], [[bm.parse_record(r, True) for r in raws]]
