"""A plain Python model of a run with --dust-reads (nh_run_dust; k_rdust in nohuman_amd/csrc/nh_dust.hip), and the database and
corpora its tests run on.  Test helper: pure Python / numpy plus the CPU oracle; it never imports the engine.

The model masks every parsed sequence ON ITS OWN with tests/dust_model.py (and, with a minimum base quality, adds the quality
mask of tests/qmask_model.py: the union; DUST sees the original bases), gives the masked sequences to the oracle, and builds
every file of the run from the oracle's answer -- the records themselves from the ORIGINAL bases: only classification may change.
This is the pattern of tests/qmask_model.py.

  lc_db             the toy taxonomy's database built WITHOUT low-complexity masking from genomes with planted stretches (a
                    microsatellite, a poly-A run): its table holds their minimizers, as a downloaded or --no-masking database does
  masked_seq        what the classifier sees of one record
  expected          every file of a run, and its stats
  e2e_corpus / ont_corpus   the inputs of tests/test_gpu_read_dust_run.py; tests/test_rdust_model.py asserts what they contain
"""
import numpy as np

from oracle import minidb
from tests import builder_model as bm
from tests import calls_model as cm
from tests import dust_model as dm
from tests import qmask_model as qm
from tests import synth

Q_E2E = 20
SATELLITE = b"AC" * 30 + b"CAG" * 20 + b"AATGG" * 12  # 180 bases (tests/test_gpu_build_db_dust.py's)
HUMAN = 9606
_DB = {}


def lc_db(seed=17, seg=400, capacity=8009):
    """synth.toy_db with the own segment of taxon 9606 made of 1 000 bases that carry SATELLITE at 100, A x 40 at 400 and
    (GAA) x 25 at 600 -> (opts, taxo, hash, genomes, Taxonomy, the own segment); built once"""
    if seed not in _DB:
        rng = np.random.default_rng(seed)
        tax = minidb.Taxonomy(synth.TOY_EDGES)
        segs = {e: synth.random_seq(rng, seg) for e in synth.TOY_EDGES}
        own = bytearray(synth.random_seq(rng, 1000))
        own[100:280] = SATELLITE
        own[400:440] = b"A" * 40
        own[600:675] = b"GAA" * 25
        segs[HUMAN] = bytes(own)

        def lineage(e):
            out = []
            while e:
                out.append(e)
                e = synth.TOY_EDGES[e]
            return out[::-1]

        leaves = [e for e in synth.TOY_EDGES if e not in synth.TOY_EDGES.values()]
        genomes = {leaf: b"N".join(segs[a] for a in lineage(leaf)) for leaf in leaves}
        hashb, _size = minidb.build_hash(tax, sorted(genomes.items()), capacity, linear_probing=True)
        ob = minidb.opts_bytes(k=minidb.DEFAULT_K, l=minidb.DEFAULT_L, spaced_mask=None, toggle=minidb.DEFAULT_TOGGLE, min_hash=0,
                               revcom_version=1)
        _DB[seed] = (ob, tax.to_bytes(), hashb, genomes, tax, bytes(own))
    return _DB[seed]


def write_db(d):
    """lc_db as a database directory"""
    import os
    ob, tb, hb = lc_db()[:3]
    os.makedirs(d, exist_ok=True)
    for name, data in (("opts.k2d", ob), ("taxo.k2d", tb), ("hash.k2d", hb)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    return str(d)


def masked_seq(r, q=0, dust=True):
    """the bases of record r as the classifier sees them: N over DUST's mask of the record's own bases, and N where a FASTQ
    record's quality is below q"""
    s = dm.mask(bytes(r.seq)) if dust else bytes(r.seq)
    if q > 0 and r.fastq:
        s = qm.mask_seq(s, r.qual, q)
    return s


def masked_fragments(records, q=0, dust=True):
    seqs = [[masked_seq(r, q, dust) for r in recs] for recs in records]
    return list(zip(*seqs)) if len(seqs) == 2 else seqs[0]


def dust_masked_bases(records):
    return sum(dm.masked_count(bytes(r.seq)) for recs in records for r in recs)


def classify(db, records, q=0, dust=True, conf=0.0):
    from oracle import oracle as orc
    paired = len(records) == 2
    bases, offs = orc.pack_reads(masked_fragments(records, q, dust), paired)
    res, _lookups, taxa, toff = db.classify(bases, offs, paired, conf, want_taxa=True)
    return res, taxa, toff


def expected(db, records, q=0, dust=True, conf=0.0):
    """qmask_model.expected for a run with --dust-reads (dust=False: the same run without it); masked_bases: DUST's alone"""
    res, taxa, toff = classify(db, records, q, dust, conf)
    ext = db.external_ids
    calls = res["call"]
    table, ids = cm.expected(records, res, ext)
    ncls = int((calls != 0).sum())
    return dict(normal=bm.expected_outputs(records, calls, ext, "normal"), keep=bm.expected_outputs(records, calls, ext, "keep"),
                masked=bm.expected_outputs(records, calls, ext, "masked"),
                k=b"".join(ln + b"\n" for ln in qm.k_lines(records, res, taxa, toff, ext)), report=qm.report(calls), calls=table, ids=ids,
                stats=(len(calls), ncls, len(calls) - ncls, sum(r.slen for recs in records for r in recs)),
                res=res, masked_bases=dust_masked_bases(records) if dust else 0)


# ---- corpora ---------------------------------------------------------------------------------------------------------------
def _fastq(header, seq, qual):
    return b"@" + header + b"\n" + seq + b"\n+\n" + qual + b"\n"


def _fasta(header, seq, width):
    if not width:
        return b">" + header + b"\n" + seq + b"\n"
    return b">" + header + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def _qualities(rng, n, q=Q_E2E):
    """scores of q .. 40 but for ten bases of 2 .. q - 1 somewhere in a read of 40 bases or more"""
    ql = bytearray(qm._qual(rng, n, q, 40))
    if n >= 40:
        a = int(rng.integers(0, n - 10))
        ql[a:a + 10] = qm._qual(rng, 10, 2, q - 1)
    return bytes(ql)


def satellite_read(rng, a=20, n=120, flank=45):
    """a microbial-like read: n bases of the planted microsatellite between random flanks the genomes do not have"""
    return synth.random_seq(rng, flank) + SATELLITE[a:a + n] + synth.random_seq(rng, flank)


def e2e_corpus(paired, n=300, seed=81, fasta=False):
    """n fragments of five kinds in turn:
      0  a read of one of the genomes without planted stretches: classified, with or without the mask;
      1  a microbial-like read carrying 100 .. 130 bases of the planted microsatellite: host without the flag, kept with it;
      2  a read of taxon 9606's own segment that begins in the microsatellite or the poly-A run and goes on for 90 bases or more
         behind it: it stays classified, with fewer clade hits and an A: run;
      3  a random read with a stretch no genome has (T x 30, a period-2 or period-4 repeat): unclassified either way, the mask shows
         in its hit list;
      4  a random read.
    FASTQ qualities are 20 .. 40 but for ten bases below 20 somewhere in every read (a run with a minimum base quality of 20 as
    well masks those).  Mate 2 of a
    paired corpus: a random read of 50 .. 70 bases, every third with a stretch, every tenth empty -- it never carries a call.
    fasta: the same reads as FASTA records, every other one in lines of 70 bases."""
    rng = np.random.default_rng(seed)
    genomes, own = lc_db()[3], lc_db()[5]
    others = [k for k in sorted(genomes) if k != HUMAN]
    items = []
    for i in range(n):
        kind = i % 5
        if kind == 0:
            g = genomes[others[int(rng.integers(0, len(others)))]]  # (a genome without planted stretches)
            ln = int(rng.integers(100, 152))
            st = int(rng.integers(0, len(g) - ln + 1))
            s = g[st:st + ln]
        elif kind == 1:
            s = satellite_read(rng, int(rng.integers(0, 50)), int(rng.integers(100, 131)), int(rng.integers(30, 50)))
        elif kind == 2:
            st = (int(rng.integers(230, 260)), int(rng.integers(405, 425)))[(i // 5) % 2]
            s = own[st:st + 150]
        elif kind == 3:
            s = bytearray(synth.random_seq(rng, int(rng.integers(90, 161))))
            rep = (b"T" * 30, b"GT" * 20, b"ACTG" * 10)[(i // 5) % 3]
            at = int(rng.integers(0, len(s) - len(rep) + 1))
            s[at:at + len(rep)] = rep
            s = bytes(s)
        else:
            s = synth.random_seq(rng, int(rng.integers(90, 161)))
        items.append((b"f%d.k%d" % (i, kind), s))
    mates = [items]
    if paired:
        second = []
        for i, (h, _s) in enumerate(items):
            s2 = bytearray(synth.random_seq(rng, 0 if i % 10 == 9 else int(rng.integers(50, 71))))
            if i % 3 == 1 and len(s2) >= 40:
                s2[5:35] = dm.stretch(rng, 30)
            second.append((h + b"/2", bytes(s2)))
        mates = [[(h + b"/1", s) for h, s in items], second]
    texts, records = [], []
    for mate in mates:
        if fasta:
            raws = [_fasta(h, s, 70 if j % 2 else 0) for j, (h, s) in enumerate(mate)]
        else:
            raws = [_fastq(h, s, _qualities(rng, len(s))) for h, s in mate]
        texts.append(b"".join(raws))
        records.append([bm.parse_record(r, not fasta) for r in raws])
    return texts, records


def ont_corpus(seed=83):
    """ONT-like single-end reads: three of 12 .. 20 kilobases stitched from the genomes (taxon 9606's own segment with its
    planted stretches among them) and random sequence, with further stretches of 20 .. 300 bases planted every few hundred
    bases -- so stretches lie across the kernel's tile borders and the classifier's cuts --, and two short reads"""
    rng = np.random.default_rng(seed)
    genomes = lc_db()[3]
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
        if ln > 1000:
            s, _where = dm.plant(rng, s, [int(x) for x in rng.integers(20, 301, size=ln // 700)], gap=401)
        ql = bytearray(qm._qual(rng, ln, Q_E2E, 40))
        for _ in range(ln // 1500):
            a = int(rng.integers(0, ln - 30))
            ql[a:a + 25] = qm._qual(rng, 25, 2, Q_E2E - 1)
        items.append((b"ont%d" % i, s, bytes(ql)))
    raws = [_fastq(h, s, ql) for h, s, ql in items]
    return [b"".join(raws)], [[bm.parse_record(r, True) for r in raws]]
