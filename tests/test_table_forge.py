"""tests/table_forge.py on the CPU: the two CPU models (oracle/k2_oracle.c, oracle/k2_literal.py) agree on every table, geometry
and probing rule that tests/test_gpu_probe_variants.py uses, on a fixed subset of each read set (SUBSET below; for the many-taxa
tables a subset that is asserted to hold fragments of more than 64 distinct taxa and a cut read with more than 30 a segment),
and every table there has what it is for: probe_runs shows each class of look-up -- run lengths, positions in a 128-byte line,
runs round the table's end, hits behind a wrap, cycles of a double-hashing step that are shorter than the table -- non-empty.
These are conditions on the inputs, not measurements: a table or read set that misses a class is changed until it has it."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import oracle as orc
from tests import build_db_util as u
from tests import table_forge as tfg
from tests import taxo_forge


def _oracle(geom, taxo, hashb, linear=True):
    odb = orc.OracleDB(tfg.opts_of(geom), taxo, hashb)
    odb.set(ambiguity_rule=u.rule(), linear_probing=linear)
    return odb


def _literal(geom, taxo, hashb, linear=True):
    db = lit.DB.from_images(tfg.opts_of(geom), taxo, hashb)
    db.linear_probing = linear
    db.ambiguity_rule = u.rule()
    return db


@pytest.fixture(scope="module", autouse=True)
def memo_minimizers():
    """k2_literal.kmer_minimizers does not look at the table: its result per (geometry, sequence) is kept, so that the same few
    reads can be classified on hundreds of tables"""
    mp = pytest.MonkeyPatch()
    plain, memo = lit.kmer_minimizers, {}

    def kept(db, seq):
        key = (db.k, db.l, db.spaced_seed_mask, db.toggle_mask, db.revcom_version, db.ambiguity_rule, seq)
        if key not in memo:
            memo[key] = plain(db, seq)
        return memo[key]

    mp.setattr(lit, "kmer_minimizers", kept)
    yield
    mp.undo()


def _subset(reads, n):
    """every (len / n)-th read of the set -- a fixed subset over all its lengths -- and the same reads as pairs"""
    se = list(reads[::max(1, len(reads) // n)])
    return se, tfg.pairs_of(se)


def _distinct(odb, frags, paired, conf=0.0):
    """distinct taxa of every fragment, by the oracle's per-k-mer taxa"""
    bases, offs = orc.pack_reads(frags, paired)
    _, _, taxa, toff = odb.classify(bases, offs, paired, conf, want_taxa=True)
    return [len(taxo_forge.distinct_taxa(taxa[int(a):int(b)])) for a, b in zip(toff[:-1], toff[1:])]


def _models_agree(geom, taxo, hashb, linear, se, pe, conf, what):
    odb, ldb = _oracle(geom, taxo, hashb, linear), _literal(geom, taxo, hashb, linear)
    for paired, reads in ((False, se), (True, pe)):
        bases, offs = orc.pack_reads(reads, paired)
        exp, lookups, taxa, toff = odb.classify(bases, offs, paired, conf, want_taxa=True)
        for i, frag in enumerate(reads):
            got = lit.classify_fragment(ldb, frag if paired else (frag,), conf)
            assert tuple(int(x) for x in exp[i]) == got[:4], (what, paired, i)
            assert taxa[int(toff[i]):int(toff[i + 1])].tolist() == got[4], (what, paired, i)
            assert int(lookups[i]) == got[5], (what, paired, i)
    odb.close()


# How many reads of a class both models classify on every table of the class: a fixed subset over all lengths (every n-th read
# of the shuffled set: 100 / 150 / 50 of 300, as reads and as pairs), not the whole set -- k2_literal's scanner is quadratic in
# a read's length and its Get walks a full table cell by cell in Python, and the whole file stays under a minute.  The segment
# class: five of its reads that stay whole and the shortest CUT read (two segments).
SUBSET = {"generic": 100, "short": 150, "mixed": 50, "segments": 8}


def _agreement_reads(cls, geom):
    reads = tfg.reads_of(cls, geom)
    se, _ = _subset(reads, SUBSET[cls])
    if cls == "segments":
        cut = min((r for r in reads if tfg.cut_reads([r])[0]), key=len)
        se = [r for r in se if not tfg.cut_reads([r])[0]][:5] + [cut]
        assert tfg.cut_reads(se) == (1, 2)  # one read of two segments
    return se, tfg.pairs_of(se)


@pytest.mark.parametrize("geom,cls", tfg.LINEAR_CASES)
def test_models_agree_on_every_linear_table(geom, cls):
    se, pe = _agreement_reads(cls, geom)
    assert len(se) >= 6 and len(pe) >= 3
    for shape in tfg.SHAPES:
        for name, hb in tfg.tables(shape, geom, cls):
            _models_agree(geom, tfg.toy_taxo(), hb, True, se, pe, 0.0, "%s %s %s" % (geom, cls, name))


@pytest.mark.parametrize("geom", tfg.DOUBLE_GEOMS)
def test_models_agree_on_every_double_hashing_table(geom):
    se, pe = _agreement_reads("mixed", geom)
    for shape in tfg.DOUBLE_SHAPES:
        for name, hb in tfg.tables(shape, geom, "mixed"):
            _models_agree(geom, tfg.toy_taxo(), hb, False, se, pe, 0.0, "%s double %s" % (geom, name))


def _many_subset(long_reads):
    """the six longest of the reads that are not cut (600 .. 1500 bases: the ones that collect more than 64 taxa), six of the
    short ones, and with long_reads the shortest cut read"""
    reads = tfg.many_reads(long_reads)
    whole = sorted((r for r in reads if not tfg.cut_reads([r])[0]), key=len)
    se = whole[-6:] + whole[2:len(whole) // 2:10][:6]
    if long_reads:
        se.append(min((r for r in reads if tfg.cut_reads([r])[0]), key=len))
    return se, tfg.pairs_of(se[:12])


@pytest.mark.parametrize("path,geom,linear,paired,long_reads", tfg.MANY_CASES)
def test_models_agree_on_the_many_taxa_tables(path, geom, linear, paired, long_reads):
    """... on fragments that overflow the lists: at least three reads and two pairs of the subset have more than 64 distinct
    taxa on either table, and with long_reads a segment of the cut read has more than 30"""
    se, pe = _many_subset(long_reads)
    taxo = tfg.many_taxonomy().to_bytes()
    for shape, fill in tfg.MANY_TABLES:
        hb = tfg.many_table(shape, fill)
        odb = _oracle(geom, taxo, hb, linear)
        assert sum(n > 64 for n in _distinct(odb, se, False)) >= 3, (path, shape)
        assert sum(n > 64 for n in _distinct(odb, pe, True)) >= 2, (path, shape)
        if long_reads:
            bases, offs = orc.pack_reads(se[-1:], False)
            taxa = odb.classify(bases, offs, False, 0.0, want_taxa=True)[2]
            assert tfg.cut_reads(se[-1:]) == (1, 2)
            assert min(len(taxo_forge.distinct_taxa(taxa[a:a + tfg.SEG_KMERS])) for a in (0, tfg.SEG_KMERS)) > 30
        odb.close()
        for conf in (0.0, 0.05):
            _models_agree(geom, taxo, hb, linear, se, pe, conf, "%s %s" % (path, shape))


def test_the_look_ups_of_the_forge_are_the_oracles():
    """lookup_minimizers lists one minimizer a look-up: as many as the oracle counts (the min-hash cut taken off)"""
    for geom, cls in tfg.LINEAR_CASES:
        reads = tfg.reads_of(cls, geom)
        odb = _oracle(geom, tfg.toy_taxo(), tfg.table("cells257", 0.5))
        bases, offs = orc.pack_reads(reads, False)
        lookups = odb.classify(bases, offs, False, 0.0)[1]
        m = tfg._looked_up(tfg._Geom(geom), tfg.minimizers_of(geom, cls))
        assert m.size == int(lookups.sum()) and m.size > 1000, (geom, cls)
        # ... and its hash is the models' (the home cells of a few look-ups, by k2_literal)
        assert tfg.fmix64(m[:50]).tolist() == [lit.fmix64(int(x)) for x in m[:50]]


def test_random_cells_is_the_random_table_of_the_probe_slot_tests():
    rng = np.random.default_rng(5)
    for cap, fill in ((1, 1.0), (33, 0.5), (257, 0.95), (100, 1.0)):
        cells, vb = tfg.cells_of(tfg.random_cells(rng, cap, fill, 26, 9))
        vals = cells & np.uint32((1 << 26) - 1)
        assert vb == 26 and cells.size == cap and vals.max() <= 9
        if fill == 1.0:
            assert (vals != 0).all()
        else:
            assert 0 < (vals != 0).sum() < cap and ((vals == 0) == (cells == 0)).all()


def test_probe_runs_by_hand():
    """a table of 8 cells written out by hand, look-ups whose homes and keys are read off the hash"""
    vb = 8
    ms = np.arange(1, 4000, dtype=np.uint64)
    hc = tfg.fmix64(ms)
    home, key = (hc % np.uint64(8)).astype(int), (hc >> np.uint64(40)).astype(int)
    a = int(np.nonzero(home == 6)[0][0])          # home 6: cells 6, 7 (other keys), 0 (its key): a hit behind a wrap
    b = int(np.nonzero((home == 6) & (key != key[a]))[0][0])  # home 6, another key: runs on to the empty cell 2
    other = max(key) + 1
    cells = np.array([key[a] << vb | 5, other << vb | 1, 0, other << vb | 1, other << vb | 1, other << vb | 1,
                      other << vb | 1, other << vb | 1], dtype=np.uint32)
    db = lit.DB.from_images(tfg.opts_of("default"), tfg.toy_taxo(), tfg.image(cells, vb))
    r = tfg.probe_runs(db, ms[[a, b]], True)
    assert r["run"].tolist() == [2, 4] and r["hit"].tolist() == [True, False] and r["wrapped"].tolist() == [True, True]
    assert r["res32"].tolist() == [6, 6] and r["to_end"].tolist() == [2, 2] and not r["returned"].any()
    assert [db.get(int(ms[a])), db.get(int(ms[b]))] == [5, 0]
    full = cells.copy()
    full[2] = other << vb | 1
    db = lit.DB.from_images(tfg.opts_of("default"), tfg.toy_taxo(), tfg.image(full, vb))
    r = tfg.probe_runs(db, ms[[b]], True)[0]
    assert r["run"] == 8 and r["returned"] and not r["hit"]  # a full table: every cell once
    r = tfg.probe_runs(db, ms[[b]], False)[0]             # double hashing: an odd step, so all 8 cells of a power of two
    assert r["cycle"] == 8 and r["run"] == 8 and r["returned"] and r["step"] % 2 == 1


# ---- what the comb tables are for

def _comb_db(geom, cls, period, cap):
    hb = tfg.table("comb%d_%d" % (period, cap), 0.0, geom, cls)
    return hb, lit.DB.from_images(tfg.opts_of(geom), tfg.toy_taxo(), hb)


@pytest.mark.parametrize("period,cap", tfg.COMBS)
@pytest.mark.parametrize("geom,cls", tfg.LINEAR_CASES)
def test_comb_is_filler_and_stops(geom, cls, period, cap):
    hb, db = _comb_db(geom, cls, period, cap)
    cells, vb = tfg.cells_of(hb)
    stops = tfg.comb_stops(cap, period)
    rest = np.ones(cap, bool)
    rest[stops] = False
    assert cells.size == cap and vb == tfg.VB_COMB and cap % period != 0
    filler = np.unique(cells[rest] >> np.uint32(vb))
    assert filler.size == 1 and ((cells[rest] & np.uint32(255)) != 0).all()
    m = tfg._looked_up(db, tfg.minimizers_of(geom, cls))
    assert int(filler[0]) not in set((tfg.fmix64(m) >> np.uint64(32 + vb)).tolist())  # no minimizer has the filler's key
    assert (cells[stops[1::2]] == 0).all() and (cells[stops[0]] & np.uint32(255)) != 0
    assert (cells[stops[0::2]] != 0).mean() > 0.5  # (a hit stop whose stretch no minimizer calls home stays empty)


@pytest.mark.parametrize("period,cap", tfg.COMBS)
@pytest.mark.parametrize("geom,cls", tfg.LINEAR_CASES)
def test_comb_covers_every_class_of_look_up(geom, cls, period, cap):
    """every class of look-up that table_forge.comb_gaps lists is non-empty on every comb"""
    _, db = _comb_db(geom, cls, period, cap)
    gaps = tfg.comb_gaps(tfg.probe_runs(db, tfg.minimizers_of(geom, cls), True), period)
    assert not gaps, "%s %s comb %d/%d: %s" % (geom, cls, period, cap, gaps)
    # the model is the literal model's Get
    for m in np.unique(tfg._looked_up(db, tfg.minimizers_of(geom, cls)))[:200]:
        hit = tfg.probe_runs(db, [m], True)[0]["hit"]
        assert bool(db.get(int(m))) == bool(hit)


# ---- double hashing

@pytest.mark.parametrize("geom", tfg.DOUBLE_GEOMS)
def test_double_hashing_tables_end_look_ups_by_coming_back(geom):
    m = np.unique(tfg.minimizers_of(geom, "mixed"))[::4]  # (each class must show in a quarter of the look-ups already)
    short_cycle = zero_step = back_on_full = False
    for shape in tfg.DOUBLE_SHAPES:
        for name, hb in tfg.tables(shape, geom, "mixed"):
            db = _literal(geom, tfg.toy_taxo(), hb, False)
            runs = tfg.probe_runs(db, m, False)
            back = runs["returned"]
            short_cycle |= bool((back & (runs["cycle"] < db.capacity) & (runs["cycle"] > 1)).any())
            zero_step |= bool((runs["step"] == 0).any())
            back_on_full |= bool(back.any() and db.size == db.capacity and db.capacity > 1)
            if db.capacity == 1:
                assert (runs["step"] == 0).all() and (runs["cycle"] == 1).all()
            for x in np.unique(m)[:100]:
                assert bool(db.get(int(x))) == bool(tfg.probe_runs(db, [x], False)[0]["hit"])
    assert short_cycle, "no look-up came back to its first cell after fewer steps than the table has cells"
    assert zero_step, "no look-up has step = 0 (mod capacity)"
    assert back_on_full, "no look-up came back to its first cell on a full table"


# ---- many taxa: the second pass

@pytest.mark.parametrize("path,geom,linear,paired,long_reads", tfg.MANY_CASES)
def test_many_taxa_reads_overflow_the_lists(path, geom, linear, paired, long_reads):
    """more than 64 distinct taxa in some fragment (the hot kernels' list), more than 30 in some segment of a cut read (a
    segment's partial), never more than 2048 (the second pass's list)"""
    reads = tfg.many_reads(long_reads)
    taxo = tfg.many_taxonomy().to_bytes()
    for shape, fill in tfg.MANY_TABLES:
        odb = _oracle(geom, taxo, tfg.many_table(shape, fill), linear)
        for pe in ((False, True) if paired else (False,)):
            frags = tfg.pairs_of(reads) if pe else list(reads)
            bases, offs = orc.pack_reads(frags, pe)
            _, _, taxa, toff = odb.classify(bases, offs, pe, 0.0, want_taxa=True)
            per = [taxo_forge.distinct_taxa(taxa[int(a):int(b)]) for a, b in zip(toff[:-1], toff[1:])]
            assert max(len(d) for d in per) > 64, (path, shape, pe)
            assert max(len(d) for d in per) <= 2048
            if long_reads:
                n_cut, n_seg = tfg.cut_reads(frags)
                assert n_cut >= 6 and n_seg <= tfg.SEG_CAP
                seg = []
                for r, a in zip(frags, toff[:-1]):
                    nk = len(r) - 34
                    if tfg.cut_reads([r])[0]:
                        seg += [len(taxo_forge.distinct_taxa(taxa[int(a) + s:int(a) + min(s + tfg.SEG_KMERS, nk)]))
                                for s in range(0, nk, tfg.SEG_KMERS)]
                assert max(seg) > 30, (path, shape)
        odb.close()


def test_the_segment_reads_are_really_cut():
    """k_prep_items cuts reads of more than 48 tiles into segments of 32: six reads of the class, and NOHUMAN_SEG_CAP of the
    GPU cases has room for all their segments (a launch whose segments do not fit classifies those reads whole)"""
    n_cut, n_seg = tfg.cut_reads(tfg.reads_of("segments"))
    assert n_cut == 6 and 12 <= n_seg <= tfg.SEG_CAP
    assert tfg.cut_reads(tfg.reads_of("generic"))[0] == 0
