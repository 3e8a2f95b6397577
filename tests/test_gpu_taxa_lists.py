"""The classifier's (taxon, count) lists at their limits (list_add, resolve_tree_big in nohuman_amd/csrc/nh_kernels.hip): 64 entries in
the hot kernel (LIST_CAP), 2048 in the second pass (BIG_LIST_CAP), NH_ECAPACITY beyond, and long lists scored on a deep tree.  The
databases are minidb images (tests/taxo_forge.py), so nothing here depends on the builder; every result is compared with the C
oracle.  tests/test_taxo_forge.py asserts on the CPU that read(N) hits exactly N distinct taxa for every N used here."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import taxo_forge as tf

pytestmark = pytest.mark.gpu
NH_ECAPACITY = -6


def _same(eng, odb, reads, paired, conf, what):
    """one batch through the engine and the oracle: the four result fields, the per-k-mer taxa, the look-ups"""
    bases, offs = orc.pack_reads(reads, paired)
    exp, lookups, etaxa, etoff = odb.classify(bases, offs, paired, conf, want_taxa=True)
    eng.reset_stats()
    got, taxa, toff = eng.classify(bases, offs, paired, conf, want_taxa=True)
    for f in ("call", "total_kmers", "clade_hits", "hit_groups"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, "%s: field %s differs at %s (got %s, oracle %s)" % (what, f, bad[:5], got[f][bad[:5]], exp[f][bad[:5]])
    assert np.array_equal(toff, etoff) and np.array_equal(taxa, etaxa), what
    st = eng.stats()
    assert st.table_lookups == int(lookups.sum()) and st.classified == int((exp["call"] != 0).sum()), what
    return exp


@pytest.fixture(scope="module")
def flat():
    from nohuman_amd import Engine
    db = tf.flat_db()
    with Engine.from_images(db["opts"], db["taxo"], db["hash"]) as eng:
        yield eng, tf.oracle_of(db)


@pytest.mark.parametrize("conf", [0.0, 0.02])
def test_around_64_distinct_taxa(flat, conf):
    """63 and 64 taxa stay in the hot kernel's list, 65 and 66 take the second pass"""
    eng, odb = flat
    for n in (63, 64, 65, 66):
        exp = _same(eng, odb, [tf.flat_read(n)], False, conf, "alone, %d taxa" % n)
        assert exp["hit_groups"][0] >= n
    short = tf.flat_short_reads()
    reads = short[:50] + [tf.flat_read(65)] + short[50:120] + [tf.flat_read(63), tf.flat_read(66)] + short[120:] + [tf.flat_read(64)]
    _same(eng, odb, reads, False, conf, "four among 200 short reads")


@pytest.mark.parametrize("n", [2047, 2048])
def test_around_2048_distinct_taxa(flat, n):
    eng, odb = flat
    exp = _same(eng, odb, [tf.flat_read(n)], False, 0.0, "single-end, the split items, %d taxa" % n)
    assert exp["call"][0] != 0 and exp["hit_groups"][0] >= n
    _same(eng, odb, [(tf.flat_read(0, 1024), tf.flat_read(1024, n))], True, 0.0, "a pair, %d taxa" % n)
    _same(eng, odb, tf.flat_short_reads() + [tf.flat_read(n)], False, 0.0, "the last of a batch of short reads, %d taxa" % n)
    _same(eng, odb, [tf.flat_read(n)], False, 0.02, "single-end, confidence 0.02, %d taxa" % n)


def _refused(fn):
    from nohuman_amd import EngineError
    with pytest.raises(EngineError) as ei:
        fn()
    assert ei.value.code == NH_ECAPACITY and "more than 2048 distinct taxa" in str(ei.value), str(ei.value)


def test_beyond_2048_distinct_taxa_is_an_error_and_the_engine_goes_on(flat, tmp_path):
    """2049 distinct taxa in one fragment: NH_ECAPACITY from classify and from a run, no records; the error word is cleared, so
    the next call on the same engine is the oracle's again"""
    eng, odb = flat
    short = tf.flat_short_reads()
    big, ok = tf.flat_read(2049), tf.flat_read(2048)
    pair = (tf.flat_read(0, 1024), tf.flat_read(1024, 2049))
    bases, offs = orc.pack_reads([big], False)
    _refused(lambda: eng.classify(bases, offs, False, 0.0))
    _same(eng, odb, [ok], False, 0.0, "single-end after the error")
    bases, offs = orc.pack_reads([pair], True)
    _refused(lambda: eng.classify(bases, offs, True, 0.0, want_taxa=True))
    _same(eng, odb, [(pair[0], tf.flat_read(1024, 2048))], True, 0.0, "a pair after the error")
    bases, offs = orc.pack_reads(short + [ok, big], False)
    _refused(lambda: eng.classify(bases, offs, False, 0.0))
    _same(eng, odb, short + [ok], False, 0.0, "the same batch without the read")
    # a whole run on a FASTQ that holds the read
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(short[:20] + [big] + short[20:40])))
    _refused(lambda: eng.run(str(fq), str(tmp_path / "out.fq")))
    _same(eng, odb, short + [ok], False, 0.0, "after the run that failed")
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(short[:20] + [ok] + short[20:40])))
    exp, _ = odb.classify(*orc.pack_reads(short[:20] + [ok] + short[20:40], False), False, 0.0)
    st = eng.run(str(fq), str(tmp_path / "out2.fq"))
    assert (st.total_sequences, st.classified) == (41, int((exp["call"] != 0).sum()))


@pytest.fixture(scope="module")
def chain():
    from nohuman_amd import Engine
    db = tf.chain_db()
    with Engine.from_images(db["opts"], db["taxo"], db["hash"]) as eng:
        yield eng, tf.oracle_of(db), db


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_long_lists_on_a_deep_tree(chain, paired):
    """caterpillar(200): lists of 70 to 140 taxa whose ancestors are in the list too, scored and climbed by resolve_tree_big"""
    eng, odb, db = chain
    reads = db["reads"][paired]
    inner = {db["tax"].internal[tf.C(i)] for i in range(1, tf.CHAIN_DEPTH + 1)}
    for conf in (0.0, 0.02, 0.3):
        exp = _same(eng, odb, reads, paired, conf, "deep tree conf=%s" % conf)
    assert {int(x) for x in exp["call"][:db["n_long"]]} & inner  # confidence 0.3: calls that climbed to an inner chain node
    keep = eng.options().minimum_hit_groups
    try:
        eng.set_options(minimum_hit_groups=3)
        odb.set(minimum_hit_groups=3)
        _same(eng, odb, reads, paired, 0.0, "deep tree, minimum_hit_groups 3")
    finally:
        eng.set_options(minimum_hit_groups=keep)
        odb.set(minimum_hit_groups=keep)
