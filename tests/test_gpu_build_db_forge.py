"""nh_build_db on inputs forged to order (tests/build_forge.py): distinct minimizers that share a compacted key on one probe path,
probes that wrap round the table's end, tables with one empty cell, the last slot of the counting set.

With shared keys the table and its size depend on the order of insertion, so two things are held:
  * batches are inserted one launch after another, so with one record a batch (NOHUMAN_BUILD_BATCH=64: a 35-base record leaves
    less than 35 bytes of room and the next one flushes first) the order of insertion is the file's, and the table equals the
    Python model's of that order cell for cell;
  * whatever the order in which waves and lanes arrive, the table is valid (build_forge.valid_table).
Every input is checked on the CPU, before the build, to reach what it is meant to reach.  The records hold no ambiguous base: the
ambiguity rule changes nothing here."""

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import build_db_util as u
from tests import build_forge as bf
from tests import synth

pytestmark = pytest.mark.gpu
CAP = 1009
NH_ECAPACITY = -6


def build(paths, out_dir, batch=None, **kw):
    import nohuman_amd
    with pytest.MonkeyPatch.context() as mp:
        if batch is None:
            mp.delenv("NOHUMAN_BUILD_BATCH", raising=False)
        else:
            mp.setenv("NOHUMAN_BUILD_BATCH", str(batch))
        return nohuman_amd.build_db(paths, str(out_dir), **kw)


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


def assert_cells_equal(got, model_blob):
    (hdr, cells), (mhdr, mcells) = got, u.cells_of(model_blob)
    assert hdr == mhdr, (hdr, mhdr)
    bad = np.flatnonzero(cells != mcells)
    assert bad.size == 0, "cells %s: %s, the model has %s" % (bad[:8], cells[bad[:8]], mcells[bad[:8]])


@pytest.fixture(scope="module")
def shared():
    """the 40 records with shared keys at capacity 1009 and the model's tables of the file's order and of the reverse"""
    recs, mins = bf.shared_key_records(CAP, np.random.default_rng(7))
    seqs = [s for _, s in recs]
    fwd, size_f = u.model_hash(seqs, CAP)
    rev, size_r = u.model_hash(seqs[::-1], CAP)
    assert len(set(mins)) == len(recs) == 40 and size_r < size_f < 40  # order-dependent, and fewer cells than minimizers
    return dict(recs=recs, seqs=seqs, mins=mins, fwd=fwd, rev=rev, size_f=size_f, size_r=size_r)


@pytest.fixture(scope="module")
def sequential(shared, tmp_path_factory):
    """one record a batch, in the file's order and reversed"""
    tmp = tmp_path_factory.mktemp("forge_seq")
    out = {}
    for name, recs in (("fwd", shared["recs"]), ("rev", shared["recs"][::-1])):
        fa = u.write_fasta(tmp / (name + ".fa"), recs)
        out[name] = (tmp / name, build([fa], tmp / name, batch=64, capacity=CAP))
    return out


def test_sequential_batches_equal_the_model(shared, sequential):
    for name, size in (("fwd", shared["size_f"]), ("rev", shared["size_r"])):
        d, st = sequential[name]
        hdr, cells = table(d)
        assert_cells_equal((hdr, cells), shared[name])
        assert st["size"] == size == hdr[1] == int((cells != 0).sum())
        assert (st["capacity"], st["distinct_minimizers"], st["sequences"], st["kmers"], st["ambiguous_kmers"]) == (CAP, 0, 40, 40, 0)
        bf.valid_table(hdr, cells, shared["mins"], CAP)


def test_sequential_batches_counted_capacity(tmp_path):
    """no capacity given: every forged minimizer is distinct, so the count and with it the capacity are known beforehand and the
    groups can be forged for that capacity; fewer cells than minimizers"""
    n = 40
    cap = u.default_capacity(n)
    recs, mins = bf.shared_key_records(cap, np.random.default_rng(8))
    assert len(recs) == n == len(set(mins))
    seqs = [s for _, s in recs]
    model, size = u.model_hash(seqs, cap)
    assert size < n
    st = build([u.write_fasta(tmp_path / "f.fa", recs)], tmp_path / "db", batch=64)
    assert (st["distinct_minimizers"], st["capacity"], st["size"]) == (n, cap, size)
    hdr, cells = table(tmp_path / "db")
    assert_cells_equal((hdr, cells), model)
    assert hdr[1] == int((cells != 0).sum()) == size
    bf.valid_table(hdr, cells, mins, cap)


@pytest.fixture(scope="module")
def concurrent(shared, tmp_path_factory):
    """the same records in one batch: a piece (a wave) each, and joined into one record (the lanes of one wave; the k-mers across
    the joins add minimizers of their own)"""
    tmp = tmp_path_factory.mktemp("forge_conc")
    long_seq = b"".join(shared["seqs"])
    mins_long, kmers_long, amb_long = u.minimizers([long_seq])
    assert set(shared["mins"]) <= mins_long and kmers_long == 40 * 35 - 34 and amb_long == 0
    out = {}
    fa = u.write_fasta(tmp / "pieces.fa", shared["recs"])
    out["pieces"] = dict(dir=tmp / "pieces", stats=build([fa], tmp / "pieces", capacity=CAP), mins=set(shared["mins"]), kmers=40)
    fa = u.write_fasta(tmp / "long.fa", [(b"joined", long_seq)])
    out["long"] = dict(dir=tmp / "long", stats=build([fa], tmp / "long", capacity=CAP), mins=mins_long, kmers=kmers_long)
    return out


@pytest.mark.parametrize("form", ["pieces", "long"])
def test_concurrent_insertion_gives_a_valid_table(concurrent, form):
    c = concurrent[form]
    hdr, cells = table(c["dir"])
    bf.valid_table(hdr, cells, c["mins"], CAP)
    st = c["stats"]
    assert st["size"] == hdr[1] and (st["kmers"], st["ambiguous_kmers"], st["capacity"]) == (c["kmers"], 0, CAP)


@pytest.mark.parametrize("which", ["sequential_reversed", "pieces", "long"])
def test_it_is_still_a_database(shared, sequential, concurrent, which):
    import nohuman_amd
    from oracle import oracle as orc
    if which == "sequential_reversed":
        d, mins = sequential["rev"][0], set(shared["mins"])
    else:
        d, mins = concurrent[which]["dir"], concurrent[which]["mins"]
    hdr, cells = table(d)
    keys = {lit.fmix64(m) >> bf.KEY_SHIFT for m in mins}
    rng = np.random.default_rng(12)
    absent = []
    shim = u._shim()
    while len(absent) < 5:  # (a key that no minimizer of the input has is in no valid table of it)
        s = synth.random_seq(rng, 35)
        (amb, m), = lit.kmer_minimizers(shim, s)
        if not amb and lit.fmix64(m) >> bf.KEY_SHIFT not in keys:
            absent.append(s)
    reads = shared["seqs"] + absent
    bases, offs = orc.pack_reads(reads, False)
    odb = orc.OracleDB(directory=str(d))
    odb.set(minimum_hit_groups=1, ambiguity_rule=u.rule())
    exp, lookups, etaxa, etoff = odb.classify(bases, offs, False, 0.0, want_taxa=True)
    with nohuman_amd.Engine.open(str(d)) as eng:
        assert eng.db_check().non_empty_cells == hdr[1] == eng.info.size
        eng.set_options(minimum_hit_groups=1)
        eng.reset_stats()
        got, taxa, toff = eng.classify(bases, offs, False, 0.0, want_taxa=True)
        assert eng.stats().table_lookups == int(lookups.sum()) == len(reads)
    n = len(shared["seqs"])
    for f, want in (("call", 2), ("total_kmers", 1), ("clade_hits", 1), ("hit_groups", 1)):
        assert np.array_equal(got[f], exp[f]), f
        assert (got[f][:n] == want).all(), (f, got[f][:n])
    assert (got["call"][n:] == 0).all() and (got["total_kmers"][n:] == 1).all()
    assert np.array_equal(toff, etoff) and np.array_equal(taxa, etaxa)
    assert taxa.tolist() == [2] * n + [0] * len(absent)


@pytest.mark.parametrize("cap", [2, 3, 4, 5, 16, 17, 33, 64, 257])
def test_tiny_table_with_one_empty_cell(tmp_path, cap):
    """capacity - 1 records, all with the last cell as their home and keys of their own: every insertion but the first wraps, the
    last one walks the whole table, cell capacity - 2 stays empty"""
    made = bf.forge(cap, [(cap - 1, None)] * (cap - 1), np.random.default_rng(cap), distinct_keys=True)
    mins = [m for m, _ in made]
    recs = [(b"r%d" % i, r) for i, (_, r) in enumerate(made)]
    model, size = u.model_hash([r for _, r in recs], cap)
    mhdr, mcells = u.cells_of(model)
    assert size == cap - 1 and np.flatnonzero(mcells == 0).tolist() == [cap - 2]
    assert sorted(bf.probe_lengths(mcells, mins, cap).tolist()) == list(range(1, cap))
    fa = u.write_fasta(tmp_path / "t.fa", recs)
    st = build([fa], tmp_path / "one", capacity=cap)
    hdr, cells = table(tmp_path / "one")
    bf.valid_table(hdr, cells, mins, cap)
    assert st["size"] == cap - 1 == hdr[1] and st["capacity"] == cap
    u.same_table((hdr, cells), (mhdr, mcells))
    st = build([fa], tmp_path / "seq", batch=64, capacity=cap)
    assert st["size"] == cap - 1
    assert_cells_equal(table(tmp_path / "seq"), model)


def test_capacity_one_is_refused(tmp_path):
    import nohuman_amd
    ((_, rec),) = bf.forge(1, [(0, None)], np.random.default_rng(1))
    fa = u.write_fasta(tmp_path / "t.fa", [(b"r", rec)])
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([fa], tmp_path / "db", capacity=1)
    assert ei.value.code == NH_ECAPACITY and not (tmp_path / "db").exists()


def test_all_but_full_table_polls_and_succeeds(tmp_path):
    """the 20 kb genome of test_gpu_build_db.py (order-free) in a table with one empty cell: probes of more than 1024 cells, so
    lanes look at `full` on the way, and nobody has raised it"""
    recs = u.genome(1)
    seqs = [s for _, s in recs]
    mins = set(u.fast_minimizers(seqs).tolist())
    cap = len(mins) + 1
    model, size, _ = u.order_free(seqs, cap, mins)
    mhdr, mcells = u.cells_of(model)
    assert size == len(mins) and bf.probe_lengths(mcells, mins, cap).max() > 1024
    st = build([u.write_fasta(tmp_path / "g.fa", recs)], tmp_path / "db", capacity=cap)
    hdr, cells = table(tmp_path / "db")
    assert st["size"] == size == hdr[1]
    u.same_table((hdr, cells), (mhdr, mcells))
    bf.valid_table(hdr, cells, mins, cap)


def test_the_counting_sets_last_slot(tmp_path):
    """60 forged minimizers whose probes start at the last slot of the counting set at 65536, 131072 and 262144 slots, in batches
    of 20 kb: group 1 is inserted wrapping at 65536 slots and carried, wrapping, through both re-insertions; groups 2 and 3 are
    inserted wrapping at the larger sizes; every group comes again after each re-insertion and must be found, not counted"""
    recs, forged, where = bf.last_slot_records(np.random.default_rng(9))
    assert all(lit.fmix64(m) & 0x3FFFF == 0x3FFFF for m in forged) and len(set(forged)) == 60
    seqs = [s for _, s in recs]
    batches, slots = bf.counting_set_slots(seqs, 20000)
    seen_at = [sorted({slots[b] for b, batch in enumerate(batches) for i, _ in batch if i in where[g]}) for g in range(3)]
    assert seen_at == [[65536, 131072, 262144], [131072, 262144], [262144]]
    assert min(i for i, _ in batches[0]) == 0 and max(where[0][:20]) in [i for i, _ in batches[0]]  # group 1 first, in one batch
    random_mins = u.fast_minimizers([s for n, s in recs if n.startswith(b"random")])
    mins = u.fast_minimizers(seqs)
    assert len(mins) == len(np.union1d(random_mins, np.array(forged, dtype=np.uint64)))
    cap = u.default_capacity(len(mins))
    u.assert_order_free_fast(mins, cap, apart=1024)
    fa = u.write_fasta(tmp_path / "g.fa", recs)
    one = build([fa], tmp_path / "one")
    assert u.longest_run(table(tmp_path / "one")[1]) < 1024
    many = build([fa], tmp_path / "many", batch=20000)
    for st in (one, many):
        assert (st["distinct_minimizers"], st["capacity"], st["size"]) == (len(mins), cap, len(mins))
    for k in ("sequences", "bases", "kmers", "ambiguous_kmers"):
        assert one[k] == many[k], k
    u.same_table(table(tmp_path / "one"), table(tmp_path / "many"))
