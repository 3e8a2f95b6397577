"""The short-read kernel's probe rounds (probe_queue_quad / probe_rounds_two_slots, nh_kernels.hip): GPU against the CPU
oracle, bit-exact, on records, per-k-mer taxa and the look-up count.  Every database here has the default geometry
(k=35, l=31) and every read fits one tile, so k_classify_short is the kernel that runs.  The cases sit where a loop that
holds one OR two look-ups per owner lane (NH_LPL) can go wrong -- queue sizes around 64 and 128, long probe runs in any
slot, look-ups carried across calls -- and hold for both builds (profiles/r07_probe_slots.txt)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

VB = 26  # value bits of the random tables: 6 key bits, unrelated minimizers match by chance all the time


def _check(eng, odb, reads, paired, conf, what):
    bases, offs = orc.pack_reads(reads, paired)
    exp, lookups, etaxa, etoff = odb.classify(bases, offs, paired, conf, want_taxa=True)
    eng.reset_stats()
    got, taxa, toff = eng.classify(bases, offs, paired, conf, want_taxa=True)
    for f in ("call", "total_kmers", "clade_hits", "hit_groups"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, "%s: field %s differs at %s (got %s, oracle %s)" % (
            what, f, bad[:5], got[f][bad[:5]], exp[f][bad[:5]])
    assert np.array_equal(toff, etoff), what
    assert np.array_equal(taxa, etaxa), what
    assert eng.stats().table_lookups == int(lookups.sum()), what
    return got


def _open(ob, tb, hb, chunk=None, copies=None):
    """an engine opened under NOHUMAN_FRAG_CHUNK / NOHUMAN_TABLE_COPIES: both are read once, when an engine is opened.
    chunk: fragments a wave claims at a time (at most 63 reads / 31 pairs).  Without it a launch too small to give every
    resident wave two chunks -- every launch of this file -- is cut into chunks of ONE batch of 4 tiles, so that each wave
    probes a single group and drains; with it a wave works through many consecutive groups and carries look-ups from one
    probe call into the next."""
    from nohuman_amd import Engine
    env = {"NOHUMAN_FRAG_CHUNK": chunk, "NOHUMAN_TABLE_COPIES": copies}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        return Engine.from_images(ob, tb, hb)
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def toy_chunked(toy):
    """the toy database in chunks of 60 reads / 31 pairs: 15 / 15 batches, that is consecutive groups, per wave"""
    ob, tb, hb, _, _ = toy
    eng = _open(ob, tb, hb, chunk=60)
    yield eng
    eng.close()


def _random_table(rng, capacity, fill):
    """hash image of `capacity` random cells (taxa 1..9 of the toy tree), a fraction `fill` of them occupied"""
    cells = np.zeros(capacity, dtype=np.uint32)
    occ = rng.random(capacity) < fill if fill < 1.0 else np.ones(capacity, bool)
    keys = rng.integers(0, 1 << 6, size=capacity, dtype=np.uint32)
    vals = rng.integers(1, 10, size=capacity, dtype=np.uint32)
    cells[occ] = ((keys[occ] << VB) | vals[occ]).astype(np.uint32)
    return struct.pack("<4Q", capacity, int(occ.sum()), 32 - VB, VB) + cells.tobytes()


def _cut(rng, genomes, ln, sub_rate=0.01):
    g = sorted(genomes)
    src = genomes[g[int(rng.integers(0, len(g)))]]
    st = int(rng.integers(0, len(src) - ln))
    s = src[st:st + ln]
    if rng.random() < 0.5:
        s = synth.revcomp(s)
    return synth.mutate(rng, s, sub_rate, 0.0, 0.0)


@pytest.mark.parametrize("seed", range(16))
def test_queue_sizes_around_the_slot_boundaries(toy, toy_oracle, toy_engine, toy_chunked, seed):
    """One launch per batch of 1 .. 9 reads (and of as many pairs with the same lengths): the groups of run starts hold
    from a handful to ~160 entries -- fewer than 64 (slot B never filled), 64 .. 128 (B partly filled), more (both
    slots refilled).  On the default engine every wave has one group (batches of 4 tiles on waves of their own); on
    the chunked one a single wave takes the whole batch: up to 5 consecutive groups, the last one of 1 or 2 tiles,
    each entered with what the one before left open."""
    _, _, _, genomes, _ = toy
    rng = np.random.default_rng(4200 + seed)
    for rep in range(2):
        for nb in (1, 2, 3, 4, 5, 8, 9):
            lens = rng.integers(35, 159, size=nb)
            if rep == 1 and seed % 4 == 0:
                lens[:] = 158  # the fullest groups: every tile has the most run starts it can have
            a = [_cut(rng, genomes, int(n)) if rng.random() < 0.5 else synth.random_seq(rng, int(n)) for n in lens]
            b = [_cut(rng, genomes, int(n)) if rng.random() < 0.5 else synth.random_seq(rng, int(n)) for n in lens]
            for name, eng in (("default", toy_engine), ("chunked", toy_chunked)):
                _check(eng, toy_oracle, a, False, 0.0, "seed %d: %d reads, %s" % (seed, nb, name))
                _check(eng, toy_oracle, list(zip(a, b)), True, 0.0, "seed %d: %d pairs, %s" % (seed, nb, name))


@pytest.mark.parametrize("capacity", [1, 17, 33, 100, 257, 4001])
def test_long_probe_runs_wrap_around_and_full_cycles(toy, capacity):
    """Random cells with 6 key bits at fills 0.5, 0.95 and 1.0: probe runs of many rounds that wrap around the end of
    the table, in whichever slot holds them; on a FULL table a miss stops after exactly one cycle (the look-up count
    and the per-k-mer taxa say so).  Single copy and staggered copies of the table, one group and many groups per wave."""
    ob, tb, _, _, _ = toy
    rng = np.random.default_rng(700 + capacity)
    for fill in (0.5, 0.95, 1.0):
        hb = _random_table(rng, capacity, fill)
        odb = orc.OracleDB(ob, tb, hb)
        reads = [synth.random_seq(rng, int(n)) for n in rng.integers(35, 159, size=300)]
        for copies in ("1", "4"):
            for chunk in (None, 60):  # one group per wave / 15 consecutive groups per wave, long runs carried between them
                with _open(ob, tb, hb, chunk=chunk, copies=copies) as eng:
                    _check(eng, odb, reads, False, 0.0,
                           "capacity %d fill %.2f copies %s chunk %s" % (capacity, fill, copies, chunk))


@pytest.fixture(scope="module")
def loaded(toy):
    """images and oracle of a table at load 0.9 (random cells, 6 key bits): one look-up in seven needs more than one
    round, so look-ups are open whenever a probe call returns"""
    ob, tb, _, _, _ = toy
    hb = _random_table(np.random.default_rng(90), 20011, 0.9)
    return ob, tb, hb, orc.OracleDB(ob, tb, hb)


@pytest.mark.parametrize("chunk", [60, 7, 24])
def test_carry_over_across_groups(loaded, chunk):
    """5 000 consecutive reads against the loaded table in chunks of 60 / 7 / 24 reads (31 / 7 / 24 pairs): a wave probes
    up to 15 groups one after the other, each call entered with the look-ups the one before left open in either slot
    (they must be resolved before it returns: the previous group is post-processed right behind it).  Reads without a
    k-mer in between make small and empty groups while both slots carry."""
    ob, tb, hb, odb = loaded
    rng = np.random.default_rng(91)
    reads = []
    for i in range(5000):
        n = int(rng.integers(0, 35)) if rng.random() < 0.08 else int(rng.integers(35, 159))
        reads.append(synth.random_seq(rng, n))
    with _open(ob, tb, hb, chunk=chunk) as eng:
        _check(eng, odb, reads, False, 0.0, "5000 reads, chunk %d" % chunk)
        _check(eng, odb, list(zip(reads[0::2], reads[1::2])), True, 0.0, "2500 pairs, chunk %d" % chunk)


def test_carry_over_across_chunks_and_a_last_chunk_of_one_pair(loaded):
    """More chunks than the grid has waves (5120 on this chip: 256 CUs x 5 workgroups x 4 waves), so that a wave
    claims further chunks behind its first and enters them with carried look-ups: 12 001 pairs in chunks of 2 are 6 001
    chunks, the last of them one pair; 24 003 reads in chunks of 4 likewise end in a chunk of three reads."""
    ob, tb, hb, odb = loaded
    rng = np.random.default_rng(94)
    seqs = [synth.random_seq(rng, int(n)) for n in rng.integers(35, 159, size=24003)]
    with _open(ob, tb, hb, chunk=2) as eng:
        _check(eng, odb, list(zip(seqs[0:24002:2], seqs[1:24002:2])), True, 0.0, "12001 pairs in chunks of 2")
    with _open(ob, tb, hb, chunk=4) as eng:
        _check(eng, odb, seqs, False, 0.0, "24003 reads in chunks of 4")


def test_single_read_and_a_last_chunk_of_one_pair(loaded):
    """the drain path alone (one read, one launch), and 73 pairs in chunks of 24: three waves with six groups each and
    a fourth whose whole launch is one pair"""
    ob, tb, hb, odb = loaded
    rng = np.random.default_rng(92)
    with _open(ob, tb, hb, chunk=24) as eng:
        for n in (35, 36, 100, 158):
            _check(eng, odb, [synth.random_seq(rng, n)], False, 0.0, "one read of %d" % n)
        pairs = [(synth.random_seq(rng, int(a)), synth.random_seq(rng, int(b)))
                 for a, b in rng.integers(35, 159, size=(24 * 3 + 1, 2))]
        _check(eng, odb, pairs, True, 0.0, "73 pairs in chunks of 24")


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("confidence", [0.0, 0.1])
def test_hits_and_misses_interleaved(toy, toy_oracle, toy_engine, toy_chunked, paired, confidence):
    """every other read cut from the inserted genomes with 1 % of its bases changed, the others random; one group per
    wave (default engine) and 15 consecutive groups per wave (chunked)"""
    _, _, _, genomes, _ = toy
    rng = np.random.default_rng(300 + int(paired))
    seqs = []
    for i in range(4000 if paired else 2000):
        n = int(rng.integers(35, 159))
        seqs.append(_cut(rng, genomes, n) if i % 2 == 0 else synth.random_seq(rng, n))
    if paired:  # hit pairs and miss pairs alternate
        seqs = [seqs[j] for i in range(0, len(seqs), 4) for j in (i, i + 2, i + 1, i + 3)]
    reads = list(zip(seqs[0::2], seqs[1::2])) if paired else seqs
    _check(toy_engine, toy_oracle, reads, paired, confidence, "paired=%s conf=%s" % (paired, confidence))
    got = _check(toy_chunked, toy_oracle, reads, paired, confidence, "paired=%s conf=%s chunked" % (paired, confidence))
    assert (got["call"] != 0).sum() > len(reads) // 4  # the hit path is really exercised


def test_wide_position_variant():
    """The first two tests of this file through the kernel variant with 64-bit cell positions, which
    NOHUMAN_FORCE_WIDE selects for small tables (once per process, hence a child)."""
    env = dict(os.environ, NOHUMAN_FORCE_WIDE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_probe_slots.py", "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "queue_sizes or long_probe_runs"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_same_batch_twice_gives_identical_records(loaded, toy_chunked):
    ob, tb, hb, _ = loaded
    rng = np.random.default_rng(93)
    reads = [synth.random_seq(rng, int(n)) for n in rng.integers(35, 159, size=3000)]
    bases, offs = orc.pack_reads(reads, False)
    with _open(ob, tb, hb, chunk=60) as eng:
        for e in (eng, toy_chunked):
            a, ta, _ = e.classify(bases, offs, False, 0.0, want_taxa=True)
            b, tb_, _ = e.classify(bases, offs, False, 0.0, want_taxa=True)
            assert a.tobytes() == b.tobytes()
            assert np.array_equal(ta, tb_)
