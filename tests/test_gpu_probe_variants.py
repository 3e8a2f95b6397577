"""Every probe implementation of the classifier (nh_kernels.hip) on the hostile tables of tests/table_forge.py: GPU against the
CPU oracle, bit-exact, on records, per-k-mer taxa with their offsets and the look-up count.  Tables: random cells at capacities
from 1 cell to a few lines and fills 0.5 / 0.95 / 1.0 (tiny and FULL tables: runs that wrap, misses that end by the budget or
by coming back), and combs (runs of every length from every position in a 128-byte line, hits and misses behind a wrap).
tests/test_table_forge.py proves on the CPU that the tables and read sets have what they are here for, and that the oracle and
the literal model agree on them.

  path                                                        test
  generic kernel, probe_queue_quad<LPL=1>, 32-bit positions   test_generic_hot
  the same with 64-bit positions                              test_rerun_with_64_bit_positions (a child: NOHUMAN_FORCE_WIDE)
  k_classify_short, table copies 2 and 8                      test_short_kernel
  the short reads through the generic kernel                  test_rerun_without_the_short_read_kernel (a child: NOHUMAN_NO_SHORT)
  generic kernel fed by k_prep_items, reads cut in segments   test_segments
  probe_queue<LINEAR=true, STD=false>, per-lane rounds        test_per_lane_linear
  probe_queue<LINEAR=false>, double hashing                   test_double_hashing
  BIG second pass behind each of them                         test_second_pass
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import build_db_util as u
from tests import table_forge as tfg

pytestmark = pytest.mark.gpu

SMALL_CHUNK = 7  # NOHUMAN_FRAG_CHUNK: a wave takes 7 fragments one after the other and carries open look-ups between them


def _expect(odb, reads, paired, conf):
    """the oracle's side of _check, computed once a (table, read set) and shared by every engine opened on the table"""
    bases, offs = orc.pack_reads(reads, paired)
    exp, lookups, etaxa, etoff = odb.classify(bases, offs, paired, conf, want_taxa=True)
    return bases, offs, exp, int(lookups.sum()), etaxa, etoff


def _check(eng, expect, paired, conf, what, long_reads=False):
    bases, offs, exp, lookups, etaxa, etoff = expect
    eng.reset_stats()
    got, taxa, toff = eng.classify(bases, offs, paired, conf, want_taxa=True, long_reads=long_reads)
    for f in ("call", "total_kmers", "clade_hits", "hit_groups"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, "%s: field %s differs at %s (got %s, oracle %s)" % (
            what, f, bad[:5], got[f][bad[:5]], exp[f][bad[:5]])
    assert np.array_equal(toff, etoff), what
    assert np.array_equal(taxa, etaxa), what
    assert eng.stats().table_lookups == lookups, what
    return got


def _open(ob, tb, hb, chunk=None, copies=None, seg_cap=None, linear=True):
    """an engine opened under NOHUMAN_FRAG_CHUNK / NOHUMAN_TABLE_COPIES / NOHUMAN_SEG_CAP (read once, when an engine is
    opened), with the probing rule and the ambiguity rule of the oracle"""
    from nohuman_amd import Engine
    env = {"NOHUMAN_FRAG_CHUNK": chunk, "NOHUMAN_TABLE_COPIES": copies, "NOHUMAN_SEG_CAP": seg_cap}
    keep = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        eng = Engine.from_images(ob, tb, hb)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.set_options(linear_probing=linear, ambiguity_rule=u.rule())
    return eng


def _oracle(ob, tb, hb, linear=True):
    odb = orc.OracleDB(ob, tb, hb)
    odb.set(linear_probing=linear, ambiguity_rule=u.rule())
    return odb


def _run(shape, geom, cls, configs, paired_too=True, linear=True, long_reads=False, seg_cap=None):
    """every table of the shape under every engine configuration (copies, chunk), single-end and as pairs"""
    ob, tb = tfg.opts_of(geom), tfg.toy_taxo()
    reads = list(tfg.reads_of(cls, geom))
    for name, hb in tfg.tables(shape, geom, cls):
        odb = _oracle(ob, tb, hb, linear)
        exp = {False: _expect(odb, reads, False, 0.0)}
        if paired_too:
            exp[True] = _expect(odb, tfg.pairs_of(reads), True, 0.0)
        odb.close()
        for copies, chunk in configs:
            with _open(ob, tb, hb, chunk=chunk, copies=copies, seg_cap=seg_cap, linear=linear) as eng:
                for paired, e in exp.items():
                    _check(eng, e, paired, 0.0, "%s %s, %s: copies %s chunk %s paired %s" % (geom, cls, name, copies, chunk, paired),
                           long_reads)
    return exp[False][2]


@pytest.mark.parametrize("shape", tfg.SHAPES)
def test_generic_hot(shape):
    """Default geometry, reads of 159 to 420 bases only: every read exceeds a tile, so k_classify_short returns at once and
    the generic kernel's quad rounds (one look-up a lane) classify every chunk; every number of table copies (copy_shift 5, 4,
    3, 2 in pick_copy / probe_src and the rounds' in_line), one group a wave and several reads a wave."""
    exp = _run(shape, "default", "generic", [(c, k) for c in (1, 2, 4, 8) for k in (None, SMALL_CHUNK)])
    if shape.startswith("comb"):
        assert (exp["call"] != 0).mean() > 0.5  # the planted minimizers recur: the hit path, not only misses


@pytest.mark.parametrize("shape", tfg.SHAPES)
def test_short_kernel(shape):
    """Reads of 35 to 158 bases, k_classify_short, with 2 and 8 copies of the table (1 and 4: test_gpu_probe_slots.py)"""
    _run(shape, "default", "short", [(c, k) for c in (2, 8) for k in (None, 60)])


@pytest.mark.parametrize("shape", tfg.SHAPES)
def test_segments(shape):
    """long_reads=True: k_prep_items lists the launch's work and the generic kernel claims items.  Six reads of the set have
    more than 48 tiles and are cut into 2 to 4 segments, each of which looks its inherited minimizer up again at its start: on
    these tables that look-up runs long or round the table, and it must not be counted.
    That the reads are cut is asserted on the host only, by table_forge.cut_reads, a model of k_prep_items' rule, with
    NOHUMAN_SEG_CAP leaving room for every segment: nh_stats has no segment count.  So this test cannot notice the silent
    fall-back of launch_classify to whole reads (use_items is false when the item buffers could not be allocated or the launch
    has more fragments than split_single_cap); the results and the look-up count it compares are the same either way."""
    reads = tfg.reads_of("segments")
    n_cut, n_seg = tfg.cut_reads(reads)
    assert n_cut == 6 and n_seg <= tfg.SEG_CAP
    _run(shape, "default", "segments", [(None, None), (8, SMALL_CHUNK)], paired_too=False, long_reads=True, seg_cap=tfg.SEG_CAP)


@pytest.mark.parametrize("shape", tfg.SHAPES)
@pytest.mark.parametrize("geom", tfg.PER_LANE)
def test_per_lane_linear(geom, shape):
    """probe_queue<LINEAR=true, STD=false>: k31/l31, k40/l25 without spaced seed, revcom_version 0, and the default k/l with a
    min-hash cut (entries handed out as QTAX_SKIP while other lanes sit in long runs); reads from below k to four tiles; the
    combs are built from the minimizers of the geometry.  Two rounds of one 16-byte load (begun up to 3 cells early near a
    line's end), then up to 16 cells a round; the wrap; the budget of a full table."""
    _run(shape, geom, "mixed", [(1, None), (2, SMALL_CHUNK), (4, None), (8, SMALL_CHUNK)])


@pytest.mark.parametrize("shape", tfg.DOUBLE_SHAPES)
@pytest.mark.parametrize("geom", tfg.DOUBLE_GEOMS)
def test_double_hashing(geom, shape):
    """linear_probing=False on both sides: steps that share a factor with the capacity come back to the first cell before
    every cell was seen (capacities 96, 255, 256 and the composite ones of the other shapes), capacity 1 has step 0, and a
    full table ends every miss that way."""
    _run(shape, geom, "mixed", [(None, None), (1, SMALL_CHUNK)], linear=False)


@pytest.mark.parametrize("confidence", [0.0, 0.05])
@pytest.mark.parametrize("path,geom,linear,paired_too,long_reads", tfg.MANY_CASES)
def test_second_pass(path, geom, linear, paired_too, long_reads, confidence):
    """A tree of 161 nodes and random cells with values over all of them: long random reads collect more than 64 distinct
    taxa by chance (more than 30 in a segment of a cut read) and go to the BIG second pass, whose look-ups run on a loaded
    and on a full table; with a confidence above 0 the 2048-entry list is scored."""
    ob, tb = tfg.opts_of(geom), tfg.many_taxonomy().to_bytes()
    reads = list(tfg.many_reads(long_reads))
    for shape, fill in tfg.MANY_TABLES:
        hb = tfg.many_table(shape, fill)
        odb = _oracle(ob, tb, hb, linear)
        exp = {False: _expect(odb, reads, False, confidence)}
        if paired_too:
            exp[True] = _expect(odb, tfg.pairs_of(reads), True, confidence)
        odb.close()
        for chunk in (None, SMALL_CHUNK):
            with _open(ob, tb, hb, chunk=chunk, seg_cap=tfg.SEG_CAP if long_reads else None, linear=linear) as eng:
                for paired, e in exp.items():
                    _check(eng, e, paired, confidence, "%s %s fill %s chunk %s paired %s" % (path, shape, fill, chunk, paired),
                           long_reads)
        assert (exp[False][2]["call"] != 0).mean() > 0.5


def _child(env_name):
    """the generic-hot, short-kernel and segment cases of this file in a fresh process under a switch that is read once a
    process (as test_wide_position_variant of test_gpu_probe_slots.py does)"""
    env = dict(os.environ, **{env_name: "1"})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_probe_variants.py", "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", "test_generic_hot or test_short_kernel or test_segments"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout


def test_rerun_with_64_bit_positions():
    """NOHUMAN_FORCE_WIDE: the same tables under the quad rounds with 64-bit cell positions (the WIDE variants of both
    kernels), which only tables of 2^32 - 256 cells or more take otherwise"""
    _child("NOHUMAN_FORCE_WIDE")


def test_rerun_without_the_short_read_kernel():
    """NOHUMAN_NO_SHORT: the short reads of the same tables through the generic kernel as well"""
    _child("NOHUMAN_NO_SHORT")
