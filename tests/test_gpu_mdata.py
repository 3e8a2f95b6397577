"""k_mdata_mark and k_mdata_count on the GPU (nh_minimizer_mark_device, nh_minimizer_count_device; nohuman_amd/csrc/nh_mdata.hip)
against tests/mdata_model.py: every test is one small launch of each, the bitmap compared bit for bit, the hit groups and the
counts number for number.  The shapes are the smallest at which the kernels can go wrong: no k-mer, one k-mer, one full tile of
124 k-mers, one k-mer in a second tile, many tiles; a minimizer's run across the tile border, with and without an N in it; the mate
border with and without the reset; concurrent waves on one word of the bitmap; probes that pass other keys and wrap round the
table's end; the bitmap's word border and its last, partial word; nothing to do; LDS bins and global bins."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u
from tests import mdata_model as mm
from tests import synth

pytestmark = pytest.mark.gpu
NH_EINVAL, NH_EDB = -1, -3


class Case:
    """an engine of its own beside the model of its database"""

    def __init__(self, ob, tb, hb):
        from nohuman_amd import Engine
        self.eng = Engine.from_images(ob, tb, hb)
        self.db = lit.DB.from_images(ob, tb, hb)
        self.db.ambiguity_rule = self.eng.ambiguity_rule()
        self.nodes = len(self.db.parent)

    def options(self, reset_per_mate=True, ambiguity_rule=None):
        if ambiguity_rule is None:
            ambiguity_rule = self.eng.ambiguity_rule()
        self.eng.set_options(reset_per_mate=int(reset_per_mate), ambiguity_rule=ambiguity_rule)
        self.db.reset_per_mate, self.db.ambiguity_rule = bool(reset_per_mate), ambiguity_rule

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def toy_case(toy):
    c = Case(toy[0], toy[1], toy[2])
    yield c
    c.close()


def launch(case, fragments, gap=b"\n", lead=b""):
    """mark, then count the marks -> (bitmap words, hit groups per node, marked cells per node)"""
    import torch
    eng = case.eng
    mates = len(fragments[0]) if fragments else 1
    text, starts, lens = bytearray(lead), [], []
    for f in fragments:
        assert len(f) == mates
        for s in f:
            starts.append(len(text))
            lens.append(len(s))
            text += s + gap
    n = len(text)
    t = torch.zeros(n + 8, dtype=torch.uint8)
    if n:
        t[:n] = torch.frombuffer(text, dtype=torch.uint8)
    d_text = t.cuda()
    d_s = torch.from_numpy(np.array(starts + [0], dtype=np.uint64).view(np.int64)).cuda()
    d_l = torch.from_numpy(np.array(lens + [0], dtype=np.uint32).view(np.int32)).cuda()
    nbytes = eng.minimizer_marks_bytes()
    assert nbytes == 4 * ((case.db.capacity + 31) // 32)
    d_marks = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
    d_groups = torch.zeros(case.nodes, dtype=torch.int64, device="cuda")
    d_counts = torch.zeros(case.nodes, dtype=torch.int64, device="cuda")
    assert d_text.data_ptr() % 4 == 0 and d_groups.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    eng.minimizer_mark_device(d_text.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), len(fragments), d_marks.data_ptr(),
                              d_groups.data_ptr(), paired=mates == 2)
    eng.minimizer_count_device(d_marks.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    return (d_marks.cpu().numpy().view(np.uint32), d_groups.cpu().numpy().view(np.uint64), d_counts.cpu().numpy().view(np.uint64))


def check(case, fragments, model=None, **kw):
    """one launch against the model (model: mm.scan of these fragments, where the caller has it already) -> (hit groups per node,
    the marked cells, hit groups per fragment) of the model"""
    marks, groups, counts = launch(case, fragments, **kw)
    want_groups, marked, per_fragment = model if model is not None else mm.scan(case.db, fragments)
    want_marks = mm.bitmap(case.db, marked)
    bad = np.flatnonzero(marks != want_marks)
    assert bad.size == 0, "bitmap words %s: %s, the model has %s" % (bad[:8], marks[bad[:8]], want_marks[bad[:8]])
    assert np.array_equal(groups, want_groups), (groups, want_groups)
    assert np.array_equal(counts, mm.cells_by_value(case.db, marked)), (counts, mm.cells_by_value(case.db, marked))
    cap = case.db.capacity
    if cap % 32:
        assert int(marks[-1]) >> (cap % 32) == 0  # no bit at or above the capacity
    return want_groups, marked, per_fragment


def long_genome(toy):
    return b"".join(g.replace(b"N", b"") for _, g in sorted(toy[3].items()))


@pytest.mark.parametrize("length", [34, 35, 158, 159, 5000])
def test_read_lengths(toy, toy_case, length):
    """no k-mer, one k-mer, one full tile (124 k-mers), one k-mer in a second tile, many tiles; at every residue of the start mod 4"""
    g = long_genome(toy)
    assert len(g) > 5100
    frags = [(g[17 + 101 * i:17 + 101 * i + length],) for i in range(1 if length == 5000 else 4)]
    model = mm.scan(toy_case.db, frags)
    for r in range(4):
        groups, marked, per_fragment = check(toy_case, frags, model, lead=b"#" * r)
    assert (int(groups.sum()) == 0) == (length == 34)
    if length == 5000:
        assert min(per_fragment) > 1000


@pytest.fixture(scope="module")
def planted():
    """one taxon; its genome holds a low-complexity stretch of 80 bases: every k-mer inside it has one minimizer"""
    rng = np.random.default_rng(71)
    genome = synth.random_seq(rng, 150) + b"A" * 80 + synth.random_seq(rng, 150)
    hashb, _ = u.model_hash([genome], 1009)
    c = Case(minidb.opts_bytes(), u.taxonomy().to_bytes(), hashb)
    yield c, genome
    c.close()


def test_a_run_across_the_tile_border_is_one_hit_group(planted):
    """the read's k-mers 110 .. 155 lie inside the stretch: one run over the border between k-mers 123 and 124"""
    case, genome = planted
    read = genome[40:290]
    default = case.eng.ambiguity_rule()
    for rule in (0, 1):
        case.options(ambiguity_rule=rule)
        km = lit.kmer_minimizers(case.db, read)
        assert len({m for _, m in km[110:156]}) == 1 and not any(a for a, _ in km[110:156])
        starts = [i for i in range(1, len(km)) if km[i][1] != km[i - 1][1]]
        assert not any(110 < i < 156 for i in starts)  # the tile border at 124 is no run start
        _, _, per_fragment = check(case, [(read,)])
        assert per_fragment == [len(starts) + 1]
        # an N in the middle of the run: the k-mers that hold it are ambiguous, both sides have the one minimizer
        with_n = read[:150] + b"N" + read[151:]
        km = lit.kmer_minimizers(case.db, with_n)
        clean = [m for a, m in km if not a]
        assert any(a for a, _ in km[116:151]) and not km[110][0] and not km[155][0] and km[110][1] == km[155][1]
        _, _, per_n = check(case, [(with_n,)])
        assert per_n == [1 + sum(1 for i in range(1, len(clean)) if clean[i] != clean[i - 1])]
        # ... and right on the tile border
        with_n = read[:130] + b"N" + read[131:]
        check(case, [(with_n,)])
    case.options(ambiguity_rule=default)


def test_the_mate_border(toy, toy_case):
    """mate 2 equal to mate 1, a read of one k-mer: two hit groups with the reset, one without; one distinct minimizer"""
    g = long_genome(toy)
    read = g[200:235]
    try:
        for reset, want in ((True, 2), (False, 1)):
            toy_case.options(reset_per_mate=reset)
            groups, marked, per_fragment = check(toy_case, [(read, read)])
            assert per_fragment == [want] and len(marked) == 1 and int(groups.sum()) == want
            # the same as two single reads: two fragments, two groups
            groups, marked, per_fragment = check(toy_case, [(read,), (read,)])
            assert per_fragment == [1, 1] and len(marked) == 1
            # a short mate 1 (no k-mer) keeps nothing from the fragment before it, long mates carry across many tiles
            check(toy_case, [(g[300:560], g[300:560]), (g[:20], g[300:560]), (g[300:560], g[:20])])
    finally:
        toy_case.options(reset_per_mate=True)


def test_64_copies_of_one_read(toy, toy_case):
    """concurrent waves set the same bits: the bitmap is idempotent, the groups add up"""
    g = long_genome(toy)
    read = g[500:650]
    one, marked1, _ = check(toy_case, [(read,)])
    many, marked, _ = check(toy_case, [(read,)] * 64)
    assert np.array_equal(many, one * np.uint64(64)) and marked == marked1 and len(marked) > 10


def test_forged_minimizers(toy):
    """records whose probes pass other keys, and probes that wrap round the table's end: the mark is on the cell where the key was
    found; cells 31, 32 and the last cell of a table of 61"""
    from tests import build_forge as bf
    rng = np.random.default_rng(5)
    cap = 61
    recs, mins = bf.shared_key_records(cap, rng, filler=4)
    more = bf.forge(cap, [(31, None), (32, None), (cap - 1, None)], rng, exclude=mins)
    seqs = [r for _, r in recs] + [r for _, r in more]
    hashb, _ = u.model_hash(seqs, cap)
    case = Case(minidb.opts_bytes(), u.taxonomy().to_bytes(), hashb)
    try:
        case.options(ambiguity_rule=u.rule())
        _, marked, per_fragment = check(case, [(s,) for s in seqs])
        assert per_fragment == [1] * len(seqs)
        homes = {lit.fmix64(m) % cap for m in mins}
        assert {31, 32, cap - 1} <= marked and marked - homes, "no mark off a home cell: the case shows nothing"
        assert any(mm.find(case.db, m)[1] < lit.fmix64(m) % cap for m in mins), "no probe wraps"
        # word 0's last bit, word 1's first, and the last word's bits alone
        for cell in (31, 32, cap - 1):
            (seq,) = [r for m, r in more if mm.find(case.db, m)[1] == cell][:1] or [None]
            if seq is not None:
                marks, _, _ = launch(case, [(seq,)])
                assert [int(w) for w in marks] == [1 << (cell & 31) if i == cell >> 5 else 0 for i in range(2)]
        # count with no bitmap: the cells of the table
        import torch
        d_counts = torch.zeros(case.nodes, dtype=torch.int64, device="cuda")
        case.eng.minimizer_count_device(0, d_counts.data_ptr())
        torch.cuda.synchronize()
        assert d_counts.cpu().numpy().tolist() == [0, 0, case.eng.info.size]
    finally:
        case.close()


def test_nothing_to_do(toy_case):
    """a read without a hit, and an empty batch: nothing is written"""
    rng = np.random.default_rng(9)
    for frags in ([(synth.random_seq(rng, 300),)], []):
        marks, groups, counts = launch(toy_case, frags)
        assert not marks.any() and not groups.any() and not counts.any()


def test_all_cells(toy_case):
    """d_marks NULL: the cells of the table per value, as the downloaded table has them; their sum is the header's size"""
    import torch
    from tests import build_taxa_util as t
    eng = toy_case.eng
    d_counts = torch.zeros(toy_case.nodes, dtype=torch.int64, device="cuda")
    eng.minimizer_count_device(0, d_counts.data_ptr())
    torch.cuda.synchronize()
    got = d_counts.cpu().numpy().tolist()
    assert got == t.value_counts(eng.download_table(), int(eng.info.value_bits), toy_case.nodes)
    assert sum(got) == eng.info.size and got == mm.cells_by_value(toy_case.db).tolist()


def test_lower_case_bases(toy, toy_case):
    g = long_genome(toy)
    read = g[700:1000]
    upper, marked_u, _ = check(toy_case, [(read,)])
    lower, marked_l, _ = check(toy_case, [(read.lower(),), (read[:150] + read[150:].lower(),)])
    assert marked_l == marked_u and np.array_equal(lower, upper * np.uint64(2))


def test_more_than_4096_nodes():
    """the global bins of k_mdata_count, marked and all cells: the heap of 4095 taxa (4097 nodes, 13 value bits)"""
    import torch
    from tests import taxo_forge as tf
    c = tf.top_case(4095)
    case = Case(minidb.opts_bytes(), c["tax"].to_bytes(), c["model"])
    try:
        assert case.nodes == 4097 and case.db.value_bits == 13
        case.options(ambiguity_rule=u.rule())
        seqs = sorted({s for recs in c["records"].values() for _, s in recs})
        groups, marked, _ = check(case, [(s,) for s in seqs] + [(seqs[0] + seqs[1],)])
        assert int((groups != 0).sum()) >= 12 and len(marked) == c["size"]  # every cell of the table is hit
        d_counts = torch.zeros(case.nodes, dtype=torch.int64, device="cuda")
        case.eng.minimizer_count_device(0, d_counts.data_ptr())
        torch.cuda.synchronize()
        got = d_counts.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, mm.cells_by_value(case.db)) and int(got.sum()) == c["size"] == case.eng.info.size
    finally:
        case.close()


def test_a_chain_of_200(toy):
    """a deep taxonomy of 401 nodes (the LDS bins with many of them in use): long reads over many taxa, single-end and paired"""
    from tests import taxo_forge as tf
    c = tf.chain_db()
    case = Case(c["opts"], c["taxo"], c["hash"])
    try:
        case.options(ambiguity_rule=u.rule())
        groups, _, _ = check(case, [(r,) for r in c["reads"][False][:6] + c["reads"][False][40:60]])
        assert int((groups != 0).sum()) > 100
        check(case, [tuple(p) for p in c["reads"][True][:3] + c["reads"][True][40:50]])
    finally:
        case.close()


def test_another_geometry_is_refused():
    import torch
    from nohuman_amd import Engine, EngineError
    ob, tb, hb, _, _ = synth.toy_db(k=31, l=27)
    with Engine.from_images(ob, tb, hb) as eng:
        buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
        with pytest.raises(EngineError) as ei:
            eng.minimizer_mark_device(buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr())
        assert ei.value.code == NH_EDB and "k is 31" in ei.value.message
        with pytest.raises(EngineError) as ei:
            eng.minimizer_count_device(buf.data_ptr(), buf.data_ptr())
        assert ei.value.code == NH_EDB
        assert not buf.any()


def test_no_linear_probing_is_refused(toy):
    import torch
    from nohuman_amd import Engine, EngineError
    with Engine.from_images(toy[0], toy[1], toy[2]) as eng:
        eng.set_options(linear_probing=0)
        buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
        with pytest.raises(EngineError) as ei:
            eng.minimizer_mark_device(buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr())
        assert ei.value.code == NH_EINVAL and "linear_probing" in ei.value.message
        assert not buf.any()
