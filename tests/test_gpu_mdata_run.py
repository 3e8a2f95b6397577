"""Runs with minimizer data (nh_run_mdata / nh_run_engine_mdata, `--report-minimizer-data`, `--minimizer-table`) on the GPU
against tests/mdata_model.py: the table, the struct array and the 8-column report of a few thousand toy reads, single and paired;
every other output of the run byte for byte what it is without the feature, in every kind of run; the numbers under a minimum base
quality, over many batches and over two logical devices; the CLI end to end on a database built with --build-db --taxa."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import minidb
from oracle import oracle as orc
from tests import build_db_util as u
from tests import mdata_model as mm
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
N_SE, N_PE = 2000, 1200


def write_fastq(path, seqs, quals=None, tag="r"):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@%s%d\n%s\n+\n%s\n" % (tag.encode(), i, s, quals[i] if quals else b"I" * len(s)))
    return str(path)


class World:
    """the toy database in a directory, reads in files, and the model's numbers of them, made once"""

    def __init__(self, toy, d):
        ob, tb, hb, genomes, _ = toy
        self.dir = d
        self.db_dir = str(d / "db")
        minidb.write_db(self.db_dir, ob, tb, hb)
        self.lit = lit.DB.from_images(ob, tb, hb)
        self.lit.ambiguity_rule = u.rule()
        self.odb = orc.OracleDB(ob, tb, hb)
        self.odb.set(ambiguity_rule=u.rule())
        self.names = mm.names_of(tb)
        rng = np.random.default_rng(21)
        self.se = synth.sample_reads(rng, genomes, N_SE, len_jitter=40)
        self.pe = synth.sample_reads(rng, genomes, N_PE, paired=True, len_jitter=40)
        self.in_se = write_fastq(d / "se.fq", self.se)
        self.in_pe = (write_fastq(d / "pe_1.fq", [a for a, _ in self.pe], tag="p"), write_fastq(d / "pe_2.fq", [b for _, b in self.pe], tag="p"))
        self.num = {False: self.model([(s,) for s in self.se]), True: self.model([tuple(p) for p in self.pe])}

    def model(self, frags):
        bases, offs = orc.pack_reads([f if len(f) == 2 else f[0] for f in frags], len(frags[0]) == 2)
        res, _ = self.odb.classify(bases, offs, len(frags[0]) == 2, 0.0)
        num = mm.numbers(self.lit, frags, res["call"].tolist(), mm.c_scanner(self.odb))
        assert num["per_fragment"] == res["hit_groups"].tolist()  # the model's hit groups are the classifier's
        num["total"] = len(frags)
        return num

    def inputs(self, paired):
        return dict(in1=self.in_pe[0], in2=self.in_pe[1]) if paired else dict(in1=self.in_se)


@pytest.fixture(scope="module")
def world(toy, tmp_path_factory):
    return World(toy, tmp_path_factory.mktemp("mdata"))


@pytest.fixture(scope="module")
def engine(world):
    from nohuman_amd import Engine
    with Engine.open(world.db_dir) as eng:
        yield eng


def run(eng, world, paired, d, **kw):
    """one run into the directory d -> the stats"""
    os.makedirs(d, exist_ok=True)
    io = world.inputs(paired)
    return eng.run(io["in1"], str(d / "o_1.fq"), in2=io.get("in2"), out2=str(d / "o_2.fq") if paired else None, **kw)


def files_of(d, skip=()):
    return {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.name not in skip}


@pytest.mark.parametrize("paired", [False, True])
def test_table_struct_and_report(world, engine, tmp_path, paired):
    num = world.num[paired]
    got = []
    st = run(engine, world, paired, tmp_path / "a", report=str(tmp_path / "a" / "rep.txt"), calls=str(tmp_path / "a" / "calls.tsv"),
             report_minimizer_data=True, minimizer_table=str(tmp_path / "a" / "m.tsv"), minimizer_data=got)
    assert st.total_sequences == num["total"]
    assert (tmp_path / "a" / "m.tsv").read_text() == mm.table(world.lit, world.names, num)
    assert got == mm.taxa_list(world.lit, num)
    rep = (tmp_path / "a" / "rep.txt").read_text()
    assert rep == mm.report(world.lit, world.names, num, num["total"])
    # without the flag: the report is what it was, and columns 4 and 5 are all that differs
    run(engine, world, paired, tmp_path / "b", report=str(tmp_path / "b" / "rep.txt"))
    assert mm.drop_minimizer_columns(rep).encode() == (tmp_path / "b" / "rep.txt").read_bytes()
    # the invariants, on what the run gave
    col7 = sum(int(line.split("\t")[-1]) for line in (tmp_path / "a" / "calls.tsv").read_text().splitlines())
    assert sum(t["minimizers_own"] for t in got) == col7 == sum(num["per_fragment"]) > 10000
    assert all(t["distinct_own"] <= min(t["minimizers_own"], t["db_cells_own"]) for t in got)
    assert sum(t["db_cells_own"] for t in got) == engine.info.size
    assert any(0 < t["distinct_own"] < t["minimizers_own"] for t in got)  # repeats happen: the bitmap is not the count


MODES = {
    "plain": dict(),
    "keep_human": dict(keep_human=True),
    "split": dict(human_out1="h_1.fq", human_out2="h_2.fq"),
    "masked": dict(mask=True),
    "gzip": dict(out_codec=2, codec_threads=2),
    "bgzf": dict(out_codec=5, codec_threads=2, human_out1="h_1.fq", human_out2="h_2.fq"),
    "taxon_out": dict(taxon_outs=[(10, "t10_1.fq", "t10_2.fq"), ("other", "to_1.fq", "to_2.fq")]),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_other_output_is_unchanged(world, engine, tmp_path, mode):
    """paired; the kraken output, the report's six columns, the read lists and the read statistics ride along in every mode"""
    def kw_for(d):
        kw = dict(MODES[mode])
        for k in ("human_out1", "human_out2"):
            if k in kw:
                kw[k] = str(d / kw[k])
        if "taxon_outs" in kw:
            kw["taxon_outs"] = [(t, str(d / a), str(d / b)) for t, a, b in kw["taxon_outs"]]
        kw.update(kraken_output=str(d / "k.txt"), report=str(d / "rep.txt"), calls=str(d / "calls.tsv"), human_ids=str(d / "ids.txt"),
                  read_stats=str(d / "stats.tsv"))
        return kw
    s0 = run(engine, world, True, tmp_path / "off", **kw_for(tmp_path / "off"))
    s1 = run(engine, world, True, tmp_path / "on", minimizer_table=str(tmp_path / "on" / "m.tsv"), report_minimizer_data=True,
             **kw_for(tmp_path / "on"))
    assert (s0.total_sequences, s0.classified, s0.total_bases) == (s1.total_sequences, s1.classified, s1.total_bases)
    off, on = files_of(tmp_path / "off"), files_of(tmp_path / "on", skip=("m.tsv",))
    on["rep.txt"] = mm.drop_minimizer_columns(on["rep.txt"].decode()).encode()
    assert sorted(off) == sorted(on) and len(off) >= 7
    for name in off:
        assert off[name] == on[name], name
    assert (tmp_path / "on" / "m.tsv").read_text() == mm.table(world.lit, world.names, world.num[True])


def test_md_with_nothing_asked_for_is_nh_run_taxa(world, engine, tmp_path):
    from nohuman_amd import _lib
    run(engine, world, False, tmp_path / "ref", report=str(tmp_path / "ref" / "rep.txt"), kraken_output=str(tmp_path / "ref" / "k.txt"))
    d = tmp_path / "md"
    d.mkdir()
    a = _lib.nh_run_args()
    a.in1, a.out1 = world.in_se.encode(), str(d / "o_1.fq").encode()
    a.report, a.kraken_output = str(d / "rep.txt").encode(), str(d / "k.txt").encode()
    a.n_devices = 1
    md = _lib.nh_minimizer_data(struct_size=C.sizeof(_lib.nh_minimizer_data), n_taxa=77)
    s = _lib.nh_stats()
    rc = _lib.lib().nh_run_engine_mdata(engine.handle, C.byref(a), None, 0, None, None, None, 0, C.byref(md), C.byref(s))
    assert rc == 0, _lib.lib().nh_last_error()
    assert files_of(d) == files_of(tmp_path / "ref") and md.n_taxa == 77 and s.total_sequences == N_SE


def test_minimum_base_quality(world, engine, tmp_path):
    """reads with low-quality stretches, Q 20: the numbers are the model's on the masked sequences"""
    rng = np.random.default_rng(33)
    seqs, quals, masked = [], [], []
    for s in world.se[:600]:
        q = bytearray(b"I" * len(s))
        for _ in range(int(rng.integers(0, 3))):
            at, n = int(rng.integers(0, max(1, len(s)))), int(rng.integers(1, 30))
            q[at:at + n] = b"#" * len(q[at:at + n])
        q = bytes(q)
        assert len(q) == len(s)
        seqs.append(s)
        quals.append(q)
        masked.append(bytes(b if c >= 33 + 20 else ord("N") for b, c in zip(s, q)))
    assert sum(m != s for m, s in zip(masked, seqs)) > 200
    inp = write_fastq(tmp_path / "lowq.fq", seqs, quals)
    num = world.model([(m,) for m in masked])
    plain = world.model([(s,) for s in seqs])
    assert not np.array_equal(num["minimizers_own"], plain["minimizers_own"])
    got = []
    engine.run(inp, str(tmp_path / "o.fq"), min_base_quality=20, minimizer_table=str(tmp_path / "m.tsv"), minimizer_data=got)
    assert got == mm.taxa_list(world.lit, num)
    assert (tmp_path / "m.tsv").read_text() == mm.table(world.lit, world.names, num)


def test_many_batches(world, engine, tmp_path, monkeypatch):
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "97")
    for paired in (False, True):
        got = []
        run(engine, world, paired, tmp_path / str(paired), minimizer_data=got, report=str(tmp_path / "rep.txt"), report_minimizer_data=True)
        assert got == mm.taxa_list(world.lit, world.num[paired])
        assert (tmp_path / "rep.txt").read_text() == mm.report(world.lit, world.names, world.num[paired], world.num[paired]["total"])


CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
res = {}
for name, ids in (("one", [0]), ("two", [0, 1])):
    got = []
    t = os.path.join(%(tmp)r, name + ".tsv")
    engine.run(%(db)r, %(in1)r, os.path.join(%(tmp)r, name + "_1.fq"), in2=%(in2)r, out2=os.path.join(%(tmp)r, name + "_2.fq"),
               device_ids=ids, threads=2, minimizer_table=t, minimizer_data=got)
    res[name] = [open(t).read(), got]
print("RESULT " + json.dumps(res))
"""


def test_two_logical_devices_or_their_bitmaps(world, tmp_path):
    """batches alternate between two devices, so most minimizers are hit on both: counts added would be too large"""
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="100")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=world.db_dir, in1=world.in_pe[0], in2=world.in_pe[1])
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "DEVICE DISCIPLINE" not in out.stderr
    res = json.loads(out.stdout.split("RESULT ")[1])
    want = mm.table(world.lit, world.names, world.num[True])
    assert res["one"][0] == want and res["two"][0] == want
    assert res["two"][1] == res["one"][1] == mm.taxa_list(world.lit, world.num[True])


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_end_to_end_on_a_built_database(tmp_path):
    """--build-db --taxa with two taxa A and B under G that share a planted stretch; reads tile A at full depth: the stretch's
    minimizers show up under G, A is covered whole, B has nothing"""
    from tests import build_taxa_util as t
    rng = np.random.default_rng(44)
    G, A, B = 7000, 7001, 7002
    stretch = synth.random_seq(rng, 500)
    ga = synth.random_seq(rng, 1500) + stretch + synth.random_seq(rng, 1000)
    gb = synth.random_seq(rng, 800) + stretch + synth.random_seq(rng, 1700)
    manifest = t.write_case(tmp_path, ((G, 1, "group G"), (A, G, "taxon A"), (B, G, "taxon B")), {A: [(b"a", ga)], B: [(b"b", gb)]})
    d = tmp_path / "db"
    p = subprocess.run([BIN, "--build-db", str(d), "--taxa", manifest], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    reads = [ga[i:i + 100] for i in range(0, len(ga) - 99, 20)]
    fq = write_fastq(tmp_path / "a.fq", reads)
    p = subprocess.run([BIN, "--db", str(d), fq, "-o", str(tmp_path / "out.fq"), "-r", str(tmp_path / "rep.txt"),
                        "--report-minimizer-data", "--minimizer-table", str(tmp_path / "m.tsv")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split("\t") for ln in (tmp_path / "m.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) + "\n" == mm.HEADER
    by = {int(r[0]): dict(zip(rows[0][2:], r[2:])) for r in rows[1:]}
    assert sorted(by) == [1, G, A]  # B has no reads and no hit: no row
    # the stretch holds ~466 k-mers that A and B share: their minimizers are G's, every one of them hit
    assert int(by[G]["minimizers_own"]) > 100 and int(by[G]["distinct_own"]) == int(by[G]["db_cells_own"]) > 100
    assert by[A]["coverage_pct"] == "100.0000" and int(by[A]["distinct_own"]) == int(by[A]["db_cells_own"]) > 500
    assert int(by[A]["minimizers_own"]) > 3 * int(by[A]["distinct_own"])  # depth five
    # G's clade holds B's cells too, which nothing hit
    assert 40.0 < float(by[G]["coverage_pct"]) < 80.0 and by[1]["coverage_pct"] == by[G]["coverage_pct"]
    assert int(by[G]["db_cells_clade"]) > int(by[G]["distinct_clade"]) == int(by[G]["distinct_own"]) + int(by[A]["distinct_own"])
    rep = [ln.split("\t") for ln in (tmp_path / "rep.txt").read_text().splitlines()]
    assert all(len(r) == 8 for r in rep)
    line = {int(r[6]): r for r in rep}
    assert (int(line[G][3]), int(line[G][4])) == (int(by[G]["minimizers_clade"]), int(by[G]["distinct_clade"]))
