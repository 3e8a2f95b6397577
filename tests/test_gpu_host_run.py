"""The host selection end to end on the GPU (nh_run_host, `--host-taxid` / `--keep-taxid`) on tests/golden/toy_db, taxonomy
1 -> {10 -> {11 -> {111, 112}, 12}, 20 -> {21, 9606}}, with batches of 64 fragments so that every run takes several batches and
slots.  The reference runs of an input are made once, WITHOUT a selection: a plain run with --calls, -k and -r, and a keep_human
run.  What a run with a selection must write comes from tests/host_model.py applied to the input's records and the calls of the
reference run's --calls table -- never from the run under test -- and the model is first held to the two reference runs.  What
reports the call (-k, -r, --calls, the per-taxon files, nh_stats) must be byte for byte the reference run's."""
import gzip
import os
import re
import subprocess
import sys

import pytest

from tests import host_model as hm
from tests import record_model
from tests import rstats_model as rm
from tests import synth
from tests import taxout_model as tm
from tests.test_gpu_taxon_out import Env, _read, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
PARENT = dict(synth.TOY_EDGES)
EXT = {0: "", 2: ".gz", 5: ".gz"}
ENV = {"NOHUMAN_BATCH_FRAGS": "64"}
TRACE = re.compile(r"host-filter: (\d+) host, (\d+) spared fragments; kernel [0-9.]+ ms")
# (host, keep): the root alone is the run without a selection
IDENTITY = ([1], [])
SELECTIONS = [([9606], []), ([10, 20], []), ([10], [11]), ([1, 9606], [20])]


def _stats(st):
    return (st.total_sequences, st.classified, st.unclassified, st.total_bases, st.table_lookups)


class Case:
    """an input, its two reference runs and what the model needs of them"""

    def __init__(self, tmp, name, in1, in2=None, fasta=False, confidence=0.0, minq=0, device_ids=(0,)):
        self.tmp, self.name, self.in1, self.in2, self.fastq = tmp, name, str(in1), str(in2) if in2 else None, not fasta
        self.confidence, self.minq, self.device_ids = confidence, minq, list(device_ids)
        self.mates = 2 if in2 else 1
        self.runs = 0
        texts = [open(p, "rb").read() for p in (self.in1, self.in2) if p]
        self.records = [record_model.py_records(gzip.decompress(t) if t[:2] == b"\x1f\x8b" else t) for t in texts]
        d = self.ref_dir = tmp / (name + "_ref")
        d.mkdir()
        with Env(ENV):
            self.ref = _run(tmp / (name + "_ref.stderr"), **self._kw(d, kraken_output=str(d / "k.txt"), report=str(d / "r.txt"),
                                                                      calls=str(d / "calls.tsv")))
            k = tmp / (name + "_keep")
            k.mkdir()
            self.keep_stats = _run(tmp / (name + "_keep.stderr"), **self._kw(k, keep_human=True))
        for tag in ("ref", "keep"):
            assert "host-filter" not in (tmp / ("%s_%s.stderr" % (name, tag))).read_text(errors="replace")  # never without a selection
        self.keep = [(k / ("o%d" % (m + 1))).read_bytes() for m in range(self.mates)]
        rows = [ln.split(b"\t") for ln in (d / "calls.tsv").read_bytes().splitlines()]
        self.calls = [int(r[2]) for r in rows]
        self.ids = [r[1] for r in rows]
        assert len(self.calls) == len(self.records[0]) == self.ref.total_sequences
        assert sum(1 for c in self.calls if c) == self.ref.classified
        # the model against the two reference runs: without a selection every classified fragment is host
        everything = hm.host_of(PARENT, [1])
        for m in range(self.mates):
            assert (d / ("o%d" % (m + 1))).read_bytes() == hm.kept(self.records[m], self.calls, everything, self.fastq)
            assert self.keep[m] == hm.removed(self.records[m], self.calls, everything, self.fastq)

    def _kw(self, d, **more):
        kw = dict(in1=self.in1, in2=self.in2, out1=str(d / "o1"), out2=str(d / "o2") if self.in2 else None, threads=4,
                  confidence=self.confidence, min_base_quality=self.minq, device_ids=self.device_ids)
        kw.update(more)
        return kw

    def run(self, host, keep, mode="plain", codec=0, with_k=True, taxon_outs=None):
        """a run with the selection and every output its mode has -> (directory, stats, the library's stderr)"""
        self.runs += 1
        d = self.tmp / ("%s_r%d" % (self.name, self.runs))
        d.mkdir()
        e = EXT[codec]
        more = dict(out1=str(d / ("o1" + e)), out2=str(d / ("o2" + e)) if self.in2 else None, out_codec=codec, report=str(d / "r.txt"),
                    calls=str(d / "calls.tsv"), human_ids=str(d / "ids.txt"), read_stats=str(d / "rs.tsv"), host_taxids=host, keep_taxids=keep)
        if with_k:
            more["kraken_output"] = str(d / "k.txt")
        if mode == "keep_human":
            more["keep_human"] = True
        if mode in ("split", "mask+split"):
            more["human_out1"] = str(d / ("h1" + e))
            if self.in2:
                more["human_out2"] = str(d / ("h2" + e))
        if mode in ("mask", "mask+split"):
            more["mask"] = True
        if taxon_outs:
            more["taxon_outs"] = [(t, str(d / ("t%d_1%s" % (i, e))), str(d / ("t%d_2%s" % (i, e))) if self.in2 else None)
                                  for i, t in enumerate(taxon_outs)]
        errf = self.tmp / ("%s_r%d.stderr" % (self.name, self.runs))
        with Env(ENV):
            st = _run(errf, **self._kw(d, **more))
        return d, st, errf.read_text(errors="replace")

    def check(self, host, keep, mode="plain", codec=0, with_k=True, taxon_outs=None, may_be_empty=False):
        """the run's outputs against the model and the reference run -> (host fragments, spared fragments)"""
        d, st, err = self.run(host, keep, mode, codec, with_k, taxon_outs)
        hmap = hm.host_of(PARENT, host, keep)
        e = EXT[codec]
        what = (self.name, host, keep, mode, codec)
        n_host = sum(1 for c in self.calls if hm.is_host(c, hmap))
        n_spared = self.ref.classified - n_host
        for m in range(self.mates):
            recs = self.records[m]
            got = _read(d / ("o%d%s" % (m + 1, e)), codec)
            want = {"plain": hm.kept, "split": hm.kept, "keep_human": hm.removed, "mask": hm.masked, "mask+split": hm.masked}[mode]
            assert got == want(recs, self.calls, hmap, self.fastq), what + ("mate", m + 1, len(got))
            if mode in ("split", "mask+split"):
                got = _read(d / ("h%d%s" % (m + 1, e)), codec)
                assert got == hm.removed(recs, self.calls, hmap, self.fastq), what + ("host file, mate", m + 1)
                assert got == hm.filter_keep_human(self.keep[m], self.fastq, hmap), what  # the keep_human output, filtered
            for i, t in enumerate(taxon_outs or []):  # the per-taxon files follow the calls, not the selection
                files, _ = tm.partition(self.keep[m], self.fastq, PARENT, taxon_outs)
                assert _read(d / ("t%d_%d%s" % (i, m + 1, e)), codec) == files[i], what + ("per-taxon file", t, m + 1)
        assert (d / "ids.txt").read_bytes() == hm.ids(self.ids, self.calls, hmap), what
        reads = [(m, hm.is_host(c, hmap), r[1], r[2] if self.fastq else None)
                 for m in range(self.mates) for r, c in zip(self.records[m], self.calls)]
        assert (d / "rs.tsv").read_bytes() == rm.table(rm.summary(reads, self.mates)), what
        # what reports the call: byte for byte the run without a selection
        for f in ("calls.tsv", "r.txt") + (("k.txt",) if with_k else ()):
            assert (d / f).read_bytes() == (self.ref_dir / f).read_bytes(), what + (f,)
        assert _stats(st) == _stats(self.ref) == _stats(self.keep_stats), what
        assert (st.host_fragments, st.spared_fragments) == (n_host, n_spared), what
        assert st.host_fragments + st.spared_fragments == st.classified
        if taxon_outs:
            assert st.taxon_fragments == tm.partition(self.keep[0], self.fastq, PARENT, taxon_outs)[1]
        tr = TRACE.findall(err)
        assert len(tr) == 1 and (int(tr[0][0]), int(tr[0][1])) == (n_host, n_spared), err[-2000:]  # once per run with a selection
        if not may_be_empty:
            assert n_host > 0 and n_spared > 0, what  # no case passes empty
        return n_host, n_spared


def _golden(paired):
    if paired:
        return os.path.join(GOLD, "reads_pe_1.fq"), os.path.join(GOLD, "reads_pe_2.fq")
    return os.path.join(GOLD, "reads_se.fq"), None


@pytest.fixture(scope="module")
def se(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("se"), "se", *_golden(False))


@pytest.fixture(scope="module")
def pe(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("pe"), "pe", *_golden(True))


# ---- 1. the root alone is the run without a selection

@pytest.mark.parametrize("paired", [False, True])
def test_the_root_is_the_run_without_a_selection(se, pe, paired):
    c = pe if paired else se
    for mode in ("plain", "keep_human", "split"):
        d, st, err = c.run(*IDENTITY, mode=mode)
        assert (st.host_fragments, st.spared_fragments) == (c.ref.classified, 0)
        for m in range(c.mates):
            want = c.keep[m] if mode == "keep_human" else (c.ref_dir / ("o%d" % (m + 1))).read_bytes()
            assert (d / ("o%d" % (m + 1))).read_bytes() == want, (mode, m)
            if mode == "split":
                assert (d / ("h%d" % (m + 1))).read_bytes() == c.keep[m]
        for f in ("calls.tsv", "r.txt", "k.txt"):
            assert (d / f).read_bytes() == (c.ref_dir / f).read_bytes(), (mode, f)
        assert len(TRACE.findall(err)) == 1
    assert c.check(*IDENTITY, mode="mask", may_be_empty=True) == (c.ref.classified, 0)


# ---- 2. every selection, plain runs

@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("host,keep", SELECTIONS)
def test_plain_runs(se, pe, paired, host, keep):
    (pe if paired else se).check(host, keep)


# ---- 3. every kind of run

@pytest.mark.parametrize("host,keep", [SELECTIONS[0], SELECTIONS[2]])
def test_keep_human_runs(se, pe, host, keep):
    se.check(host, keep, mode="keep_human")
    pe.check(host, keep, mode="keep_human")


@pytest.mark.parametrize("host,keep", [SELECTIONS[1], SELECTIONS[3]])
def test_split_runs(se, pe, host, keep):
    se.check(host, keep, mode="split")
    pe.check(host, keep, mode="split")


@pytest.mark.parametrize("host,keep", [SELECTIONS[0], SELECTIONS[2]])
def test_masked_runs(se, pe, host, keep):
    se.check(host, keep, mode="mask")
    pe.check(host, keep, mode="mask+split")


def test_per_taxon_outputs_follow_the_calls(se, pe):
    sel = [10, 11, 9606, tm.OTHER]
    pe.check([10], [11], mode="split", taxon_outs=sel)
    se.check([1, 9606], [20], taxon_outs=sel)


@pytest.mark.parametrize("codec", [2, 5])
def test_gzip_and_bgzf_outputs(se, pe, codec):
    """without -k the GPU encoders take the kept records from HBM: a spared record there is a raw span like an unclassified one"""
    se.check([10], [11], codec=codec, with_k=False)
    pe.check([9606], [], mode="split", codec=codec, with_k=False)
    pe.check([10, 20], [], mode="mask", codec=codec)


def test_gzip_input(tmp_path, pe):
    """gzip in, gzip out: the batches of the reader on the GPU have no text on the host unless a kept record needs rewriting"""
    ins = []
    for i, p in enumerate((pe.in1, pe.in2)):
        ins.append(tmp_path / ("in%d.fq.gz" % (i + 1)))
        ins[-1].write_bytes(gzip.compress(open(p, "rb").read()))
    c = Case(tmp_path, "gz", *ins)
    assert c.calls == pe.calls
    c.check([10], [11], codec=2, with_k=False)
    c.check([1, 9606], [20], mode="split", codec=2, with_k=False)


def test_minimum_base_quality(tmp_path):
    """Q 20 on reads whose qualities are lowered over a stretch: the calls change, the selection follows the masked calls"""
    recs = record_model.py_records(open(_golden(False)[0], "rb").read())
    p = tmp_path / "q.fq"
    p.write_bytes(b"".join(h + b"\n" + s + b"\n+\n" + (b"#" * (len(q) // 2) + q[len(q) // 2:] if i % 3 == 0 else q) + b"\n"
                           for i, (h, s, q) in enumerate(recs)))
    c = Case(tmp_path, "q", p, minq=20)
    c.check([10, 20], [])
    c.check([10], [11], mode="split")


def test_fasta_input(tmp_path):
    recs = record_model.py_records(open(_golden(False)[0], "rb").read())
    p = tmp_path / "in.fa"
    p.write_bytes(b"".join(b">" + h[1:] + b"\n" + s + b"\n" for h, s, _ in recs))
    c = Case(tmp_path, "fa", p, fasta=True)
    c.check([9606], [], mode="split")
    c.check([10], [11])
    c.check([1, 9606], [20], mode="mask")


def test_a_taxid_without_reads(tmp_path, se):
    """confidence 0.5 on the reads that are not called 9606 there: the selection takes nothing, every classified read is spared"""
    first = Case(tmp_path, "half", se.in1, confidence=0.5)
    assert 0 < first.calls.count(9606) < 10 and first.ref.classified < se.ref.classified
    p = tmp_path / "no9606.fq"
    p.write_bytes(b"".join(hm.normalised(r, True) for r, c in zip(first.records[0], first.calls) if c != 9606))
    c = Case(tmp_path, "none", p, confidence=0.5)
    assert 9606 not in c.calls and c.ref.classified == first.ref.classified - first.calls.count(9606)
    for mode in ("plain", "split", "mask"):
        assert c.check([9606], [], mode=mode, may_be_empty=True) == (0, c.ref.classified)
    assert c.check([20], [21])[0] > 0  # (and a neighbour that does take some)


# ---- 4. two logical devices

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.argv = ["x"]
import pathlib
from tests import test_gpu_host_run as t
tmp = pathlib.Path(%(tmp)r)
for paired in (False, True):
    c = t.Case(tmp, "two%%d" %% paired, *t._golden(paired), device_ids=(0, 1))
    print("COUNTS", paired, c.check([10], [11], mode="split"), c.check([1, 9606], [20], mode="mask"), c.check([9606], [], codec=2))
print("CHILD OK")
"""


def test_two_logical_devices(tmp_path):
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path))
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "CHILD OK" in out.stdout
    assert "DEVICE DISCIPLINE" not in out.stderr


# ---- 5. a taxid the taxonomy does not hold

def test_unknown_taxid_is_refused_before_anything_is_written(tmp_path):
    from nohuman_amd import Engine, engine
    in1, in2 = _golden(True)
    d = tmp_path / "bad"
    d.mkdir()
    kw = dict(in2=in2, out2=str(d / "o2.fq"), kraken_output=str(d / "k.txt"), report=str(d / "r.txt"), calls=str(d / "c.tsv"),
              human_out1=str(d / "h1.fq"), human_out2=str(d / "h2.fq"))
    for sel in (dict(host_taxids=[10, 4242]), dict(host_taxids=[1], keep_taxids=[4243])):
        with pytest.raises(engine.EngineError) as ei:
            engine.run(DB, in1, str(d / "o1.fq"), **kw, **sel)
        assert ei.value.code == -1 and ("4242" in str(ei.value) or "4243" in str(ei.value))
        with Engine.open(DB) as eng:
            with pytest.raises(engine.EngineError) as ei:
                eng.run(in1, str(d / "o1.fq"), **kw, **sel)
            assert ei.value.code == -1 and "taxonomy" in str(ei.value)
            st = eng.run(in1, str(d / "x1.fq"), in2=in2, out2=str(d / "x2.fq"), host_taxids=[9606])  # the engine goes on
            assert st.host_fragments > 0 and st.spared_fragments > 0
            os.unlink(d / "x1.fq"), os.unlink(d / "x2.fq")
        assert list(d.iterdir()) == []


# ---- 6. the CLI

@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_end_to_end(tmp_path, pe):
    d = tmp_path
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)

    def cli(args):
        r = subprocess.run([BIN, "--db", DB, "-t", "4"] + args, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stderr
    plain = cli(["-o", str(d / "n_1.fq"), "-O", str(d / "n_2.fq"), pe.in1, pe.in2])
    assert "host sequences removed" not in plain and "Host clades" not in plain
    err = cli(["-o", str(d / "s_1.fq"), "-O", str(d / "s_2.fq"), "--human-out1", str(d / "h_1.fq"), "--human-out2", str(d / "h_2.fq"),
               "--host-taxid", "10", "--keep-taxid", "11", "--host-taxid", "9606", pe.in1, pe.in2])
    hmap = hm.host_of(PARENT, [10, 9606], [11])
    for m in range(2):
        assert (d / ("s_%d.fq" % (m + 1))).read_bytes() == hm.kept(pe.records[m], pe.calls, hmap, True)
        assert (d / ("h_%d.fq" % (m + 1))).read_bytes() == hm.removed(pe.records[m], pe.calls, hmap, True)
    n_host = sum(1 for c in pe.calls if hm.is_host(c, hmap))
    assert 0 < n_host < pe.ref.classified
    assert "Host clades: 10 (taxon10), 9606 (taxon9606); kept clades: 11 (taxon11)" in err, err  # the names are the database's
    lines = err.splitlines()
    at = [i for i, ln in enumerate(lines) if "sequences classified as human" in ln]
    assert len(at) == 1 and "%d / %d " % (pe.ref.classified, pe.ref.total_sequences) in lines[at[0]]
    assert ("%d host sequences removed; %d classified sequences outside the host clades kept" % (n_host, pe.ref.classified - n_host)) in lines[at[0] + 1]
    assert not any(p.name.endswith(".partial") for p in d.iterdir())
