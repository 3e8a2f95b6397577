"""The read lists on the GPU (nh_run_ex, `--calls` / `--human-ids`; nohuman_amd/csrc/nh_calls.hip): both files, byte for
byte, against the Python model of tests/calls_model.py, fed with the records as Python parses them and with the results of
Engine.classify on the same reads.  tests/test_calls_model.py asserts what the corpora contain.

The toy taxonomy has no external id of more than four digits (9606 is the largest): test_wide_taxon_ids patches the
taxonomy image to get ids of up to ten digits."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import calls_model as cm
from tests.test_gpu_mask import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
TRACE = re.compile(r"calls: (\d+) lines, (\d+) bytes; ids: (\d+) lines, (\d+) bytes built on device; (\d+) fetched to host")


def _first_diff(a, b):
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), i, a[max(0, i - 30):i + 30], b[max(0, i - 30):i + 30])


def _ext_ids(eng, n=10):
    return [eng.external_id(i) for i in range(n)]


def _results(eng, records, conf=0.0):
    from oracle import oracle as orc
    paired = len(records) == 2
    bases, offs = orc.pack_reads(cm.fragments(records), paired)
    return eng.classify(bases, offs, paired, conf)


def _inputs(tmp, name, texts, fasta=False, gz=False):
    ins = []
    for m, text in enumerate(texts):
        p = tmp / ("%s_in%d.%s%s" % (name, m + 1, "fa" if fasta else "fq", ".gz" if gz else ""))
        p.write_bytes(gzip.compress(text, 6) if gz else text)
        ins.append(str(p))
    return ins + [None] * (2 - len(ins))


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_lists(tmp, name, eng, ins, env=None, lists=True, **kw):
    """one run of `eng` on the inputs -> (calls bytes, ids bytes, stderr, the run's paths, stats); lists False: the same
    run without the two flags"""
    d = tmp / name
    d.mkdir()
    p = {x: str(d / x) for x in ("o1", "o2", "c", "i", "k", "r", "h1", "h2")}
    in1, in2 = ins
    args = dict(in2=in2, out2=p["o2"] if in2 else None, threads=4)
    if lists:
        args.update(calls=p["c"], human_ids=p["i"])
    for k, v in kw.items():
        args[k] = p[v] if isinstance(v, str) and v in p else v
    errf = tmp / (name + ".stderr")
    st = _with_env(dict(env or {}, NOHUMAN_TRACE="1"), lambda: _run(lambda: eng.run(in1, p["o1"], **args), errf))
    rd = lambda q: open(q, "rb").read() if os.path.exists(q) else None  # noqa: E731
    return rd(p["c"]), rd(p["i"]), errf.read_bytes().decode(errors="replace"), p, st


def check(tmp, name, eng, texts, records, ext=None, fasta=False, gz=False, env=None, both_kinds=True, **kw):
    """a run with both lists against the model; the trace line's counts against the files.  Returns the run's stderr."""
    res = _results(eng, records, kw.get("confidence", 0.0))
    ncls = int((res["call"] != 0).sum())
    if both_kinds:
        assert ncls >= 10 and len(res) - ncls >= 10, (name, ncls, len(res))
    want_c, want_i = cm.expected(records, res, ext or _ext_ids(eng))
    got_c, got_i, err, _p, st = run_lists(tmp, name, eng, _inputs(tmp, name, texts, fasta, gz), env=env, **kw)
    assert got_c == want_c, (name, "calls", _first_diff(got_c, want_c))
    assert got_i == want_i, (name, "ids", _first_diff(got_i, want_i))
    assert st.total_sequences == len(res) and st.classified == ncls
    t = TRACE.findall(err)
    assert len(t) == 1, err[-2000:]
    assert [int(x) for x in t[0][:4]] == [len(res), len(want_c), ncls, len(want_i)], (name, t)
    return err


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025, 2049])
def test_fragment_counts(tmp_path, toy, toy_engine, n, paired):
    texts, records = cm.reads_corpus(toy[3], n, paired)
    check(tmp_path, "n%d" % n, toy_engine, texts, records)


@pytest.mark.parametrize("paired", [False, True])
def test_one_fragment(tmp_path, toy, toy_engine, paired):
    """a run of one fragment cannot hold both kinds: one run of a human read, one of a random read"""
    texts, records = cm.reads_corpus(toy[3], 64, paired)
    res = _results(toy_engine, records)
    for kind, f in (("human", int(np.argmax(res["call"] != 0))), ("other", int(np.argmax(res["call"] == 0)))):
        assert (res["call"][f] != 0) == (kind == "human")
        one = [[r[f]] for r in records]
        check(tmp_path, "one_" + kind, toy_engine, [r[0].raw for r in one], one, both_kinds=False)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("fasta", [False, True])
def test_id_and_number_edge_cases(tmp_path, toy, toy_engine, paired, fasta):
    """ids of 1 to 5 and of 300 bytes, /1 /2 /3 endings (trimmed in the paired run only), the id "/1", tabs, comments, CRLF,
    an empty sequence, reads of 9 ... 1000 bases; as FASTQ and as FASTA"""
    texts, records = cm.edge_corpus(toy[3], paired, fasta)
    check(tmp_path, "edge", toy_engine, texts, records, fasta=fasta)
    # ... and cut into batches that split the blocks of the builder
    check(tmp_path, "edge_b", toy_engine, texts, records, fasta=fasta, env={"NOHUMAN_BATCH_FRAGS": "17"})


def test_wide_taxon_ids(tmp_path, toy):
    """external ids of 1, 4, 7 and 10 digits, one above 2^32 (the toy taxonomy itself stops at four digits)"""
    from nohuman_amd import Engine
    from tests import builder_model as bm
    ob, tb, hb, genomes, _ = toy
    texts, records = cm.reads_corpus(genomes, 300, False, seed=5)
    with Engine.from_images(ob, bm.patch_external_ids(tb, bm.DIGIT_IDS), hb) as eng:
        assert _ext_ids(eng, len(bm.DIGIT_IDS)) == bm.DIGIT_IDS
        res = _results(eng, records)
        assert {len(str(bm.DIGIT_IDS[int(c)])) for c in res["call"] if c} >= {4, 7, 10}
        check(tmp_path, "digits", eng, texts, records, ext=bm.DIGIT_IDS)


def test_scan_carry(tmp_path, toy, toy_engine):
    """more than 256 builder blocks in one batch: the scan of the block sums takes a second round and carries the sum over"""
    text, records, unit, reps = cm.carry_corpus(toy[3])
    res = np.tile(_results(toy_engine, [unit]), reps)
    ncls = int((res["call"] != 0).sum())
    assert ncls >= 10 and len(res) - ncls >= 10 and len(res) > 256 * cm.BLOCK
    want_c, want_i = cm.expected(records, res, _ext_ids(toy_engine))
    got_c, got_i, err, _p, _st = run_lists(tmp_path, "carry", toy_engine, _inputs(tmp_path, "carry", [text]),
                                           env={"NOHUMAN_BATCH_FRAGS": str(cm.CARRY_BATCH_FRAGS)})
    assert got_c == want_c, _first_diff(got_c, want_c)
    assert got_i == want_i, _first_diff(got_i, want_i)


def test_no_human_reads_and_only_human_reads(tmp_path, toy, toy_engine):
    rng = np.random.default_rng(3)
    from tests import synth
    none = cm._build([[(b"u%d" % i, synth.random_seq(rng, 100), b"\n") for i in range(300)]])
    only = cm._build([[(b"h%d" % i, cm._human(rng, toy[3], 120), b"\n") for i in range(300)]])
    assert not (_results(toy_engine, none[1])["call"] != 0).any() and (_results(toy_engine, only[1])["call"] != 0).all()
    check(tmp_path, "none", toy_engine, *none, both_kinds=False)
    assert (tmp_path / "none" / "i").read_bytes() == b"" and (tmp_path / "none" / "c").read_bytes().count(b"\n") == 300
    check(tmp_path, "only", toy_engine, *only, both_kinds=False)
    assert (tmp_path / "only" / "i").read_bytes().count(b"\n") == 300


@pytest.mark.parametrize("paired", [False, True])
def test_agreement_with_kraken_output(tmp_path, toy, toy_engine, paired):
    """a run with -k and --calls together: `cut -f1-4` of the two files are equal"""
    texts, records = cm.edge_corpus(toy[3], paired)
    got_c, _i, _err, p, _st = run_lists(tmp_path, "k", toy_engine, _inputs(tmp_path, "k", texts), kraken_output="k")
    cut = lambda text: [ln.split(b"\t")[:4] for ln in text.splitlines()]  # noqa: E731
    assert cut(got_c) == cut(open(p["k"], "rb").read()) and len(cut(got_c)) == len(records[0])


@pytest.mark.parametrize("paired", [False, True])
def test_run_modes(tmp_path, toy, toy_engine, paired):
    """the same two lists from a normal, a -H, a split and a masked run; the runs' other outputs byte for byte what the
    same runs write without the new flags"""
    texts, records = cm.reads_corpus(toy[3], 700, paired, seed=17)
    res = _results(toy_engine, records, 0.1)
    want = cm.expected(records, res, _ext_ids(toy_engine))
    ins = _inputs(tmp_path, "m", texts)
    modes = {"normal": {}, "keep": dict(keep_human=True), "split": dict(human_out1="h1", human_out2="h2" if paired else None),
             "mask": dict(mask=True), "mask_split": dict(mask=True, human_out1="h1", human_out2="h2" if paired else None)}
    for mode, kw in modes.items():
        kw = dict(kw, confidence=0.1, kraken_output="k", report="r")
        c, i, _err, p, st = run_lists(tmp_path, mode, toy_engine, ins, **kw)
        assert (c, i) == want, (mode, _first_diff(c, want[0]), _first_diff(i, want[1]))
        _c, _i, _err, q, st0 = run_lists(tmp_path, mode + "_plain", toy_engine, ins, lists=False, **kw)
        assert _c is None and _i is None
        for x in ("o1", "o2", "k", "r", "h1", "h2"):
            assert os.path.exists(p[x]) == os.path.exists(q[x]), (mode, x)
            if os.path.exists(p[x]):
                assert open(p[x], "rb").read() == open(q[x], "rb").read(), (mode, x)
        assert (st.total_sequences, st.classified, st.total_bases) == (st0.total_sequences, st0.classified, st0.total_bases)


@pytest.mark.parametrize("slots", ["1", None])
def test_small_batches(tmp_path, toy, toy_engine, slots):
    """more than five batches (halves of the paired files used whole), on one stream slot and on the default four"""
    texts, records = cm.reads_corpus(toy[3], 1025, True, seed=19)
    env = {"NOHUMAN_BATCH_FRAGS": "100"}
    if slots:
        env["NOHUMAN_SLOTS"] = slots
    check(tmp_path, "b", toy_engine, texts, records, env=env)
    texts, records = cm.reads_corpus(toy[3], 1025, False, seed=19)
    check(tmp_path, "b_se", toy_engine, texts, records, env=dict(env, NOHUMAN_BATCH_TEXT="20000"))


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
for name, ids in (("one", [0]), ("two", [0, 1])):
    d = os.path.join(%(tmp)r, name)
    os.mkdir(d)
    engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=ids, threads=4,
               calls=os.path.join(d, "c"), human_ids=os.path.join(d, "i"))
print("CHILD OK")
"""


def test_two_logical_devices(tmp_path, toy, toy_engine):
    """NOHUMAN_FAKE_DEVICES=2: batches in turn on two logical devices, the discipline checked at every launch and copy"""
    texts, records = cm.reads_corpus(toy[3], 1025, True, seed=29)
    want = cm.expected(records, _results(toy_engine, records), _ext_ids(toy_engine))
    in1, in2 = _inputs(tmp_path, "d", texts)
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="100")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, in1=in1, in2=in2)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    for name in ("one", "two"):
        got = tuple((tmp_path / name / x).read_bytes() for x in ("c", "i"))
        assert got == want, (name, _first_diff(got[0], want[0]), _first_diff(got[1], want[1]))


@pytest.mark.parametrize("paired", [False, True])
def test_reader_on_the_gpu_fetches_only_the_lists(tmp_path, toy, toy_engine, paired):
    """gzip in, gzip out, the reader on the GPU: what came back to the host is the two lists and nothing else"""
    texts, records = cm.reads_corpus(toy[3], 1025, paired, seed=37)
    err = check(tmp_path, "gz", toy_engine, texts, records, gz=True, out_codec=2,
                env={"NOHUMAN_GZ_READER": "device", "NOHUMAN_BATCH_FRAGS": "300"})
    assert "gzip reader: GPU" in err and "host" not in [ln for ln in err.splitlines() if "gzip reader:" in ln][0], err[-2000:]
    sizes = sum(os.path.getsize(tmp_path / "gz" / x) for x in ("c", "i"))
    assert int(TRACE.findall(err)[0][4]) == sizes, (TRACE.findall(err), sizes)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli(tmp_path, toy, toy_engine):
    texts, records = cm.reads_corpus(toy[3], 300, True, seed=41)
    want = cm.expected(records, _results(toy_engine, records), _ext_ids(toy_engine))
    in1, in2 = _inputs(tmp_path, "cli", texts)
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    d = tmp_path
    args = ["-t", "4", "-o", str(d / "o_1.fq"), "-O", str(d / "o_2.fq"), "--calls", str(d / "c.tsv"), "--human-ids", str(d / "i.txt"), in1, in2]
    r = subprocess.run([BIN, "--db", DB] + args, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ((d / "c.tsv").read_bytes(), (d / "i.txt").read_bytes()) == want
    assert 'Calls table written to: "%s"' % (d / "c.tsv") in r.stderr and 'Human read ids written to: "%s"' % (d / "i.txt") in r.stderr
    assert not any(p.name.endswith(".partial") for p in d.iterdir())
    # a run that fails (three files that are no database) leaves neither file nor a .partial behind
    bad = d / "bad_db"
    bad.mkdir()
    for n in ("hash.k2d", "opts.k2d", "taxo.k2d"):
        (bad / n).write_bytes(b"not a database " * 8)
    for x in ("c.tsv", "i.txt", "o_1.fq", "o_2.fq"):
        os.unlink(d / x)
    r = subprocess.run([BIN, "--db", str(bad)] + args, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Failed to run kraken2" in r.stderr, r.stderr[-2000:]
    left = sorted(p.name for p in d.iterdir() if p.name.startswith(("c.tsv", "i.txt")))
    assert left == [], left
