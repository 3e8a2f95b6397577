"""A run that the host refuses in a later batch while earlier batches are in flight (nh_run.hip: the shutdown of the pipeline).
A FASTQ of 300 short records whose record 171 has a quality line one byte shorter than its sequence, batches of 50: a plain run
passes such a record through; with a minimum base quality, or with read statistics, the fourth batch is refused before anything
of it is launched (NH_EIO, the message names the file, the read and what cannot be done), the three batches before it are
drained and the run returns.  The same engine then runs the golden file of the same shape and writes the golden bytes: slots,
buffers and the engine's streams were given back.  Every case is a child process with a time limit: a hang fails the case."""
import gzip
import json
import os
import subprocess
import sys

import pytest

from tests.fastq_util import read_fastq
from tests.test_gpu_run import _expected, _fastq_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
N_RECORDS, BAD = 300, 171
NH_EIO = -2
# shape -> (paired, the run's keywords; a value that names a file of the run is replaced by its path)
SHAPES = {
    "single": (False, {}),
    "paired": (True, {}),
    "split_gzip": (True, {"human_out1": "h1", "human_out2": "h2", "out_codec": 2}),
    "masked": (False, {"mask": True}),
}

CHILD = r"""
import json, os, sys
spec = json.load(open(sys.argv[1]))
sys.path.insert(0, spec["root"])
os.environ["NOHUMAN_BATCH_FRAGS"] = "50"
from nohuman_amd import Engine, EngineError
res = {}
with Engine.open(spec["db"]) as eng:
    def go(name, ins, **feature):
        d = os.path.join(spec["tmp"], name)
        os.mkdir(d)
        kw = {k: os.path.join(d, v) if isinstance(v, str) else v for k, v in spec["kw"].items()}
        if ins[1]:
            kw.update(in2=ins[1], out2=os.path.join(d, "o2"))
        try:
            st = eng.run(ins[0], os.path.join(d, "o1"), threads=4, **kw, **feature)
            res[name] = {"ok": True, "total": st.total_sequences, "classified": st.classified}
        except EngineError as e:
            res[name] = {"ok": False, "code": e.code, "message": e.message}
    go("control", spec["bad"])
    go("minq", spec["bad"], min_base_quality=10)
    go("good_after_minq", spec["good"])
    go("rstats", spec["bad"], read_stats=os.path.join(spec["tmp"], "rstats.tsv"))
    go("good_after_rstats", spec["good"])
json.dump(res, open(os.path.join(spec["tmp"], "result.json"), "w"))
print("CHILD OK")
"""


def _bad_inputs(tmp, paired):
    """300 records a file, the golden reads in turn under ids of their own; the last file's record 171 lacks a quality"""
    ins = []
    for m, name in enumerate(("reads_pe_1.fq", "reads_pe_2.fq") if paired else ("reads_se.fq",)):
        src = read_fastq(os.path.join(GOLD, name))
        last = m == (1 if paired else 0)
        text = b""
        for i in range(N_RECORDS):
            _h, _rid, seq, quals = src[i % len(src)]
            if last and i + 1 == BAD:
                quals = quals[:-1]
            text += b"@r%d/%d\n%s\n+\n%s\n" % (i + 1, m + 1, seq, quals)
        p = tmp / ("bad_%d.fq" % (m + 1))
        p.write_bytes(text)
        ins.append(str(p))
    return ins + [None] * (2 - len(ins))


def _golden_files(shape, paired):
    """what a run of `shape` writes for the golden reads: {file of the run: bytes}"""
    _, ext, _recs, calls = _expected("expected_pe.json" if paired else "expected_se.json", 0.0)
    want = {}
    for m, name in enumerate(("reads_pe_1.fq", "reads_pe_2.fq") if paired else ("reads_se.fq",)):
        reads = read_fastq(os.path.join(GOLD, name))
        assert len(reads) == len(calls)
        kept = [i for i, c in enumerate(calls) if not c]
        if shape == "masked":  # every record; a classified one's bases as N
            want["o%d" % (m + 1)] = _fastq_bytes([(h, rid, b"N" * len(seq) if calls[i] else seq, q) for i, (h, rid, seq, q) in enumerate(reads)])
            continue
        want["o%d" % (m + 1)] = _fastq_bytes([reads[i] for i in kept])
        if shape == "split_gzip":
            human = [i for i, c in enumerate(calls) if c]
            want["h%d" % (m + 1)] = _fastq_bytes([reads[i] for i in human], [b" kraken:taxid|%d" % ext[calls[i]] for i in human])
    return want, len(calls), sum(1 for c in calls if c)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_refused_batch_behind_batches_in_flight(tmp_path, shape):
    paired, kw = SHAPES[shape]
    bad = _bad_inputs(tmp_path, paired)
    good = [os.path.join(GOLD, "reads_pe_1.fq"), os.path.join(GOLD, "reads_pe_2.fq")] if paired else [os.path.join(GOLD, "reads_se.fq"), None]
    spec = dict(root=ROOT, db=DB, tmp=str(tmp_path), kw=kw, bad=bad, good=good)
    (tmp_path / "spec.json").write_text(json.dumps(spec))
    (tmp_path / "child.py").write_text(CHILD)
    out = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "spec.json")], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads((tmp_path / "result.json").read_text())
    # a plain run passes the record through
    assert res["control"]["ok"] and res["control"]["total"] == N_RECORDS, res["control"]
    bad_file = bad[1] if paired else bad[0]
    for name, words in (("minq", "--minimum-base-quality cannot mask"), ("rstats", "--read-stats cannot count")):
        r = res[name]
        assert not r["ok"] and r["code"] == NH_EIO, (name, r)
        assert bad_file in r["message"] and "read %d:" % BAD in r["message"] and words in r["message"], (name, r)
    want, n, n_class = _golden_files(shape, paired)
    codec = kw.get("out_codec", 0)
    for name in ("good_after_minq", "good_after_rstats"):
        r = res[name]
        assert r["ok"] and (r["total"], r["classified"]) == (n, n_class), (name, r)
        for f, data in want.items():
            got = (tmp_path / name / f).read_bytes()
            assert (gzip.decompress(got) if codec == 2 else got) == data, (shape, name, f)
