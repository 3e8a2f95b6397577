"""Masked runs on the GPU (nh_run_mask, `--mask`): every read is written, in input order, a human read's bases replaced by
'N', its text built in HBM (nohuman_amd/csrc/nh_mask.hip).  Every case compares a masked run with the normal run and the -H
run on the same inputs, record by record; on the goldens the masked output is also built here in Python from the input
file and the oracle's calls."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.fastq_util import read_fastq
from tests.test_gpu_human_out import EXT, _golden, _read, _shapes, _stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
TRACE = re.compile(r"mask: (\d+) records masked, (\d+) written, (\d+) bytes built on device; (\d+) fetched to host; "
                   r"builder kernels ([0-9.]+) ms")
WHOLE = re.compile(r"mask: [^\n]*; (\d+) of (\d+) blocks copied whole")  # (behind what TRACE matches)
SFX = re.compile(rb" kraken:taxid\|\d+$")


def records(text, fasta=False):
    """an output's records (normalised form: one line a field) -> list of tuples of lines"""
    if not text:
        return []
    assert text.endswith(b"\n")
    lines = text[:-1].split(b"\n")
    k = 2 if fasta else 4
    assert len(lines) % k == 0
    return [tuple(lines[i:i + k]) for i in range(0, len(lines), k)]


def masked(rec):
    """a -H run's record -> the masked run's: the suffix stripped, the sequence as N"""
    h = SFX.sub(b"", rec[0])
    assert h != rec[0], rec[0]
    return (h, b"N" * len(rec[1])) + rec[2:]


def _run(fn, errf):
    saved = os.dup(2)  # the trace line: the library writes to fd 2
    fd = os.open(str(errf), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    os.close(fd)
    try:
        return fn()
    finally:
        os.dup2(saved, 2)
        os.close(saved)


def compare(tmp, name, in1, in2=None, codec=0, conf=0.0, device_ids=(0,), env=None, engine_obj=None, want_k=True,
            fasta=False, human=False):
    """normal run, -H run, masked run: every masked record is the normal run's (unclassified) or the -H run's with the
    suffix stripped and the sequence as N (classified); -k, -r and the stats are the normal run's.  human: the masked run
    also writes human outputs, compared with a split run's.  Returns (stats, trace, masked text per mate); trace[5:7]: how
    many blocks the builder copied whole, and how many there were."""
    from nohuman_amd import engine
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    os.environ["NOHUMAN_TRACE"] = "1"
    try:
        tags = ("n", "h", "m") + (("s",) if human else ())
        paths, stats = {}, {}
        for tag in tags:
            d = tmp / ("%s_%s" % (name, tag))
            d.mkdir()
            paths[tag] = {x: str(d / (x + EXT[codec])) for x in ("o1", "o2", "h1", "h2")}
            paths[tag].update(k=str(d / "k.txt"), r=str(d / "r.txt"))
        for tag in tags:
            p = paths[tag]
            kw = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"] if (want_k or tag == "n") else None,
                      report=p["r"], confidence=conf, threads=4, out_codec=codec, keep_human=tag == "h", mask=tag == "m")
            if tag in ("s", "m") and human:
                kw.update(human_out1=p["h1"], human_out2=p["h2"] if in2 else None)
            if engine_obj is not None:
                fn = lambda: engine_obj.run(in1, p["o1"], **kw)  # noqa: E731
            else:
                fn = lambda: engine.run(DB, in1, p["o1"], device_ids=list(device_ids), **kw)  # noqa: E731
            errf = tmp / ("%s_%s.stderr" % (name, tag))
            stats[tag] = _run(fn, errf)
            if tag == "m":
                err = errf.read_bytes().decode(errors="replace")
                t = TRACE.findall(err)
                assert len(t) == 1, err[-3000:]
                w = WHOLE.findall(err)
                assert len(w) == 1, err[-3000:]
                trace = tuple(int(x) for x in t[0][:4]) + (float(t[0][4]),) + tuple(int(x) for x in w[0])
        n, h, m = paths["n"], paths["h"], paths["m"]
        calls = [ln.split(b"\t")[0] == b"C" for ln in open(n["k"], "rb").read().splitlines()]
        mates = ("1", "2") if in2 else ("1",)
        texts = {}
        for mt in mates:
            fa = fasta if mt == "1" else False
            texts[mt] = _read(m["o" + mt], codec)
            got = records(texts[mt], fa)
            nr = iter(records(_read(n["o" + mt], codec), fa))
            hr = iter(records(_read(h["o" + mt], codec), fa))
            assert len(got) == len(calls) == stats["m"].total_sequences, (name, mt, len(got), len(calls))
            for i, (rec, c) in enumerate(zip(got, calls)):
                want = masked(next(hr)) if c else next(nr)
                assert rec == want, (name, mt, i, rec[:2], want[:2])
            assert next(nr, None) is None and next(hr, None) is None, name
        if want_k:
            assert open(m["k"], "rb").read() == open(n["k"], "rb").read(), name
        assert open(m["r"], "rb").read() == open(n["r"], "rb").read(), name
        assert _stats(stats["m"]) == _stats(stats["n"]) == _stats(stats["h"]), name
        nm = len(mates)
        assert trace[0] == stats["m"].classified * nm and trace[1] == stats["m"].total_sequences * nm, (name, trace)
        assert trace[2] == sum(len(t) for t in texts.values()), (name, trace)
        if human:
            s = paths["s"]
            for mt in mates:
                assert _read(m["h" + mt], codec) == _read(s["h" + mt], codec), (name, "human mate", mt)
                assert _read(s["o" + mt], codec) == _read(n["o" + mt], codec), (name, "split non-human mate", mt)
        return stats["m"], trace, texts
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def oracle_masked(in1, in2, conf):
    """the masked output of the goldens built in Python: input records and the oracle's calls"""
    from oracle import oracle as orc
    recs = [read_fastq(p) for p in (in1, in2) if p]
    paired = in2 is not None
    frags = [tuple(r[i][2] for r in recs) if paired else recs[0][i][2] for i in range(len(recs[0]))]
    bases, offs = orc.pack_reads(frags, paired)
    out, _ = orc.OracleDB(directory=DB).classify(bases, offs, paired, conf)
    calls = out["call"] != 0
    texts = [b"".join(h + b"\n" + (b"N" * len(s) if c else s) + b"\n+\n" + q + b"\n" for (h, _i, s, q), c in zip(r, calls))
             for r in recs]
    return texts, int(calls.sum())


@pytest.mark.parametrize("codec", [0, 2, 4])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("conf", [0.0, 0.1])
def test_masked_goldens_equal_the_oracle(tmp_path, codec, paired, conf):
    in1, in2 = _golden(paired)
    st, trace, texts = compare(tmp_path, "g", in1, in2, codec=codec, conf=conf, want_k=False)
    want, ncls = oracle_masked(in1, in2, conf)
    assert 0 < st.classified == ncls < st.total_sequences
    for mt, w in zip(("1", "2"), want):
        assert texts[mt] == w, (mt, codec, paired, conf)
    if codec == 2:
        assert trace[3] == 0  # plain FASTQ into GPU gzip encoders, no -k: the masked text never leaves HBM
    else:
        assert trace[3] == trace[2]  # host encoders get exactly the built bytes, no more


def test_masked_run_on_an_opened_engine_and_host_gzip(tmp_path):
    from nohuman_amd import Engine
    in1, in2 = _golden(True)
    with Engine.open(DB) as eng:
        compare(tmp_path, "eng", in1, in2, codec=2, engine_obj=eng)
    _, trace, _ = compare(tmp_path, "hostgz", in1, in2, codec=2, env={"NOHUMAN_GZIP": "host"}, want_k=False)
    assert trace[3] == trace[2] > 0


@pytest.mark.parametrize("codec", [0, 2, 4])
def test_masked_run_with_human_outputs(tmp_path, codec):
    in1, in2 = _golden(True)
    compare(tmp_path, "pe", in1, in2, codec=codec, human=True)
    in1, _ = _golden(False)
    compare(tmp_path, "se", in1, codec=codec, human=True, want_k=False)


@pytest.mark.parametrize("reader", ["host", "device"])
@pytest.mark.parametrize("paired", [False, True])
def test_gzip_inputs_under_either_reader(tmp_path, reader, paired):
    in1, in2 = _golden(paired)
    g1 = tmp_path / "r_1.fq.gz"
    g1.write_bytes(gzip.compress(open(in1, "rb").read() * 3, 6))
    g2 = None
    if in2:
        g2 = tmp_path / "r_2.fq.gz"
        g2.write_bytes(gzip.compress(open(in2, "rb").read() * 3, 6))
    env = {"NOHUMAN_GZ_READER": reader, "NOHUMAN_GZDEV_SEG": "16384", "NOHUMAN_GZDEV_STRETCH": "2048", "NOHUMAN_BATCH_FRAGS": "100"}
    for codec in (0, 2):
        compare(tmp_path, "gzk%d" % codec, str(g1), str(g2) if g2 else None, codec=codec, env=env)
    _, trace, _ = compare(tmp_path, "gz", str(g1), str(g2) if g2 else None, codec=2, env=env, want_k=False)
    assert trace[3] == 0  # gzip -> gzip, one device, no -k: nothing is fetched to the host, whichever reader


@pytest.mark.parametrize("codec", [0, 2])
def test_record_shapes_small_batches(tmp_path, codec):
    """CRLF, "+id" lines, trailing blanks on headers, empty sequences; no final newline; halves of unequal length"""
    body = _shapes()
    p = tmp_path / "shapes.fq"
    p.write_bytes(body)
    st, _, _ = compare(tmp_path, "plain", str(p), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50"})
    assert 0 < st.classified < st.total_sequences
    p0 = tmp_path / "nofinal.fq"
    p0.write_bytes(body.rstrip(b"\r\n"))
    compare(tmp_path, "nofinal", str(p0), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "64"})
    g = tmp_path / "shapes.fq.gz"
    g.write_bytes(gzip.compress(body, 6))
    for reader in ("device", "host"):
        compare(tmp_path, "gz_" + reader, str(g), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50", "NOHUMAN_GZ_READER": reader})
    rs = read_fastq(os.path.join(GOLD, "reads_se.fq"))
    m2 = b"".join(h + b"/2\n" + s + b"\n+\n" + q + b"\n" for h, _id, s, q in rs)
    p2 = tmp_path / "shapes_2.fq"
    p2.write_bytes(m2)
    compare(tmp_path, "parts", str(p), str(p2), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50", "NOHUMAN_BATCH_TEXT": "3000"})
    # a classified fragment whose mate 1 has an empty sequence: its masked record is "header\n\n+\n\n"
    got = records(_read(tmp_path / "parts_m" / ("o1" + EXT[codec]), codec))
    calls = [ln.split(b"\t")[0] == b"C" for ln in open(tmp_path / "parts_n" / "k.txt", "rb").read().splitlines()]
    assert any(c and r[1] == b"" for r, c in zip(got, calls)), "no classified record with an empty sequence"


def test_large_batches_take_the_fast_path(tmp_path):
    """plain four-line FASTQ in batches of thousands of records: whole blocks of raw text copied, N filled in after"""
    rs = read_fastq(os.path.join(GOLD, "reads_se.fq"))
    body = b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for h, _i, s, q in rs) * 40
    p = tmp_path / "big.fq"
    p.write_bytes(body)
    for codec in (0, 2):
        st, trace, _ = compare(tmp_path, "big%d" % codec, str(p), codec=codec, want_k=False)
        assert st.total_sequences >= 4096 and st.classified > 0
        assert trace[5] == trace[6] > 1, trace  # every block copied whole, and more than one of them


def test_multiline_fasta_and_ultra_long_reads(tmp_path, toy):
    from tests import synth
    _, _, _, genomes, _ = toy
    rng = np.random.default_rng(11)
    allg = b"".join(genomes[k] for k in sorted(genomes))
    reads = []
    for ln in (300_000, 70_000, 90_000, 150, 35, 200_000, 0):
        parts = []
        while sum(map(len, parts)) < ln:
            if rng.random() < 0.6:
                st = int(rng.integers(0, len(allg) - 2000))
                parts.append(allg[st:st + int(rng.integers(200, 2000))])
            else:
                parts.append(synth.random_seq(rng, int(rng.integers(500, 3000))))
        reads.append(synth.mutate(rng, b"".join(parts)[:ln], 0.02, 0.0005, 0.0) if ln else b"")
    fa = b"".join(b">long%d desc\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads))
    fa1 = b"".join(b">one%d\n%s\n" % (i, r) for i, r in enumerate(reads) if r)
    fq = b"".join(b"@long%d\n%s\n+\n%s\n" % (i, r, b"5" * len(r)) for i, r in enumerate(reads))
    for name, data, fasta in (("r.fa", fa, True), ("one.fa", fa1, True), ("r.fq", fq, False)):
        p = tmp_path / name
        p.write_bytes(data)
        for codec in (0, 2):
            st, _, _ = compare(tmp_path, "%s_%d" % (name.replace(".", "_"), codec), str(p), codec=codec, fasta=fasta)
            assert st.classified >= 1


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.argv = ["x"]
import pathlib
from tests import test_gpu_mask as t
tmp = pathlib.Path(%(tmp)r)
for codec in (0, 2):
    _, trace, _ = t.compare(tmp, "two_%%d" %% codec, %(in1)r, %(in2)r, codec=codec, device_ids=(0, 1))
    print("TRACE", codec, trace)
_, trace, _ = t.compare(tmp, "two_h", %(in1)r, %(in2)r, codec=2, device_ids=(0, 1), human=True)
print("CHILD OK")
"""


def test_two_logical_devices(tmp_path):
    in1, in2 = _golden(True)
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="64")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), in1=in1, in2=in2)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "CHILD OK" in out.stdout
    assert "DEVICE DISCIPLINE" not in out.stderr


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_mask_equals_the_library(tmp_path):
    from nohuman_amd import engine
    in1, in2 = _golden(True)
    d = tmp_path
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--mask", "-o", str(d / "c_1.fq.gz"), "-O", str(d / "c_2.fq.gz"), in1, in2],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Masking human reads..." in r.stderr and "Removing human reads..." not in r.stderr
    engine.run(DB, in1, str(d / "l_1.fq.gz"), in2=in2, out2=str(d / "l_2.fq.gz"), threads=4, out_codec=2, mask=True)
    for m in ("1", "2"):
        assert _read(d / ("c_%s.fq.gz" % m), 2) == _read(d / ("l_%s.fq.gz" % m), 2)
    want, _ = oracle_masked(in1, in2, 0.0)
    assert _read(d / "c_1.fq.gz", 2) == want[0]
    assert not any(p.name.endswith(".partial") for p in d.iterdir())
    # with human outputs: the same masked files, the human reads beside them
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--mask", "-o", str(d / "x_1.fq"), "-O", str(d / "x_2.fq"),
                        "--human-out1", str(d / "xh_1.fq"), "--human-out2", str(d / "xh_2.fq"), in1, in2],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(d / "x_1.fq", "rb").read() == want[0]
    assert all(SFX.search(rec[0]) for rec in records(open(d / "xh_1.fq", "rb").read()))
