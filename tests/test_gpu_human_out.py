"""Split runs on the GPU (nh_run_split, `--human-out1` / `--human-out2`): one pass writes the non-human reads exactly as a
keep_human=0 run and the human reads exactly as a keep_human=1 run, their classified-out text built in HBM
(nohuman_amd/csrc/nh_split.hip).  Every case compares a split run with the two runs it replaces, on the same inputs."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.fastq_util import read_fastq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
EXT = {0: ".fq", 2: ".fq.gz", 4: ".fq.zst"}
TRACE = re.compile(r"human-out: (\d+) records, (\d+) bytes built on device; (\d+) fetched to host")


def _read(path, codec):
    raw = open(path, "rb").read()
    if codec == 2:
        assert raw[:2] == b"\x1f\x8b", path
        return gzip.decompress(raw)
    if codec == 4:
        from tests.test_codec import _zstd_decompress
        assert raw[:4] == b"\x28\xb5\x2f\xfd", path
        return _zstd_decompress(raw, 64 << 20)
    return raw


def _stats(st):
    return (st.total_sequences, st.classified, st.unclassified, st.total_bases, st.table_lookups)


def compare(tmp, name, in1, in2=None, codec=0, conf=0.0, device_ids=(0,), env=None, engine_obj=None, want_k=True):
    """keep_human=0 run, keep_human=1 run, split run: the split run's files must be theirs.  Returns (stats, trace numbers).
    want_k: with a -k file (its read ids need the batches' text on the host)."""
    from nohuman_amd import engine
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    os.environ["NOHUMAN_TRACE"] = "1"
    try:
        paths = {}
        for tag in ("n", "h", "s"):
            d = tmp / ("%s_%s" % (name, tag))
            d.mkdir()
            paths[tag] = {x: str(d / (x + EXT[codec])) for x in ("o1", "o2", "h1", "h2")}
            paths[tag].update(k=str(d / "k.txt"), r=str(d / "r.txt"))
        stats = {}
        for tag in ("n", "h", "s"):
            p = paths[tag]
            kw = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"] if want_k else None, report=p["r"], confidence=conf, threads=4,
                      out_codec=codec, keep_human=tag == "h")
            if tag == "s":
                kw.update(human_out1=p["h1"], human_out2=p["h2"] if in2 else None)
            errf = tmp / ("%s_%s.stderr" % (name, tag))  # the trace line: the library writes to fd 2
            saved = os.dup(2)
            fd = os.open(str(errf), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            os.dup2(fd, 2)
            os.close(fd)
            try:
                if engine_obj is not None:
                    stats[tag] = engine_obj.run(in1, p["o1"], **kw)
                else:
                    stats[tag] = engine.run(DB, in1, p["o1"], device_ids=list(device_ids), **kw)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            err = errf.read_bytes()
            if tag == "s":
                m = TRACE.findall(err.decode(errors="replace"))
                assert len(m) == 1, err[-3000:]
                trace = tuple(int(x) for x in m[0])
        n, h, s = paths["n"], paths["h"], paths["s"]
        mates = ("1", "2") if in2 else ("1",)
        for m in mates:
            assert _read(s["o" + m], codec) == _read(n["o" + m], codec), (name, "non-human mate", m)
            assert _read(s["h" + m], codec) == _read(h["o" + m], codec), (name, "human mate", m)
        if want_k:
            assert open(s["k"], "rb").read() == open(n["k"], "rb").read(), name
        assert open(s["r"], "rb").read() == open(n["r"], "rb").read(), name
        assert _stats(stats["s"]) == _stats(stats["n"]) == _stats(stats["h"]), name
        assert trace[0] == stats["s"].classified, (name, trace)
        built = sum(len(_read(s["h" + m], codec)) for m in mates)
        assert trace[1] == built, (name, trace, built)
        return stats["s"], trace
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _golden(paired):
    if paired:
        return os.path.join(GOLD, "reads_pe_1.fq"), os.path.join(GOLD, "reads_pe_2.fq")
    return os.path.join(GOLD, "reads_se.fq"), None


@pytest.mark.parametrize("codec", [0, 2, 4])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("conf", [0.0, 0.5])
def test_split_run_equals_the_two_runs(tmp_path, codec, paired, conf):
    """the toy multi-taxon database: external ids of one to four digits in the suffix"""
    in1, in2 = _golden(paired)
    st, trace = compare(tmp_path, "c", in1, in2, codec=codec, conf=conf)
    assert 0 < st.classified < st.total_sequences
    if codec == 2:
        assert trace[2] == 0  # plain FASTQ into GPU gzip encoders: the built text never leaves HBM
    else:
        assert trace[2] == trace[1]  # host encoders get exactly the built bytes, no more


def test_split_run_on_an_opened_engine_and_host_gzip(tmp_path):
    from nohuman_amd import Engine
    in1, in2 = _golden(True)
    with Engine.open(DB) as eng:
        compare(tmp_path, "eng", in1, in2, codec=2, engine_obj=eng)
    _, trace = compare(tmp_path, "hostgz", in1, in2, codec=2, env={"NOHUMAN_GZIP": "host"})
    assert trace[2] == trace[1] > 0


@pytest.mark.parametrize("reader", ["host", "device"])
@pytest.mark.parametrize("paired", [False, True])
def test_gzip_inputs_under_either_reader(tmp_path, reader, paired):
    def plain_plus(path):  # the goldens' "+id" lines made plain: a kept "+id" record makes the writer fetch its batch's text
        lines = open(path, "rb").read().split(b"\n")
        return b"\n".join(b"+" if i % 4 == 2 else ln for i, ln in enumerate(lines))
    in1, in2 = _golden(paired)
    g1 = tmp_path / "r_1.fq.gz"
    g1.write_bytes(gzip.compress(plain_plus(in1) * 3, 6))
    g2 = None
    if in2:
        g2 = tmp_path / "r_2.fq.gz"
        g2.write_bytes(gzip.compress(plain_plus(in2) * 3, 6))
    env = {"NOHUMAN_GZ_READER": reader, "NOHUMAN_GZDEV_SEG": "16384", "NOHUMAN_GZDEV_STRETCH": "2048", "NOHUMAN_BATCH_FRAGS": "100"}
    compare(tmp_path, "gzk", str(g1), str(g2) if g2 else None, codec=2, env=env)
    _, trace = compare(tmp_path, "gz", str(g1), str(g2) if g2 else None, codec=2, env=env, want_k=False)
    # gzip -> gzip, one device, no -k: neither side's text is fetched to the host, whichever reader
    assert trace[2] == 0
    compare(tmp_path, "gzplain", str(g1), str(g2) if g2 else None, codec=0, env=env)


def _shapes():
    """the record shapes the host parser normalises: CRLF, "+id" lines, trailing blanks on headers, empty sequences"""
    rs = read_fastq(os.path.join(GOLD, "reads_se.fq"))
    parts = []
    for i, (h, _id, s, q) in enumerate(rs):
        kind = i % 6
        nl, plus = (b"\r\n", b"+") if kind == 0 else (b"\n", b"+" + h[1:] if kind == 1 else b"+")
        if kind == 2:
            h = h + b" some description\t x  "
        if kind == 3:
            s, q = b"", b""
        parts.append(h + nl + s + nl + plus + nl + q + nl)
    return b"".join(parts)


@pytest.mark.parametrize("codec", [0, 2])
def test_record_shapes_small_batches(tmp_path, codec):
    body = _shapes()
    p = tmp_path / "shapes.fq"
    p.write_bytes(body)
    compare(tmp_path, "plain", str(p), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50"})
    g = tmp_path / "shapes.fq.gz"
    g.write_bytes(gzip.compress(body, 6))
    for reader in ("device", "host"):
        compare(tmp_path, "gz_" + reader, str(g), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50", "NOHUMAN_GZ_READER": reader})
    # paired: mate 2 is the original read, so that a fragment whose mate 1 has an EMPTY sequence is still classified through
    # its mate 2 and its empty record goes to human_out1; halves used in parts (batches cut by text)
    rs = read_fastq(os.path.join(GOLD, "reads_se.fq"))
    m2 = b"".join(h + b"/2\n" + s + b"\n+\n" + q + b"\n" for h, _id, s, q in rs)
    p2 = tmp_path / "shapes_2.fq"
    p2.write_bytes(m2)
    compare(tmp_path, "parts", str(p), str(p2), codec=codec, env={"NOHUMAN_BATCH_FRAGS": "50", "NOHUMAN_BATCH_TEXT": "3000"})
    human1 = _read(tmp_path / "parts_s" / ("h1" + EXT[codec]), codec)
    empty = [r for r in human1.split(b"\n@")[1:] if re.match(rb"[^\n]* kraken:taxid\|\d+\n\n\+\n\n", r)]
    assert empty, "no classified record with an empty sequence reached human_out1"


def test_multiline_fasta_and_ultra_long_reads(tmp_path, toy):
    from tests import synth
    _, _, _, genomes, _ = toy
    rng = np.random.default_rng(7)
    allg = b"".join(genomes[k] for k in sorted(genomes))
    reads = []
    for ln in (300_000, 70_000, 90_000, 150, 35, 200_000):
        parts = []
        while sum(map(len, parts)) < ln:
            if rng.random() < 0.6:
                st = int(rng.integers(0, len(allg) - 2000))
                parts.append(allg[st:st + int(rng.integers(200, 2000))])
            else:
                parts.append(synth.random_seq(rng, int(rng.integers(500, 3000))))
        reads.append(synth.mutate(rng, b"".join(parts)[:ln], 0.02, 0.0005, 0.0))
    fa = b"".join(b">long%d desc\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads))
    fq = b"".join(b"@long%d\n%s\n+\n%s\n" % (i, r, b"5" * len(r)) for i, r in enumerate(reads))
    for name, data in (("r.fa", fa), ("r.fq", fq)):
        p = tmp_path / name
        p.write_bytes(data)
        st, _ = compare(tmp_path, name.replace(".", "_"), str(p), codec=2)
        assert st.classified >= 1
        compare(tmp_path, name.replace(".", "_") + "_plain", str(p), codec=0)


def test_one_side_empty(tmp_path):
    """no human read at all, and every read human: the empty side matches the reference run's file (an empty gzip member)"""
    exp = json.load(open(os.path.join(GOLD, "expected_se.json")))
    calls = [r["by_conf"]["0.0"][0] for r in exp["records"]]
    rs = read_fastq(os.path.join(GOLD, "reads_se.fq"))
    for name, want in (("none_human", False), ("all_human", True)):
        body = b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, _i, s, q), c in zip(rs, calls) if bool(c) == want)
        p = tmp_path / (name + ".fq")
        p.write_bytes(body)
        for codec in (0, 2, 4):
            st, trace = compare(tmp_path, "%s_%d" % (name, codec), str(p), codec=codec)
            assert st.classified == (st.total_sequences if want else 0)
            assert (trace[1] > 0) == want


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.argv = ["x"]
import pathlib
from tests import test_gpu_human_out as t
tmp = pathlib.Path(%(tmp)r)
for codec in (0, 2):
    _, trace = t.compare(tmp, "two_%%d" %% codec, %(in1)r, %(in2)r, codec=codec, device_ids=(0, 1))
    print("TRACE", codec, trace)
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
def test_cli_one_split_run_equals_two_runs(tmp_path):
    in1, in2 = _golden(True)
    def cli(args):
        e = dict(os.environ)
        e.pop("NOHUMAN_DB", None)
        r = subprocess.run([BIN, "--db", DB, "-t", "4"] + args, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stderr
    d = tmp_path
    cli(["-o", str(d / "n_1.fq.gz"), "-O", str(d / "n_2.fq.gz"), in1, in2])
    cli(["-H", "-o", str(d / "h_1.fq.gz"), "-O", str(d / "h_2.fq.gz"), in1, in2])
    err = cli(["-o", str(d / "s_1.fq.gz"), "-O", str(d / "s_2.fq.gz"), "--human-out1", str(d / "sh_1.fq.gz"),
               "--human-out2", str(d / "sh_2.fq.gz"), in1, in2])
    for m in ("1", "2"):
        assert _read(d / ("s_%s.fq.gz" % m), 2) == _read(d / ("n_%s.fq.gz" % m), 2)
        assert _read(d / ("sh_%s.fq.gz" % m), 2) == _read(d / ("h_%s.fq.gz" % m), 2)
        assert 'Human reads written to: "%s"' % (d / ("sh_%s.fq.gz" % m)) in err
    assert not any(p.name.endswith(".partial") for p in d.iterdir())
