"""Runs with --host-cut on the GPU (nh_run_hostcut, `--host-cut`, `--host-gap INT`, `--host-min-piece INT`; k_cover_mark,
k_cover_close and the cut builder behind the classifier): out1 and the seven counts against tests/hostcut_model.py applied to the
parsed input -- the sequences as the classifier reads them, the calls from the CPU oracle --, and EVERY OTHER output of the run, the
host intervals' file included, byte for byte, against the same masked run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import bam_model as bm
from tests import builder_model as bmod
from tests import hostcut_model as hc
from tests import qmask_model as qm
from tests import rdust_model as rd
from tests.test_gpu_hostbases_run import build, chimeras
from tests.test_gpu_intervals_run import host_table, run
from tests.test_gpu_minq_run import FILES, _inputs, stats_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
K = 35
GAP = K - 1
M = 40
Q = qm.Q_E2E
TRACE = "host-cut: %d host bases: %d in %d pieces, %d cut (%d by closing), %d in short runs; %d reads dropped"
_CACHE = {}


def toy_lit(toy):
    if "toy" not in _CACHE:
        _CACHE["toy"] = lit.DB.from_images(toy[0], toy[1], toy[2])
    return _CACHE["toy"]


def corpus(toy):
    """the chimeras as plain four-line FASTQ -> (texts, records), computed once"""
    if "se" not in _CACHE:
        _CACHE["se"] = build([chimeras(toy)])
    return _CACHE["se"]


def model(toy, odb, records, gap, m, q=0, host_of=None, key=None):
    """-> (out1, the seven counts, per fragment its pieces or None, the host calls); key: cached under it"""
    if key is not None and (key, gap, m, q) in _CACHE:
        return _CACHE[key, gap, m, q]
    frags = rd.masked_fragments(records, q, False)
    calls = [int(c) for c in rd.classify(odb, records, q, False)[0]["call"]]
    host_calls = [c if c and (host_of is None or host_of[c]) else 0 for c in calls]
    out = hc.outputs(toy_lit(toy), records[0], frags, host_calls, gap, m, host_of) + (host_calls,)
    if key is not None:
        _CACHE[key, gap, m, q] = out
    return out


def check_corpus(want):
    """gap 34, pieces of at least 40: the inserts of 24..47 bases give closed runs, short runs and pieces; a host read has two
    pieces, another none"""
    _text, counts, cuts, host_calls = want
    c = dict(zip(hc.COUNTS, counts))
    assert c["closed_bases"] > 0 and c["short_bases"] > 0 and c["pieces"] > 0 and c["dropped_reads"] > 0
    assert c["host_bases"] == c["piece_bases"] + c["cut_bases"] + c["short_bases"]
    assert sum(1 for x in host_calls if x) >= len(host_calls) * 3 // 4
    assert any(ps is not None and len(ps) >= 2 for ps in cuts) and any(ps is not None and not ps for ps in cuts)


def case(tmp, eng, ins, want, gap, m, env=None, bed=True, **kw):
    """the run with the flag against the model, everything else against the masked run without it"""
    text, counts = want[0], want[1]
    with_, bed1, err, st = run(tmp, "with", eng, ins, bed, env, host_cut=True, host_gap=gap, host_min_piece=m, **kw)
    without, bed0, err0, st0 = run(tmp, "without", eng, ins, bed, env, mask=True, **kw)
    got = with_["o1"]
    assert got is not None
    if got != text:
        i = next((k for k in range(min(len(text), len(got))) if got[k] != text[k]), min(len(text), len(got)))
        raise AssertionError("out1 (%d bytes, the model %d) differs from the model at byte %d: %r / %r" % (
            len(got), len(text), i, got[max(0, i - 60):i + 40], text[max(0, i - 60):i + 40]))
    assert without["o1"] != text  # (the masked run blanks whole reads)
    assert tuple(getattr(st, k) for k in hc.COUNTS) == counts
    assert TRACE % (counts[0], counts[2], counts[1], counts[3], counts[6], counts[4], counts[5]) in err, err[-2000:]
    assert "host-cut:" not in err0 and not hasattr(st0, "pieces")
    for x in FILES:
        if x != "o1":
            assert with_[x] == without[x], (x, "differs between the run with the flag and the run without")
    assert with_["k"] and stats_of(st) == stats_of(st0)
    assert bed1 == bed0 and (bed1 is not None) == bed  # (the BED is the coverage before the closing)
    if bed:
        assert (st.interval_fragments, st.intervals, st.covered_bases) == (st0.interval_fragments, st0.intervals, st0.covered_bases)
    return with_, st


@pytest.mark.parametrize("gap,m", [(0, 1), (0, M), (GAP, 1), (GAP, M)])
def test_fastq_in_three_batches(tmp_path, toy, toy_oracle, toy_engine, gap, m):
    texts, records = corpus(toy)
    want = model(toy, toy_oracle, records, gap, m, key="se")
    check_corpus(model(toy, toy_oracle, records, GAP, M, key="se"))
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, gap, m, env={"NOHUMAN_BATCH_FRAGS": "40"})


def test_crlf_and_plus_id_lines(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = build([chimeras(toy)], shape=lambda i: ("crlf", "plusid", "plain")[i % 3])
    want = model(toy, toy_oracle, records, GAP, M)
    assert want[1] == model(toy, toy_oracle, corpus(toy)[1], GAP, M, key="se")[1]  # (the same reads: the same counts)
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, GAP, M)


def test_fasta(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = build([chimeras(toy)], fastq_file=False)
    p = tmp_path / "in.fa"
    p.write_bytes(texts[0])
    case(tmp_path, toy_engine, [str(p), None], model(toy, toy_oracle, records, GAP, M), GAP, M)


def test_gzip_output(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = corpus(toy)
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, M, key="se"), GAP, M, out_codec=2)


def test_single_end_bam_input(tmp_path, toy, toy_oracle, toy_engine):
    """the coordinates are those of the FASTQ text the reader transcodes to: every other record is stored reverse-complemented"""
    stream = bm.forge_header()
    for i, (h, s, ql) in enumerate(chimeras(toy, n=60)):
        stream += bm.forge_record(h, s, bytes(x - 33 for x in ql), flag=16 if i % 2 else 0)
    text = bm.to_fastq(stream)[0]
    records = [bmod.parse_file(text, True)]
    p = tmp_path / "in.bam"
    p.write_bytes(bm.bgzf(stream))
    want = model(toy, toy_oracle, records, GAP, M)
    assert want[1][1] > 0 and want[1][3] > 0
    case(tmp_path, toy_engine, [str(p), None], want, GAP, M)


def test_host_taxid(tmp_path, toy, toy_oracle, toy_engine):
    """--host-taxid 111: a k-mer whose value is an ancestor of 111 is no host k-mer, a read called above 111 no host fragment"""
    ldb = toy_lit(toy)
    texts, records = corpus(toy)
    want = model(toy, toy_oracle, records, GAP, M, host_of=host_table(ldb, {111}, set()))
    plain = model(toy, toy_oracle, records, GAP, M, key="se")
    assert 0 < want[1][3] < plain[1][3]
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, GAP, M, host_taxids=[111])


def test_minimum_base_quality(tmp_path, toy, toy_oracle, toy_engine):
    """the coverage is that of the quality-masked copy, the pieces carry the input's bases"""
    texts, records = corpus(toy)
    want = model(toy, toy_oracle, records, 0, 1, q=Q)
    plain = model(toy, toy_oracle, records, 0, 1, key="se")
    assert want[0] != plain[0] and want[1][2] > plain[1][2]  # (low qualities inside a host part: more is left uncovered)
    masked = rd.masked_fragments(records, Q, False)
    assert any(bytes(s) != r.seq for s, r in zip(masked, records[0]))
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, 0, 1, min_base_quality=Q)


def test_human_out1(tmp_path, toy, toy_oracle, toy_engine):
    """--human-out1: the host records whole, as -H writes them"""
    texts, records = corpus(toy)
    with_, _st = case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, M, key="se"), GAP, M, human_out1="h1")
    assert with_["h1"] and b"kraken:taxid|" in with_["h1"] and b":0-" not in with_["h1"].split(b"\n")[0]


def test_without_the_host_intervals_file(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = corpus(toy)
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, M, key="se"), GAP, M, bed=False,
         env={"NOHUMAN_BATCH_FRAGS": "50"})


def test_paired_input_is_refused(tmp_path, toy, toy_engine):
    from nohuman_amd import EngineError
    texts, _records = corpus(toy)
    in1, _ = _inputs(tmp_path, "in", texts)
    with pytest.raises(EngineError) as ei:
        toy_engine.run(in1, str(tmp_path / "o1.fq"), in2=in1, out2=str(tmp_path / "o2.fq"), host_cut=True)
    assert ei.value.code == -1 and "single-end" in ei.value.message
    assert not (tmp_path / "o1.fq").exists() and not (tmp_path / "o2.fq").exists()


def test_a_database_the_mark_pass_does_not_support_is_refused(tmp_path, toy):
    from nohuman_amd import Engine, EngineError
    from tests import table_forge as tfg
    texts, _records = corpus(toy)
    in1, _ = _inputs(tmp_path, "in", texts)
    with Engine.from_images(tfg.opts_of("k31l31"), tfg.toy_taxo(), tfg.table(tfg.SHAPES[0], 0.5)) as eng:
        with pytest.raises(EngineError) as ei:
            eng.run(in1, str(tmp_path / "o.fq"), host_cut=True, host_gap=GAP)
        assert ei.value.code == -1 and "k is 31" in ei.value.message
    assert not (tmp_path / "o.fq").exists()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
d = %(tmp)r
st = engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), device_ids=[0, 1], threads=4, kraken_output=os.path.join(d, "k"),
                host_intervals=os.path.join(d, "bed"), host_cut=True, host_gap=%(gap)d, host_min_piece=%(m)d)
print("CHILD OK " + " ".join(str(getattr(st, k)) for k in %(counts)r))
"""


def test_two_logical_devices(tmp_path, toy, toy_oracle):
    """NOHUMAN_FAKE_DEVICES=2: batches in turn on two logical devices, the discipline checked at every launch and copy; the
    devices' counts are summed"""
    texts, records = corpus(toy)
    want = model(toy, toy_oracle, records, GAP, M, key="se")
    in1, _ = _inputs(tmp_path, "d", texts)
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="20")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, in1=in1, gap=GAP, m=M, counts=hc.COUNTS)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK " + " ".join(str(x) for x in want[1]) in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    assert (tmp_path / "o1").read_bytes() == want[0]


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_equals_the_library(tmp_path, toy, toy_oracle):
    texts, records = corpus(toy)
    want = model(toy, toy_oracle, records, GAP, M, key="se")
    in1, _ = _inputs(tmp_path, "cli", texts)
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    o = {x: str(tmp_path / x) for x in ("o1", "k", "bed")}
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "-v", "-o", o["o1"], "-k", o["k"], "--host-intervals", o["bed"], "--host-cut", "--host-gap", str(GAP),
                        "--host-min-piece", str(M), in1], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(o["o1"], "rb").read() == want[0]
    c = dict(zip(hc.COUNTS, want[1]))
    assert "Host cut: %d bases of the human reads: %d written in %d pieces of at least %d bases, %d cut out (%d of them by closing" % (
        c["host_bases"], c["piece_bases"], c["pieces"], M, c["cut_bases"], c["closed_bases"]) in r.stderr, r.stderr[-2000:]
    assert not any(p.name.endswith(".partial") for p in tmp_path.iterdir())
