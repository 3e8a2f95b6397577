"""Runs with --host-bases-only on the GPU (nh_run_hostbases, `--host-bases-only`, `--host-gap INT`; k_cover_mark, k_cover_close and
the mask builder's bitmap form behind the classifier): the mates' outputs and the three counts against tests/hitmask_model.py
applied to the parsed input -- the sequences as the classifier reads them, the calls from the CPU oracle --, and EVERY OTHER output
of the run, the host intervals' file included, byte for byte, against the same masked run without the flag."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import builder_model as bmod
from tests import hitmask_model as hm
from tests import intervals_model as im
from tests import qmask_model as qm
from tests import rdust_model as rd
from tests import synth
from tests.test_gpu_intervals_run import host_table, run
from tests.test_gpu_minq_run import FILES, _inputs, stats_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
K = 35
GAP = K - 1
Q = qm.Q_E2E
WHOLE = re.compile(r"mask: [^\n]*; (\d+) of (\d+) blocks copied whole")
_CACHE = {}


def toy_lit(toy):
    if "toy" not in _CACHE:
        _CACHE["toy"] = lit.DB.from_images(toy[0], toy[1], toy[2])
    return _CACHE["toy"]


# ---- the corpus: chimeric reads ------------------------------------------------------------------------------------------------
def chimeras(toy, n=120, seed=5):
    """[(header without its first byte, sequence, qualities)]: random 10 .. 49 + host 45 .. 79 + a random insert of 24 + i % 24 + host
    45 .. 79 + random 0 .. 39.  The qualities are good but for a stretch of low ones inside the second host part of every third read.
    The headers' lengths vary, so that the sequences start at every residue mod 4 in the text."""
    rng = np.random.default_rng(seed)
    g = toy[3][111]

    def host(ln):
        at = int(rng.integers(0, len(g) - ln + 1))
        return g[at:at + ln]

    out = []
    for i in range(n):
        a, h1 = synth.random_seq(rng, int(rng.integers(10, 50))), host(int(rng.integers(45, 80)))
        ins, h2 = synth.random_seq(rng, 24 + i % 24), host(int(rng.integers(45, 80)))
        z = synth.random_seq(rng, int(rng.integers(0, 40)))
        s = a + h1 + ins + h2 + z
        ql = bytearray(qm._qual(rng, len(s), Q, 40))
        if i % 3 == 0:
            at = len(a) + len(h1) + len(ins) + 20
            ql[at:at + 6] = qm._qual(rng, 6, 2, Q - 1)
        out.append((b"c%d%s" % (i, b"x" * (i % 5)), s, bytes(ql)))
    return out


def fastq(h, s, ql, shape="plain"):
    if shape == "plain":
        return b"@" + h + b"\n" + s + b"\n+\n" + ql + b"\n"
    if shape == "crlf":
        return b"@" + h + b"\r\n" + s + b"\r\n+\r\n" + ql + b"\r\n"
    assert shape == "plusid"
    return b"@" + h + b"\n" + s + b"\n+" + h + b"\n" + ql + b"\n"


def build(mates, fastq_file=True, shape=lambda i: "plain"):
    """mates: per mate the list of (header, sequence, qualities) -> (texts, records)"""
    texts, records = [], []
    for items in mates:
        raws = [fastq(h, s, ql, shape(i)) if fastq_file else b">" + h + b"\n" + s + b"\n" for i, (h, s, ql) in enumerate(items)]
        texts.append(b"".join(raws))
        records.append([bmod.parse_record(r, fastq_file) for r in raws])
    return texts, records


def mate2_of(items, seed=6):
    rng = np.random.default_rng(seed)
    out = []
    for h, _s, _q in items:
        s2 = synth.random_seq(rng, int(rng.integers(50, 71)))
        out.append((h + b"/2", s2, qm._qual(rng, len(s2), Q, 40)))
    return out


def corpus(toy, name):
    """"se", "pe" (mate 2: random reads), "ep" (the files swapped: the host reads are mate 2) -> (texts, records), computed once"""
    if name == "ep":
        texts, records = corpus(toy, "pe")
        return texts[::-1], records[::-1]
    if name not in _CACHE:
        items = chimeras(toy)
        mates = [items] if name == "se" else [[(h + b"/1", s, q) for h, s, q in items], mate2_of(items)]
        _CACHE[name] = build(mates)
    return _CACHE[name]


# ---- the model of a run ---------------------------------------------------------------------------------------------------------
def model(toy, odb, records, gap, q=0, host_of=None, key=None):
    """-> (per mate the output, the three counts, the masks, the host calls); key: cached under it"""
    if key is not None and (key, gap, q) in _CACHE:
        return _CACHE[key, gap, q]
    frags = rd.masked_fragments(records, q, False)
    if len(records) == 1:
        frags = [(s,) for s in frags]
    calls = [int(c) for c in rd.classify(odb, records, q, False)[0]["call"]]
    host_calls = [c if c and (host_of is None or host_of[c]) else 0 for c in calls]
    out = hm.outputs(toy_lit(toy), records, frags, host_calls, gap, host_of) + (host_calls,)
    if key is not None:
        _CACHE[key, gap, q] = out
    return out


def inner_runs(masks):
    """the lengths of the uncovered runs with a covered base on each side, over every host sequence"""
    out = []
    for row in masks:
        for m in row:
            if m is None:
                continue
            cov = m[0]
            out += [b - a for a, b in im.runs(~cov) if a > 0 and b < len(cov)]
    return out


def check_corpus(records, want0, want34):
    """what the recipe promises, asserted on the model: every host fragment partly masked and partly kept; for gap 34 runs of exactly
    34 (closed) and of exactly 35 (kept); the mask's transitions at every residue mod 32 of the text, the sequences' starts at every
    residue mod 4"""
    masks, host_calls = want0[2], want0[3]
    assert sum(1 for c in host_calls if c) >= len(host_calls) * 3 // 4
    for row, c in zip(masks, host_calls):
        if c:
            closed = np.concatenate([m[1] for m in row])
            assert closed.any() and not closed.all()
    runs = inner_runs(masks)
    assert GAP in runs and GAP + 1 in runs and min(runs) < GAP - 5 and max(runs) > GAP + 5, sorted(set(runs))
    assert want34[1][2] > 0 and want34[1][1] == want0[1][1] + want34[1][2] and want34[1][0] == want0[1][0]
    starts, trans = set(), set()
    for recs, col in zip(records, zip(*want34[2])):
        at = 0
        for r, m in zip(recs, col):
            starts.add((at + r.s) % 4)
            if m is not None:
                d = np.nonzero(np.diff(m[1].astype(np.int8)))[0] + 1
                trans |= {int(at + r.s + x) % 32 for x in d}
            at += len(r.raw)
    assert starts == set(range(4)) and trans == set(range(32)), (starts, sorted(trans))


# ---- one case: the run with the flag against the model, everything else against the run without it ---------------------------
def case(tmp, eng, ins, want, gap, env=None, bed=True, fast=None, **kw):
    texts, counts = want[0], want[1]
    with_, bed1, err, st = run(tmp, "with", eng, ins, bed, env, mask=True, host_bases_only=True, host_gap=gap, **kw)
    without, bed0, err0, st0 = run(tmp, "without", eng, ins, bed, env, mask=True, **kw)
    for m, text in enumerate(texts):
        got = with_["o%d" % (m + 1)]
        assert got is not None and len(got) == len(text), (m, len(got or b""), len(text))
        if got != text:
            i = next(k for k in range(len(text)) if got[k] != text[k])
            raise AssertionError("mate %d differs from the model at byte %d: %r / %r" % (m + 1, i, got[max(0, i - 60):i + 40], text[max(0, i - 60):i + 40]))
        assert without["o%d" % (m + 1)] != text  # (the masked run blanks whole reads)
    assert (st.host_bases, st.masked_bases, st.closed_bases) == counts
    assert "host-bases-only: %d of %d host bases masked, %d by closing" % (counts[1], counts[0], counts[2]) in err, err[-2000:]
    assert "host-bases-only:" not in err0 and not hasattr(st0, "host_bases")
    for x in FILES:
        if x not in ("o1", "o2"):
            assert with_[x] == without[x], (x, "differs between the run with the flag and the run without")
    assert with_["k"] and stats_of(st) == stats_of(st0)
    assert bed1 == bed0 and (bed1 is not None) == bed  # (the BED is the coverage before the closing)
    if bed:
        assert (st.interval_fragments, st.intervals, st.covered_bases) == (st0.interval_fragments, st0.intervals, st0.covered_bases)
    w = WHOLE.findall(err)
    assert len(w) == 1, err[-2000:]
    if fast is True:
        assert int(w[0][0]) == int(w[0][1]) > 0, w  # plain four-line FASTQ: every block copied whole, the bases filled in after
    elif fast is False:
        assert int(w[0][0]) == 0 < int(w[0][1]), w
    return with_, st


@pytest.mark.parametrize("gap", [0, GAP])
@pytest.mark.parametrize("name", ["se", "pe", "ep"])
def test_fastq_in_batches(tmp_path, toy, toy_oracle, toy_engine, name, gap):
    """plain four-line FASTQ, three batches on the slots in turn: the FAST path"""
    texts, records = corpus(toy, name)
    want = model(toy, toy_oracle, records, gap, key=name)
    if name == "se":
        check_corpus(records, model(toy, toy_oracle, records, 0, key=name), model(toy, toy_oracle, records, GAP, key=name))
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, gap, env={"NOHUMAN_BATCH_FRAGS": "40"}, fast=True)


@pytest.mark.parametrize("gap", [0, GAP])
def test_crlf_and_plus_id_lines_take_the_record_path(tmp_path, toy, toy_oracle, toy_engine, gap):
    items = chimeras(toy)
    texts, records = build([items], shape=lambda i: ("crlf", "plusid", "plain")[i % 3])
    want = model(toy, toy_oracle, records, gap)
    assert want[1] == model(toy, toy_oracle, corpus(toy, "se")[1], gap, key="se")[1]  # (the same reads: the same counts)
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, gap, fast=False)


def test_fasta(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = build([chimeras(toy)], fastq_file=False)
    p = tmp_path / "in.fa"
    p.write_bytes(texts[0])
    case(tmp_path, toy_engine, [str(p), None], model(toy, toy_oracle, records, GAP), GAP)


@pytest.mark.parametrize("shape", ["plain", "crlf"])
def test_sequences_of_length_0_1_34_35_36(tmp_path, toy, toy_oracle, toy_engine, shape):
    """host sequences too short for a k-mer, of one k-mer and of two, among the chimeras, on both paths of the builder"""
    g = toy[3][111]
    items = chimeras(toy, n=30)
    for j, ln in enumerate((0, 1, 34, 35, 36, 35, 36, 0)):
        s = g[500 + 40 * j:500 + 40 * j + ln]
        items.insert(3 * j + 1, (b"short%d" % j, s, b"I" * ln))
    texts, records = build([items], shape=lambda i: shape)
    want = model(toy, toy_oracle, records, GAP)
    lens = {r.slen for r, c in zip(records[0], want[3]) if c}
    assert lens & {35, 36}  # (a host fragment of one or two k-mers)
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, GAP, fast=shape == "plain")


@pytest.mark.parametrize("gap", [0, GAP])
def test_more_than_two_builder_blocks_in_one_batch(tmp_path, toy, toy_oracle, toy_engine, gap):
    """the corpus 20 times under new ids, one batch of 2400 fragments: three builder blocks and their boundaries"""
    _t, records = corpus(toy, "se")
    base = model(toy, toy_oracle, records, gap, key="se")
    raws, outs = [], []
    for rep in range(20):
        for r, row in zip(records[0], base[2]):
            raw = b"@r%d." % rep + r.raw[1:]
            raws.append(raw)
            outs.append(hm.put(bmod.parse_record(raw, True), None if row[0] is None else row[0][1]))
    want = ([b"".join(outs)], tuple(20 * x for x in base[1]))
    p = tmp_path / "in.fq"
    p.write_bytes(b"".join(raws))
    case(tmp_path, toy_engine, [str(p), None], want, gap, env={"NOHUMAN_BATCH_FRAGS": "4000"}, fast=True)


def test_a_long_read_with_many_alternations(tmp_path, toy, toy_oracle, toy_engine):
    """one read of about 6 kb, host and random stretches in turn: more than a cover piece (3968 k-mers), many bitmap words"""
    rng = np.random.default_rng(12)
    g = toy[3][111]
    parts = []
    for j in range(34):
        ln = int(rng.integers(90, 200))
        at = int(rng.integers(0, len(g) - ln + 1))
        parts += [g[at:at + ln], synth.random_seq(rng, 20 + j % 30)]
    s = b"".join(parts)
    assert 5500 < len(s) < 7500 and len(s) - K + 1 > 3968
    items = [(b"long", s, b"I" * len(s))] + chimeras(toy, n=3)
    texts, records = build([items])
    for gap in (0, GAP):
        want = model(toy, toy_oracle, records, gap)
        cov = want[2][0][0][0]
        assert want[3][0] and len(im.runs(cov)) >= 20
        d = tmp_path / ("g%d" % gap)
        d.mkdir()
        case(d, toy_engine, _inputs(d, "in", texts), want, gap)


def test_gzip_output(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = corpus(toy, "pe")
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, key="pe"), GAP, out_codec=2)


def test_human_outputs(tmp_path, toy, toy_oracle, toy_engine):
    """--human-out1/2: the host records as -H writes them, unmasked"""
    texts, records = corpus(toy, "pe")
    with_, _st = case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, key="pe"), GAP,
                      human_out1="h1", human_out2="h2")
    assert with_["h1"] and with_["h2"] and b"kraken:taxid|" in with_["h1"]


def test_host_taxid(tmp_path, toy, toy_oracle, toy_engine):
    """--host-taxid 111: a k-mer whose value is an ancestor of 111 is no host k-mer, a read called above 111 no host fragment"""
    ldb = toy_lit(toy)
    texts, records = corpus(toy, "se")
    want = model(toy, toy_oracle, records, GAP, host_of=host_table(ldb, {111}, set()))
    plain = model(toy, toy_oracle, records, GAP, key="se")
    assert 0 < want[1][1] < plain[1][1]
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, GAP, host_taxids=[111])


def test_minimum_base_quality(tmp_path, toy, toy_oracle, toy_engine):
    """the coverage is that of the quality-masked copy, the bases written are the input's: host bases of low quality stay as they are"""
    texts, records = corpus(toy, "se")
    want = model(toy, toy_oracle, records, 0, q=Q)
    plain = model(toy, toy_oracle, records, 0, key="se")
    kept = 0
    for r, row, prow in zip(records[0], want[2], plain[2]):
        if row[0] is None or prow[0] is None:
            continue
        low = np.frombuffer(r.qual, dtype=np.uint8).astype(np.int64) - 33 < Q
        kept += int((low & prow[0][1] & ~row[0][1]).sum())  # low quality, masked without the threshold, written unchanged with it
    assert kept >= 20 and want[0] != plain[0]
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, 0, min_base_quality=Q)


def test_without_the_host_intervals_file(tmp_path, toy, toy_oracle, toy_engine):
    """the mode alone: the mark pass runs for the mask, no record and no line is built"""
    texts, records = corpus(toy, "pe")
    case(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy, toy_oracle, records, GAP, key="pe"), GAP, bed=False,
         env={"NOHUMAN_BATCH_FRAGS": "50"})


def test_a_database_the_mark_pass_does_not_support_is_refused(tmp_path, toy):
    from nohuman_amd import Engine, EngineError
    from tests import table_forge as tfg
    texts, _records = corpus(toy, "se")
    in1, _ = _inputs(tmp_path, "in", texts)
    with Engine.from_images(tfg.opts_of("k31l31"), tfg.toy_taxo(), tfg.table(tfg.SHAPES[0], 0.5)) as eng:
        with pytest.raises(EngineError) as ei:
            eng.run(in1, str(tmp_path / "o.fq"), host_bases_only=True, host_gap=GAP)
        assert ei.value.code == -1 and "k is 31" in ei.value.message
    assert not (tmp_path / "o.fq").exists()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
d = %(tmp)r
st = engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=[0, 1], threads=4,
                kraken_output=os.path.join(d, "k"), host_intervals=os.path.join(d, "bed"), host_bases_only=True, host_gap=%(gap)d)
print("CHILD OK %%d %%d %%d" %% (st.host_bases, st.masked_bases, st.closed_bases))
"""


def test_two_logical_devices(tmp_path, toy, toy_oracle):
    """NOHUMAN_FAKE_DEVICES=2: batches in turn on two logical devices, the discipline checked at every launch and copy; the
    devices' counts are summed"""
    texts, records = corpus(toy, "pe")
    want = model(toy, toy_oracle, records, GAP, key="pe")
    in1, in2 = _inputs(tmp_path, "d", texts)
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="20")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, in1=in1, in2=in2, gap=GAP)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK %d %d %d" % want[1] in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    assert [(tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()] == want[0]


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_equals_the_library(tmp_path, toy, toy_oracle):
    texts, records = corpus(toy, "pe")
    want = model(toy, toy_oracle, records, GAP, key="pe")
    in1, in2 = _inputs(tmp_path, "cli", texts)
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    o = {x: str(tmp_path / x) for x in ("o1", "o2", "k", "bed")}
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "-v", "-o", o["o1"], "-O", o["o2"], "-k", o["k"], "--host-intervals", o["bed"],
                        "--host-bases-only", "--host-gap", str(GAP), in1, in2], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [open(o["o1"], "rb").read(), open(o["o2"], "rb").read()] == want[0]
    assert "Host bases only: %d of %d bases of the human reads written as N, %d of them by closing" % (want[1][1], want[1][0], want[1][2]) in r.stderr, r.stderr[-2000:]
    assert not any(p.name.endswith(".partial") for p in tmp_path.iterdir())
