"""The output builders on the GPU (nohuman_amd/csrc/nh_mask.hip, nh_split.hip) against the Python model of
tests/builder_model.py: every output file of a normal, a -H, a split and a masked run, byte for byte, with the calls of the
CPU oracle -- never of a GPU run.  The corpora are the ones tests/test_builder_model.py examines: FAST copies at every
shift, FAST blocks beside others, batches of 1023 / 1024 / 1025 / 2049 records, short classified sequences at every
residue, more than 256 blocks in one batch, suffixes of up to ten digits.  The masked run's trace line must report as many
blocks copied whole as the model's plan has FAST blocks."""
import gzip
import os
import re

import numpy as np
import pytest

from tests import builder_model as bm
from tests.test_gpu_human_out import EXT, _read, _stats
from tests.test_gpu_mask import TRACE, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
WHOLE = re.compile(r"mask: [^\n]*; (\d+) of (\d+) blocks copied whole")


@pytest.fixture(scope="module")
def db():
    from oracle import oracle as orc
    return orc.OracleDB(directory=DB)


def _first_diff(a, b):
    n = min(len(a), len(b))
    x = np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8)
    i = int(np.argmax(x)) if x.any() else n
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), i, a[max(0, i - 20):i + 20], b[max(0, i - 20):i + 20])


def check_runs(tmp, name, texts, records, calls, ext, batch_frags, codec=0, env=None, gz=False, engine_obj=None,
               tags=("n", "h", "s", "m"), want_k=True):
    """the runs of `tags` (n: normal, h: -H, s: split, m: masked) on the corpus, every output file against the model;
    the split and the masked run's -k, -r and stats against the normal run's; the masked run's count of FAST blocks
    against block_plan's.  Returns the masked run's stderr."""
    from nohuman_amd import engine
    env = dict(env or {}, NOHUMAN_BATCH_FRAGS=str(batch_frags), NOHUMAN_TRACE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ins = []
        for m, (text, recs) in enumerate(zip(texts, records)):
            p = tmp / ("%s_in%d.%s%s" % (name, m + 1, "fq" if recs[0].fastq else "fa", ".gz" if gz else ""))
            if not p.exists():
                p.write_bytes(gzip.compress(text, 6) if gz else text)
            ins.append(str(p))
        in1, in2 = ins[0], ins[1] if len(ins) == 2 else None
        mates = ("1", "2") if in2 else ("1",)
        paths, stats, err = {}, {}, ""
        for tag in tags:
            d = tmp / ("%s_%s" % (name, tag))
            d.mkdir()
            p = paths[tag] = {x: str(d / (x + EXT[codec])) for x in ("o1", "o2", "h1", "h2")}
            p.update(k=str(d / "k.txt"), r=str(d / "r.txt"))
            kw = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"] if want_k else None, report=p["r"],
                      threads=4, out_codec=codec, keep_human=tag == "h", mask=tag == "m")
            if tag == "s":
                kw.update(human_out1=p["h1"], human_out2=p["h2"] if in2 else None)
            if engine_obj is not None:
                fn = lambda: engine_obj.run(in1, p["o1"], **kw)  # noqa: E731
            else:
                fn = lambda: engine.run(DB, in1, p["o1"], device_ids=[0], **kw)  # noqa: E731
            errf = tmp / ("%s_%s.stderr" % (name, tag))
            stats[tag] = _run(fn, errf)
            if tag == "m":
                err = errf.read_bytes().decode(errors="replace")
        want = {mode: bm.expected_outputs(records, calls, ext, mode) for mode in ("normal", "keep", "human", "masked")}
        files = {"n": [("o", "normal")], "h": [("o", "keep")], "s": [("o", "normal"), ("h", "human")], "m": [("o", "masked")]}
        for tag in tags:
            for side, mode in files[tag]:
                for i, mt in enumerate(mates):
                    got = _read(paths[tag][side + mt], codec)
                    assert got == want[mode][i], (name, tag, side + mt, mode, _first_diff(got, want[mode][i]))
            assert stats[tag].total_sequences == len(calls) and stats[tag].classified == int((calls != 0).sum()), (name, tag)
        for tag in tags:
            if tag in ("s", "m") and "n" in tags:
                if want_k:
                    assert open(paths[tag]["k"], "rb").read() == open(paths["n"]["k"], "rb").read(), (name, tag)
                assert open(paths[tag]["r"], "rb").read() == open(paths["n"]["r"], "rb").read(), (name, tag)
                assert _stats(stats[tag]) == _stats(stats["n"]), (name, tag)
        if "m" in tags:
            plan = bm.block_plan(records, calls, batch_frags)
            t, w = TRACE.findall(err), WHOLE.findall(err)
            assert len(t) == 1 and len(w) == 1, err[-3000:]
            assert int(t[0][0]) == int((calls != 0).sum()) * len(mates) and int(t[0][1]) == len(calls) * len(mates), (name, t)
            assert int(t[0][2]) == sum(len(x) for x in want["masked"]), (name, t)
            fast, blocks = sum(1 for p in plan if p["fast"]), len(plan)
            print(name, "blocks copied whole:", w[0], "plan:", (fast, blocks))
            assert (int(w[0][0]), int(w[0][1])) == (fast, blocks), (name, w, fast, blocks)
        return err
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _corpus(name, toy, db):
    spec = bm.CORPORA[name]
    texts, records = bm.corpus(spec, toy[3])
    return spec, texts, records, bm.oracle_calls(db, records)


@pytest.mark.parametrize("codec", [0, 2])
@pytest.mark.parametrize("name", ["se", "pe"])
def test_fastq_corpora_every_run_equals_the_model(tmp_path, toy, db, name, codec):
    """single-end and paired FASTQ; codec 2 keeps the built text in HBM for the gzip encoder on the GPU"""
    spec, texts, records, calls = _corpus(name, toy, db)
    check_runs(tmp_path, name, texts, records, calls, db.external_ids, spec["batch_frags"], codec=codec)
    if codec == 2:  # without -k the masked text never leaves HBM
        check_runs(tmp_path, name + "_nok", texts, records, calls, db.external_ids, spec["batch_frags"], codec=codec,
                   tags=("m",), want_k=False)


@pytest.mark.parametrize("codec", [0, 2])
def test_fasta_mate_1(tmp_path, toy, db, codec):
    """mate 1 one-line and multi-line FASTA (the reader joins the lines in place), mate 2 FASTQ"""
    spec, texts, records, calls = _corpus("fa", toy, db)
    check_runs(tmp_path, "fa", texts, records, calls, db.external_ids, spec["batch_frags"], codec=codec)


@pytest.mark.parametrize("reader", ["host", "device"])
def test_gzipped_corpus_under_either_reader(tmp_path, toy, db, reader):
    """plain four-line FASTQ (the reader on the GPU takes no other shape); paired, so both readers cut at batch_frags"""
    spec, texts, records, calls = _corpus("gz", toy, db)
    for codec in (0, 2):
        err = check_runs(tmp_path, "gz%d" % codec, texts, records, calls, db.external_ids, spec["batch_frags"], codec=codec,
                         env={"NOHUMAN_GZ_READER": reader}, gz=True, want_k=codec == 0)
        assert ("gzip reader: GPU / GPU" in err) == (reader == "device"), err[-2000:]


def test_more_than_256_blocks_in_one_batch(tmp_path, toy, db):
    """the scan kernels take 256 blocks a round and carry the sum over: 264 blocks of a 270000-fragment batch, the first
    of them not FAST, so every later offset is unaligned as well"""
    _t, head = bm.corpus(bm.CARRY_HEAD, toy[3])
    _t, unit = bm.corpus(bm.CARRY_UNIT, toy[3])
    records = [h + u * bm.CARRY_REPS for h, u in zip(head, unit)]
    texts = [b"".join(r.raw for r in h) + b"".join(r.raw for r in u) * bm.CARRY_REPS for h, u in zip(head, unit)]
    calls = np.concatenate([bm.oracle_calls(db, head)] + [bm.oracle_calls(db, unit)] * bm.CARRY_REPS)
    assert len(calls) > 262144
    check_runs(tmp_path, "carry", texts, records, calls, db.external_ids, bm.CARRY_BATCH_FRAGS, tags=("s", "m"), want_k=False)


def test_suffix_digits(tmp_path, toy):
    """external ids of 1, 4, 7 and 10 digits (one above 2^32) in the suffix of the human side and of a -H run"""
    from nohuman_amd import Engine
    from oracle import oracle as orc
    ob, tb, hb, genomes, _ = toy
    tb2 = bm.patch_external_ids(tb, bm.DIGIT_IDS)
    odb = orc.OracleDB(ob, tb2, hb)
    assert [int(x) for x in odb.external_ids] == bm.DIGIT_IDS
    texts, records = bm.corpus(bm.DIGITS, genomes)
    calls = bm.oracle_calls(odb, records)
    assert {len(str(bm.DIGIT_IDS[int(c)])) for c in calls if c} == {1, 4, 7, 10}
    with Engine.from_images(ob, tb2, hb) as eng:
        for codec in (0, 2):
            check_runs(tmp_path, "dig%d" % codec, texts, records, calls, odb.external_ids, bm.DIGITS["batch_frags"],
                       codec=codec, engine_obj=eng, tags=("n", "h", "s"))
