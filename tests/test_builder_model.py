"""The model of the output builders (tests/builder_model.py) against the goldens, and the conditions that keep
tests/test_gpu_builders.py from testing nothing: computed from the model and the CPU oracle alone, for the same corpora
(same seeds, same specs) the GPU test runs.  A count of zero fails here: the generator is adjusted, never the condition."""
import json
import os

import numpy as np
import pytest

from tests import builder_model as bm
from tests.fastq_util import read_fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")


@pytest.fixture(scope="module")
def db():
    from oracle import oracle as orc
    return orc.OracleDB(directory=DB)


@pytest.fixture(scope="module")
def plans(toy, db):
    """corpus name -> (records, calls, block_plan)"""
    out = {}
    for name, spec in bm.CORPORA.items():
        _texts, records = bm.corpus(spec, toy[3])
        calls = bm.oracle_calls(db, records)
        out[name] = (records, calls, bm.block_plan(records, calls, spec["batch_frags"]))
    return out


def _golden_records(paired):
    names = ("reads_pe_1.fq", "reads_pe_2.fq") if paired else ("reads_se.fq",)
    paths = [os.path.join(GOLD, n) for n in names]
    return paths, [bm.parse_file(open(p, "rb").read(), True) for p in paths]


@pytest.mark.parametrize("paired", [False, True])
def test_goldens_calls_and_masked_text(db, paired):
    """the model's records give the oracle the reads of expected_*.json, and its masked text is oracle_masked()'s"""
    from tests.test_gpu_mask import oracle_masked
    paths, records = _golden_records(paired)
    exp = json.load(open(os.path.join(GOLD, "expected_pe.json" if paired else "expected_se.json")))
    assert [[r.slen for r in fr] for fr in zip(*records)] == [e["len"] for e in exp["records"]]
    calls = bm.oracle_calls(db, records)
    assert [int(c) for c in calls] == [e["by_conf"]["0.0"][0] for e in exp["records"]]
    ext = db.external_ids
    assert [int(x) for x in ext] == exp["meta"]["external_ids"]
    want, ncls = oracle_masked(paths[0], paths[1] if paired else None, 0.0)
    assert ncls == int((calls != 0).sum()) > 0
    assert bm.expected_outputs(records, calls, ext, "masked") == want
    # the other three modes against the same file read by the fixtures' own reader
    for recs, path, got_n, got_h in zip(records, paths, bm.expected_outputs(records, calls, ext, "normal"),
                                        bm.expected_outputs(records, calls, ext, "keep")):
        rs = read_fastq(path)
        assert got_n == b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, _i, s, q), c in zip(rs, calls) if c == 0)
        assert got_h == b"".join(h + b" kraken:taxid|%d\n" % ext[c] + s + b"\n+\n" + q + b"\n"
                                 for (h, _i, s, q), c in zip(rs, calls) if c != 0)
    assert bm.expected_outputs(records, calls, ext, "human") == bm.expected_outputs(records, calls, ext, "keep")


def test_corpora_are_deterministic_and_parse_as_written(toy):
    for name, spec in bm.CORPORA.items():
        texts, records = bm.corpus(spec, toy[3])
        again, _ = bm.make_corpus(np.random.default_rng(spec["seed"]), toy[3], spec)
        assert again == texts, name
        for m, (text, recs) in enumerate(zip(texts, records)):
            assert text == b"".join(r.raw for r in recs)
            assert all(2 <= r.hlen <= 60 and (r.slen <= 5 or 30 <= r.slen <= 40 or 100 <= r.slen <= 300) for r in recs), name
            assert {r.slen for r in recs} >= set(range(6)) | {30, 40}, name
            if recs[0].fastq:  # the fixtures' own FASTQ reader sees the same fields
                assert [(r.header, r.seq, r.qual) for r in recs] == [(h, s, q) for h, _i, s, q in read_fastq_bytes(text)], (name, m)
            else:
                assert all(b"\n" not in r.seq and len(r.text) == len(r.raw) for r in recs)
                assert any(r.raw.count(b"\n") > 2 for r in recs), "no multi-line FASTA record"


def read_fastq_bytes(text):
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".fq") as f:
        f.write(text)
        f.flush()
        return read_fastq(f.name)


def _blocks(plans):
    return [(name, p) for name, (_r, _c, plan) in plans.items() for p in plan]


def test_every_shift_has_a_whole_fast_block_for_each_mate(plans):
    for mate in (0, 1):
        for sh in range(4):
            n = sum(1 for _n, p in _blocks(plans) if p["fast"] and p["mate"] == mate and p["shift"] == sh and p["n"] == bm.BLOCK)
            print("mate", mate, "shift", sh, "whole FAST blocks:", n)
            assert n >= 1, (mate, sh)
    # the first-block normalised record is what moves them: without a non-FAST block in front, a batch's shift is 0
    for name, (_r, _c, plan) in plans.items():
        for p in plan:
            if p["shift"]:
                assert any(not q["fast"] for q in plan if (q["batch"], q["mate"]) == (p["batch"], p["mate"]) and q["block"] < p["block"])


def test_fast_and_other_blocks_side_by_side(plans):
    after = before = 0
    for name, (_r, _c, plan) in plans.items():
        for a, b in zip(plan, plan[1:]):
            if (a["batch"], a["mate"]) == (b["batch"], b["mate"]):
                after += (not a["fast"]) and b["fast"]
                before += a["fast"] and (not b["fast"])
    print("FAST directly after a non-FAST block:", after, "; the reverse:", before)
    assert after >= 1 and before >= 1


def test_batch_sizes_at_the_block_edges(plans):
    sizes = {p["batch_n"] for _n, p in _blocks(plans)}
    assert sizes >= {1023, 1024, 1025, 2049}, sizes
    for name, (_r, calls, plan) in plans.items():  # the plan's batches are the reader's: batch_frags each, the rest last
        bf = bm.CORPORA[name]["batch_frags"]
        per = {p["batch"]: p["batch_n"] for p in plan}
        assert list(per.values()) == [min(bf, len(calls) - i) for i in range(0, len(calls), bf)]


def test_short_classified_sequences_in_both_kinds_of_block(plans):
    for fast in (True, False):
        seen = {}
        for _n, p in _blocks(plans):
            if p["fast"] == fast:
                for o, slen in p["cls"]:
                    if slen <= 5:
                        seen[(slen, o & 3)] = seen.get((slen, o & 3), 0) + 1
        print("FAST" if fast else "non-FAST", sorted(seen.items()))
        for slen in range(6):
            for res in range(4):
                assert seen.get((slen, res), 0) >= 1, (fast, slen, res)


def test_long_classified_sequences_start_and_end_at_every_residue(plans):
    for fast in (True, False):
        seen = {((o & 3), ((o + slen) & 3)) for _n, p in _blocks(plans) if p["fast"] == fast for o, slen in p["cls"] if slen >= 64}
        assert len(seen) == 16, (fast, sorted(seen))


def test_blocks_with_all_some_and_no_record_classified(plans):
    whole = [p for _n, p in _blocks(plans) if p["n"] == bm.BLOCK]
    assert any(0 < p["ncls"] < p["n"] for p in whole)
    assert any(p["ncls"] == 0 for p in whole)
    assert any(p["ncls"] == p["n"] for p in whole)


def test_output_offsets_of_the_plan_are_those_of_the_masked_text(plans, db):
    """block_plan's offsets against expected_outputs: the N runs of the masked text lie where the plan says"""
    for name, (records, calls, plan) in plans.items():
        masked = bm.expected_outputs(records, calls, db.external_ids, "masked")
        bf = bm.CORPORA[name]["batch_frags"]
        start = [[0], [0]]  # per mate: where each batch's output begins in the file
        for m, recs in enumerate(records):
            for i in range(0, len(recs), bf):
                start[m].append(start[m][-1] + sum(r.out_len for r in recs[i:i + bf]))
        for p in plan:
            for o, slen in p["cls"]:
                at = start[p["mate"]][p["batch"]] + o
                assert masked[p["mate"]][at - 1:at + slen + 1] == b"\n" + b"N" * slen + b"\n", (name, p["batch"], p["block"], o)


def test_the_carry_corpus_needs_a_second_round_of_the_scan(toy, db):
    _t, head = bm.corpus(bm.CARRY_HEAD, toy[3])
    _t, unit = bm.corpus(bm.CARRY_UNIT, toy[3])
    records = [h + u * bm.CARRY_REPS for h, u in zip(head, unit)]
    calls = np.concatenate([bm.oracle_calls(db, head)] + [bm.oracle_calls(db, unit)] * bm.CARRY_REPS)
    assert len(calls) > 262144 and 0 < int((calls != 0).sum()) < len(calls)
    plan = bm.block_plan(records, calls, bm.CARRY_BATCH_FRAGS)
    first = [p for p in plan if p["batch"] == 0 and p["mate"] == 0]
    assert len(first) > 256 and first[0]["batch_n"] == bm.CARRY_BATCH_FRAGS
    for mate in (0, 1):
        blocks = [p for p in plan if p["batch"] == 0 and p["mate"] == mate]
        assert not blocks[0]["fast"] and all(p["fast"] and p["shift"] == 1 for p in blocks[1:])
        assert any(p["ncls"] for p in blocks[256:])
    assert all(30 <= r.slen <= 40 and r.hlen <= 10 for recs in records for r in recs[:1001])


def test_digit_ids_cover_one_four_seven_and_ten_digits():
    assert {len(str(e)) for e in bm.DIGIT_IDS[1:]} == {1, 4, 7, 10} and max(bm.DIGIT_IDS) > 1 << 32
