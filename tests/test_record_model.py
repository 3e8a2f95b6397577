"""The record model of tests/record_model.py against the HOST reader (BlockReader through nh_debug_reader_dump), record by
record: header / id / sequence / quality lengths, the canonical flag and raw length, the batch each record came in, digests of
its bytes, the batches' sizes and how the input ended.  No GPU: this pins the reference tests/test_gpu_record_index.py holds
the reader on the GPU to."""
import collections
import gzip

import numpy as np
import pytest

from tests import record_model as rm


def _shapes_text():
    rng = np.random.default_rng(7)
    return b"".join(rm.make_record(rng, s, slen=int(rng.integers(0, 30))) for s in rm.SHAPES for _ in range(2))


def _body(n=5):
    rng = np.random.default_rng(8)
    return b"".join(rm.make_record(rng, "plain", slen=12) for _ in range(n))


CORPUS = {"shapes": _shapes_text(), "one": _body(1)}
for _name in rm.ENDS:
    CORPUS["end:" + _name] = rm.with_end(_body(), _name)
    if rm.ENDS[_name][1] in (rm.BLANK, rm.LONE_AT) and rm.ENDS[_name][0].endswith(b"\n"):
        CORPUS["end+garbage:" + _name] = rm.with_end(_body(), _name, garbage=True)
CORPUS["first:blank"] = rm.with_end(b"", "blank")
CORPUS["first:at"] = rm.with_end(b"", "at")
CORPUS["first:bad"] = rm.with_end(b"", "bad_full")
CORPUS["first:cut2"] = rm.with_end(b"", "cut2")


def _check(path, text, batch_recs, max_text):
    parsed = rm.parse(text)
    got = rm.dump(path, 0, batch_recs, max_text)
    return rm.verdict(got, parsed, rm.host_batches(parsed, batch_recs, max_text), batch_recs, max_text)


@pytest.mark.parametrize("max_text", [0, 150])
@pytest.mark.parametrize("batch_recs", [1, 3, 256])
@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_host_reader_matches_the_model(tmp_path, monkeypatch, chunk, batch_recs, max_text):
    """plain files and gzip, reads of 1, 7 and 4096 bytes, batches of 1, 3 and 256 records and a text budget that cuts them"""
    monkeypatch.setenv("NOHUMAN_READ_CHUNK", str(chunk))
    bad = []
    for name, text in CORPUS.items():
        plain, gz = tmp_path / "x.fq", tmp_path / "x.fq.gz"
        plain.write_bytes(text)
        gz.write_bytes(gzip.compress(text))
        for p in (plain, gz):
            why = _check(p, text, batch_recs, max_text)
            if why:
                bad.append("%s (%s): %s" % (name, p.name, why))
    assert not bad, "\n".join(bad)


def test_the_corpus_ends_in_every_way_the_model_knows():
    kinds = collections.Counter(rm.parse(t).end for t in CORPUS.values())
    assert set(kinds) == set(rm.END_KINDS), kinds
    for name, (_tail, kind) in rm.ENDS.items():
        assert rm.parse(CORPUS["end:" + name]).end == kind, name
    assert set(rm.shapes_of(rm.parse(CORPUS["shapes"]))) >= set(rm.SHAPES)


def test_the_model_agrees_with_the_whole_file_model():
    """the record table says what py_records (tests/test_reader.py's model) says, where that one has an answer"""
    for name, text in CORPUS.items():
        p = rm.parse(text)
        if p.end in (rm.MALFORMED, rm.UNRECOGNISED):
            with pytest.raises(ValueError):
                rm.py_records(text)
            continue
        recs = rm.py_records(text)
        assert len(recs) == len(p.recs), name
        d, _raw = rm.digests(p)
        assert [rm.fnv(r) for r in recs] == [int(x) for x in d], name


def test_a_repeated_text_repeats_its_records():
    """rm.repeat (the model of a large periodic text without parsing it byte by byte) is what parse says"""
    a, b = rm.repeat(rm.parse(CORPUS["shapes"]), 3), rm.parse(CORPUS["shapes"] * 3)
    assert a.text == b.text and (a.end, a.stop) == (b.end, b.stop)
    assert np.array_equal(a.recs, b.recs) and np.array_equal(a.lines, b.lines)


def test_the_appended_newline_changes_the_last_record_only():
    """The reader on the GPU appends the newline a text's last line lacks.  From the model alone: that makes a last record
    canonical that is not on the host, one byte longer, and changes nothing else."""
    for name, text in CORPUS.items():
        a, b = rm.parse(text), rm.parse(rm.device_text(text))
        assert (a.end, a.message, len(a.recs)) == (b.end, b.message, len(b.recs)), name
        ea, eb = rm.expected(a, rm.host_batches(a, 3, 0)), rm.expected(b, rm.host_batches(b, 3, 0))
        diff = np.argwhere(ea != eb)
        if len(diff):
            assert not text.endswith(b"\n") and set(diff[:, 0]) == {len(a.recs) - 1}, name
            assert {rm.FIELDS[f] for f in diff[:, 1]} == {"canonical", "raw_len", "raw_digest"}, name
            assert eb[-1, 4] == 1 and ea[-1, 4] == 0 and a.recs[-1, rm.R_END] + 1 == b.recs[-1, rm.R_END] == len(text) + 1, name


def test_the_fuzz_seeds_cover_every_shape_and_every_end_twice():
    shapes, ends = collections.Counter(), collections.Counter()
    for seed in rm.FUZZ_SEEDS:
        p = rm.parse(rm.fuzz_case(seed)[0])
        for s in rm.shapes_of(p):
            shapes[s] += 1
        ends[p.end] += 1
    assert all(shapes[s] >= 2 for s in rm.SHAPES + ("blank_header",)), shapes
    assert all(ends[k] >= 2 for k in rm.END_KINDS), ends


@pytest.mark.parametrize("seed", rm.FUZZ_SEEDS)
def test_host_reader_matches_the_model_on_the_fuzz_seeds(tmp_path, monkeypatch, seed):
    text, k = rm.fuzz_case(seed)
    monkeypatch.setenv("NOHUMAN_READ_CHUNK", str(max(k["chunk"], 7)))
    p = tmp_path / "f.fq.gz"
    p.write_bytes(gzip.compress(text, k["level"]))
    assert _check(p, text, k["batch_recs"], k["max_text"]) is None
