"""BamReader on the GPU through the reader dump hook (nh_debug_reader_dump, reader 2) against the models: the records are those
tests/record_model.py parses out of the FASTQ text tests/bam_model.py transcodes the file to, cut into batches by BlockReader's
rule (record_model._cut) -- for batches of 1, 3 and 4096 records, a text budget that cuts after every record and none at all, BGZF
members of 64, 1000 and 65280 bytes, and the chain's window filled a few bytes at a time."""
import pytest

from tests import bam_model as bm
from tests import record_model as rm

pytestmark = pytest.mark.gpu
BAM = 2


@pytest.fixture(scope="module")
def corpus():
    stream = bm.corpus_stream()
    text = bm.to_fastq(stream)[0]
    return stream, rm.parse(text)


@pytest.mark.parametrize("member", [64, 1000, 65280])
@pytest.mark.parametrize("max_text", [1, 0])
@pytest.mark.parametrize("batch_recs", [1, 3, 4096])
def test_batches_and_records(tmp_path, corpus, monkeypatch, batch_recs, max_text, member):
    stream, parsed = corpus
    p = tmp_path / "c.bam"
    p.write_bytes(bm.bgzf(stream, member, eof=member != 1000))
    monkeypatch.setenv("NOHUMAN_BAM_CHUNK", {64: "5", 1000: "333", 65280: "4194304"}[member])
    got = rm.dump(p, BAM, batch_recs, max_text)
    batches = rm.host_batches(parsed, batch_recs, max_text)
    assert len(batches) == (len(parsed.recs) if batch_recs == 1 or max_text else (len(parsed.recs) + batch_recs - 1) // batch_recs)
    assert rm.verdict(got, parsed, batches, batch_recs, max_text) is None
    assert got.recs[:, 4].all()  # every record canonical: raw_end set


def test_a_text_budget_in_between(tmp_path, corpus):
    """a budget some records reach alone and others only together"""
    stream, parsed = corpus
    p = tmp_path / "c.bam"
    p.write_bytes(bm.bgzf(stream))
    for batch_recs, max_text in ((7, 300), (5, 600)):
        batches = rm.host_batches(parsed, batch_recs, max_text)
        assert len({n for n, _ in batches}) > 2
        assert rm.verdict(rm.dump(p, BAM, batch_recs, max_text), parsed, batches, batch_recs, max_text) is None


def test_only_skipped_records(tmp_path):
    stream = bm.forge_header(refs=[(b"chr1", 10)]) + b"".join(
        bm.forge_record(b"s%d" % i, b"ACGT" * (i % 3), bytes(4 * (i % 3)), flag=bm.SECONDARY if i % 3 else 0) for i in range(40))
    assert bm.to_fastq(stream)[1].reads == 0
    p = tmp_path / "skipped.bam"
    p.write_bytes(bm.bgzf(stream, 100))
    got = rm.dump(p, BAM, 3, 0)
    assert (len(got.recs), got.batches, got.end, got.message) == (0, [], rm.EOF, "")


def test_a_malformed_record_is_an_error_not_a_short_read(tmp_path, corpus):
    stream = corpus[0]
    p = tmp_path / "cut.bam"
    p.write_bytes(bm.bgzf(stream[:-5], 1000))
    got = rm.dump(p, BAM, 4096, 0)
    assert got.end == rm.ERROR and "ends inside record" in got.message and len(got.recs) == 0
