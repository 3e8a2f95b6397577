"""The paired BamReader on the GPU through the reader dump hook (nh_debug_reader_dump, readers 3 and 4: its halves of mate 1 and of
mate 2) against the models: each half's records are those tests/record_model.py parses out of the mate's FASTQ text that
tests/bam_pair_model.py transcodes the file to -- the digests of the dump hold the transcoded bytes to the model's --, cut into
batches by the pair rule (bam_pair_model.cut_pairs: up to N pairs, cut after the pair at which either mate's text reaches the
budget) -- for batches of 1, 3 and 4096 pairs, a text budget that cuts after every pair and none at all, BGZF members of 64, 1000
and 65280 bytes and the chain's window filled a few bytes at a time.  Both halves always hold the same number of records, so a
pair never straddles a batch."""
import pytest

from tests import bam_model as bm
from tests import bam_pair_model as pm
from tests import record_model as rm

pytestmark = pytest.mark.gpu
MATE1, MATE2 = 3, 4


@pytest.fixture(scope="module")
def corpus():
    stream = pm.corpus_stream()
    t1, t2, _ = pm.to_fastq_pair(stream)
    return stream, rm.parse(t1), rm.parse(t2)


def both_halves(path, stream, parsed, batch_pairs, max_text):
    """the two dumps held to the model; -> the model's batches"""
    cuts = pm.cut_pairs(stream, batch_pairs, max_text)
    got = [rm.dump(path, reader, batch_pairs, max_text) for reader in (MATE1, MATE2)]
    for m in (0, 1):
        batches = [(n, t[m]) for n, *t in cuts]
        assert got[m].end == rm.EOF and got[m].message == ""
        assert got[m].batches == batches, (m, got[m].batches[:5], batches[:5])
        assert rm.mismatch(got[m].recs, rm.expected(parsed[m], batches)) is None
        assert got[m].recs[:, 4].all()  # every record canonical: raw_end set
    # the same number of records in both halves of every batch: a pair never straddles one
    assert [n for n, _ in got[0].batches] == [n for n, _ in got[1].batches]
    assert (got[0].recs[:, 6] == got[1].recs[:, 6]).all()
    return cuts


@pytest.mark.parametrize("member", [64, 1000, 65280])
@pytest.mark.parametrize("max_text", [1, 0])
@pytest.mark.parametrize("batch_pairs", [1, 3, 4096])
def test_batches_and_records_of_both_halves(tmp_path, corpus, monkeypatch, batch_pairs, max_text, member):
    stream, p1, p2 = corpus
    p = tmp_path / "c.bam"
    p.write_bytes(bm.bgzf(stream, member, eof=member != 1000))
    monkeypatch.setenv("NOHUMAN_BAM_CHUNK", {64: "5", 1000: "333", 65280: "4194304"}[member])
    cuts = both_halves(p, stream, (p1, p2), batch_pairs, max_text)
    n = len(p1.recs)
    assert len(p2.recs) == n and len(cuts) == (n if batch_pairs == 1 or max_text else (n + batch_pairs - 1) // batch_pairs)


def test_a_text_budget_that_either_mate_reaches(tmp_path, corpus):
    """budgets some pairs reach alone -- by mate 1 or by mate 2 -- and others only together"""
    stream, p1, p2 = corpus
    p = tmp_path / "c.bam"
    p.write_bytes(bm.bgzf(stream))
    for batch_pairs, max_text in ((7, 300), (5, 600)):
        cuts = both_halves(p, stream, (p1, p2), batch_pairs, max_text)
        assert len({n for n, _, _ in cuts}) > 2
        full = [c for c in cuts if c[0] < batch_pairs and (c[1] >= max_text or c[2] >= max_text)]
        assert any(c[1] >= max_text > c[2] for c in full) and any(c[2] >= max_text > c[1] for c in full)


def test_an_orphan_is_an_error_in_both_halves_and_nothing_of_its_batch_goes_out(tmp_path, corpus):
    stream = corpus[0] + bm.forge_record(b"orphan", b"ACGT", bytes(4), flag=pm.P1)
    n_records = len(pm.records(stream))
    p = tmp_path / "orphan.bam"
    p.write_bytes(bm.bgzf(stream, 1000))
    for reader in (MATE1, MATE2):
        got = rm.dump(p, reader, 4096, 0)
        assert got.end == rm.ERROR and "record %d (orphan) is the last kept record and has no mate" % n_records in got.message and len(got.recs) == 0
        got = rm.dump(p, reader, 5, 0)  # (the whole batches in front of it have gone out)
        assert got.end == rm.ERROR and len(got.recs) == len(corpus[1].recs) // 5 * 5 and got.batches == [(5, t) for _, t in got.batches]


def test_a_single_end_file_is_not_for_these_readers(tmp_path):
    p = tmp_path / "se.bam"
    p.write_bytes(bm.bgzf(bm.corpus_stream()))
    with pytest.raises(RuntimeError) as ei:
        rm.dump(p, MATE1, 3, 0)
    assert "no paired BAM" in str(ei.value)
