"""The host side of the paired BAM reader (nohuman_amd/csrc/nh_bam.cpp: the pair chain in BamStream, nh_bam_scan, nh_bam_scan_pairs,
nh_bam_paired) against tests/bam_pair_model.py: counts and the three digests of the forged corpus -- the file-order FASTQ and each
mate's -- with the window filled 1, 5 and 7 bytes at a time and BGZF members of 64, 1000 and 65280 bytes; every refusal of a pair
chain with its ordinal and a fragment of its message, with and without bgzip's EOF member; and a single-end file with a late 0x1
record, which is refused as it always was.  No GPU."""
import pytest

import nohuman_amd
from nohuman_amd import EngineError
from tests import bam_model as bm
from tests import bam_pair_model as pm
from tests.test_bam_scan import model_digest, write

EINVAL, EIO = -1, -2


@pytest.fixture(scope="module")
def corpus():
    stream = pm.corpus_stream()
    t1, t2, pc = pm.to_fastq_pair(stream)
    text, counts = pm.file_order_fastq(stream)
    return stream, counts, pc, (model_digest(text), model_digest(t1), model_digest(t2))


def test_the_model_s_corpus_holds_what_it_promises():
    stream = pm.corpus_stream()
    ps = pm.pairs(stream)
    recs = pm.records(stream)
    assert pm.is_paired(stream) and not bm.kept(recs[0]) and recs[0].flag & 0x1
    assert any(a is m2 for _, m2, a, _ in ps) and any(a is m1 for m1, _, a, _ in ps)  # mate 2 first, mate 1 first
    assert any(b.ordinal - a.ordinal > 1 for _, _, a, b in ps)  # skipped records between two mates
    assert {(bool(m1.flag & bm.REVERSE), bool(m2.flag & bm.REVERSE)) for m1, m2, _, _ in ps} == {(False, False), (False, True), (True, False), (True, True)}
    assert any((m1.qual[0] == 0xFF) != (m2.qual[0] == 0xFF) for m1, m2, _, _ in ps)
    assert any(m1.l_seq < 10 and m2.l_seq >= 40_000 for m1, m2, _, _ in ps)
    assert not bm.kept(recs[-1])
    t1, t2, pc = pm.to_fastq_pair(stream)
    assert t1.count(b"\n") == t2.count(b"\n") == 4 * pc.pairs and b"/1\n" not in t1 and b"/2\n" not in t2
    with pytest.raises(bm.BamError):
        bm.records(stream)  # (the single-end model refuses the file, as the single-end reader did)


@pytest.mark.parametrize("chunk,member", [(1, 65280), (5, 64), (7, 1000), (4096, 65280)])
def test_counts_and_three_digests(tmp_path, corpus, monkeypatch, chunk, member):
    stream, counts, pc, digests = corpus
    monkeypatch.setenv("NOHUMAN_BAM_CHUNK", str(chunk))
    for eof in (True, False):
        p = write(tmp_path, "c%d.bam" % eof, bm.bgzf(stream, member, eof))
        assert nohuman_amd.bam_paired(p) is True
        info = nohuman_amd.bam_scan(p)
        assert info[:7] == tuple(counts) and info.digest == digests[0]
        info2, pairs = nohuman_amd.bam_scan_pairs(p, threads=2)
        assert info2 == info
        assert pairs == (True, pc.pairs, pc.bases1, pc.bases2, digests[1], digests[2])
        assert 2 * pairs.pairs == info.reads and pairs.bases1 + pairs.bases2 == info.bases


def test_a_single_end_file_through_the_pair_scan(tmp_path):
    stream = bm.corpus_stream()
    p = write(tmp_path, "se.bam", bm.bgzf(stream))
    info, pairs = nohuman_amd.bam_scan_pairs(p)
    assert info == nohuman_amd.bam_scan(p) and info[:7] == tuple(bm.to_fastq(stream)[1])
    assert pairs == (False, 0, 0, 0, model_digest(b""), model_digest(b""))
    assert nohuman_amd.bam_paired(p) is False
    fq = write(tmp_path, "x.fq", b"@r\nACGT\n+\nIIII\n")
    assert nohuman_amd.bam_paired(fq) is False and nohuman_amd.bam_paired(str(tmp_path / "none.bam")) is False
    with pytest.raises(EngineError) as ei:
        nohuman_amd.bam_scan_pairs(fq)
    assert ei.value.code == EINVAL


def _broken():
    """name -> (stream, the model's kind, the ordinal, a fragment of the message)"""
    rng_seq = b"ACGTACGTAC"
    q = bytes(10)
    hdr = bm.forge_header()
    good = b"".join(r for i in range(2) for r in pm.forge_pair(b"g%d" % i, rng_seq, rng_seq[:7], q, q[:7], mate2_first=i == 1))  # records 1..4
    rec = lambda name, flag, seq=rng_seq: bm.forge_record(name, seq, bytes(len(seq)), flag=flag)  # noqa: E731
    sec = bm.forge_record(b"sec", b"ACGT", None, flag=bm.SECONDARY | pm.P2)
    out = {}
    out["unpaired record"] = (hdr + good + rec(b"x", 0) + rec(b"x", pm.P2), "not paired", 5, "record 5 (x) is not paired")
    out["unpaired second"] = (hdr + good + rec(b"x", pm.P1) + rec(b"x", 0x80), "not paired", 6, "record 6 (x) is not paired")
    out["neither mate"] = (hdr + good + rec(b"x", bm.PAIRED) + rec(b"x", pm.P2), "mate flags", 5, "record 5 (x) has neither of the flags 0x40 and 0x80")
    out["both mates"] = (hdr + good + rec(b"x", pm.P1) + rec(b"x", pm.P1 | pm.MATE2), "mate flags", 6, "record 6 (x) has both of the flags 0x40 and 0x80")
    out["same mate"] = (hdr + good + rec(b"x", pm.P2) + sec + rec(b"x", pm.P2), "same mate", 7, "record 7 (x) and record 5 are both mate 2")
    out["two names"] = (hdr + good + rec(b"x", pm.P1) + rec(b"y", pm.P2) + rec(b"y", pm.P1), "not collated", 6, "record 6 (y) follows record 5 (x)")
    out["orphan at the end"] = (hdr + good + rec(b"x", pm.P1) + sec, "no mate", 5, "record 5 (x) is the last kept record and has no mate")
    out["orphan alone"] = (hdr + rec(b"only", pm.P2), "no mate", 1, "record 1 (only) is the last kept record and has no mate")
    # a kept record whose mate is empty (and therefore skipped) is an orphan: the next kept record has another name
    out["empty mate"] = (hdr + good + rec(b"x", pm.P1) + rec(b"x", pm.P2, b"") + b"".join(pm.forge_pair(b"z", rng_seq, rng_seq, q, q)),
                         "not collated", 7, "record 7 (z) follows record 5 (x)")
    out["empty mate at the end"] = (hdr + good + rec(b"x", pm.P2, b"") + rec(b"x", pm.P1), "no mate", 6, "record 6 (x) is the last kept record")
    return out


BROKEN = _broken()


@pytest.mark.parametrize("case", sorted(BROKEN))
def test_refusals_of_the_pair_chain(tmp_path, case):
    stream, kind, ordinal, message = BROKEN[case]
    with pytest.raises(pm.PairError) as mi:
        pm.pairs(stream)
    assert (mi.value.kind, mi.value.ordinal) == (kind, ordinal)
    for eof in (True, False):
        p = write(tmp_path, "bad%d.bam" % eof, bm.bgzf(stream, 1000, eof))
        assert nohuman_amd.bam_paired(p) is True  # (paired by its first kept record, whatever comes after)
        for scan in (nohuman_amd.bam_scan, nohuman_amd.bam_scan_pairs):
            with pytest.raises(EngineError) as ei:
                scan(p)
            assert ei.value.code == EIO and message in ei.value.message, ei.value.message
            if kind in ("not collated", "no mate"):
                assert "samtools collate" in ei.value.message


def test_a_late_paired_record_in_a_single_end_file_is_refused_as_ever(tmp_path):
    hdr = bm.forge_header()
    good = bm.forge_record(b"ok", b"ACGT", bytes(4))
    late = bm.forge_record(b"mate", b"ACGT", bytes(4), flag=pm.P1)
    sec_first = bm.forge_record(b"early", b"ACGT", bytes(4), flag=bm.SECONDARY | pm.P1)
    for stream, message in ((hdr + good + late, "record 2 (mate) is paired"),
                            (hdr + good + good + late + bm.forge_record(b"mate", b"ACGT", bytes(4), flag=pm.P2), "record 3 (mate) is paired"),
                            (hdr + sec_first + good, "record 1 (early) is paired"),  # (the first 0x1 record of a single-end file, skipped or not)
                            (hdr + sec_first, "record 1 (early) is paired")):
        with pytest.raises(bm.BamError) as mi:
            bm.records(stream)
        assert mi.value.kind == "paired" and "record %d " % mi.value.ordinal in message
        for eof in (True, False):
            p = write(tmp_path, "late.bam", bm.bgzf(stream, 1000, eof))
            assert nohuman_amd.bam_paired(p) is False
            for scan in (nohuman_amd.bam_scan, nohuman_amd.bam_scan_pairs):
                with pytest.raises(EngineError) as ei:
                    scan(p)
                assert ei.value.code == EIO and message in ei.value.message and "samtools fastq -1" in ei.value.message, ei.value.message
