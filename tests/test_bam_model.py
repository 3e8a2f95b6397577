"""tests/bam_model.py, the specification of BAM input, held to what it must say by itself: the nibble reversal is the IUPAC
complement, a forged record comes back as the FASTQ written out by hand, and the model's text is canonical four-line FASTQ for the
parser model every reader here is held to (tests/record_model.py)."""
import numpy as np

from tests import bam_model as bm
from tests import record_model as rm


def test_nibble_reversal_is_the_iupac_complement():
    assert len(bm.ALPHABET) == 16 and len(bm.COMPLEMENT) == 16
    for code, letter in enumerate(bm.ALPHABET.decode()):
        assert bm.ALPHABET.decode()[bm.rev4(code)] == bm.COMPLEMENT[letter], letter
        assert bm.rev4(bm.rev4(code)) == code
    # the pairs as the specification lists them, by code
    assert [(c, bm.rev4(c)) for c in (1, 2, 3, 5, 7, 11)] == [(1, 8), (2, 4), (3, 12), (5, 10), (7, 14), (11, 13)]
    assert all(bm.rev4(c) == c for c in (0, 6, 9, 15))  # '=', S, W, N


def test_forge_then_model_round_trip():
    recs = [
        bm.forge_record(b"r1", b"ACGTN", bytes([0, 1, 40, 60, 93])),
        bm.forge_record(b"r2 desc", b"AACGM", bytes([10, 11, 12, 13, 14]), flag=bm.REVERSE, cigar=[5 << 4], tags=b"NMC\x01", ref_id=0, pos=7),
        bm.forge_record(b"sec", b"ACGT", bytes(4), flag=bm.SECONDARY),
        bm.forge_record(b"sup", b"ACGT", bytes(4), flag=bm.SUPPLEMENTARY | bm.REVERSE),
        bm.forge_record(b"empty", b"", b""),
        bm.forge_record(b"r3", b"TTG", None),
        bm.forge_record(b"r4", b"TTGR", None, flag=bm.REVERSE),
    ]
    stream = bm.forge_header(refs=[(b"chr1", 1000)]) + b"".join(recs)
    text, counts, texts, keep = bm.to_fastq(stream)
    assert text == (b"@r1\nACGTN\n+\n!\"I]~\n"
                    b"@r2 desc\nKCGTT\n+\n/.-,+\n"
                    b"@r3\nTTG\n+\n\"\"\"\n"
                    b"@r4\nYCAA\n+\n\"\"\"\"\n")
    assert counts == bm.Counts(records=7, reads=4, bases=17, skipped_secondary=2, skipped_empty=1, reverse_complemented=2, missing_qualities=2)
    assert [r.ordinal for r in keep] == [1, 2, 6, 7] and b"".join(texts) == text
    t = bm.kernel_table(keep, texts)
    assert t[:, 1].tolist() == [0, 18, 41, 55] and int(t[0, 0]) == len(bm.forge_header(refs=[(b"chr1", 1000)]))


def test_framing_round_trips_and_refusals_of_the_model():
    import gzip
    stream = bm.corpus_stream()
    for member in (64, 1000, 65280):
        for eof in (True, False):
            assert gzip.decompress(bm.bgzf(stream, member, eof)) == stream
    hdr = bm.forge_header()
    good = bm.forge_record(b"a", b"ACGT", bytes(4))
    for kind, data in (("ends inside", hdr[:10]), ("ends inside", hdr + good[:20]), ("ends inside", hdr + good[:-1]),
                       ("paired", hdr + good + bm.forge_record(b"p", b"AC", bytes(2), flag=bm.PAIRED))):
        try:
            bm.records(data)
        except bm.BamError as e:
            assert e.kind == kind
        else:
            raise AssertionError(kind)


def test_model_text_is_canonical_fastq():
    text, counts, texts, keep = bm.to_fastq(bm.corpus_stream())
    p = rm.parse(text)
    assert p.end == rm.END_OF_TEXT and len(p.recs) == counts.reads == len(texts)
    assert p.recs[:, rm.R_CANON].all()
    assert (p.recs[:, rm.R_END] - p.recs[:, rm.R_START]).tolist() == [len(x) for x in texts]
    assert (p.recs[:, rm.R_SE] - p.recs[:, rm.R_S]).tolist() == [r.l_seq for r in keep]
    assert (p.recs[:, rm.R_QE] - p.recs[:, rm.R_Q]).tolist() == [r.l_seq for r in keep]
    assert (p.recs[:, rm.R_HE] - p.recs[:, rm.R_START]).tolist() == [1 + len(r.name) for r in keep]
    # the corpus holds what its docstring says
    lens = {r.l_seq for r in keep}
    assert set(bm.LENGTHS) <= lens
    assert {len(r.name) for r in keep} >= {1, 254}
    assert {r.offset % 4 for r in keep} == {0, 1, 2, 3}
    starts = np.cumsum([0] + [len(x) for x in texts[:-1]])
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    assert counts.skipped_secondary and counts.skipped_empty and counts.reverse_complemented and counts.missing_qualities
    assert int(p.recs[-1, rm.R_IDLEN]) == 4  # "last one  with blanks": the id ends at the first blank
