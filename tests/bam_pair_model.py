"""Paired BAM in plain Python: the specification of the paired BAM reader and of BAM output of pairs (nohuman_amd/csrc/nh_bam.*,
nh_bamout.hip), on the forge of tests/bam_model.py.  Nothing here calls the library.

  records        every record of an inflated stream, paired ones included (bam_model.records refuses them)
  is_paired      a file is paired iff its first kept record has flag 0x1 (a file without a kept record is single-end)
  pairs          the kept records two by two, in file order -> [(mate 1, mate 2, the one that lies first, the other)]
  to_fastq_pair  (text1, text2, counts): the two FASTQ files a paired run is the run on
  select_pairs   the inflated stream of a BAM output of pairs
  cut_pairs      the paired reader's batches
  corpus         the forged file the scan, reader and kernel tests share

The rules: kept is bam_model.kept.  In a paired file two neighbouring kept records (skipped ones in between are stepped over) form
a pair iff both have 0x1, exactly one has 0x40 and the other 0x80, and their names are equal byte for byte; the 0x40 record is mate 1
whichever comes first.  Anything else is PairError with the ordinal of the record that breaks the chain -- looked at in this order:
the record's own flags (0x1, then 0x40 / 0x80), its name against the first record's, its mate number against the first record's; a
last kept record without a partner is refused under its own ordinal.  Each mate is transcoded as a single-end record is: no /1 /2."""
import collections
import contextlib

import numpy as np

from tests import bam_model as bm

MATE1, MATE2 = 0x40, 0x80
P1, P2 = bm.PAIRED | MATE1, bm.PAIRED | MATE2


class PairError(bm.BamError):
    """kind: "not paired" (a kept record without 0x1), "mate flags" (both or neither of 0x40 / 0x80), "same mate", "not collated"
    (two names), "no mate" (the last kept record)"""


@contextlib.contextmanager
def _paired_records_allowed():
    """bam_model.records with its refusal of flag 0x1 switched off: the walk and every other refusal are its own"""
    old = bm.PAIRED
    bm.PAIRED = 0
    try:
        yield
    finally:
        bm.PAIRED = old


def records(stream):
    with _paired_records_allowed():
        return bm.records(stream)


def is_paired(stream):
    for r in records(stream):
        if bm.kept(r):
            return bool(r.flag & 0x1)
    return False


def pairs(stream):
    """-> [(mate1, mate2, first, second)] of bam_model.Rec; PairError as the reader refuses; a single-end stream: bam_model's rules"""
    if not is_paired(stream):
        recs = bm.records(stream)  # (a 0x1 record anywhere in a single-end file: BamError("paired"))
        if not any(bm.kept(r) for r in recs):
            return []  # (no kept record: no pair either)
        raise ValueError("not a paired stream")
    out, first = [], None
    for r in records(stream):
        if not bm.kept(r):
            continue
        if not r.flag & 0x1:
            raise PairError("not paired", r.ordinal)
        if bool(r.flag & MATE1) == bool(r.flag & MATE2):
            raise PairError("mate flags", r.ordinal)
        if first is None:
            first = r
            continue
        if r.name != first.name:
            raise PairError("not collated", r.ordinal)
        if (r.flag & 0xC0) == (first.flag & 0xC0):
            raise PairError("same mate", r.ordinal)
        out.append((first, r, first, r) if first.flag & MATE1 else (r, first, first, r))
        first = None
    if first is not None:
        raise PairError("no mate", first.ordinal)
    return out


PairCounts = collections.namedtuple("PairCounts", "pairs bases1 bases2")


def to_fastq_pair(stream):
    """-> (text1, text2, PairCounts): mate 1's and mate 2's FASTQ, a record a pair each, in the order of the pairs"""
    ps = pairs(stream)
    t1 = b"".join(bm.record_text(m1) for m1, _, _, _ in ps)
    t2 = b"".join(bm.record_text(m2) for _, m2, _, _ in ps)
    return t1, t2, PairCounts(len(ps), sum(m1.l_seq for m1, _, _, _ in ps), sum(m2.l_seq for _, m2, _, _ in ps))


def file_order_fastq(stream):
    """the FASTQ of every kept record in file order (what nh_bam_scan digests), and bam_model's Counts"""
    with _paired_records_allowed():
        text, counts, _, _ = bm.to_fastq(stream)
    return text, counts


def header_bytes(stream):
    recs = records(stream)
    return stream[:recs[0].offset] if recs else stream


def _bytes(stream, r):
    return stream[r.offset:r.offset + 4 + r.block_size]


def selected_pair_bytes(stream, host_flags, want, skip=()):
    """the records of the pairs whose host flag is `want`, both of a pair, in file order; skip: pairs left out"""
    ps = pairs(stream)
    assert len(host_flags) == len(ps), (len(host_flags), len(ps))
    return b"".join(_bytes(stream, a) + _bytes(stream, b) for i, ((_, _, a, b), h) in enumerate(zip(ps, host_flags))
                    if bool(h) == bool(want) and i not in skip)


def select_pairs(stream, host_flags, want):
    """the inflated stream of a BAM output: the header, then both records of every pair whose host flag is `want`, in file order,
    each as it lies in the input; skipped records are written nowhere"""
    return header_bytes(stream) + selected_pair_bytes(stream, host_flags, want)


def parse(out_stream):
    """-> (the header's bytes, [the bytes of each record]): an output must still be a BAM stream (bamout_model.parse, on records)"""
    return header_bytes(out_stream), [_bytes(out_stream, r) for r in records(out_stream)]


def pair_table(stream, base=0):
    """what the builder takes: (pairs, 2) uint64 -- where the pair's two records lie, in file order, less `base`"""
    return np.array([(a.offset - base, b.offset - base) for _, _, a, b in pairs(stream)], np.uint64).reshape(-1, 2)


def cut_pairs(stream, batch_pairs, max_text):
    """the paired reader's batches -> [(pairs, bytes of mate 1's text, of mate 2's)]: up to batch_pairs pairs, cut after the pair at
    which either mate's text reaches max_text (0: no budget)"""
    out, n, t1, t2 = [], 0, 0, 0
    for m1, m2, _, _ in pairs(stream):
        n, t1, t2 = n + 1, t1 + len(bm.record_text(m1)), t2 + len(bm.record_text(m2))
        if n == batch_pairs or (max_text and (t1 >= max_text or t2 >= max_text)):
            out.append((n, t1, t2))
            n, t1, t2 = 0, 0, 0
    if n:
        out.append((n, t1, t2))
    return out


# ---- the corpus -------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _seq(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def forge_pair(name, seq1, seq2, qual1=None, qual2=None, rev=(0, 0), mate2_first=False, between=(), tags=(b"", b""), extra_flag=0):
    """the records of one pair: mate 1 and mate 2 (or the other way round), with `between` records (skipped ones) between them"""
    m1 = bm.forge_record(name, seq1, qual1, flag=P1 | extra_flag | (bm.REVERSE if rev[0] else 0), tags=tags[0])
    m2 = bm.forge_record(name, seq2, qual2, flag=P2 | extra_flag | (bm.REVERSE if rev[1] else 0), tags=tags[1])
    return [m2] + list(between) + [m1] if mate2_first else [m1] + list(between) + [m2]


def skipped(rng, k):
    """a secondary, a supplementary and an empty record -- all with 0x1, as the records of paired alignments have"""
    return [bm.forge_record(b"sec%d" % k, b"ACGTAC", None, flag=bm.SECONDARY | P1, cigar=[(6 << 4)]),
            bm.forge_record(b"sup%d" % k, _seq(rng, 9), bytes(9), flag=bm.SUPPLEMENTARY | P2 | bm.REVERSE),
            bm.forge_record(b"empty%d" % k, b"", b"", flag=0x4)]


def corpus_records(seed=7, long_mate=40_000):
    """the shared file's records: forward / reverse mates in all four combinations, absent qualities on one mate, mate 2 stored
    first, skipped records before, between and after mates, tags, mates of unequal length, and one pair of a few bases beside 40 kb"""
    rng = np.random.default_rng(seed)
    out = skipped(rng, 0)[:2]  # (in front of the first kept record: their 0x1 does not make the file anything)
    for k in range(24):
        L1, L2 = (1, 2, 3, 7, 63, 64, 65, 150, 151, 255, 256, 257)[k % 12], (150, 5, 64, 1, 257, 3, 149, 150, 2, 256, 65, 8)[k % 12]
        q1 = None if k % 5 == 1 else rng.integers(0, 94, L1, dtype=np.uint8).tobytes()
        q2 = None if k % 5 == 3 else rng.integers(0, 94, L2, dtype=np.uint8).tobytes()
        name = b"pair%d" % k if k % 4 else b"p%d with a comment" % k
        sk = skipped(rng, k)
        between = sk[:1 + k % 3] if k % 3 == 1 else ()
        out += forge_pair(name, _seq(rng, L1), _seq(rng, L2), q1, q2, rev=(k & 1, (k >> 1) & 1), mate2_first=k % 3 == 2, between=between,
                          tags=((b"RGZgroup1\0", b"NMC\x03")[k % 2], (b"", b"RGZgroup1\0MCZ10M\0")[k % 2]), extra_flag=0x4 | 0x8 if k % 2 else 0x2)
        if k % 4 == 3:
            out += sk[k % 3:]
    # a few bases beside 40 kb, the long mate stored first
    out += forge_pair(b"long", _seq(rng, 5), _seq(rng, long_mate), bytes(5), rng.integers(0, 60, long_mate, dtype=np.uint8).tobytes(),
                      rev=(0, 1), mate2_first=True)
    out += forge_pair(b"last", _seq(rng, 30), _seq(rng, 31), bytes(30), None)
    out += skipped(rng, 99)
    return out


def corpus_stream(seed=7, long_mate=40_000):
    return bm.forge_header(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@RG\tID:group1\n") + b"".join(corpus_records(seed, long_mate))


def many_pairs(n, seed=3):
    """n short pairs, every third stored mate 2 first, a skipped record between the mates of every 50th: the builder's block tests"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L1, L2 = 1 + i % 13, 1 + (i * 7) % 11
        out += forge_pair(b"r%d" % i, _seq(rng, L1), _seq(rng, L2), bytes([i % 40]) * L1, None if i % 9 == 0 else bytes([i % 33]) * L2,
                          rev=(i & 1, 0), mate2_first=i % 3 == 0, between=skipped(rng, i)[:1] if i % 50 == 49 else (),
                          tags=(b"NMC\x01" if i % 3 == 0 else b"", b""))
    return bm.forge_header() + b"".join(out)
