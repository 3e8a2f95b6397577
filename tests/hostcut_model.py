"""The specification of --host-cut (nh_run_hostcut; nohuman_amd/csrc/nh_cut.hip): a masked run that cuts the stretches the closed
coverage covers out of a host fragment and writes what is left as records of their own.  Pure Python on tests/hitmask_model.py and
tests/intervals_model.py: it calls nothing of the library.

  pieces         the maximal runs [a, b) of uncovered bases of one sequence with b - a >= min_piece, runs at an end included
  tally          the counts of one host sequence: (host_bases, pieces, piece_bases, cut_bases, short_bases, dropped_reads)
  piece_record   a piece's record: the header cut behind the id, ":<a>-<b>", the rest of the header, the INPUT's bases [a, b) and,
                 FASTQ, the qualities [a, b)
  text_of        out1 of a batch from the records, which of them are host and their closed coverage; the six counts
  outputs        out1 and the seven counts of a run (closed_bases last), from the sequences as the classifier read them
  max_pieces     P(L) = (L + k) / (M + k), 0 where L < M: the most pieces a sequence of L bases has
  output_cap     the builder's output capacity: the mask builder's plus P(slen) * (hlen + 29) a record
"""
import numpy as np

from tests import hitmask_model as hm
from tests import intervals_model as im

K = 35
COUNTS = ("host_bases", "pieces", "piece_bases", "cut_bases", "short_bases", "dropped_reads", "closed_bases")


def pieces(closed, min_piece):
    """closed: per base of one sequence, covered after the closing -> [(a, b)]"""
    closed = np.asarray(closed, dtype=bool)
    return [(a, b) for a, b in im.runs(~closed) if b - a >= min_piece]


def tally(closed, min_piece):
    closed = np.asarray(closed, dtype=bool)
    unc = im.runs(~closed)
    kept = [(a, b) for a, b in unc if b - a >= min_piece]
    piece_bases = sum(b - a for a, b in kept)
    short = sum(b - a for a, b in unc) - piece_bases
    return (len(closed), len(kept), piece_bases, int(closed.sum()), short, int(not kept))


def piece_record(r, a, b):
    """r: tests/builder_model.Rec; the id ends at the first space, tab or '\\r' of the header (the reader's idlen)"""
    head = 1 + len(im.record_id(r.header, False))
    out = r.header[:head] + b":%d-%d" % (a, b) + r.header[head:] + b"\n" + r.seq[a:b]
    if r.fastq:
        assert r.qlen == r.slen
        out += b"\n+\n" + r.qual[a:b]
    return out + b"\n"


def text_of(records, host, closed, min_piece):
    """records: the Rec of every fragment; host: per fragment, it is a host fragment; closed: per host fragment its closed
    coverage (anything for the others) -> (out1, the six counts, per fragment its pieces or None)"""
    parts, cuts = [], []
    total = [0] * 6
    for r, h, c in zip(records, host, closed):
        if not h:
            parts.append(hm.put(r))
            cuts.append(None)
            continue
        assert len(c) == r.slen
        ps = pieces(c, min_piece)
        parts += [piece_record(r, a, b) for a, b in ps]
        cuts.append(ps)
        total = [x + y for x, y in zip(total, tally(c, min_piece))]
    return b"".join(parts), tuple(total), cuts


def outputs(db, records, read_as, host_calls, gap, min_piece, host_of=None):
    """records: the list of Rec (single-end); read_as: per fragment its sequence as the classifier read it (the quality- or
    DUST-masked copy where the run has one); host_calls: per fragment its call AFTER the host selection
    -> (out1, the seven counts in the order of COUNTS, per fragment its pieces or None)"""
    memo = {}
    closed, added = [], 0
    for r, seq, call in zip(records, read_as, host_calls):
        if int(call) == 0:
            closed.append(None)
            continue
        assert len(seq) == r.slen
        _cov, c, a = hm.sequence_mask(db, bytes(seq), gap, host_of, memo)
        closed.append(c)
        added += a
    text, six, cuts = text_of(records, [int(c) != 0 for c in host_calls], closed, min_piece)
    return text, six + (added,), cuts


def max_pieces(length, min_piece, k=K):
    return 0 if length < min_piece else (length + k) // (min_piece + k)


def output_cap(records, min_piece, mask_cap):
    """mask_cap: the mask builder's capacity for the same records"""
    return mask_cap + sum(max_pieces(r.slen, min_piece) * (r.hlen + 29) for r in records)


def kmer_union(rng, n, p, k=K):
    """a coverage as the mark pass can leave it: a union of k-mers of a sequence of n bases, each of its n - k + 1 k-mers with
    probability p"""
    cov = np.zeros(n, dtype=bool)
    if n >= k:
        for i in np.nonzero(rng.random(n - k + 1) < p)[0]:
            cov[i:i + k] = True
    return cov
