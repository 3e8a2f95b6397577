"""The specification of --host-bases-only (nh_run_hostbases; nohuman_amd/csrc/nh_cover.hip k_cover_close, nh_mask.hip): a masked run
that writes N only over the bases that host k-mers cover.  Pure Python on tests/intervals_model.py and oracle/k2_literal.py: it calls
nothing of the library.

  close          the gap closing: a maximal run of uncovered bases [a, b) of ONE sequence with a covered base on each side in that
                 sequence (a > 0, b < len) and b - a <= gap becomes covered; a run that touches an end of the sequence never is;
                 gap 0 changes nothing
  close_words    the same on a bitmap laid out as the mark pass leaves it (one bit a byte of the text), sequence by sequence
  sequence_mask  (cov, closed) of one sequence as the classifier read it
  put            a record as the masked run writes it (nh_run.hip put_record()), the sequence with N where `mask` is set and the
                 INPUT's own base elsewhere
  outputs        the mates' outputs of a run and the three counts
"""
import numpy as np

from tests import intervals_model as im


def close(cov, gap):
    """cov: per base, covered -> (closed, the bases that only the closing set)"""
    cov = np.asarray(cov, dtype=bool)
    out = cov.copy()
    n = len(cov)
    added = 0
    if gap <= 0 or n == 0:
        return out, 0
    unc = im.runs(~cov)
    for a, b in unc:
        if a > 0 and b < n and b - a <= gap:
            out[a:b] = True
            added += b - a
    return out, added


def bits_of(words, text_len):
    return np.unpackbits(np.asarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:text_len].astype(bool)


def close_words(words, text_len, recs, gap, skip=()):
    """words: the bitmap (uint32, bit p & 31 of word p >> 5: byte p of the text); recs: (start, length) of every sequence, closed one
    after the other on its own bits (sequences back to back share a word, never a run); skip: the sequences that leave the text
    -> (the bitmap, the bases set)"""
    nw = (text_len + 31) // 32
    bits = np.zeros(nw * 32, dtype=bool)
    bits[:text_len] = bits_of(words, text_len)
    total = 0
    for i, (s, n) in enumerate(recs):
        if i in skip:
            continue
        c, added = close(bits[s:s + n], gap)
        bits[s:s + n] = c
        total += added
    return np.packbits(bits.reshape(-1, 32).astype(np.uint8), axis=1, bitorder="little").view("<u4").reshape(-1), total


def sequence_mask(db, seq, gap, host_of=None, memo=None):
    """seq: the sequence AS THE CLASSIFIER READ IT -> (cov, closed, the bases only the closing set)"""
    cov = im.covered(db, seq, host_of, memo)
    closed, added = close(cov, gap)
    return cov, closed, added


def put(r, mask=None):
    """the masked run's record of r (tests/builder_model.Rec); mask: None (no base is touched) or per base of r.seq"""
    seq = bytes(r.seq)
    if mask is not None:
        assert len(mask) == len(seq)
        seq = bytes(ord("N") if m else c for c, m in zip(seq, mask))
    out = r.header + b"\n" + seq
    if r.fastq:
        out += b"\n+\n" + r.qual
    return out + b"\n"


def outputs(db, records, read_as, host_calls, gap, host_of=None):
    """records: per mate the list of Rec; read_as: per fragment the tuple of its mates' sequences as the classifier read them (the
    quality- or DUST-masked copy where the run has one); host_calls: per fragment its call AFTER the host selection (not 0: a host
    fragment, exactly the fragments a masked run blanks)
    -> (per mate the bytes of out1 / out2, (host_bases, masked_bases, closed_bases), per fragment and mate (cov, closed) or None)"""
    memo = {}
    parts = [[] for _ in records]
    host_bases = masked = closed_only = 0
    masks = []
    for f, call in enumerate(host_calls):
        row = []
        for m, recs in enumerate(records):
            r = recs[f]
            if int(call) == 0:
                parts[m].append(put(r))
                row.append(None)
                continue
            seq = bytes(read_as[f][m])
            assert len(seq) == r.slen
            cov, closed, added = sequence_mask(db, seq, gap, host_of, memo)
            host_bases += r.slen
            masked += int(closed.sum())
            closed_only += added
            parts[m].append(put(r, closed))
            row.append((cov, closed))
        masks.append(row)
    return [b"".join(p) for p in parts], (host_bases, masked, closed_only), masks
