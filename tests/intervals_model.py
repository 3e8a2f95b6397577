"""The specification of --host-intervals (nh_run_intervals; nohuman_amd/csrc/nh_cover.hip): which k-mers of a sequence are host
k-mers, which bases they cover, the intervals, and the BED file of a run.  Pure Python on oracle/k2_literal.py: it calls nothing
of the library.

  kmer_facts     per k-mer (ambiguous, minimizer): oracle/k2_literal.kmer_minimizers in linear time (tests/test_intervals_model.py
                 compares the two), so that reads of tens of kilobases can be modelled
  host_kmers     per k-mer: it is a host k-mer -- not ambiguous under the database's ambiguity rule, its minimizer looked up (the
                 minimum_acceptable_hash_value filter as in the classifier), found with a non-zero value v, and host_of[v] where a
                 one-byte-a-node table is given
  covered        per base: a host k-mer contains it
  intervals      the maximal runs of covered bases, 0-based and half-open
  from_hits      the covered bases derived from a per-k-mer hit list instead (the oracle's, or the classifier's d_kmer_taxa)
  bed            the file: <id> \\t <start> \\t <end> \\t <mate> \\t <external taxid of the fragment's call> \\n, and the three counts
"""
import numpy as np

from oracle import k2_literal as lit

ID_END = b" \t\r"


def kmer_facts(db, seq):
    """[(ambiguous, minimizer or None)] for the k-mers of seq, k-mer i = seq[i, i + k)"""
    k, l, n = db.k, db.l, len(seq)
    lmask = (1 << (2 * l)) - 1
    toggle = db.toggle_mask & lmask
    cand = [None] * n       # the candidate of the l-mer ENDING at j, None where it holds an ambiguous byte
    last_bad = [-1] * n     # the last ambiguous byte at or before j
    fwd = rc = 0
    bad = -1
    for j, ch in enumerate(seq):
        c = lit._CODE.get(ch, -1)
        if c < 0:
            bad, c = j, 0
        last_bad[j] = bad
        fwd = ((fwd << 2) | c) & lmask
        rc = (rc >> 2) | ((3 - c) << (2 * (l - 1)))
        if j >= l - 1 and j - bad >= l:
            r = rc if db.revcom_version != 0 else lit.reverse_complement(fwd, l, 0)
            canon = min(fwd, r)
            if db.spaced_seed_mask:
                canon &= db.spaced_seed_mask
            cand[j] = canon ^ toggle
    span = l if db.ambiguity_rule == 0 else max(l, k - 1)
    out = []
    for e in range(k - 1, n):
        p = last_bad[e]
        if p > e - span:
            out.append((True, None))
            continue
        lo = max(e - (k - l), p + l)
        out.append((False, min(cand[lo:e + 1]) ^ toggle))
    return out


def host_kmers(db, seq, host_of=None, _memo=None):
    """per k-mer of seq: True where it is a host k-mer.  host_of: None (every non-zero value is host) or one byte a node"""
    memo = {} if _memo is None else _memo
    out = []
    for ambiguous, mz in kmer_facts(db, seq):
        if ambiguous:
            out.append(False)
            continue
        if mz not in memo:
            v = 0
            if not (db.min_hash and lit.fmix64(mz) < db.min_hash):
                v = db.get(mz)
            memo[mz] = bool(v) and (host_of is None or bool(host_of[v]))
        out.append(memo[mz])
    return out


def cover_of(flags, k, n):
    """per base of a sequence of n bases: covered by a k-mer whose flag is set"""
    cov = np.zeros(n, dtype=bool)
    for i, h in enumerate(flags):
        if h:
            cov[i:i + k] = True
    return cov


def covered(db, seq, host_of=None, _memo=None):
    return cover_of(host_kmers(db, seq, host_of, _memo), db.k, len(seq))


def runs(cov):
    """the maximal runs of True: [(start, end)], half-open"""
    d = np.diff(np.concatenate(([0], cov.astype(np.int8), [0])))
    return list(zip((int(x) for x in np.nonzero(d == 1)[0]), (int(x) for x in np.nonzero(d == -1)[0])))


def intervals(db, seq, host_of=None, _memo=None):
    return runs(covered(db, seq, host_of, _memo))


def from_hits(taxa, k, n, ambiguous=lit.AMBIG, border=lit.BORDER):
    """the covered bases of a sequence of n bases from its per-k-mer hit list: an entry is host when it is neither 0 nor a marker"""
    return cover_of([t not in (0, ambiguous, border) for t in taxa], k, n)


def record_id(header, paired):
    """the calls table's id: mate 1's header behind '@' / '>' up to the first space, tab or '\\r'; a paired run drops a trailing
    /1 or /2 from an id longer than two bytes (kraken2 TrimPairInfo)"""
    i = header[1:]
    for x, c in enumerate(i):
        if c in ID_END:
            i = i[:x]
            break
    if paired and len(i) > 2 and i[-2:] in (b"/1", b"/2"):
        i = i[:-2]
    return i


def bed(db, headers, fragments, calls, ext_ids, host_of=None):
    """headers: mate 1's header line of every fragment; fragments: per fragment the tuple of its mates' sequences AS THE
    CLASSIFIER READS THEM; calls: the internal taxon of every fragment's call; ext_ids: internal -> external taxon id.
    -> (the file's bytes, (fragments with a line, intervals, covered bases))"""
    memo, lines = {}, []
    n_frag = n_ivl = n_cov = 0
    for f, mates in enumerate(fragments):
        paired = len(mates) == 2
        rid = record_id(headers[f], paired)
        taxid = int(ext_ids[calls[f]]) if calls[f] else 0
        any_line = False
        for m, seq in enumerate(mates):
            for s, e in intervals(db, seq, host_of, memo):
                lines.append(b"%s\t%d\t%d\t%d\t%d\n" % (rid, s, e, m + 1, taxid))
                n_ivl += 1
                n_cov += e - s
                any_line = True
        n_frag += any_line
    return b"".join(lines), (n_frag, n_ivl, n_cov)


def cover_words(text_len, recs, covs):
    """the bitmap of a text: uint32 words, bit (p & 31) of word p >> 5 set for every covered byte p; recs: (start, length) of
    every sequence, covs: its per-base cover"""
    bits = np.zeros(((text_len + 31) // 32) * 32, dtype=np.uint8)
    for (s, n), c in zip(recs, covs):
        bits[s:s + n] |= c.astype(np.uint8)
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def records_of(recs, covs):
    """[(seq, start, end)] in the order of the sequence table, then by start"""
    return [(i, s, e) for i, c in enumerate(covs) for s, e in runs(c)]
