"""A plain Python / numpy model of the read statistics (nh_run_rstats, `--read-stats`; nohuman_amd/csrc/nh_rstats.hip): the
SPECIFICATION of the accumulators, of median and N50 and of the table.  Test helper: it never imports the engine.

A read is (mate, human, sequence bytes, quality bytes or None); every function below takes a list of them.
  reads_of_text     the reads of a batch text given as (sequence start, length, quality start) records and per-fragment calls
  reads_of_records  the reads of parsed records (tests/builder_model.py) per mate and per-fragment calls
  accumulate        the four accumulators [class][mate] as a (2, 2, 102) uint64 array with the layout of nh_read_class
  median / n50      of a list of lengths
  summary           accumulators, medians, N50s and mates: what nh_read_stats holds
  table             the text of the table from a summary

Definitions (the project's own, not seqkit's): a read of length 0 is a read; min_len of an empty class is reported as 0; gc
counts the bytes in GCgc over ALL bases, other the bytes not in ACGTacgt; qhist[q] counts the bases of the records that have
qualities whose quality byte, read as unsigned, less 33 and clamped to 0 .. 93, is q; the median is the lower nearest-rank element
(0-based index ceil(n / 2) - 1 of the ascending lengths); N50 is the largest L such that the reads of length >= L hold at least
half of the bases (2 * sum >= bases); both are 0 for an empty set; the input set is the two classes together."""
import math

import numpy as np

QBINS = 94
WORDS = 8 + QBINS
READS, BASES, MIN_LEN, MAX_LEN, GC, OTHER, QUAL_READS, QUAL_BASES = range(8)
NONE = 2 ** 64 - 1
SETS = ("input", "nonhuman", "human")
HEADER = "set\tmate\treads\tbases\tmin_len\tmean_len\tmedian_len\tmax_len\tN50\tgc_pct\tother_bases\tq20_pct\tq30_pct\tmean_qual\n"
_IS_GC = np.zeros(256, dtype=bool)
_IS_GC[list(b"GCgc")] = True
_IS_ACGT = np.zeros(256, dtype=bool)
_IS_ACGT[list(b"ACGTacgt")] = True


def reads_of_text(text, recs, calls, mates=1, bad=()):
    """recs[i] = (sequence start, length, quality start or NONE); fragment i // mates has calls[i // mates]; the records whose
    index is in `bad` are left out"""
    text = bytes(text)
    out = []
    for i, (s, n, q) in enumerate(recs):
        if i in bad:
            continue
        out.append((i % mates, bool(calls[i // mates]), text[s:s + n], None if q == NONE else text[q:q + n]))
    return out


def reads_of_records(records, calls):
    """records: per mate the parsed records; a FASTA record has no qualities"""
    out = []
    for m, recs in enumerate(records):
        assert len(recs) == len(calls)
        for r, c in zip(recs, calls):
            out.append((m, bool(c), bytes(r.seq), bytes(r.qual) if r.fastq else None))
    return out


def empty():
    a = np.zeros((2, 2, WORDS), dtype=np.uint64)
    a[:, :, MIN_LEN] = NONE
    return a


def accumulate(reads, acc=None):
    """the accumulators as the kernel leaves them (an empty one keeps min_len all-ones); acc: added to"""
    acc = empty() if acc is None else acc.copy()
    for mate, human, seq, qual in reads:
        a = acc[int(human), mate]
        n = len(seq)
        b = np.frombuffer(seq, dtype=np.uint8)
        a[READS] += 1
        a[BASES] += n
        a[MIN_LEN] = min(int(a[MIN_LEN]), n)
        a[MAX_LEN] = max(int(a[MAX_LEN]), n)
        a[GC] += int(_IS_GC[b].sum())
        a[OTHER] += int((~_IS_ACGT[b]).sum())
        if qual is not None:
            assert len(qual) == n
            a[QUAL_READS] += 1
            a[QUAL_BASES] += n
            q = np.clip(np.frombuffer(qual, dtype=np.uint8).astype(np.int64) - 33, 0, QBINS - 1)
            a[8:] += np.bincount(q, minlength=QBINS).astype(np.uint64)
    return acc


def median(lens):
    s = sorted(lens)
    return s[(len(s) + 1) // 2 - 1] if s else 0


def n50(lens):
    total, acc = sum(lens), 0
    for L in sorted(lens, reverse=True):
        acc += L
        if 2 * acc >= total:
            return L
    return 0


def summary(reads, mates):
    """dict: cls (2, 2, 102) with min_len 0 for an empty class, median and n50 (3, 2), mates"""
    cls = accumulate(reads)
    cls[:, :, MIN_LEN][cls[:, :, READS] == 0] = 0
    med = np.zeros((3, 2), dtype=np.uint64)
    n5 = np.zeros((3, 2), dtype=np.uint64)
    for m in range(mates):
        per = [[len(seq) for mate, human, seq, _q in reads if mate == m and human == bool(c)] for c in range(2)]
        for st, lens in enumerate((per[0] + per[1], per[0], per[1])):
            med[st, m], n5[st, m] = median(lens), n50(lens)
    return dict(cls=cls, median=med, n50=n5, mates=mates)


def _ratio(num, den):
    return "NA" if den == 0 else "%.2f" % (num / den)


def row(name, mate, a, med, n5):
    """one line of the table from one accumulator (102 integers, min_len 0 when empty)"""
    a = [int(x) for x in a]
    qh = a[8:]
    err = 0.0
    for q in range(QBINS):
        err += float(qh[q]) * math.pow(10.0, -float(q) / 10.0)
    mean_q = "NA" if a[QUAL_BASES] == 0 else "%.2f" % (-10.0 * math.log10(err / float(a[QUAL_BASES])))
    cols = [name, str(mate + 1), str(a[READS]), str(a[BASES]), str(a[MIN_LEN] if a[READS] else 0), _ratio(float(a[BASES]), a[READS]),
            str(int(med)), str(a[MAX_LEN] if a[READS] else 0), str(int(n5)), _ratio(100.0 * float(a[GC]), a[BASES]), str(a[OTHER]),
            _ratio(100.0 * float(sum(qh[20:])), a[QUAL_BASES]), _ratio(100.0 * float(sum(qh[30:])), a[QUAL_BASES]), mean_q]
    return "\t".join(cols) + "\n"


def union(u, h):
    """the input set's accumulator: the two classes together"""
    c = u + h
    ur, hr = int(u[READS]), int(h[READS])
    c[MIN_LEN] = h[MIN_LEN] if not ur else u[MIN_LEN] if not hr else min(int(u[MIN_LEN]), int(h[MIN_LEN]))
    c[MAX_LEN] = max(int(u[MAX_LEN]) if ur else 0, int(h[MAX_LEN]) if hr else 0)
    return c


def table(sm):
    out = [HEADER]
    for st, name in enumerate(SETS):
        for m in range(sm["mates"]):
            a = sm["cls"][st - 1, m] if st else union(sm["cls"][0, m], sm["cls"][1, m])
            out.append(row(name, m, a, sm["median"][st, m], sm["n50"][st, m]))
    return "".join(out).encode()


def fill_struct(sm, raw):
    """a summary into an nh_read_stats (the ctypes struct of nohuman_amd/_lib.py, passed in: no import here)"""
    for c in range(2):
        for m in range(2):
            k = raw.cls[c][m]
            a = [int(x) for x in sm["cls"][c, m]]
            (k.reads, k.bases, k.min_len, k.max_len, k.gc, k.other, k.qual_reads, k.qual_bases) = a[:8]
            for q in range(QBINS):
                k.qhist[q] = a[8 + q]
    for st in range(3):
        for m in range(2):
            raw.median_len[st][m] = int(sm["median"][st, m])
            raw.n50[st][m] = int(sm["n50"][st, m])
    raw.mates = sm["mates"]
    return raw


def summary_of_struct(raw):
    """an nh_read_stats as a summary"""
    cls = np.zeros((2, 2, WORDS), dtype=np.uint64)
    for c in range(2):
        for m in range(2):
            k = raw.cls[c][m]
            cls[c, m, :8] = [k.reads, k.bases, k.min_len, k.max_len, k.gc, k.other, k.qual_reads, k.qual_bases]
            cls[c, m, 8:] = list(k.qhist)
    med = np.array([[raw.median_len[st][m] for m in range(2)] for st in range(3)], dtype=np.uint64)
    n5 = np.array([[raw.n50[st][m] for m in range(2)] for st in range(3)], dtype=np.uint64)
    return dict(cls=cls, median=med, n50=n5, mates=int(raw.mates))


INT_COLUMNS = (0, 1, 2, 3, 4, 6, 7, 8, 10)  # of a table row: compared byte for byte; the others are %.2f ratios or NA


def same_table(got, want):
    """the library's table against the model's: the integer columns byte for byte, the %.2f columns within one unit of the
    last printed digit (the two sides may differ in log10 / pow by an ulp); returns a description of the first difference"""
    g, w = got.decode().splitlines(), want.decode().splitlines()
    if len(g) != len(w) or g[0] != w[0]:
        return "header or line count: %r / %r" % (g[:1], w[:1])
    for a, b in zip(g[1:], w[1:]):
        ca, cb = a.split("\t"), b.split("\t")
        if len(ca) != 14 or len(cb) != 14:
            return "columns: %r / %r" % (a, b)
        for i in range(14):
            if i in INT_COLUMNS or "NA" in (ca[i], cb[i]):
                if ca[i] != cb[i]:
                    return "column %d: %r / %r" % (i, a, b)
            elif len(ca[i].split(".")[-1]) != 2 or abs(float(ca[i]) - float(cb[i])) > 0.0100001:
                return "column %d: %r / %r" % (i, a, b)
    return None
