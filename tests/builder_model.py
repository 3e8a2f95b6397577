"""A plain Python model of what the output builders of a run must write, and of how the device splits that work
(nohuman_amd/csrc/nh_mask.hip, nh_split.hip; the host's put_record() in nh_run.hip).  Test helper: pure Python / numpy,
it never imports the engine.

  make_corpus       input text of one or two mate files with, per record, the fields the reader parses from it
  expected_outputs  the exact bytes of a normal, a -H, a split run's human side and a masked run, from the records and the
                    CPU oracle's calls
  block_plan        per batch, mate and block of 1024 records: whether the mask builder copies the block whole (FAST), the
                    shift of that copy, and where the sequences of the classified records lie in the output
"""
import numpy as np

from tests import synth

BLOCK = 1024  # records of one builder block (MB_FRAGS / HB_FRAGS)
WS = b" \t\r\n\v\f"  # isspace()
HCHARS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", dtype=np.uint8)
QCHARS = np.frombuffer(b"#$%&'()*+,-./0123456789:;<=>?ABCDEFGHIJ", dtype=np.uint8)
FASTQ_SHAPES = ("crlf", "plusid", "blanks", "empty", "plain")


class Rec:
    """one record: raw (its bytes in the file), text (the same bytes as the builders see them: a multi-line FASTA sequence
    joined in place by the reader), and the parsed fields as offsets into text"""
    __slots__ = ("raw", "text", "fastq", "hlen", "s", "slen", "q", "qlen", "kind")

    @property
    def header(self):
        return self.text[:self.hlen]

    @property
    def seq(self):
        return self.text[self.s:self.s + self.slen]

    @property
    def qual(self):
        return self.text[self.q:self.q + self.qlen]

    @property
    def out_len(self):
        return self.hlen + 1 + self.slen + 1 + (3 + self.qlen if self.fastq else 0)


def _lines(raw, p=0):
    """std::getline over raw[p:]: (start, end without the newline, next, terminated)"""
    out = []
    while p < len(raw):
        e = raw.find(b"\n", p)
        if e < 0:
            out.append((p, len(raw), len(raw), False))
            break
        out.append((p, e, e + 1, True))
        p = e + 1
    return out


def _rstrip(raw, b, e):
    while e > b and raw[e - 1] in WS:
        e -= 1
    return e


def parse_record(raw, fastq, kind="?"):
    """the reader's view of one whole record (kraken2's record rules: every field without its trailing white space)"""
    r = Rec()
    r.raw, r.fastq, r.kind = bytes(raw), fastq, kind
    ln = _lines(raw)
    assert ln and raw[:1] == (b"@" if fastq else b">")
    r.hlen = _rstrip(raw, ln[0][0], ln[0][1])
    assert r.hlen >= 2
    if fastq:
        assert len(ln) == 4, raw
        r.s, r.slen = ln[1][0], _rstrip(raw, ln[1][0], ln[1][1]) - ln[1][0]
        r.q, r.qlen = ln[3][0], _rstrip(raw, ln[3][0], ln[3][1]) - ln[3][0]
        r.text = r.raw
    else:
        t = bytearray(raw)
        dst = ln[0][2]
        r.s = dst
        for b, e, _nx, _term in ln[1:]:
            n = _rstrip(raw, b, e) - b
            t[dst:dst + n] = raw[b:b + n]  # (memmove to the left: the source is read before it is overwritten)
            dst += n
        r.slen = dst - r.s
        r.q, r.qlen = r.s + r.slen, 0
        r.text = bytes(t)
    return r


def _header(rng, first, n):
    """a header line of n bytes (2..60) without white space at its end; some have a description after a blank"""
    h = bytearray(first + HCHARS[rng.integers(0, HCHARS.size, size=n - 1)].tobytes())
    if n >= 8 and rng.random() < 0.3:
        h[int(rng.integers(2, n - 2))] = 0x20
    return bytes(h)


def _read_len(rng, p_short):
    u = rng.random()
    if u < p_short:
        return int(rng.integers(0, 6))
    if u < p_short + 0.25:
        return int(rng.integers(30, 41))
    return int(rng.integers(100, 301))


def _sequence(rng, allg, n, human):
    if not human or n == 0:
        return synth.random_seq(rng, n)
    st = int(rng.integers(0, len(allg) - n))
    s = allg[st:st + n]
    if rng.random() < 0.5:
        s = synth.revcomp(s)
    return synth.mutate(rng, s, 0.01, 0.0, 0.0)


def _fastq_raw(h, s, q, shape, pad=b""):
    if shape == "crlf":
        return h + b"\r\n" + s + b"\r\n+\r\n" + q + b"\r\n"
    if shape == "plusid":
        return h + b"\n" + s + b"\n+" + h[1:] + b"\n" + q + b"\n"
    if shape == "blanks":
        return h + pad + b"\n" + s + b"\n+\n" + q + b"\n"
    if shape == "empty":
        return h + b"\n\n+\n\n"
    return h + b"\n" + s + b"\n+\n" + q + b"\n"


def _fasta_raw(h, s, shape, width, pad=b""):
    if shape == "multi" and len(s) > width:
        return h + pad + b"\n" + b"".join(s[j:j + width] + b"\n" for j in range(0, len(s), width))
    return h + pad + b"\n" + s + b"\n"


def _pad(rng, n):
    """n blanks and tabs (a header's trailing white space)"""
    return bytes(rng.choice(np.frombuffer(b" \t", dtype=np.uint8), size=n).tobytes())


def make_corpus(rng, toy_genomes, spec):
    """-> (texts, records): per mate the file's bytes and the list of its Rec.  Deterministic for a given rng.

    spec: paired (bool); fasta1 (bool: mate 1 is FASTA, its shapes one-line / multi-line); batch_frags; last_n (records of
    the last batch, default batch_frags); batches: per batch the kinds of its blocks of 1024 records (the last block of a
    batch holds what is left of it).  A kind is a dict:
      form   "fast": every record in output form; "shapes": records of the shapes the reader normalises among them;
             "norm": in output form but for its first record, whose header has trailing blanks
      delta  with "shapes" / "norm": (raw length - output length) of the block's records, mod 4 -- the shift of the FAST
             copies behind it in the same batch moves by this much (None: as it comes)
      human  None: human and other reads mixed; 1: every fragment has a long human read; 0: none has one
    p_short (default 0.2): share of reads of 0..5 bases.  nofinal: the last record of the last file ends without a newline.
    """
    paired, fasta1 = bool(spec.get("paired")), bool(spec.get("fasta1"))
    mates = 2 if paired else 1
    bf = int(spec["batch_frags"])
    p_short = spec.get("p_short", 0.2)
    hmax = spec.get("header_max", 60)
    lens = spec.get("read_len")  # (lo, hi): every read's length drawn from it instead of the three ranges
    allg = b"".join(toy_genomes[k] for k in sorted(toy_genomes))
    records = [[] for _ in range(mates)]
    nb = len(spec["batches"])
    for bi, kinds in enumerate(spec["batches"]):
        n = bf if bi < nb - 1 else int(spec.get("last_n", bf))
        assert len(kinds) == (n + BLOCK - 1) // BLOCK, (bi, n, len(kinds))
        for ki, kind in enumerate(kinds):
            cnt = min(BLOCK, n - ki * BLOCK)
            form, human = kind["form"], kind.get("human")
            block = [[] for _ in range(mates)]
            for i in range(cnt):
                frag_human = rng.random() < 0.5 if human is None else bool(human)
                which = int(rng.integers(0, mates))  # the mate that carries the human read (the other one: any read)
                shape_i = int(rng.integers(0, 8))
                for m in range(mates):
                    fastq = not (fasta1 and m == 0)
                    if lens:
                        ln = int(rng.integers(lens[0], lens[1] + 1))
                    elif human is not None and m == which:
                        ln = int(rng.integers(200, 301))  # long enough to be called (1) on its own
                    else:
                        ln = _read_len(rng, p_short)
                    hum = frag_human and (m == which or rng.random() < 0.5)
                    s = _sequence(rng, allg, ln, hum)
                    h = _header(rng, b"@" if fastq else b">", int(rng.integers(2, hmax + 1)))
                    q = QCHARS[rng.integers(0, QCHARS.size, size=ln)].tobytes()
                    shape = "plain"
                    if form == "shapes" and shape_i < 5:
                        shape = FASTQ_SHAPES[shape_i] if fastq else "multi"
                    if form == "norm" and i == 0:
                        shape = "blanks"
                    pad = _pad(rng, int(rng.integers(1, 9))) if shape == "blanks" else b""
                    if fastq:
                        raw = _fastq_raw(h, s, q, shape, pad)
                    else:
                        raw = _fasta_raw(h, s, shape, int(rng.integers(7, 61)), pad)
                    block[m].append(parse_record(raw, fastq, shape))
            for m in range(mates):
                want = kind.get("delta")
                if form != "fast" and want is not None:  # one more blank record (or longer blanks) brings the delta there
                    fix = next(i for i, r in enumerate(block[m]) if r.kind in ("blanks", "plain", "one"))
                    r = block[m][fix]
                    have = sum(len(x.raw) - x.out_len for x in block[m]) - (len(r.raw) - r.out_len)
                    k = (want - have) % 4 or 4
                    raw = r.raw[:r.hlen] + _pad(rng, k) + r.raw[_lines(r.raw)[0][1]:]
                    block[m][fix] = parse_record(raw, r.fastq, "blanks")
                    assert sum(len(x.raw) - x.out_len for x in block[m]) % 4 == want % 4
                records[m].extend(block[m])
    if spec.get("nofinal"):
        r = records[-1][-1]
        assert r.raw.endswith(b"\n") and not r.raw.endswith(b"\r\n") and r.fastq
        records[-1][-1] = parse_record(r.raw[:-1], r.fastq, "nofinal")
    texts = [b"".join(r.raw for r in recs) for recs in records]
    return texts, records


def fragments(records):
    """the reads of each fragment, as oracle.pack_reads() takes them"""
    if len(records) == 2:
        return [(a.seq, b.seq) for a, b in zip(*records)]
    return [a.seq for a in records[0]]


def _put(r, suffix=b"", mask=False):
    """nh_run.hip put_record()"""
    out = r.header + suffix + b"\n" + (b"N" * r.slen if mask else r.seq)
    if r.fastq:
        out += b"\n+\n" + r.qual
    return out + b"\n"


def expected_outputs(records, calls, ext_ids, mode):
    """per mate the bytes of out1 / out2 of a run.  calls: the oracle's call of every fragment (internal taxon id, 0: not
    classified); ext_ids: internal -> external id.  mode: "normal" (the unclassified records), "keep" (a -H run: the
    classified records, " kraken:taxid|<external id>" behind the header), "human" (the human side of a split run: the same
    bytes as "keep"), "masked" (every record, a classified one's sequence as N)."""
    assert mode in ("normal", "keep", "human", "masked")
    assert all(len(recs) == len(calls) for recs in records)
    out = []
    for recs in records:
        parts = []
        for r, c in zip(recs, calls):
            c = int(c)
            if mode == "masked":
                parts.append(_put(r, mask=c != 0))
            elif mode == "normal":
                if c == 0:
                    parts.append(_put(r))
            elif c != 0:
                parts.append(_put(r, b" kraken:taxid|%d" % int(ext_ids[c])))
        out.append(b"".join(parts))
    return out


def _in_output_form(t, ntext, gap, r, h):
    """nh_mask.hip in_output_form(): text[h, h + out_len) is byte for byte the record's output.  gap: the bytes of the
    batch's text that no file filled (between the mates' texts): what a check reads there is not defined."""
    def at(i):
        assert not (gap[0] <= i < gap[1]), "the model would read bytes between the mates' texts"
        return t[i]
    n = r.out_len
    if h + n > ntext:
        return False
    s, q = h + r.s, h + r.q
    if at(h + r.hlen) != 0x0A or s != h + r.hlen + 1 or at(s + r.slen) != 0x0A:
        return False
    if not r.fastq:
        return True
    return at(s + r.slen + 1) == 0x2B and at(s + r.slen + 2) == 0x0A and q == s + r.slen + 3 and at(q + r.qlen) == 0x0A


def block_plan(records, calls, batch_frags):
    """-> list of dicts, one per batch, mate and block of 1024 records, in that order:
      batch, mate, block, batch_n (fragments of the batch), n (records of the block), fast, h0 (text offset of the block's
      first record), base (output offset of the block), shift ((h0 - base) & 3), ncls (classified records),
      cls: per classified record (output offset of its sequence, its length).
    The batches are the reader's: batch_frags records each, the rest in the last; a batch's text is its records' text from
    offset 0 for mate 1 and from the next multiple of 256 behind (length of mate 1's text + 8) for mate 2.  (Halves of
    unequal record counts, used in parts -- NOHUMAN_BATCH_TEXT on paired input -- start a batch inside a half's text, at
    any shift; the plan does not model them and the corpora here do not produce them.)"""
    mates = len(records)
    nfrag = len(calls)
    plan = []
    for bi, f0 in enumerate(range(0, nfrag, batch_frags)):
        f1 = min(nfrag, f0 + batch_frags)
        len1 = sum(len(r.raw) for r in records[0][f0:f1])
        base2 = (len1 + 8 + 255) & ~255
        len2 = sum(len(r.raw) for r in records[1][f0:f1]) if mates == 2 else 0
        ntext = base2 + len2 if mates == 2 else len1
        t = bytearray(ntext)
        t[0:len1] = b"".join(r.text for r in records[0][f0:f1])
        if mates == 2:
            t[base2:] = b"".join(r.text for r in records[1][f0:f1])
        gap = (len1, base2) if mates == 2 else (ntext, ntext)
        for m in range(mates):
            h, hs = base2 if m else 0, []
            for r in records[m][f0:f1]:
                hs.append(h)
                h += len(r.raw)
            base = 0
            for k, b0 in enumerate(range(f0, f1, BLOCK)):
                b1 = min(f1, b0 + BLOCK)
                recs = records[m][b0:b1]
                fast = True
                for j, r in enumerate(recs):
                    hj = hs[b0 - f0 + j]
                    fast = fast and _in_output_form(t, ntext, gap, r, hj)
                    if fast and j + 1 < len(recs):  # the next record of the block starts where this one ends
                        fast = hs[b0 - f0 + j + 1] == hj + r.out_len
                    if not fast:
                        break
                cls, o = [], base
                for j, r in enumerate(recs):
                    if int(calls[b0 + j]) != 0:
                        cls.append((o + r.hlen + 1, r.slen))
                    o += r.out_len
                h0 = hs[b0 - f0]
                plan.append(dict(batch=bi, mate=m, block=k, batch_n=f1 - f0, n=len(recs), fast=fast, h0=h0, base=base,
                                 shift=(h0 - base) & 3, ncls=len(cls), cls=cls))
                base = o
    return plan


# ---- the corpora of tests/test_gpu_builders.py, and what tests/test_builder_model.py requires of them ---------------------
def F(human=None):
    return dict(form="fast", human=human)


def N(delta):
    return dict(form="norm", delta=delta)


def S(delta=None):
    return dict(form="shapes", delta=delta)


# Batches of 2049 records are blocks of 1024, 1024 and 1: a normalised record in the first block moves every later block
# of the batch by its delta, so the FAST copies behind it run with that shift.
CORPORA = {
    # paired FASTQ: every shift for both mates, FAST beside other blocks, batches of 2049 and 1023
    "pe": dict(seed=101, paired=True, batch_frags=2049, last_n=1023, nofinal=True,
               batches=[[F(), S(1), F()], [N(1), F(), F()], [N(2), F(), F()], [N(3), F(), F()], [S(), S(), F()], [S()]]),
    # single-end FASTQ: batches of 1025 and 1024; a block with every record classified, one with none
    "se": dict(seed=102, paired=False, batch_frags=1025, last_n=1024, nofinal=True,
               batches=[[F(1), F()], [F(0), F()], [N(3), F()], [S(2)]]),
    # mate 1 FASTA (one-line and multi-line records), mate 2 FASTQ
    "fa": dict(seed=103, paired=True, fasta1=True, batch_frags=2049, last_n=500,
               batches=[[N(1), F(), F()], [F(), S(2), F()], [S()]]),
    # plain four-line FASTQ for the gzip readers (the reader on the GPU takes no other shape)
    "gz": dict(seed=104, paired=True, batch_frags=2049, last_n=1025, batches=[[F(), F(), F()], [F(), F(), F()], [F(), F()]]),
}
# the scan's carry: one record with trailing blanks, then a unit of 1000 short pairs CARRY_REPS times: 271001 fragments,
# the first batch 270000 of them = 264 blocks (the scan kernels take 256 a round), every block but the first FAST at shift 1
CARRY_BATCH_FRAGS = 270000
CARRY_REPS = 271
CARRY_HEAD = dict(seed=105, paired=True, batch_frags=1, header_max=10, read_len=(30, 40), batches=[[N(1)]])
CARRY_UNIT = dict(seed=106, paired=True, batch_frags=1000, header_max=10, read_len=(30, 40), batches=[[F()]])
# external ids of 1, 4, 7 and 10 digits for the toy taxonomy's nodes (internal ids 1..9; the last one above 2^32)
DIGIT_IDS = [0, 5, 7, 3, 4321, 1012, 7654321, 9606001, 1234567890, 4294967301]
DIGITS = dict(seed=107, paired=False, batch_frags=1500, batches=[[S(), F()]])

_CACHE = {}


def corpus(spec, toy_genomes):
    """make_corpus(), once per spec and process"""
    key = spec["seed"]
    if key not in _CACHE:
        _CACHE[key] = make_corpus(np.random.default_rng(spec["seed"]), toy_genomes, spec)
    return _CACHE[key]


def oracle_calls(db, records):
    """the CPU oracle's call of every fragment (oracle.OracleDB), confidence 0"""
    from oracle import oracle as orc
    paired = len(records) == 2
    bases, offs = orc.pack_reads(fragments(records), paired)
    out, _ = db.classify(bases, offs, paired, 0.0)
    return out["call"].copy()


def patch_external_ids(taxo, ids):
    """a taxonomy image with other external ids (K2TAXDAT: 32 bytes, then 7 words a node, the sixth its external id)"""
    import struct
    t = bytearray(taxo)
    assert t[:8] == b"K2TAXDAT" and struct.unpack_from("<Q", t, 8)[0] == len(ids)
    for i, e in enumerate(ids):
        struct.pack_into("<Q", t, 32 + 56 * i + 40, e)
    return bytes(t)


def parse_file(text, fastq):
    """a whole input file -> its records (four lines a FASTQ record; a FASTA record runs to the next line starting '>')"""
    ln = _lines(text)
    if fastq:
        assert len(ln) % 4 == 0
        cuts = [ln[i][0] for i in range(0, len(ln), 4)]
    else:
        cuts = [b for b, _e, _nx, _t in ln if text[b:b + 1] == b">"]
    cuts.append(len(text))
    return [parse_record(text[a:b], fastq) for a, b in zip(cuts, cuts[1:])]
