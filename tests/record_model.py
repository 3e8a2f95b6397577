"""A plain Python statement of the record semantics of the readers (kraken2's BatchSequenceReader: getline + StripString,
SURVEY.md A.6), the corpus the record tests share, and the binding of the library's reader dump hook.

  py_records / fnv   the whole-file model tests/test_reader.py holds nh_fastx_scan to
  parse / repeat     FASTQ text -> per record the fields of a RecRef, digests of its bytes, and how the input ended
  host_batches / device_batches / piece_records   how the two readers cut the records into batches
  expected           the table nh_debug_reader_dump must hand back for a text
  dump               nh_debug_reader_dump through ctypes (test support: not part of include/nohuman_engine.h)
  make_record, SHAPES, ENDS, with_end, shapes_of, fuzz_case   the corpus

The model never looks at what a reader returned: what it says comes from the text alone."""
import collections
import ctypes as C
import os

import numpy as np

WS = b" \t\n\v\f\r"  # C isspace()
FNV0, FNVP = 0xcbf29ce484222325, 0x100000001b3
M64 = 0xFFFFFFFFFFFFFFFF


def fnv(parts):
    h = FNV0
    for p in parts:
        for b in p:
            h = ((h ^ b) * FNVP) & M64
        h = ((h ^ 0) * FNVP) & M64
    return h


def py_records(data: bytes):
    """kraken2 BatchSequenceReader semantics, line by line (getline + StripString)."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # a final newline does not start another line
    i, recs, fmt = 0, [], None
    while i < len(lines):
        h = lines[i].rstrip()
        i += 1
        if fmt is None:
            fmt = "fq" if h[:1] == b"@" else "fa" if h[:1] == b">" else None
            if fmt is None:
                raise ValueError("unrecognized file format")
        if fmt == "fq":
            if not h:
                break
            if h[:1] != b"@":
                raise ValueError("malformed FASTQ")
            if len(h) <= 1 or i + 2 >= len(lines):  # sequence, '+' and quality lines must exist
                break
            seq, qual = lines[i].rstrip(), lines[i + 2].rstrip()
            i += 3
            recs.append((h, seq, qual))
        else:
            if h[:1] != b">":
                raise ValueError("malformed FASTA")
            if len(h) <= 1:
                break
            seq = b""
            while i < len(lines) and lines[i][:1] != b">":
                seq += lines[i].rstrip()
                i += 1
            recs.append((h, seq, b""))
    return recs


# ---- the record table -------------------------------------------------------------------------------------------------------
END_OF_TEXT, BLANK, LONE_AT, TRUNCATED, MALFORMED, UNRECOGNISED = "end of text", "blank header line", "lone @", "truncated record", "malformed", "unrecognised format"
END_KINDS = (END_OF_TEXT, BLANK, LONE_AT, TRUNCATED, MALFORMED, UNRECOGNISED)
FIELDS = ("hlen", "idlen", "slen", "qlen", "canonical", "raw_len", "batch", "digest", "raw_digest")
UNRECOGNISED_TEXT = "sequence reader - unrecognized file format"

# recs: int64 array, a row a record: start, end (the next record's start), header end, id length, sequence start, sequence end,
# quality start, quality end, canonical.  lines: (n, 3) start, end without the newline, terminated.  stop: index of the line
# the parser stopped at (len(lines): the end of the text).
Parsed = collections.namedtuple("Parsed", "text recs end message lines stop")
R_START, R_END, R_HE, R_IDLEN, R_S, R_SE, R_Q, R_QE, R_CANON = range(9)


def line_table(text):
    """std::getline over the text: per line its start, its end without the newline, and whether a newline ended it"""
    buf = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(buf == 10).astype(np.int64)
    starts = np.concatenate(([0], nl + 1))
    ends = np.concatenate((nl, [len(text)]))
    term = np.ones(len(starts), np.int64)
    term[-1] = 0
    if starts[-1] == len(text):  # nothing behind the last newline (or no text at all): no line
        starts, ends, term = starts[:-1], ends[:-1], term[:-1]
    return np.stack([starts, ends, term], axis=1)


def _rstrip(text, b, e):
    while e > b and text[e - 1] in WS:
        e -= 1
    return e


def parse(text):
    """the host parser (nh_fastx.cpp parse_one), FASTQ only, record by record"""
    lines = line_table(text)
    n = len(lines)
    lt = lines.tolist()
    recs, i, end, message = [], 0, END_OF_TEXT, ""
    while i < n:
        b0, e0, t0 = lt[i]
        he = _rstrip(text, b0, e0)
        if i == 0 and (he == b0 or text[b0] != 0x40):
            assert text[b0:b0 + 1] != b">", "the model is of FASTQ"
            end, message = UNRECOGNISED, UNRECOGNISED_TEXT
            break
        if he == b0:
            end = BLANK
            break
        if text[b0] != 0x40:
            end, message = MALFORMED, "malformed FASTQ file (exp. '@', saw \"%s\"), aborting" % text[b0:he].decode("latin-1")
            break
        if he - b0 <= 1:
            end = LONE_AT
            break
        if i + 3 >= n:  # the text ends inside the record: dropped
            end = TRUNCATED
            break
        ie = b0 + 1
        while ie < he and text[ie] not in b" \t\r":
            ie += 1
        (b1, e1, t1), (b2, e2, t2), (b3, e3, t3) = lt[i + 1], lt[i + 2], lt[i + 3]
        se, qe = _rstrip(text, b1, e1), _rstrip(text, b3, e3)
        canon = t0 and t1 and t2 and t3 and he == e0 and se == e1 and qe == e3 and e2 - b2 == 1 and text[b2] == 0x2B
        recs.append((b0, e3 + t3, he, ie - b0 - 1, b1, se, b3, qe, int(bool(canon))))
        i += 4
    return Parsed(text, np.array(recs, np.int64).reshape(len(recs), 9), end, message, lines, i)


def repeat(parsed, times):
    """parse(text * times) for a text of whole records that ends with a newline: the same records, moved"""
    assert parsed.end == END_OF_TEXT and parsed.text.endswith(b"\n") and parsed.stop == len(parsed.lines) == 4 * len(parsed.recs)
    n = len(parsed.text)
    shift = np.zeros(9, np.int64)
    shift[[R_START, R_END, R_HE, R_S, R_SE, R_Q, R_QE]] = n
    recs = np.concatenate([parsed.recs + k * shift for k in range(times)])
    lines = np.concatenate([parsed.lines + k * np.array([n, n, 0]) for k in range(times)])
    return Parsed(parsed.text * times, recs, END_OF_TEXT, "", lines, len(lines))


def device_text(text):
    """the reader on the GPU appends the newline a text's last line lacks"""
    return text if not text or text.endswith(b"\n") else text + b"\n"


def _mix(h, buf, starts, lens):
    """FNV-1a of buf[starts[i] : starts[i] + lens[i]] into h[i], and the separator step -- all records at once"""
    for i in range(int(lens.max()) if len(lens) else 0):
        idx = np.flatnonzero(lens > i)
        h[idx] = (h[idx] ^ buf[starts[idx] + i].astype(np.uint64)) * np.uint64(FNVP)
    h *= np.uint64(FNVP)
    return h


def digests(parsed):
    """per record: the digest of header, sequence and qualities (mixed like nh_fastx_scan, every record from the start value)
    and, for a canonical record, the digest of its raw bytes (else 0)"""
    r = parsed.recs
    buf = np.frombuffer(parsed.text, np.uint8)
    h = np.full(len(r), FNV0, np.uint64)
    _mix(h, buf, r[:, R_START], r[:, R_HE] - r[:, R_START])
    _mix(h, buf, r[:, R_S], r[:, R_SE] - r[:, R_S])
    _mix(h, buf, r[:, R_Q], r[:, R_QE] - r[:, R_Q])
    raw = np.full(len(r), FNV0, np.uint64)
    _mix(raw, buf, r[:, R_START], np.where(r[:, R_CANON] == 1, r[:, R_END] - r[:, R_START], 0))
    raw[r[:, R_CANON] == 0] = 0
    return h, raw


# ---- batches ----------------------------------------------------------------------------------------------------------------
def _cut(sizes, batch_recs, max_text):
    """records of the given sizes from a batch's first on: up to batch_recs, cut behind the record that reaches max_text"""
    out, n, pos = [], 0, 0
    for s in sizes:
        n, pos = n + 1, pos + s
        if n == batch_recs or (max_text and pos >= max_text):
            out.append((n, pos))
            n, pos = 0, 0
    if n:
        out.append((n, pos))
    return out


def host_batches(parsed, batch_recs, max_text):
    """BlockReader::next_batch: the next batch begins where the one before ended"""
    sizes = (parsed.recs[:, R_END] - parsed.recs[:, R_START]).tolist()
    return _cut(sizes, batch_recs, max_text)


def piece_records(parsed, piece_starts, max_text):
    """how many records each piece of the reader on the GPU hands out.  Single-end (max_text != 0): every record that is
    complete in the text the piece holds; paired (max_text == 0): the pieces do not show, batches are whole."""
    ends = parsed.recs[:, R_END]
    if not max_text or len(piece_starts) <= 1:
        return [len(ends)]
    out, done = [], 0
    for nxt in list(piece_starts[1:]):
        k = int(np.searchsorted(ends, nxt, side="right"))  # records that end at or before the next piece's body
        out.append(k - done)
        done = k
    out.append(len(ends) - done)
    return out


def device_batches(parsed, batch_recs, max_text, piece_starts=()):
    """DevFastqReader: a piece's records in groups of batch_recs from its first; a group that exceeds max_text goes out in
    parts, each cut behind the record that reaches the budget"""
    sizes = (parsed.recs[:, R_END] - parsed.recs[:, R_START]).tolist()
    out, r = [], 0
    for n in piece_records(parsed, piece_starts, max_text):
        for g in range(r, r + n, batch_recs):
            out.extend(_cut(sizes[g:min(r + n, g + batch_recs)], batch_recs, max_text))
        r += n
    return out


def expected(parsed, batches):
    """the record table of nh_debug_reader_dump: a row of FIELDS a record"""
    r = parsed.recs
    out = np.zeros((len(r), len(FIELDS)), np.uint64)
    out[:, 0] = r[:, R_HE] - r[:, R_START]
    out[:, 1] = r[:, R_IDLEN]
    out[:, 2] = r[:, R_SE] - r[:, R_S]
    out[:, 3] = r[:, R_QE] - r[:, R_Q]
    out[:, 4] = r[:, R_CANON]
    out[:, 5] = np.where(r[:, R_CANON] == 1, r[:, R_END] - r[:, R_START], 0)
    assert sum(n for n, _ in batches) == len(r)
    out[:, 6] = np.repeat(np.arange(len(batches)), [n for n, _ in batches])
    out[:, 7], out[:, 8] = digests(parsed)
    return out


# ---- the hook ---------------------------------------------------------------------------------------------------------------
Dump = collections.namedtuple("Dump", "recs batches end message pieces")
EOF, HANDOVER, ERROR = 0, 1, 2


def dump(path, reader, batch_recs, max_text, device=0, rec_cap=1 << 16):
    """nh_debug_reader_dump: reader 0 the host's BlockReader, 1 the reader on the GPU"""
    from nohuman_amd import _lib
    L = _lib.lib()
    fn = L.nh_debug_reader_dump
    U = C.POINTER(C.c_uint64)
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, U, C.c_uint64, U, U, C.c_uint64, U, U, C.c_uint64, U,
                   C.POINTER(C.c_int), C.c_char_p, C.c_uint64]
    recs = np.zeros((rec_cap, len(FIELDS)), np.uint64)
    batches = np.zeros((rec_cap, 2), np.uint64)
    pieces = np.zeros(4096, np.uint64)
    nr, nb, npc, end = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    msg = C.create_string_buffer(1 << 16)
    rc = fn(os.fsencode(str(path)), reader, device, batch_recs, max_text, recs.ctypes.data_as(U), rec_cap, C.byref(nr),
            batches.ctypes.data_as(U), rec_cap, C.byref(nb), pieces.ctypes.data_as(U), len(pieces), C.byref(npc), C.byref(end), msg,
            len(msg))
    if rc != 0:
        raise RuntimeError(L.nh_last_error().decode("latin-1"))
    return Dump(recs[:nr.value].copy(), [(int(a), int(b)) for a, b in batches[:nb.value]], end.value, msg.value.decode("latin-1"),
                [int(x) for x in pieces[:npc.value]])


def mismatch(got, want):
    """None, or a sentence that names the first record and field that differ"""
    if got.shape != want.shape:
        return "%d records, the model has %d" % (len(got), len(want))
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    r, f = (int(x) for x in bad[0])
    return "record %d, %s: %d, the model says %d (%d cells differ)" % (r, FIELDS[f], int(got[r, f]), int(want[r, f]), len(bad))


# ---- the corpus -------------------------------------------------------------------------------------------------------------
SHAPES = ("plain", "crlf", "plusid", "plusblank", "desc_ws", "id_tab", "id_space", "id_cr", "empty", "qual_at", "qual_plus", "seq_at",
          "id1")
_ID = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", np.uint8)
_Q = np.frombuffer(b"#$%&'()*,-./0123456789:;<=>?ABCDEFGHIJ", np.uint8)  # (neither '@' nor '+')
_B = np.frombuffer(b"ACGT", np.uint8)


def _word(rng, n):
    return _ID[rng.integers(0, _ID.size, n)].tobytes()


def make_record(rng, shape, hlen=None, slen=None):
    """one four-line record of the shape; hlen: bytes of the header line without what the shape puts behind it"""
    hlen = int(rng.integers(4, 40)) if hlen is None else hlen
    slen = int(rng.integers(1, 120)) if slen is None else slen
    assert hlen >= 2
    h = b"@" + _word(rng, hlen - 1)
    s = _B[rng.integers(0, 4, slen)].tobytes()
    q = _Q[rng.integers(0, _Q.size, slen)].tobytes()
    plus, eol = b"+", [b"\n"] * 4
    if shape == "crlf":
        eol = [b"\r\n"] * 4
    elif shape == "plusid":
        plus = b"+" + h[1:]
    elif shape == "plusblank":
        plus = b"+ "
    elif shape == "desc_ws":
        h = h[:max(2, hlen // 2)] + b" " + _word(rng, 3) + b" x"
        eol = [b"\t\n", b"\v\n", b"\f\n", b" \t\v\f\n"]
    elif shape in ("id_tab", "id_space", "id_cr"):
        h = h + {"id_tab": b"\t", "id_space": b" ", "id_cr": b"\r"}[shape] + _word(rng, 5)
    elif shape == "empty":
        s = q = b""
    elif shape == "qual_at":
        q = b"@" + q[1:] if q else b"@"
        s = s or b"A"
    elif shape == "qual_plus":
        q = b"+" + q[1:] if q else b"+"
        s = s or b"A"
    elif shape == "seq_at":
        s = b"@" + s[1:] if s else b"@"
        q = q or b"I"
    elif shape == "id1":
        h = h[:2]
    else:
        assert shape == "plain", shape
    return h + eol[0] + s + eol[1] + plus + eol[2] + q + eol[3]


def shapes_of(parsed):
    """which of SHAPES (and "blank_header": '@' and blanks only, at the line the parser stopped at) the text's records show --
    from the model's table alone"""
    t, seen = parsed.text, collections.Counter()
    lt = parsed.lines.tolist()
    for k, r in enumerate(parsed.recs.tolist()):
        ls = lt[4 * k:4 * k + 4]  # (records are four lines each from the text's first line on)
        assert ls[0][0] == r[R_START]
        raw = [t[b:e] for b, e, _ in ls]
        tags = set()
        if all(x.endswith(b"\r") for x in raw):
            tags.add("crlf")
        if len(raw[2].rstrip()) > 1:
            tags.add("plusid")
        if raw[2][:1] == b"+" and raw[2][1:2] in (b" ", b"\t") and not raw[2][1:].strip(WS):
            tags.add("plusblank")
        if all(x[-1:] in (b"\t", b"\v", b"\f") for x in raw):
            tags.add("desc_ws")
        after = t[r[R_START] + 1 + r[R_IDLEN]:r[R_HE]][:1]
        if after in (b"\t", b" ", b"\r"):
            tags.add({b"\t": "id_tab", b" ": "id_space", b"\r": "id_cr"}[after])
        if r[R_SE] == r[R_S] and r[R_QE] == r[R_Q]:
            tags.add("empty")
        if t[r[R_Q]:r[R_QE]][:1] == b"@":
            tags.add("qual_at")
        if t[r[R_Q]:r[R_QE]][:1] == b"+":
            tags.add("qual_plus")
        if t[r[R_S]:r[R_SE]][:1] == b"@":
            tags.add("seq_at")
        if r[R_IDLEN] == 1:
            tags.add("id1")
        if r[R_CANON]:
            tags.add("plain")
        seen.update(tags)
    if parsed.end == LONE_AT and lt[parsed.stop][1] - lt[parsed.stop][0] > 1:
        seen["blank_header"] += 1
    return seen


# how a text can end: name -> (what stands behind the good records, the model's end kind)
_REC = b"@tail.1 d\nACGTACGT\n+\nIIIIIIII\n"
_BAD = b"Xtail\nACGT\n+\nIIII\n"  # a full record without '@'
ENDS = {
    "newline": (b"", END_OF_TEXT),
    "no_final_newline": (_REC[:-1], END_OF_TEXT),
    "blank": (b"\n" + _REC, BLANK),
    "blank_ws": (b" \t\r\n" + _REC, BLANK),
    "blank_last": (b"\n", BLANK),
    "at": (b"@\n" + _REC[_REC.index(b"\n") + 1:] + _REC, LONE_AT),
    "at_blanks": (b"@ \t\n" + _REC[_REC.index(b"\n") + 1:] + _REC, LONE_AT),
    "at_last": (b"@", LONE_AT),
    "cut1": (b"@tail.2 d\n", TRUNCATED),
    "cut1_open": (b"@tail.2 d", TRUNCATED),
    "cut2": (b"@tail.2\nACGT\n", TRUNCATED),
    "cut3": (b"@tail.2\nACGT\n+\n", TRUNCATED),
    "cut3_open": (b"@tail.2\nACGT\n+", TRUNCATED),
    "bad1": (b"X\n", MALFORMED),
    "bad1_ws": (b"X \r\n", MALFORMED),
    "bad1_seq": (b"ACGT", MALFORMED),
    "bad2": (b"X\nACGT\n", MALFORMED),
    "bad2_seq": (b"ACGT\nIIII\n", MALFORMED),
    "bad3": (b"X \r\nACGT\n+\n", MALFORMED),
    "bad3_seq": (b"ACGT\n+\nIIII", MALFORMED),
    "bad_full": (_BAD + _REC, MALFORMED),
    "bad_long": (b"A" * 250 + b"\nACGT\n+\nIIII\n" + _REC, MALFORMED),  # (the message quotes the whole line)
    "bad_then_blank": (_BAD + b"\n" + _REC, MALFORMED),
    "blank_then_bad": (b"\n" + _BAD + _REC, BLANK),
    "at_then_bad": (b"@\n" + _BAD, LONE_AT),
    "blank_then_cut_bad": (b"\nX\nACGT\n", BLANK),
}
GARBAGE = b"\x01\x02 no fastq at all \xff\n\n@\n+\n" * 40


def with_end(body, name, garbage=False):
    """the good records, the end, and (behind an end that stops the parser for good) text no reader may look at"""
    tail, kind = ENDS[name]
    if garbage:
        assert kind in (BLANK, LONE_AT) and tail.endswith(b"\n")
        tail += GARBAGE
    return body + tail


FUZZ_SEEDS = range(32)


def fuzz_case(seed):
    """-> (text, knobs): 50 to 400 records of shapes drawn from SHAPES, an end drawn from ENDS, and the readers' knobs"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(50, 401))
    names = sorted(ENDS)
    extra = ("at_blanks", "newline", "no_final_newline", "cut3", "blank_ws", "bad3_seq")
    end = names[seed] if seed < len(names) else extra[(seed - len(names)) % len(extra)]
    body = b"".join(make_record(rng, SHAPES[int(rng.integers(0, len(SHAPES)))]) for _ in range(n))
    if seed % 16 == 5:  # nothing a parser recognises in front
        body = b""
        end = ("bad1", "blank")[seed // 16]
    knobs = dict(batch_recs=int(rng.choice([1, 3, 7, 64, 256, 1000])), max_text=int(rng.choice([0, 0, 300, 2000, 50000])),
                 seg=int(rng.choice([16384, 65536])), stretch=int(rng.choice([2048, 4096])), chunk=int(rng.choice([1, 7, 4096])),
                 level=int(rng.choice([1, 6])))
    return with_end(body, end, garbage=bool(rng.integers(0, 2)) and ENDS[end][1] in (BLANK, LONE_AT) and ENDS[end][0].endswith(b"\n")), knobs


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def _full(batch, batch_recs, max_text):
    return batch[0] == batch_recs or bool(max_text and batch[1] >= max_text)


def verdict(got, parsed, batches, batch_recs, max_text, on_device=False):
    """None, or what of a reader's dump differs from the model.  parsed / batches: the model's, for the reader in question.
    Input that ends in an error: the records in front of it go out in whole batches only, as far as the reader got (the host
    reader: every whole batch; the reader on the GPU: those of the pieces before) -- what did go out is held to the model."""
    want = expected(parsed, batches)
    if parsed.end == UNRECOGNISED:  # (the reader on the GPU hands the file to the host parser, which says so)
        end = (HANDOVER, "") if on_device else (ERROR, UNRECOGNISED_TEXT)
    elif parsed.end == MALFORMED:
        end = (ERROR, parsed.message)
        if not on_device:
            while batches and not _full(batches[-1], batch_recs, max_text):
                batches = batches[:-1]
        else:
            batches = batches[:len(got.batches)]
        want = want[:sum(n for n, _ in batches)]
    else:
        end = (EOF, "")
    if (got.end, got.message) != end:
        return "the input ended with %r, the model says %r (%s)" % ((got.end, got.message), end, parsed.end)
    if got.batches != batches:
        k = next((i for i, (a, b) in enumerate(zip(got.batches, batches)) if a != b), min(len(got.batches), len(batches)))
        return "batch %d of %d: (records, text) %r, the model says %r of %d" % (
            k, len(got.batches), got.batches[k] if k < len(got.batches) else None, batches[k] if k < len(batches) else None, len(batches))
    return mismatch(got.recs, want)
