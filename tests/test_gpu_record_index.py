"""The record index of the gzip reader on the GPU (DevFastqImpl in nh_gunzip.hip: k_nl_count, k_nl_scan, k_nl_list, k_records,
and the host side that stitches pieces and cuts batches) against the record model of tests/record_model.py, record by record,
through nh_debug_reader_dump: the reader alone, no engine.  tests/test_record_model.py holds the host reader to the same
model.  Newlines at the edges the kernels have (tile, vector tail, a thread's span, more than 1024 tiles, a workgroup of
records), every record shape, every way a text can end, and piece boundaries at every phase of a record."""
import collections
import gzip
import zlib

import numpy as np
import pytest

from tests import record_model as rm

pytestmark = pytest.mark.gpu

TILE = 16384  # bytes of text a workgroup of the newline kernels takes
SPAN = 64     # bytes a thread of k_nl_list takes


def _env(monkeypatch, room=1 << 20, seg=65536, stretch=4096):
    # (tests/test_gpu_reader_default.py _small_scale: the product's sizes scaled down)
    monkeypatch.setenv("NOHUMAN_GZDEV_MIN_BYTES", "0")
    monkeypatch.setenv("NOHUMAN_GZDEV_ROOM", str(room))
    monkeypatch.setenv("NOHUMAN_GZDEV_SEG", str(seg))
    monkeypatch.setenv("NOHUMAN_GZDEV_STRETCH", str(stretch))


def _device(tmp_path, text, batch_recs, max_text, level=6, rec_cap=1 << 16):
    """-> (the dump of the reader on the GPU, the model's parse of the text, None or what differs from the model)"""
    p = tmp_path / "x.fq.gz"
    p.write_bytes(gzip.compress(text, level))
    got = rm.dump(p, 1, batch_recs, max_text, rec_cap=rec_cap)
    parsed = rm.parse(rm.device_text(text))
    batches = rm.device_batches(parsed, batch_recs, max_text, got.pieces)
    return got, parsed, rm.verdict(got, parsed, batches, batch_recs, max_text, on_device=True)


def _report(bad):
    assert not bad, "%d cases differ from the model:\n%s" % (len(bad), "\n".join(bad))


# ---- newline placement ------------------------------------------------------------------------------------------------------
def _filler(i, eol):
    return b"@r%05d" % i + eol + b"ACGTACGT" + eol + b"+" + eol + b"IIIIHHHH" + eol


def _steered(pos, which, crlf, total=None):
    """records whose line `which` (0 header .. 3 qualities) of one record ends with its newline at byte `pos`; with `total`
    the text is exactly that long (a last record's header is padded)"""
    eol = b"\r\n" if crlf else b"\n"
    unit = len(_filler(0, eol))
    out, cur, i = [], 0, 0
    while cur + 2 * unit + 8 <= pos:
        out.append(_filler(i, eol))
        cur, i = cur + unit, i + 1
    lines = [b"@s%05d" % i, b"ACGTACGT", b"+", b"IIIIHHHH"]
    at = cur + sum(len(x) + len(eol) for x in lines[:which + 1]) - 1  # where the newline stands without padding
    assert pos >= at, (pos, at)
    lines[0] += b"." * (pos - at)
    rec = eol.join(lines) + eol
    out.append(rec)
    cur, i = cur + len(rec), i + 1
    if total is None:
        out.extend(_filler(i + k, eol) for k in range(3))
    else:
        while cur + 2 * unit <= total:
            out.append(_filler(i, eol))
            cur, i = cur + unit, i + 1
        if cur < total:
            assert total - cur >= unit, (total, cur)
            last = _filler(i, eol)
            out.append(last[:7] + b"." * (total - cur - unit) + last[7:])
    text = b"".join(out)
    assert text[pos:pos + 1] == b"\n" and (not crlf or text[pos - 1:pos] == b"\r") and (total is None or len(text) == total)
    return text


def _near_end(total, d, crlf):
    """a text of `total` bytes whose last record's header line ends with its newline `d` bytes from the end"""
    eol = b"\r\n" if crlf else b"\n"
    room = d - 1 - 1 - 3 * len(eol)  # sequence and qualities share what the plus line and the line ends leave
    assert room >= 2
    tail = b"ACGTACGT"[:room // 2] + eol + b"+" + eol + b"IIIIHHHH"[:room - room // 2] + eol
    unit = len(_filler(0, eol))
    out, cur, i = [], 0, 0
    while cur + 2 * unit + d <= total:
        out.append(_filler(i, eol))
        cur, i = cur + unit, i + 1
    head = b"@e%05d" % i
    pad = total - d + 1 - len(eol) - cur - len(head)
    assert pad >= 0
    text = b"".join(out) + head + b"." * pad + eol + tail
    assert len(text) == total and text[total - d:total - d + 1] == b"\n" and len(tail) == d - 1
    return text


def test_newlines_at_the_edges_of_tiles_spans_and_the_vector_tail(tmp_path, monkeypatch):
    _env(monkeypatch)
    cases = {}
    for crlf in (False, True):
        tag = "crlf" if crlf else "lf"
        for k, pos in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE)):
            cases["%s tile edge %d" % (tag, pos)] = _steered(pos, k % 4, crlf)
        for k, pos in enumerate((100 * SPAN + 63, 101 * SPAN, 101 * SPAN + 1, TILE + 3 * SPAN + 63, TILE + 4 * SPAN, TILE + 4 * SPAN + 1)):
            cases["%s span edge %d" % (tag, pos)] = _steered(pos, (k + 1) % 4, crlf)
        for total in (TILE, TILE + 1, TILE + 15):
            for d in (15, 16, 17):
                cases["%s %d bytes, newline %d from the end" % (tag, total, d)] = _near_end(total, d, crlf)
        cases["%s one tile" % tag] = _steered(5000, 1, crlf, total=TILE)
        cases["%s one tile and a byte" % tag] = _steered(5000, 2, crlf, total=TILE + 1)
        cases["%s one tile, no final newline" % tag] = _steered(5000, 2, crlf, total=TILE + 1)[:-1]
    long = b"@long.1 d\n" + b"ACGT" * 10000 + b"\n+\nIIIII\n" + b"@long.2\nACGTA\n+long.2\n" + b"5" * 40000 + b"\n"
    cases["lines of 40000 bytes"] = _filler(0, b"\n") * 3 + long + _filler(1, b"\n") * 3
    bad = []
    for name, text in cases.items():
        got, parsed, why = _device(tmp_path, text, 64, 0)
        if len(got.pieces) != 1:
            why = "%d pieces: the case is about one piece's tiles" % len(got.pieces)
        if why or parsed.end != rm.END_OF_TEXT:
            bad.append("%s: %s" % (name, why or parsed.end))
    _report(bad)


def test_more_tiles_than_the_scan_has_threads(tmp_path, monkeypatch):
    """some 1100 tiles of short records in one piece: k_nl_scan sums two tiles a thread"""
    _env(monkeypatch, room=64 << 20, seg=64 << 20)
    rng = np.random.default_rng(11)
    block = b"".join(rm.make_record(rng, rm.SHAPES[k % len(rm.SHAPES)], hlen=int(rng.integers(4, 12)), slen=int(rng.integers(0, 24))) for k in range(512))
    text = block * (1100 * TILE // len(block) + 1)
    assert 1024 * TILE < len(text) < 19_000_000
    n = text.count(b"\n") // 4
    p = tmp_path / "x.fq.gz"
    p.write_bytes(gzip.compress(text, 1))
    got = rm.dump(p, 1, 4096, 0, rec_cap=n + 16)
    parsed = rm.repeat(rm.parse(block), len(text) // len(block))
    assert len(got.pieces) == 1 and len(parsed.recs) == n and parsed.text == text
    why = rm.verdict(got, parsed, rm.device_batches(parsed, 4096, 0), 4096, 0, on_device=True)
    assert why is None, why


# ---- record counts and the batch cut ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_text", [0, 700])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_record_counts_around_a_workgroup_and_the_batch_cut(tmp_path, monkeypatch, n, max_text):
    """max_text 0: whole batches, the rest carried (paired inputs); 700: batches go out in parts, cut behind the record that
    reaches the budget (single-end)"""
    _env(monkeypatch)
    rng = np.random.default_rng(n)
    text = b"".join(rm.make_record(rng, "plain", hlen=int(rng.integers(4, 30)), slen=int(rng.integers(1, 60))) for _ in range(n))
    bad = []
    for batch_recs in (1, 7, 256, 300, 4096):
        got, parsed, why = _device(tmp_path, text, batch_recs, max_text)
        if why is None and max_text and n > 7 and batch_recs > 7 and all(k == batch_recs for k, _ in got.batches[:-1]):
            why = "no batch was cut by text: the case is about the cut"
        if why or len(parsed.recs) != n:
            bad.append("%d records in batches of %d: %s" % (n, batch_recs, why))
    _report(bad)


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_text", [0, 400])
def test_every_record_shape(tmp_path, monkeypatch, max_text):
    _env(monkeypatch)
    rng = np.random.default_rng(21)
    cases = {s: b"".join(rm.make_record(rng, s) for _ in range(20)) for s in rm.SHAPES}
    cases["mixed"] = b"".join(rm.make_record(rng, rm.SHAPES[int(rng.integers(0, len(rm.SHAPES)))]) for _ in range(300))
    cases["blank_header"] = cases["plain"] + b"@ \t \nACGT\n+\nIIII\n" + cases["crlf"]
    seen, bad = collections.Counter(), []
    for name, text in cases.items():
        got, parsed, why = _device(tmp_path, text, 7, max_text)
        seen.update(rm.shapes_of(parsed).keys())
        if why or rm.shapes_of(parsed)[name] < (1 if name == "blank_header" else 20) and name != "mixed":
            bad.append("%s: %s" % (name, why or "the text does not show the shape"))
    assert set(seen) >= set(rm.SHAPES) | {"blank_header"}, seen
    _report(bad)


# ---- ends of the input ------------------------------------------------------------------------------------------------------
def _random_records(rng, n_bytes, shapes=("plain",), lo=40, hi=300):
    """records of lo..hi bytes with random bases and qualities (text that compresses poorly)"""
    out, size = [], 0
    while size < n_bytes:
        want = int(rng.integers(lo, hi + 1))
        hlen = int(rng.integers(4, 20))
        slen = max(1, (want - hlen - 8) // 2)
        out.append(rm.make_record(rng, shapes[int(rng.integers(0, len(shapes)))], hlen=hlen, slen=slen))
        size += len(out[-1])
    return out


@pytest.mark.parametrize("where", ["first batch", "later batch", "later piece", "non-last piece"])
def test_every_way_a_text_can_end(tmp_path, monkeypatch, where):
    """each end of tests/record_model.py ENDS: the error's text with the quoted line, or the records in front of it and not one
    more.  "non-last piece": the ends that stop a parser for good (blank line, lone '@'), with valid records and with garbage
    behind them that fill further pieces."""
    rng = np.random.default_rng(31)
    if where in ("first batch", "later batch"):
        _env(monkeypatch)
        body = b"".join(rm.make_record(rng, "plain", slen=20) for _ in range(5 if where == "first batch" else 40))
        modes = [(256, 0), (256, 300)] if where == "first batch" else [(7, 0), (7, 300)]
    else:
        _env(monkeypatch, seg=16384, stretch=2048)
        body = b"".join(_random_records(rng, 90_000))
        modes = [(64, 0), (64, 5000)]
    # (90 KB that compress to some 40: what stands behind an end fills two more pieces of 16 KiB of gzip and more)
    behind = b"".join(_random_records(rng, 90_000))
    noise = rng.integers(1, 256, 90_000, dtype=np.uint8).tobytes()
    bad = []
    for name, (_tail, kind) in rm.ENDS.items():
        texts = {"": rm.with_end(body, name)}
        if where == "non-last piece":
            if kind not in (rm.BLANK, rm.LONE_AT) or not _tail.endswith(b"\n"):
                continue
            texts = {" + records": texts[""] + behind, " + garbage": rm.with_end(body, name, garbage=True) + noise}
        for more, text in texts.items():
            for batch_recs, max_text in modes:
                got, parsed, why = _device(tmp_path, text, batch_recs, max_text)
                if why is None and parsed.end != kind:
                    why = "the model says %s, the corpus %s" % (parsed.end, kind)
                if why is None and where.endswith("piece") and len(got.pieces) < 2:
                    why = "one piece"
                if why:
                    bad.append("%s%s, batches of %d, text budget %d: %s" % (name, more, batch_recs, max_text, why))
    _report(bad)


def test_texts_that_begin_with_their_end(tmp_path, monkeypatch):
    """nothing in front: no FASTQ at all is the host parser's business (a handover, no reason given), a lone '@' or a header
    with nothing behind it is an empty input"""
    _env(monkeypatch)
    bad = []
    for name in rm.ENDS:
        got, parsed, why = _device(tmp_path, rm.with_end(b"", name), 7, 0)
        if why:
            bad.append("%s: %s" % (name, why))
    _report(bad)


# ---- piece boundaries and the carry -----------------------------------------------------------------------------------------
CLASSES = ("inside a header", "inside a sequence", "inside a plus line", "inside a quality line", "directly behind a newline",
           "between \\r and \\n")


def _boundary_class(text, lines, at):
    """where in a record the piece boundary `at` (the first byte of a piece's body) fell, from the model's line table"""
    k = int(np.searchsorted(lines[:, 0], at, side="right")) - 1
    if lines[k, 0] == at:
        return CLASSES[4]
    if text[at - 1:at + 1] == b"\r\n":
        return CLASSES[5]
    return CLASSES[k % 4]


def _phase_cuts(parsed, every=4000):
    """text offsets some `every` bytes apart, at the six phases of a record (CLASSES) in turn"""
    t, r, lines = parsed.text, parsed.recs, parsed.lines
    cuts, k, j = [], 0, 0
    while True:
        k = int(np.searchsorted(r[:, rm.R_START], (cuts[-1] if cuts else 0) + every))
        while j % 6 == 5 and k < len(r) and t[r[k, rm.R_HE]:r[k, rm.R_HE] + 2] != b"\r\n":
            k += 1  # (the next record with CRLF line ends)
        if k >= len(r):
            return cuts
        cuts.append(int((r[k, rm.R_START] + 2, r[k, rm.R_S] + 1, lines[4 * k + 2, 0] + 1, r[k, rm.R_Q] + 1, r[k, rm.R_START], r[k, rm.R_HE] + 1)[j % 6]))
        j += 1


def _gzip_in_blocks(text, cuts, level=6):
    """one gzip member whose writer ended a deflate block at each of the text offsets (zlib's Z_BLOCK: no marker, no byte
    alignment -- the blocks look like any others)"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    out, a = [], 0
    for b in cuts:
        out += [c.compress(text[a:b]), c.flush(zlib.Z_BLOCK)]
        a = b
    return b"".join(out + [c.compress(text[a:]), c.flush()])


@pytest.mark.parametrize("max_text", [0, 3000])
def test_piece_boundaries_at_every_phase_of_a_record(tmp_path, monkeypatch, max_text):
    """400 KB of text that compresses poorly in pieces of 16 KiB of gzip; a first record of 0..63 more bytes moves every cut.
    What a piece could not hand out is carried in front of the next one (any alignment).  A piece begins at a deflate block's
    start.  zlib ends its own blocks where its symbol buffer is full -- in 64 such files always inside a header, sequence or
    quality line, the line ends being swallowed by matches --, so three files in four come from a writer that also ends a
    block every 4 KB or so, at each phase of a record in turn; where the pieces' boundaries fell is read off the reader."""
    _env(monkeypatch, seg=16384, stretch=2048)
    recs = _random_records(np.random.default_rng(41), 400_000, shapes=("crlf", "crlf", "crlf", "plusid", "plusid", "plain"))
    seen, bad = collections.Counter(), []
    p = tmp_path / "x.fq.gz"
    for k in range(64):
        text = b"@p" + b"x" * k + b"\nACGT\n+\nIIII\n" + b"".join(recs)
        parsed = rm.parse(text)
        p.write_bytes(gzip.compress(text, 6) if k % 4 == 3 else _gzip_in_blocks(text, _phase_cuts(parsed)))
        got = rm.dump(p, 1, 100, max_text)
        why = rm.verdict(got, parsed, rm.device_batches(parsed, 100, max_text, got.pieces), 100, max_text, on_device=True)
        if why is None and len(got.pieces) < 2:
            why = "one piece"
        if why or parsed.end != rm.END_OF_TEXT:
            bad.append("prefix %d: %s" % (k, why or parsed.end))
        seen.update(_boundary_class(text, parsed.lines, at) for at in got.pieces[1:])
    _report(bad)
    assert all(seen[c] for c in CLASSES), seen


# ---- seeded fuzz ------------------------------------------------------------------------------------------------------------
# (that the seeds show every shape and every end at least twice: tests/test_record_model.py, without a GPU)
@pytest.mark.parametrize("group", range(4))
def test_model_host_reader_and_gpu_reader_agree_on_the_fuzz_seeds(tmp_path, monkeypatch, group):
    bad = []
    for seed in rm.FUZZ_SEEDS[group::4]:
        text, k = rm.fuzz_case(seed)
        _env(monkeypatch, seg=k["seg"], stretch=k["stretch"])
        monkeypatch.setenv("NOHUMAN_READ_CHUNK", str(max(k["chunk"], 7)))
        got, parsed, why = _device(tmp_path, text, k["batch_recs"], k["max_text"], level=k["level"])
        if why:
            bad.append("seed %d, the reader on the GPU (%s): %s" % (seed, parsed.end, why))
        hp = rm.parse(text)
        host = rm.dump(tmp_path / "x.fq.gz", 0, k["batch_recs"], k["max_text"])
        why = rm.verdict(host, hp, rm.host_batches(hp, k["batch_recs"], k["max_text"]), k["batch_recs"], k["max_text"])
        if why:
            bad.append("seed %d, the host reader (%s): %s" % (seed, hp.end, why))
    _report(bad)
