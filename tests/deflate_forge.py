"""A DEFLATE / gzip stream forge (a helper of the tests, not a test): streams written bit by bit from RFC 1951 and RFC 1952,
in the dialects zlib never writes -- repeat codes that run from the literal/length into the distance code lengths (libdeflate
does), code lengths of up to 15 bits by decree, a single distance code, length 258 as symbol 284 + extra 31, stored blocks at
every bit alignment, member headers with every field -- and the malformed ones a reader must refuse.

A token is a literal byte (an int) or a match (length, distance); replay(tokens) is the text, so the forge knows what a
stream must inflate to without any decoder.  (length, distance, ALT) writes length 258 as symbol 284 with extra 31; the raw
forms ("sym", s) and ("symd", ls, lx, ds, dx) write symbols by number for the malformed cases and have no replay.

corpus() returns the named cases (name, gz, text or None, features, members): `features` is what the case REALLY contains,
noted by the writers as they emit it (code lengths used by tokens, repeat codes that cross the boundary, extra bits at
their minimum and maximum, ...), so that the suite can assert that every construct it claims to cover is still there.

The GPU reader decodes a stretch of the stream into a slot of 16 * stretch + 65536 symbols; so that it, and not the host
decoder behind it, does the work, the forge keeps every aligned 1 KiB of a valid case's stream at 16 KiB of text or less
(dense constructs are diluted with literals) and the Huffman blocks of multi-stretch cases at 1 KiB or less (a stored
block is as long as its data; it cannot be shorter), and asserts both."""
import bisect
import functools
import heapq
import os
import struct
import zlib
from collections import namedtuple

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ALT = "alt258"
WSIZE = 32768
RING_DMAX = 1495      # the GPU decoder's ring: sources further back come from HBM ("far")
RATIO_BYTES = 1024    # every aligned RATIO_BYTES of stream ...
RATIO_TEXT = 16384    # ... inflates to at most this much text
BLOCK_BYTES = 1024    # Huffman blocks of multi-stretch cases

Case = namedtuple("Case", "name gz text features members")


# ---- bits ------------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB first: the first bit written is bit 0 of the first byte (RFC 1951 3.1.1)"""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def pos(self):
        return len(self.buf) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def put_bytes(self, b):
        assert self.n & 7 == 0
        self.buf += self.acc.to_bytes(self.n >> 3, "little")
        self.acc = 0
        self.n = 0
        self.buf += b

    def getvalue(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """RFC 1951 3.2.2: the codes of a list of code lengths, bit-reversed so that put(code, length) writes them (Huffman
    codes go most significant bit first); None where the length is 0.  Over-subscribed sets get codes too (cut to
    their lengths): the malformed cases need them."""
    maxl = max(lens) if lens else 0
    count = [0] * (maxl + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt = [0] * (maxl + 2)
    code = 0
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(_rev(nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 is a complete set"""
    return sum(32768 >> l for l in lens if l)


def huff_lengths(freq, limit):
    """code lengths of at most `limit` bits for the symbols with freq > 0: Huffman's, then clamped and repaired to a
    complete set.  One used symbol gets length 1 (the one incomplete set DEFLATE allows)."""
    used = [i for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(freq[i], n, i) for n, i in enumerate(used)]
    heapq.heapify(heap)
    parent = {}
    n = len(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        node = ("n", n)
        parent[a[2]] = node
        parent[b[2]] = node
        heapq.heappush(heap, (a[0] + b[0], n, node))
        n += 1
    for i in used:
        d, x = 0, i
        while x in parent:
            x = parent[x]
            d += 1
        lens[i] = min(d, limit)
    cap = 1 << limit
    k = sum(1 << (limit - lens[i]) for i in used)
    order = sorted(used, key=lambda i: (-lens[i], freq[i]))
    while k > cap:  # over-subscribed by the clamp: lengthen the longest codes that still can be
        for i in order:
            if lens[i] < limit:
                k -= 1 << (limit - lens[i] - 1)
                lens[i] += 1
                break
        order.sort(key=lambda i: (-lens[i], freq[i]))
    while k < cap:  # room left: shorten a code that fits
        for i in sorted(used, key=lambda i: (-lens[i], -freq[i])):
            if lens[i] > 1 and k + (1 << (limit - lens[i])) <= cap:
                k += 1 << (limit - lens[i])
                lens[i] -= 1
                break
    return lens


def random_complete_set(n, limit, rng, staircase=False):
    """n code lengths of a complete set, none above `limit`: leaves split at random (or always the deepest: 1, 2, 3, ...)"""
    assert 2 <= n <= (1 << limit)
    ls = [1, 1]
    while len(ls) < n:
        can = [i for i, l in enumerate(ls) if l < limit]
        i = max(can, key=lambda j: ls[j]) if staircase else can[int(rng.integers(0, len(can)))]
        ls[i] += 1
        ls.append(ls[i])
    return sorted(ls)


# ---- tokens ----------------------------------------------------------------------------------------------------------
LEN_SYM = {}
for _s in range(29):
    for _x in range(1 << LEXT[_s]):
        if LBASE[_s] + _x <= 258 and (LBASE[_s] + _x) not in LEN_SYM or _s == 28:
            LEN_SYM[LBASE[_s] + _x] = (257 + _s, LEXT[_s], _x)  # (258 ends up as symbol 285, no extra bits)


def dist_sym(d):
    s = bisect.bisect_right(DBASE, d) - 1
    return s, DEXT[s], d - DBASE[s]


def replay(tokens, history=b""):
    """the text a token list stands for (None when it holds raw symbols); `history` only lends context, it is not returned"""
    out = bytearray(history)
    h = len(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if isinstance(t[0], str):
            return None
        length, d = t[0], t[1]
        assert 1 <= d <= len(out), "distance %d at position %d" % (d, len(out))
        if d >= length:
            out += out[len(out) - d:len(out) - d + length]
        else:
            unit = bytes(out[len(out) - d:])
            out += (unit * (length // d + 1))[:length]
    return bytes(out[h:])


def relay(text, chain=8):
    """a small greedy LZ77 tokeniser over hash chains of three bytes: real text in tokens, for any dialect to encode"""
    tokens = []
    heads = {}
    i, n = 0, len(text)
    while i < n:
        best, bd = 0, 0
        if i + 3 <= n:
            key = text[i:i + 3]
            cands = heads.get(key)
            if cands:
                cur = text[i:i + 258]
                for c in reversed(cands[-chain:]):
                    if i - c > WSIZE:
                        break
                    m = len(os.path.commonprefix([cur, text[c:c + 258]]))
                    if m > best:
                        best, bd = m, i - c
                        if m == 258:
                            break
        if best >= 3:
            tokens.append((best, bd))
            step = best
        else:
            tokens.append(text[i])
            step = 1
        for j in range(i, min(i + step, n - 2)):
            heads.setdefault(text[j:j + 3], []).append(j)
        i += step
    return tokens


# ---- blocks ----------------------------------------------------------------------------------------------------------
class Block:
    """one DEFLATE block, rendered: Huffman blocks as an integer of nbits bits (they do not care where they start),
    stored blocks when the member knows the alignment.  marks: (bits from the block's start, text so far) after every token."""

    def __init__(self, kind, final, tokens):
        self.kind, self.final, self.tokens = kind, final, tokens
        self.bits = self.nbits = 0
        self.data = b""
        self.mark_bits, self.mark_out = [], []
        self.features = set()
        self.raw_len = None  # stored blocks: (LEN, NLEN) to write instead of the true ones

    def render(self, at_bit):
        if self.kind != "stored":
            return self.bits, self.nbits, self.mark_bits, self.mark_out
        w = BitWriter()
        sh = at_bit % 8  # (rendered at the member's bit phase, then shifted back: the padding depends on it)
        w.put(0, sh)
        w.put(1 if self.final else 0, 1)
        w.put(0, 2)
        w.align()
        pad = w.pos() - sh - 3
        n = len(self.data)
        ln, nl = self.raw_len if self.raw_len else (n, n ^ 0xFFFF)
        w.put(ln, 16)
        w.put(nl, 16)
        w.put_bytes(self.data)
        mb = [3 + pad + 32 + 8 * k for k in range(0, n + 1, 256)] + [3 + pad + 32 + 8 * n]
        mo = list(range(0, n + 1, 256)) + [n]
        return int.from_bytes(w.getvalue(), "little") >> sh, w.pos() - sh, mb, mo


def stored_block(data, final=False, raw_len=None):
    assert len(data) <= 65535
    b = Block("stored", final, list(data))
    b.data = bytes(data)
    b.raw_len = raw_len
    return b


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _emit_tokens(w, b, tokens, lit_lens, dist_lens, base):
    """the tokens and the end-of-block code; notes in b.features what was really written"""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    f = b.features
    out = 0
    far_run = 0
    last_far = None  # (bit start, first text position, end) of the last short far match
    used_l, used_d = set(), set()
    mb, mo = b.mark_bits, b.mark_out
    bp = w.pos()
    put = w.put
    seen_ll = set()
    for t in tokens:
        p0 = bp
        if t.__class__ is int:
            ll = lit_lens[t]
            assert ll, "literal %d has no code" % t
            put(lc[t], ll)
            bp += ll
            seen_ll.add(ll)
            out += 1
            far_run = 0
            mb.append(bp)
            mo.append(out)
            continue
        elif t[0] == "sym":
            w.put(lc[t[1]], lit_lens[t[1]])
        elif t[0] == "symd":
            _, ls, lx, ds, dx = t
            w.put(lc[ls], lit_lens[ls])
            w.put(lx, LEXT[ls - 257] if ls - 257 < 29 else 0)
            w.put(dc[ds], dist_lens[ds])
            w.put(dx, DEXT[ds] if ds < 30 else 0)
        else:
            length, d = t[0], t[1]
            if len(t) > 2:
                assert length == 258
                ls, lxn, lx = 284, 5, 31
                f.add("258_as_284")
            else:
                ls, lxn, lx = LEN_SYM[length]
                if length == 258:
                    f.add("258_as_285")
            ds, dxn, dx = dist_sym(d)
            assert lc[ls] is not None and dc[ds] is not None, "no code for (%d, %d)" % (length, d)
            ll, dl = lit_lens[ls], dist_lens[ds]
            w.put(lc[ls], ll)
            w.put(lx, lxn)
            w.put(dc[ds], dl)
            w.put(dx, dxn)
            used_l.add(ls)
            used_d.add(ds)
            f.add("litcode=%d" % ll)
            f.add("distcode=%d" % dl)
            if ll > 9:
                f.add("litcode>root")
            if dl > 8:
                f.add("distcode>root")
            if ll > 9 and dl > 8:
                f.add("both>root")
            if ll + lxn + dl + dxn == 48:
                f.add("token48")
            if lx == 0:
                f.add("lensym_%d_min" % ls)
            if lx == (1 << lxn) - 1 and len(t) == 2 or ls == 284 and lx == 30:
                f.add("lensym_%d_max" % ls)
            if dx == 0:
                f.add("distsym_%d_min" % ds)
            if dx == (1 << dxn) - 1:
                f.add("distsym_%d_max" % ds)
            if d < 64:
                f.add("near_lane_mod_D")
                if length == 3:
                    f.add("near_lane_mod_D_L3")
                if length == 258:
                    f.add("near_lane_mod_D_L258")
            elif d <= RING_DMAX:
                if length > 64 and d < length:
                    f.add("ring_long_overlap")
            else:
                f.add("far_long" if length > 64 else "far_short")
                if d > out:
                    f.add("far_source_before_block")
            if out == 0 and d == 32768 and length == 258 and not mo:
                f.add("d32768_l258_first_token")
            if last_far and d <= RING_DMAX and p0 - last_far[0] < 40 and last_far[1] <= base + out - d < last_far[2]:
                f.add("copy_from_far_in_window")
            bp = w.pos()
            if d > RING_DMAX and length <= 64 and bp - p0 <= 12:
                far_run += 1
                if far_run >= 12:  # a token every 12 bits or less: any 64 bits of this run hold five starts
                    f.add("five_far_in_window")
                last_far = (p0, base + out, base + out + length)
            else:
                far_run = 0
            out += length
        bp = w.pos()
        mb.append(bp)
        mo.append(out)
    for ll in seen_ll:
        f.add("litcode=%d" % ll)
        if ll > 9:
            f.add("litcode>root")
    used_l |= set(t for t in tokens if t.__class__ is int)
    if lc[256] is not None:
        w.put(lc[256], lit_lens[256])
        f.add("litcode=%d" % lit_lens[256])
    mb.append(w.pos())
    mo.append(out)
    return used_l, used_d


def fixed_block(tokens, final=False, base=0):
    b = Block("fixed", final, tokens)
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    _emit_tokens(w, b, tokens, FIXED_LIT, FIXED_DIST, base)
    b.bits, b.nbits = int.from_bytes(w.getvalue(), "little"), w.pos()
    return b


class Hdr:
    """how a dynamic block's header is written.  rle: "none" every length by itself; "zlib" runs inside the literal/length
    and inside the distance lengths; "cross" greedy over both as one sequence (RFC 1951 3.2.7 allows it, libdeflate does
    it); "zero16" like cross, but runs of zeros as a 17 followed by 16s (which then repeat 0).  hclen: "min" or 19.
    pad: HLIT = 286 and HDIST = 30, zero lengths behind the last used symbol.  cl_lens: the code-length code's lengths by
    decree (19 of them).  The rest is for malformed headers: syms = the (symbol, extra) list itself, counts = the
    (nlit, ndist) to put in the header whatever the lists hold."""

    def __init__(self, rle="zlib", hclen="min", pad=False, cl_lens=None, syms=None, counts=None):
        self.rle, self.hclen, self.pad, self.cl_lens, self.syms, self.counts = rle, hclen, pad, cl_lens, syms, counts


def _runs(seq, lo, zero16):
    """(symbol, extra, index, count) for seq, greedy; lo = the index of seq[0] in the whole sequence"""
    out = []
    i, n = 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            if zero16 and run >= 6:
                out.append((17, 0, lo + i, 3))
                i += 3
                rem = run - 3
                while rem:
                    take = min(6, rem)
                    if rem - take in (1, 2):
                        take = rem - 3
                    out.append((16, take - 3, lo + i, take))
                    i += take
                    rem -= take
                continue
            while run >= 3:
                take = min(138, run)  # (one or two zeros left over go out as themselves)
                out.append((18, take - 11, lo + i, take) if take >= 11 else (17, take - 3, lo + i, take))
                i += take
                run -= take
            for _ in range(run):
                out.append((0, 0, lo + i, 1))
                i += 1
        else:
            out.append((v, 0, lo + i, 1))
            i += 1
            run -= 1
            while run >= 3:
                take = min(6, run)
                out.append((16, take - 3, lo + i, take))
                i += take
                run -= take
            for _ in range(run):
                out.append((v, 0, lo + i, 1))
                i += 1
    return out


def dynamic_block(tokens, lit_lens, dist_lens, final=False, header=None, base=0):
    h = header or Hdr()
    b = Block("dynamic", final, tokens)
    f = b.features
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if h.pad:
        lit_lens += [0] * (286 - len(lit_lens))
        dist_lens += [0] * (30 - len(dist_lens))
    elif not h.counts:
        while len(lit_lens) > 257 and lit_lens[-1] == 0:
            lit_lens.pop()
        while len(dist_lens) > 1 and dist_lens[-1] == 0:
            dist_lens.pop()
    nlit, ndist = h.counts if h.counts else (len(lit_lens), len(dist_lens))
    if h.syms is not None:
        syms = [(s, x, 0, 0) for s, x in h.syms]
    elif h.rle == "none":
        syms = [(v, 0, i, 1) for i, v in enumerate(lit_lens + dist_lens)]
    elif h.rle == "zlib":
        syms = _runs(lit_lens, 0, False) + _runs(dist_lens, len(lit_lens), False)
    else:
        syms = _runs(lit_lens + dist_lens, 0, h.rle == "zero16")
    if h.cl_lens is not None:
        cl_lens = list(h.cl_lens)
    else:
        freq = [0] * 19
        for s in syms:
            freq[s[0]] += 1
        if sum(1 for x in freq if x) < 2:  # the code-length code must be complete: a second, unused, one-bit code
            freq[0 if not freq[0] else 1] += 1
        cl_lens = huff_lengths(freq, 7)
    ncl = 19 if h.hclen == 19 else max(4, max(i for i in range(19) if cl_lens[CLORDER[i]]) + 1)
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(nlit - 257, 5)
    w.put(ndist - 1, 5)
    w.put(ncl - 4, 4)
    for i in range(ncl):
        w.put(cl_lens[CLORDER[i]], 3)
    cc = canonical(cl_lens)
    prev_zero_run = False
    for s, x, at, cnt in syms:
        assert cc[s] is not None, "code-length symbol %d has no code" % s
        w.put(cc[s], cl_lens[s])
        if s == 16:
            w.put(x, 2)
            if prev_zero_run:
                f.add("rep16_after_zero_run")
        elif s == 17:
            w.put(x, 3)
        elif s == 18:
            w.put(x, 7)
        if s >= 16 and at < nlit < at + cnt:
            f.add("rep%d_cross" % s)
        prev_zero_run = s in (17, 18) or (s == 16 and prev_zero_run)
    if not any(s[0] >= 16 for s in syms):
        f.add("no_rle")
    if ncl == 19:
        f.add("hclen19")
    if max(cl_lens) == 7 and any(cl_lens[s[0]] == 7 for s in syms):
        f.add("clcode7")
    if nlit == 286:
        f.add("hlit286")
    if ndist == 30:
        f.add("hdist30")
    if h.pad:
        f.add("zero_padded_counts")
    used_l, used_d = _emit_tokens(w, b, tokens, lit_lens, dist_lens, base)
    nd = [l for l in dist_lens if l]
    if len(nd) == 1 and nd[0] == 1:
        f.add("one_dist_code_used" if used_d else "one_dist_code_unused")
    if ndist == 1 and dist_lens[0] == 0 and not used_d:
        f.add("hdist1_len0_literals_only")
    if [i for i, l in enumerate(lit_lens) if l] == [256] and lit_lens[256] == 1:
        f.add("eob_only_block")
    if nlit == 286 and ndist == 30 and len(used_l) == 285 and len(used_d) == 30:
        f.add("every_symbol_used")
    b.bits, b.nbits = int.from_bytes(w.getvalue(), "little"), w.pos()
    return b


def auto_lens(tokens, limit=15):
    """code lengths from the tokens' own frequencies; like zlib, never fewer than two distance codes"""
    fl, fd = [0] * 286, [0] * 30
    fl[256] = 1
    for t in tokens:
        if isinstance(t, int):
            fl[t] += 1
        else:
            fl[284 if len(t) > 2 else LEN_SYM[t[0]][0]] += 1
            fd[dist_sym(t[1])[0]] += 1
    if sum(1 for x in fl if x) < 2:
        fl[0 if not fl[0] else 1] += 1
    k = 0
    while sum(1 for x in fd if x) < 2:
        if not fd[k]:
            fd[k] = 1
        k += 1
    return huff_lengths(fl, limit), huff_lengths(fd, min(limit, 15))


def dilute(tokens, lit_lens, dist_lens, filler, per_byte=10):
    """literals behind matches that are too dense: never more than per_byte bytes of text a byte of stream, counted from
    any token on.  filler: the literal bytes to choose from, in turn; those with the longest codes are taken (a long code
    pays for the most text)"""
    filler = [c for c in filler if lit_lens[c]]
    top = max(lit_lens[c] for c in filler)
    filler = [c for c in filler if lit_lens[c] >= min(top, 6)]
    out = []
    k = 0
    debt = 0.0  # text bytes ahead of per_byte * stream bytes
    for t in tokens:
        out.append(t)
        if t.__class__ is int:
            debt += 1 - per_byte * lit_lens[t] / 8
        else:
            ls, lxn = (284, 5) if len(t) > 2 else LEN_SYM[t[0]][:2]
            ds, dxn, _ = dist_sym(t[1])
            debt += t[0] - per_byte * (lit_lens[ls] + lxn + dist_lens[ds] + dxn) / 8
        while debt > 0:
            c = filler[k % len(filler)]
            k += 1
            out.append(c)
            debt += 1 - per_byte * lit_lens[c] / 8
        if debt < 0:
            debt = 0.0
    return out


def dyn_blocks(tokens, base, header=None, per=150, limit=15, lens=None, max_bytes=BLOCK_BYTES):
    """tokens as a run of non-final dynamic blocks of at most max_bytes each, code lengths from each block's own tokens
    (or lens(tokens) -> (lit_lens, dist_lens, tokens'))"""
    blocks = []
    i = 0
    while i < len(tokens):
        n = per
        while True:
            part = tokens[i:i + n]
            if lens:
                ll, dl, part2 = lens(part)
            else:
                ll, dl = auto_lens(part, limit)
                part2 = part
            hd = header() if callable(header) else header
            b = dynamic_block(part2, ll, dl, False, hd, base)
            if b.nbits <= 8 * max_bytes or n == 1:
                break
            n = max(1, min(n // 2, int(n * 8 * max_bytes * 0.8 / b.nbits)))
        assert b.nbits <= 8 * max_bytes, "one token does not fit a block of %d bytes" % max_bytes
        blocks.append(b)
        base += text_len(part2)
        i += n
    return blocks


def text_len(tokens):
    """the length of a token list's text without building it"""
    return sum(1 if isinstance(t, int) else t[0] for t in tokens)


# ---- members ---------------------------------------------------------------------------------------------------------
class Member:
    def __init__(self):
        self.gz = b""
        self.text = b""
        self.features = set()
        self.mark_bits, self.mark_out = [], []  # bits from the member's first byte / text of the member
        self.block_bits = []                     # (kind, bits) of every block
        self.counts = 1


def member(blocks, text=None, name=None, comment=None, extra=None, hcrc=False, crc=None, isize=None, flg_or=0, cut_bits=None):
    """a gzip member (RFC 1952): header with the fields asked for, the blocks, CRC-32 and ISIZE of `text` (the replay of
    the blocks' tokens when None; None again when they hold raw symbols).  crc / isize: wrong ones, for the malformed cases;
    cut_bits: the deflate stream is cut after that many bits and no trailer follows."""
    m = Member()
    flg = flg_or | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    hd = b"\x1f\x8b\x08" + bytes([flg]) + bytes(4) + b"\x00\xff"
    if extra is not None:
        hd += struct.pack("<H", len(extra)) + extra
        m.features.add("fextra%d" % len(extra))
    if name is not None:
        hd += name + b"\0"
        m.features.add("fname%d" % len(name))
    if comment is not None:
        hd += comment + b"\0"
        m.features.add("fcomment%d" % len(comment))
    if hcrc:
        hd += struct.pack("<H", zlib.crc32(hd) & 0xFFFF)
        m.features.add("fhcrc")
    if extra is not None and name is not None and comment is not None and hcrc:
        m.features.add("all_header_fields")
    w = BitWriter()
    tokens = []
    out = 0
    for b in blocks:
        at = w.pos()
        bits, nbits, mb, mo = b.render(at)
        if b.kind == "stored":
            m.features.add("stored%d_align%d" % (len(b.data), at % 8))
        w.put(bits, nbits)
        m.mark_bits += [8 * len(hd) + at + x for x in mb]
        m.mark_out += [out + x for x in mo]
        m.block_bits.append((b.kind, nbits))
        m.features |= b.features
        tokens += b.tokens
        out = m.mark_out[-1] if m.mark_out else out
    if text is None:
        text = replay(tokens)
    m.text = text
    body = w.getvalue()
    if cut_bits is not None:
        m.gz = hd + body[:(cut_bits + 7) // 8]
        return m
    t = text if text is not None else b""
    m.gz = hd + body + struct.pack("<II", zlib.crc32(t) if crc is None else crc, (len(t) & 0xFFFFFFFF) if isize is None else isize)
    return m


def check_room(name, members, multi):
    """the forge's own promise: the GPU decoder's slots hold every valid case"""
    bits, outs = [], []
    b0 = o0 = 0
    for m in members:
        bits += [b0 + x for x in m.mark_bits]
        outs += [o0 + x for x in m.mark_out]
        b0 += 8 * len(m.gz)
        o0 += len(m.text)
        if multi:
            for kind, nb in m.block_bits:
                assert kind == "stored" or nb <= 8 * BLOCK_BYTES, "%s: a %s block of %d bits" % (name, kind, nb)
    if not bits:
        return 0
    bits, outs = np.asarray(bits, np.int64), np.asarray(outs, np.int64)
    edges = np.arange(0, b0 + 8 * RATIO_BYTES, 8 * RATIO_BYTES, dtype=np.int64)
    # text of every token that touches the window [edge, edge + 8 KiBit): from the last token that ended before it to
    # the first that ends at or behind its end
    lo = np.searchsorted(bits, edges[:-1], "right") - 1
    hi = np.minimum(np.searchsorted(bits, edges[1:], "left"), len(bits) - 1)
    t_lo = np.where(lo >= 0, outs[np.maximum(lo, 0)], 0)
    worst = int((outs[hi] - t_lo).max()) if len(edges) > 1 else 0
    assert worst <= RATIO_TEXT, "%s: %d bytes of text from 1 KiB of stream" % (name, worst)
    return worst


# ---- the corpus ------------------------------------------------------------------------------------------------------
def _fastq(rng, n):
    out = []
    size = 0
    i = 0
    while size < n:
        seq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100)])
        q = bytes((rng.integers(0, 8, 100) + 70).astype(np.uint8))
        rec = b"@r%d\n%s\n+\n%s\n" % (i, seq, q)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n]


def _preamble(rng, n):
    """n bytes of text in stored blocks (the cheapest way to fill the window), and their tokens' count"""
    data = _fastq(rng, n)
    return [stored_block(data[i:i + 60000]) for i in range(0, n, 60000)], data


def _pick_extra(rng, nbits, cap=None):
    hi = (1 << nbits) - 1
    if cap is not None:
        hi = min(hi, cap)
    r = int(rng.integers(0, 3))
    return 0 if r == 0 else hi if r == 1 else int(rng.integers(0, hi + 1))


def _gen(rng, n, pos, lits, lensyms, distsyms, p_match=0.4):
    """n random tokens from the given literal bytes, length symbols and distance symbols; extras at their minimum, their
    maximum or anywhere; distances never beyond the text so far (pos) or the window"""
    toks = []
    for _ in range(n):
        ds_ok = [s for s in distsyms if DBASE[s] <= min(pos, WSIZE)]
        if lensyms and ds_ok and rng.random() < p_match:
            ls = lensyms[int(rng.integers(0, len(lensyms)))]
            ds = ds_ok[int(rng.integers(0, len(ds_ok)))]
            length = 258 if ls == 285 else LBASE[ls - 257] + _pick_extra(rng, LEXT[ls - 257])
            d = DBASE[ds] + _pick_extra(rng, DEXT[ds], min(pos, WSIZE) - DBASE[ds])
            if ls == 284 and length == 258:
                toks.append((258, d, ALT))
            else:
                toks.append((length, d))
            pos += length
        else:
            toks.append(lits[int(rng.integers(0, len(lits)))])
            pos += 1
    return toks


LITS = list(b"ACGTN\n@+IFH#")


def _decreed(rng, lit_ls, dist_ls, lits, lensyms, distsyms):
    """lens(tokens) for dyn_blocks: the sorted length lists lit_ls / dist_ls dealt out to the symbols at random, block by
    block; tokens diluted to the ratio"""
    def lens(part):
        ls_syms = list(lits) + [256] + list(lensyms)
        assert len(ls_syms) == len(lit_ls) and len(distsyms) == len(dist_ls)
        perm = list(rng.permutation(len(ls_syms)))
        ll = [0] * 286
        for s, k in zip(ls_syms, perm):
            ll[s] = lit_ls[k]
        dl = [0] * 30
        for s, k in zip(distsyms, rng.permutation(len(distsyms))):
            dl[s] = dist_ls[int(k)]
        return ll, dl, dilute(part, ll, dl, lits)
    return lens


def _headers_cycle():
    opts = [Hdr("cross"), Hdr("zlib"), Hdr("none"), Hdr("cross", pad=True), Hdr("zero16", pad=True), Hdr("zlib", hclen=19), Hdr("cross", hclen=19, pad=True)]
    state = {"i": 0}

    def nxt():
        state["i"] += 1
        return opts[state["i"] % len(opts)]
    return nxt


def _final_empty():
    return fixed_block([], True)


def _valid_cases():
    rng = np.random.default_rng(1951)
    cases = []

    def add(name, members, multi=False, trailing=b"", count=None):
        if isinstance(members, Member):
            members = [members]
        feats = set()
        for m in members:
            assert m.text is not None
            feats |= m.features
        check_room(name, members, multi)
        cases.append((name, b"".join(m.gz for m in members) + trailing, b"".join(m.text for m in members), feats,
                      count if count is not None else len(members), multi))

    stair = random_complete_set(16, 15, rng, staircase=True)  # 1, 2, ..., 14, 15, 15
    assert stair == list(range(1, 15)) + [15, 15]
    lensyms5 = [257, 264, 270, 281, 284, 285]
    # -- code lengths
    pre, ptext = _preamble(rng, 33000)
    toks = _gen(rng, 2500, len(ptext), LITS[:9], lensyms5, [0, 1])
    blocks = dyn_blocks(toks, len(ptext), _headers_cycle(), lens=_decreed(rng, stair, [1, 1], LITS[:9], lensyms5, [0, 1]))
    add("staircase_lit", member(pre + blocks + [_final_empty()]), True)
    dsy = [0, 2, 5, 8, 11, 14, 17, 19, 20, 22, 24, 25, 26, 27, 28, 29]
    toks = _gen(rng, 2500, len(ptext), LITS, [257, 258, 262, 265, 270, 273], dsy, 0.6)
    ll18 = random_complete_set(19, 6, rng)
    blocks = dyn_blocks(toks, len(ptext), _headers_cycle(), lens=_decreed(rng, ll18, stair, LITS, [257, 258, 262, 265, 270, 273], dsy))
    add("staircase_dist", member(pre + blocks + [_final_empty()]), True)
    toks = _gen(rng, 3000, len(ptext), LITS[:9], lensyms5, dsy, 0.6)
    blocks = dyn_blocks(toks, len(ptext), _headers_cycle(), lens=_decreed(rng, stair, stair, LITS[:9], lensyms5, dsy))
    # the longest token there is: 15 + 5 + 15 + 13 bits, in a block of its own codes
    ll = [0] * 286
    dl = [0] * 30
    for s, l in zip([65, 67, 71, 84, 78, 10, 64, 43, 73, 256, 257, 264, 270, 285, 281, 284], stair):
        ll[s] = l
    for s, l in zip([0, 2, 5, 8, 11, 14, 17, 19, 20, 22, 24, 25, 26, 27, 28, 29], stair):
        dl[s] = l
    t48 = []
    for k in range(40):
        t48 += [(131 + (k % 32), 24577 + 191 * k), (258, 16385 + 8191, ALT), (227 + 30, 32768)]
    t48 = dilute(t48, ll, dl, [65])
    blocks += dyn_blocks(t48, len(ptext) + text_len(toks), Hdr("cross"), lens=lambda p: (ll, dl, p))
    add("staircase_both", member(pre + blocks + [_final_empty()]), True)
    # codes of exactly 9 and 10 bits (literals / lengths) and 8 and 9 bits (distances): the root tables' edge
    edge_l = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]
    assert kraft(edge_l) == 32768
    edge_d = [1, 2, 3, 4, 5, 6, 7, 8, 9, 9]
    assert kraft(edge_d) == 32768
    e_lits = LITS[:6]
    e_lens = [257, 260, 266, 275]
    e_dist = [0, 1, 3, 6, 9, 12, 15, 18, 21, 23]
    toks = _gen(rng, 2500, len(ptext), e_lits, e_lens, e_dist, 0.5)
    blocks = dyn_blocks(toks, len(ptext), _headers_cycle(), lens=_decreed(rng, edge_l, edge_d, e_lits, e_lens, e_dist))
    add("root_edge_codes", member(pre + blocks + [_final_empty()]), True)
    # HLIT = 286, HDIST = 30, every symbol used
    toks = list(range(256))
    for s in range(29):
        for x in sorted({0, (1 << LEXT[s]) - 1 if s != 27 else 30}):
            for ds in range(30):
                if s == 28 and ds % 7:
                    continue
                d = DBASE[ds] + (0 if (s + ds) % 2 else (1 << DEXT[ds]) - 1)
                toks.append((LBASE[s] + x, d))
    toks.append((258, 5, ALT))
    allsym = auto_lens(toks + list(range(256)) * 3)
    toks = dilute(toks, allsym[0], allsym[1], list(range(256)))
    add("every_symbol", member(pre + [dynamic_block(toks, allsym[0], allsym[1], False, Hdr("cross"), len(ptext)), _final_empty()]))
    # the same symbols in small blocks: every length and distance symbol at its minimal and maximal extra bits, multi-stretch
    blocks = dyn_blocks(toks, len(ptext), _headers_cycle(), per=120)
    add("every_symbol_small_blocks", member(pre + blocks + [_final_empty()]), True)

    # -- header coding
    text = _fastq(rng, 3000)
    lt = list(text)
    # the literal/length lengths end on the value the distance lengths start with: a 16 crosses; on zeros: 17 / 18 cross
    fl = [0] * 286
    for c in lt:
        fl[c] += 1
    fl[256] = 1
    for s in (280, 281, 282, 283, 284, 285):
        fl[s] = 1
    l2 = huff_lengths(fl, 15)
    v = l2[285]
    # distance lengths: a complete set that starts with the value the literal/length list ends with, four times
    assert l2[283] == l2[284] == l2[285] == v, "the three rare symbols share a length"
    dset = [v, v, v, v]
    rest = 32768 - 4 * (32768 >> v)
    lcur = 1
    while rest:
        if rest >= 32768 >> lcur:
            dset.append(lcur)
            rest -= 32768 >> lcur
        lcur += 1
    assert kraft(dset) == 32768 and len(dset) <= 30
    cross16 = dynamic_block(lt, l2, dset, False, Hdr("cross"))
    assert "rep16_cross" in cross16.features
    zeros_l = auto_lens(lt)[0]
    zeros_l = zeros_l + [0] * (286 - len(zeros_l))        # ends in zeros behind 256 ...
    zd = [0] * 12 + [1, 1]                                  # ... and the distances start with twelve: an 18 crosses
    cross18 = dynamic_block(lt, zeros_l, zd, False, Hdr("cross", pad=False, counts=(286, 14)))
    assert "rep18_cross" in cross18.features
    zl17 = zeros_l[:259]                                   # 257, 258 zero + three zero distances: a 17 of five crosses
    zl17[257] = zl17[258] = 0
    cross17 = dynamic_block(lt, zl17, [0, 0, 0, 1, 1], False, Hdr("cross", counts=(259, 5)))
    assert "rep17_cross" in cross17.features
    z16 = dynamic_block(lt, zeros_l, [0] * 28 + [1, 1], False, Hdr("zero16", counts=(286, 30)))
    assert "rep16_after_zero_run" in z16.features
    st7 = [3] * 3 + [4] * 8 + [5] * 2 + [6] * 2 + [7] * 4  # HCLEN = 19: all nineteen code-length symbols have codes
    assert kraft(st7) == 32768
    # the 7-bit codes go to lengths the block really uses, the short ones to the repeat codes
    usedl = sorted(set(l for l in l2 if l), key=lambda l: -l2.count(l))
    order = [16, 17, 18, 0] + usedl + [x for x in range(1, 16) if x not in usedl]
    cl7 = [0] * 19
    rare_first = order[::-1]
    for s, l in zip(rare_first, sorted(st7, reverse=True)):
        cl7[s] = l
    # make sure a 7-bit code is used: give 7 bits to the two least frequent lengths that ARE used
    u = [x for x in rare_first if x in usedl][:2]
    seven = [s for s in range(19) if cl7[s] == 7]
    for a, b_ in zip(u, seven):
        cl7[a], cl7[b_] = cl7[b_], cl7[a]
    h19 = dynamic_block(lt, l2, dset, False, Hdr("zlib", hclen=19, cl_lens=cl7))
    assert "hclen19" in h19.features and "clcode7" in h19.features
    norle = dynamic_block(lt, l2, dset, False, Hdr("none"))
    for nm, b in (("rep16_crosses", cross16), ("rep18_crosses", cross18), ("rep17_crosses", cross17), ("rep16_after_zeros", z16),
                  ("hclen19_clcode7", h19), ("no_rle_header", norle)):
        add("hdr_" + nm, member([b, b, _final_empty()]))

    # -- degenerate but legal sets
    t1 = lt[:200] + [(3, 1)] * 5 + lt[200:400]
    la = auto_lens(t1)[0]
    add("one_dist_code_used", member([dynamic_block(t1, la, [1]), dynamic_block([(3, 4) if isinstance(t, tuple) else t for t in t1], la, [0, 0, 0, 1]), _final_empty()]))
    add("one_dist_code_unused", member([dynamic_block(lt, l2, [1]), dynamic_block(lt, l2, [0, 0, 1], False, Hdr("cross")), _final_empty()]))
    add("hdist1_len0", member([dynamic_block(lt, l2, [0]), dynamic_block(lt, l2, [0], False, Hdr("none")), _final_empty()]))
    eob = [0] * 256 + [1]
    add("eob_only", member([dynamic_block(lt, l2, [0]), dynamic_block([], eob, [0]), dynamic_block([], eob, [1]),
                            dynamic_block(lt, l2, [0]), dynamic_block([], eob, [0], True)]))

    # -- lengths and distances
    toks = [(258, 32768)] + lt[:300]
    l3 = auto_lens(toks + lt)
    toks = dilute(toks, l3[0], l3[1], lt)
    add("d32768_l258_first", member(pre + [dynamic_block(toks, l3[0], l3[1], False, Hdr("cross"), len(ptext)),
                                           dynamic_block(toks, l3[0], l3[1], False, Hdr("zlib"), len(ptext) + text_len(toks)), _final_empty()]))
    toks = []
    for d in range(1, 64):
        for length in sorted({3, 4, d, d + 1, 2 * d + 1, 63, 64, 65, 129, 257, 258} - {0, 1, 2}):
            toks.append((length, d))
            toks += lt[(d * 7) % 1000:(d * 7) % 1000 + 3]
    l4 = auto_lens(toks + lt)
    blocks = dyn_blocks(lt[:100] + toks, 0, _headers_cycle(), per=60, lens=lambda p: l4 + (dilute(p, l4[0], l4[1], lt),))
    add("near_lane_mod_D", member(blocks + [_final_empty()]), True)
    toks = []
    for d in (64, 65, 100, 127, 128, 129, 200, 255, 256, 257):
        for length in (65, 128, 129, 257, 258):
            if d < length:
                toks += [(length, d)] + lt[d:d + 5]
    for d in (1000, 1494, 1495):  # (D < L cannot hold beyond 257: long matches of the ring without overlap)
        toks += [(258, d), (65, d)] + lt[:7]
    l5 = auto_lens(toks + lt)
    blocks = dyn_blocks(lt[:1500] + toks * 12, 0, _headers_cycle(), per=60, lens=lambda p: l5 + (dilute(p, l5[0], l5[1], lt),))
    add("ring_long_overlap", member(blocks + [_final_empty()]), True)
    toks = []
    for d in (1496, 1497, 2000, 2047, 2048, 2049, 4096, 20000, 32767, 32768):
        for length in (3, 4, 63, 64, 65, 66, 128, 258):
            toks += [(length, d)] + lt[length:length + 4]
    l6 = auto_lens(toks + lt)
    blocks = dyn_blocks(toks * 3, len(ptext), _headers_cycle(), per=40, lens=lambda p: l6 + (dilute(p, l6[0], l6[1], lt),))
    add("far_short_and_long", member(pre + blocks + [_final_empty()]), True)
    # five far matches and more in 64 bits of stream: 1-bit codes for length 3 and for distance symbol 21 (9 extra bits)
    ll = [0] * 286
    ll[257] = 1
    for s, l in zip([65, 67, 71, 84, 10, 256, 258, 259], [4] * 8):
        ll[s] = l
    assert kraft(ll) == 32768
    dl = [0] * 30
    dl[21], dl[2], dl[0] = 1, 2, 2
    toks = []
    for k in range(60):
        toks += [(3, 1537 + (37 * k + j * 101) % 512) for j in range(14)] + [65, 67]
        toks += [(3, 1600 + k), (3, 3), (3, 1700 + k), (4, 3), (3, 1800 + k), (5, 1)] + [71, 84, 10]
    blocks = dyn_blocks(toks, len(ptext), Hdr("cross"), per=400, lens=lambda p: (ll, dl, p))
    assert any("five_far_in_window" in b.features and "copy_from_far_in_window" in b.features for b in blocks)
    add("five_far_in_a_window", member(pre + blocks + [_final_empty()]), True)

    # -- blocks
    for n in (0, 1, 65535):
        data = _fastq(rng, n)
        # dynamic blocks of one literal more each in front move the stored header through the bit positions
        run = []
        seen = set()
        k = 0
        while len(seen) < 8 and k < 200:
            trial = run + [dynamic_block(lt[:20 + k], l2, dset)]
            mm = member(trial + [stored_block(data), _final_empty()])
            a = [f for f in mm.features if f.startswith("stored%d_align" % n)]
            if set(a) - seen:
                seen |= set(a)
                run = trial + [stored_block(data)]
            k += 1
        assert len(seen) == 8, (n, seen)
        add("stored_%d_every_alignment" % n, member(run + [_final_empty()]))
    one_lit = [dynamic_block([lt[i]], *auto_lens([lt[i]]), False, Hdr(("cross", "none", "zlib")[i % 3])) for i in range(400)]
    m = member(one_lit + [_final_empty()])
    m.features.add("many_one_literal_blocks")
    add("one_literal_blocks", m, True)
    ftoks = relay(ptext[:24000])
    blocks = []
    base = 0
    for i in range(0, len(ftoks), 300):
        part = ftoks[i:i + 300]
        if (i // 300) % 2:
            b = fixed_block(part, False, base)
            assert any(not isinstance(t, int) for t in part)
        else:
            b = dyn_blocks(part, base, Hdr("cross"), per=300)
            blocks += b
            b = None
        if b:
            blocks.append(b)
        base += text_len(part)
    m = member(blocks + [_final_empty()])
    assert m.text == ptext[:24000]
    m.features.add("fixed_with_matches_between_dynamic")
    add("fixed_between_dynamic", m, True)
    # a final block in the middle of a chunk, a second member behind it, whose first match reaches its first byte
    t2 = relay(ptext[24000:33000])
    m1 = member(dyn_blocks(ftoks[:3000], 0, Hdr("cross"), per=200) + [fixed_block(lt[:10], True)])
    sec = lt[:77] + [(77, 77)] + lt[100:400] + [(258, 77 + 77 + 300)] + lt[:50]
    m2 = member(dyn_blocks(sec, 0, Hdr("cross"), per=500) + dyn_blocks(t2, text_len(sec), Hdr("zlib"), per=200) + [_final_empty()])
    m2.features |= {"final_mid_chunk_then_member", "match_to_member_start"}
    add("two_members_match_to_start", [m1, m2], True)

    # -- member headers
    body = dyn_blocks(ftoks[:400], 0, Hdr("cross"), per=200) + [_final_empty()]
    nm = lambda n: bytes(97 + (i % 26) for i in range(n))
    for n in (63, 64, 65, 200):
        ms1 = [member(body, name=nm(n)), member(body, name=nm(n)), member(body, comment=nm(n)), member(body, name=nm(n), comment=nm(n))]
        add("hdr_name_comment_%d" % n, ms1)
    add("hdr_fextra_0", [member(body, extra=b""), member(body, extra=b""), member(body)])
    xb = bytes(rng.integers(1, 256, 65535, dtype=np.uint8))
    add("hdr_fextra_65535", [member(body, extra=xb), member(body, extra=xb), member(body)])
    add("hdr_fhcrc", [member(body, hcrc=True), member(body, hcrc=True), member(body)])
    allm = lambda: member(body, extra=b"ab\x03\x00xyz", name=nm(65), comment=nm(200), hcrc=True)
    add("hdr_all_fields", [allm(), allm(), allm()])
    bad2 = bytearray(member(body).gz)
    bad2[3] |= 0x20
    mm = member(body)
    mm.features.add("reserved_flg_tail")
    add("hdr_reserved_flg_is_trailing_garbage", [mm], trailing=bytes(bad2))

    # -- real text, relaid in libdeflate's habits
    gold = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reads_se.fq"), "rb").read()
    lines = gold.split(b"\n")
    assert len(lines) % 4 == 1 and all(l.startswith(b"@") for l in lines[:-1:4])  # four lines a record
    recs = lambda a, b: b"".join(l + b"\n" for l in lines[4 * a:4 * b])
    fq = recs(0, 150) + recs(0, 100) + recs(60, 200)  # repeated: matches at every distance up to the window
    rt = relay(fq)
    hs = [Hdr("cross", pad=True), Hdr("cross"), Hdr("zero16", pad=True)]
    cnt = {"i": 0}

    def hd():
        cnt["i"] += 1
        return hs[cnt["i"] % 3]
    blocks = dyn_blocks(rt, 0, hd, per=300)
    m = member(blocks + [_final_empty()])
    assert m.text == fq
    m.features.add("fastq_relaid")
    add("fastq_relaid", m, True)

    # -- the seeded sweep
    for seed in range(20):
        r = np.random.default_rng(5000 + seed)
        blocks, _ = _preamble(r, int(r.integers(1, 40000)))
        pos = sum(len(b.data) for b in blocks)
        hc = _headers_cycle()
        rounds, huff_bits = int(r.integers(8, 30)), 0
        while rounds > 0 or huff_bits < 80000:  # (several stretches of Huffman blocks, whatever the dice say)
            rounds -= 1
            kind = int(r.integers(0, 10))
            nl, ndl, nd = int(r.integers(2, 40)), int(r.integers(1, 20)), int(r.integers(2, 25))
            lits = [int(x) for x in r.choice(256, nl, replace=False)]
            lsy = [int(x) for x in r.choice(np.arange(257, 286), ndl, replace=False)]
            dsy2 = [int(x) for x in r.choice(30, nd, replace=False)]
            toks = _gen(r, int(r.integers(1, 250)), pos, lits, lsy, dsy2, float(r.random()) * 0.7)
            if kind == 0:
                data = bytes(r.integers(0, 256, int(r.integers(0, 3000)), dtype=np.uint8))
                blocks.append(stored_block(data))
                pos += len(data)
                continue
            if kind == 1:
                toks = dilute(toks, FIXED_LIT, FIXED_DIST, lits)
                for i in range(0, len(toks), 200):  # (a token of a fixed block is 31 bits at the most)
                    blocks.append(fixed_block(toks[i:i + 200], False, pos))
                    huff_bits += blocks[-1].nbits
                    pos += text_len(toks[i:i + 200])
                continue
            lim = int(r.integers(9, 16))
            lset = random_complete_set(nl + 1 + ndl, max(lim, 7), r)
            dset2 = random_complete_set(nd, max(min(lim, 15), 5), r)
            bs = dyn_blocks(toks, pos, hc, per=120, lens=_decreed(r, lset, dset2, lits, lsy, dsy2))
            blocks += bs
            huff_bits += sum(b.nbits for b in bs)
            pos += sum(text_len(b.tokens) for b in bs)
        m = member(blocks + [_final_empty()])
        m.features.add("sweep")
        add("sweep_%02d" % seed, m, True)
    return cases


def _invalid_cases():
    rng = np.random.default_rng(1952)
    cases = []
    text = _fastq(rng, 1500)
    lt = list(text)
    ll, _ = auto_lens(lt + [(3, 1), (4, 2)])
    ll = ll + [0] * (286 - len(ll))
    good = dynamic_block(lt, ll, [1, 1])

    def add(name, m, trailing=b""):
        ms = m if isinstance(m, list) else [m]
        cases.append((name, b"".join(x.gz for x in ms) + trailing, None, {"invalid:" + name}, 0, False))

    def fin(*blocks, **kw):
        return member(list(blocks) + [_final_empty()], text=kw.pop("text", text), **kw)

    # incomplete sets.  The literal/length hole: one code lengthened by a bit, a code nothing uses
    hole = list(ll)
    hole[max(s for s in range(256) if hole[s] == max(hole))] += 1
    assert kraft(hole) < 32768
    add("incomplete_litlen_hole_unused", fin(good, dynamic_block(lt, hole, [1, 1])))
    add("incomplete_dist_two_codes", fin(good, dynamic_block(lt, ll, [1, 2])))
    add("incomplete_dist_three_codes_used", fin(good, dynamic_block(lt[:50] + [(3, 1), (4, 2)] + lt[50:], ll, [2, 2, 2])))
    cl = [0] * 19
    used = sorted(set(ll + [1, 1]) | {0})
    for s in used:
        cl[s] = 4
    assert kraft(cl) < 32768
    add("incomplete_code_length_code", fin(good, dynamic_block(lt, ll, [1, 1], False, Hdr("none", cl_lens=cl))))
    # over-subscribed sets
    over = list(ll)
    over[max(s for s in range(256) if over[s] == max(over))] -= 1
    assert kraft(over) > 32768
    add("oversubscribed_litlen", fin(good, dynamic_block(lt, over, [1, 1])))
    add("oversubscribed_dist", fin(good, dynamic_block(lt, ll, [1, 1, 1])))
    cl = [0] * 19
    for s in used:
        cl[s] = 3
    cl[used[0]] = 1
    cl[used[1]] = 1
    assert kraft(cl) > 32768
    add("oversubscribed_code_length_code", fin(good, dynamic_block(lt, ll, [1, 1], False, Hdr("none", cl_lens=cl))))
    # no end-of-block code: the set is complete without it
    f2 = [0] * 286
    for c in lt:
        f2[c] += 1
    noeob = huff_lengths(f2, 15)
    assert noeob[256] == 0 and kraft(noeob) == 32768
    add("no_end_of_block_code", fin(good, dynamic_block(lt, noeob, [1, 1])))
    # HLIT = 287 / HDIST = 31: counts the format has no symbols for
    add("hlit_287", fin(good, dynamic_block(lt, ll + [0], [1, 1], False, Hdr("zlib", counts=(287, 2)))))
    add("hdist_31", fin(good, dynamic_block(lt, ll, [1, 1] + [0] * 29, False, Hdr("zlib", counts=(286, 31)))))
    # repeat codes that have nothing to repeat, or repeat too far
    cl = [0] * 19
    for s in (16, 17, 18, 0, 1, 8, 9, 10):
        cl[s] = 3
    first16 = [(16, 0)] + [(8, 0)] * 283 + [(1, 0)] * 2
    add("repeat_16_first", fin(good, dynamic_block(lt, [8] * 286, [1, 1], False, Hdr(syms=first16, cl_lens=cl, counts=(286, 2)))))
    past = [(8, 0)] * 144 + [(9, 0)] * 112 + [(8, 0)] * 24 + [(8, 0)] * 5 + [(1, 0)] + [(16, 3)]  # 286 + 1, then six more of 2
    add("repeat_past_the_counts", fin(good, dynamic_block(lt, [8] * 286, [1, 1], False, Hdr(syms=past, cl_lens=cl, counts=(286, 2)))))
    past18 = [(8, 0)] * 144 + [(9, 0)] * 112 + [(8, 0)] * 24 + [(18, 127)]
    add("zero_run_past_the_counts", fin(good, dynamic_block(lt, [8] * 286, [1, 1], False, Hdr(syms=past18, cl_lens=cl, counts=(286, 2)))))
    # block type 3; stored LEN / NLEN
    b3 = Block("raw", False, [])
    b3.bits, b3.nbits = 0b110, 3
    add("btype_3", fin(good, b3))
    add("stored_len_nlen_mismatch", fin(good, stored_block(text[:100], False, raw_len=(100, 100))))
    # symbols the fixed code has codes for and the format has no meaning for
    for s in (286, 287):
        add("fixed_litlen_symbol_%d" % s, fin(good, fixed_block(lt[:20] + [("sym", s)] + lt[20:40])))
    for s in (30, 31):
        add("fixed_dist_symbol_%d" % s, fin(good, fixed_block(lt[:20] + [("symd", 257, 0, s, 0)] + lt[20:40])))
    # distances beyond what has been written: the CRCs are those of the text a reader would get that takes the bytes in
    # front of the member's start for granted (zeros before the first member, the member before for a later one)
    t1 = lt[:10] + [(3, 11)] + lt[10:50]
    r1 = replay(t1, b"\0")
    add("distance_before_first_member", member([dynamic_block(t1, *auto_lens(t1)), _final_empty()], text=r1))
    first = member([good, _final_empty()])
    r2 = replay(t1, text)
    add("distance_before_later_member", [first, member([dynamic_block(t1, *auto_lens(t1)), _final_empty()], text=r2)])
    # (no distance code says 32769: the furthest reach is 32768 with 32767 bytes of the member written, behind a member
    #  whose text fills the window -- a reader that decodes chunks apart sees only "the window" there)
    big = _fastq(rng, 40000)
    firstbig = member([stored_block(big), _final_empty()])
    body = _fastq(rng, 32767)
    tail_t = [(200, 32768)] + lt[:300]
    blocks = [stored_block(body[:30000]), stored_block(body[30000:])] + dyn_blocks(tail_t, 32767, Hdr("cross"), per=100)
    r3 = body + replay(tail_t, (big + body))
    add("distance_32768_at_32767_of_later_member", [firstbig, member(blocks + [_final_empty()], text=r3)])
    # the same behind a piece boundary of the GPU reader (pieces of 40 KiB), in a piece that goes to the host decoder
    # because text beyond 16 : 1 follows: the member has 9000 bytes when the distance asks for 20000
    head = lt * 6
    bad = lt[:50] + [(100, 20000)] + lt[:50]
    dense = [65] + [(258, 1)] * 1500
    blocks = dyn_blocks(head, 0, Hdr("cross"), per=300) + [dynamic_block(bad, *auto_lens(bad)), dynamic_block(dense, *auto_lens(dense))]
    first38 = member([stored_block(big[:38000]), _final_empty()])
    assert len(first38.gz) < 40960 < len(first38.gz) + sum(b.nbits for b in blocks[:-2]) // 8
    add("distance_before_member_behind_dense_text",
        [first38, member(blocks + [_final_empty()], text=replay(head + bad + dense, big[:38000]))])
    # the stream ends inside a token, the CRC-32 is wrong, ISIZE is wrong
    cutm = member([good, _final_empty()], cut_bits=good.nbits // 2 + 3)
    add("ends_inside_a_token", cutm)
    add("wrong_crc", member([good, _final_empty()], crc=zlib.crc32(text) ^ 0x00010000))
    add("wrong_isize", member([good, _final_empty()], isize=len(text) + 1))
    return cases


REQUIRED = (
    ["litcode=%d" % n for n in (1, 9, 10, 15)] + ["distcode=%d" % n for n in (1, 8, 9, 15)] +
    ["litcode>root", "distcode>root", "both>root", "token48", "hlit286", "hdist30", "every_symbol_used", "zero_padded_counts",
     "rep16_cross", "rep17_cross", "rep18_cross", "rep16_after_zero_run", "hclen19", "clcode7", "no_rle",
     "one_dist_code_used", "one_dist_code_unused", "hdist1_len0_literals_only", "eob_only_block",
     "258_as_285", "258_as_284", "d32768_l258_first_token", "near_lane_mod_D", "near_lane_mod_D_L3", "near_lane_mod_D_L258",
     "ring_long_overlap", "far_short", "far_long", "far_source_before_block", "five_far_in_window", "copy_from_far_in_window",
     "many_one_literal_blocks", "fixed_with_matches_between_dynamic", "final_mid_chunk_then_member", "match_to_member_start",
     "fextra0", "fextra65535", "fhcrc", "all_header_fields", "reserved_flg_tail", "fastq_relaid", "sweep"] +
    ["lensym_%d_%s" % (s, e) for s in range(257, 286) for e in ("min", "max")] +
    ["distsym_%d_%s" % (s, e) for s in range(30) for e in ("min", "max")] +
    ["stored%d_align%d" % (n, a) for n in (0, 1, 65535) for a in range(8)] +
    ["fname%d" % n for n in (63, 64, 65, 200)] + ["fcomment%d" % n for n in (63, 64, 65, 200)]
)
REQUIRED_INVALID = [
    "incomplete_litlen_hole_unused", "incomplete_dist_two_codes", "incomplete_code_length_code", "oversubscribed_litlen",
    "oversubscribed_dist", "oversubscribed_code_length_code", "no_end_of_block_code", "hlit_287", "hdist_31", "repeat_16_first",
    "repeat_past_the_counts", "zero_run_past_the_counts", "incomplete_dist_three_codes_used",
    "distance_before_member_behind_dense_text", "btype_3", "stored_len_nlen_mismatch", "fixed_litlen_symbol_286", "fixed_litlen_symbol_287",
    "fixed_dist_symbol_30", "fixed_dist_symbol_31", "distance_before_first_member", "distance_before_later_member",
    "distance_32768_at_32767_of_later_member", "ends_inside_a_token", "wrong_crc", "wrong_isize",
]


@functools.lru_cache(maxsize=None)
def _all():
    return tuple(_valid_cases()), tuple(_invalid_cases())


def corpus():
    """every case, valid ones (text is bytes) first"""
    v, i = _all()
    return [Case(*c[:5]) for c in v + i]


def multi_stretch(name):
    v, _ = _all()
    return any(c[0] == name and c[5] for c in v)
