"""BAM input in plain Python: the specification of the BAM reader (nohuman_amd/csrc/nh_bam.*), and the forge the tests make their
files with.  Nothing here calls the library.

  forge_record / forge_header / bgzf   bytes of a record, of a header, and a stream framed as BGZF members of a chosen size
  records                              the inflated stream -> every record's fields (BamError for a malformed stream)
  to_fastq                             the inflated stream -> (the FASTQ text, the counts of nh_bam_scan, per kept record its text)
  COMPLEMENT                           the IUPAC complement, letter by letter: what the nibble reversal is held to
  corpus                               the forged file the scan, kernel and reader tests share

The rules: secondary / supplementary records (flag 0x900) and records without bases are skipped and counted; a
paired record (0x1) is an error; "@" + name, bases from ALPHABET, "+", qualities + 33 -- absent qualities (first byte 0xFF) all '"';
a reverse-strand record (0x10) is reverse-complemented and its qualities reversed; no tags in the header."""
import collections
import struct
import zlib

import numpy as np

ALPHABET = b"=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(ALPHABET)}
# the IUPAC complement as a table of letters ('=' stands for itself)
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "W": "W", "S": "S", "V": "B", "B": "V",
              "H": "D", "D": "H", "N": "N", "=": "="}
BGZF_HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
BGZF_EOF = BGZF_HEADER + bytes([0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
PAIRED, REVERSE, SECONDARY, SUPPLEMENTARY = 0x1, 0x10, 0x100, 0x800


class BamError(ValueError):
    """a malformed stream: `kind` is one of the refusals of the reader, `ordinal` the record's (1-based, 0: the header)"""

    def __init__(self, kind, ordinal=0):
        super().__init__("%s (record %d)" % (kind, ordinal))
        self.kind, self.ordinal = kind, ordinal


def rev4(n):
    """the 4-bit reversal of a nibble: the complement in BAM's code"""
    return (n & 1) << 3 | (n & 2) << 1 | (n & 4) >> 1 | (n & 8) >> 3


# ---- the forge --------------------------------------------------------------------------------------------------------------
def forge_record(name, seq, qual=None, flag=0, cigar=(), tags=b"", ref_id=-1, pos=-1, mapq=0, pad=0):
    """name: bytes; seq: bytes of ALPHABET letters; qual: bytes of Phred values or None (absent: 0xFF); cigar: uint32 words"""
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= CODE[c] << (0 if i & 1 else 4)
    q = bytes(qual) if qual is not None else b"\xff" * len(seq)
    assert len(q) == len(seq) and len(name) < 255
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name) + 1, mapq, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + q + tags + b"\0" * pad
    return struct.pack("<i", len(body)) + body


def forge_header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def bgzf_member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    size = len(BGZF_HEADER) + 2 + len(cdata) + 8
    assert size <= 65536
    return BGZF_HEADER + struct.pack("<H", size - 1) + cdata + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(stream, member=65280, eof=True, level=6):
    """the stream as BGZF members of `member` inflated bytes each (the last one shorter), with or without bgzip's EOF member"""
    out = b"".join(bgzf_member(stream[i:i + member], level) for i in range(0, len(stream), member))
    return out + (BGZF_EOF if eof else b"")


# ---- the model --------------------------------------------------------------------------------------------------------------
Rec = collections.namedtuple("Rec", "ordinal offset block_size flag name packed l_seq qual")


def records(stream):
    """every record of the inflated stream, in order; BamError as the reader refuses"""
    if stream[:4] != b"BAM\1":
        raise BamError("no magic")
    at = 4

    def need(n, ordinal=0):
        if at + n > len(stream):
            raise BamError("ends inside", ordinal)

    need(4)
    l_text, = struct.unpack_from("<i", stream, at)
    if l_text < 0:
        raise BamError("negative l_text")
    at += 4
    need(l_text + 4)
    at += l_text
    n_ref, = struct.unpack_from("<i", stream, at)
    if n_ref < 0:
        raise BamError("negative n_ref")
    at += 4
    for _ in range(n_ref):
        need(4)
        l_name, = struct.unpack_from("<i", stream, at)
        if l_name < 0:
            raise BamError("negative l_name")
        at += 4
        need(l_name + 4)
        at += l_name + 4
    out, ordinal = [], 0
    while at < len(stream):
        ordinal += 1
        need(4, ordinal)
        block_size, = struct.unpack_from("<i", stream, at)
        if block_size < 32:
            raise BamError("block_size", ordinal)
        need(36, ordinal)
        l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHI", stream, at + 12)
        if l_read_name == 0:
            raise BamError("l_read_name", ordinal)
        if block_size < 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            raise BamError("block_size", ordinal)
        need(4 + block_size, ordinal)
        name_at = at + 36
        if stream[name_at + l_read_name - 1] != 0:
            raise BamError("no NUL", ordinal)
        if flag & PAIRED:
            raise BamError("paired", ordinal)
        name = stream[name_at:name_at + l_read_name - 1]
        if not flag & (SECONDARY | SUPPLEMENTARY) and l_seq > 0 and (b"\n" in name or not name.rstrip(b" \t\n\v\f\r")):
            raise BamError("name", ordinal)  # (it could not stand in a FASTQ header line)
        seq_at = name_at + l_read_name + 4 * n_cigar
        qual_at = seq_at + (l_seq + 1) // 2
        out.append(Rec(ordinal, at, block_size, flag, stream[name_at:name_at + l_read_name - 1], stream[seq_at:qual_at], l_seq,
                       stream[qual_at:qual_at + l_seq]))
        at += 4 + block_size
    return out


def kept(rec):
    return not rec.flag & (SECONDARY | SUPPLEMENTARY) and rec.l_seq > 0


def record_text(rec):
    """the FASTQ record of one kept record"""
    codes = [(rec.packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(rec.l_seq)]
    if rec.qual[0] == 0xFF:
        qual = b'"' * rec.l_seq
    else:
        qual = bytes((q + 33) & 0xFF for q in rec.qual)
    if rec.flag & REVERSE:
        codes = [rev4(c) for c in reversed(codes)]
        qual = qual[::-1]
    return b"@" + rec.name + b"\n" + bytes(ALPHABET[c] for c in codes) + b"\n+\n" + qual + b"\n"


Counts = collections.namedtuple("Counts", "records reads bases skipped_secondary skipped_empty reverse_complemented missing_qualities")


def to_fastq(stream):
    """-> (text, Counts, [the text of each kept record], [the kept Rec])"""
    recs = records(stream)
    keep = [r for r in recs if kept(r)]
    texts = [record_text(r) for r in keep]
    c = Counts(len(recs), len(keep), sum(r.l_seq for r in keep), sum(1 for r in recs if r.flag & (SECONDARY | SUPPLEMENTARY)),
               sum(1 for r in recs if not r.flag & (SECONDARY | SUPPLEMENTARY) and r.l_seq == 0),
               sum(1 for r in keep if r.flag & REVERSE), sum(1 for r in keep if r.qual[0] == 0xFF))
    return b"".join(texts), c, texts, keep


def kernel_table(keep, texts, base=0):
    """what the kernel takes for these kept records: (n, 2) uint64 -- the offset of block_size less `base`, the offset of '@'"""
    t = np.zeros((len(keep), 2), np.uint64)
    pos = 0
    for i, (r, x) in enumerate(zip(keep, texts)):
        t[i] = (r.offset - base, pos)
        pos += len(x)
    return t


# ---- the corpus -------------------------------------------------------------------------------------------------------------
LENGTHS = tuple(range(1, 10)) + (63, 64, 65, 255, 256, 257)
_IUPAC = np.frombuffer(ALPHABET, np.uint8)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_NAME = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", np.uint8)


def _name(rng, n):
    return _NAME[rng.integers(0, _NAME.size, n)].tobytes()


def corpus_records(seed=5):
    """the forged records of the shared file: the length ladder, forward and reverse, with and without qualities, CIGARs and
    tags, names of 1 and 254 characters and of every length mod 4, and secondary, supplementary and empty records in between"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for rev in (0, REVERSE):
        for L in LENGTHS:
            k += 1
            letters = _IUPAC if k % 3 == 0 else _ACGT
            seq = letters[rng.integers(0, letters.size, L)].tobytes()
            qual = None if k % 5 == 0 else rng.integers(0, 94, L, dtype=np.uint8).tobytes()
            if qual is not None and k % 7 == 0:
                qual = bytes([93]) + qual[1:]
            name = _name(rng, 1 if k == 3 else 254 if k == 11 else 5 + k % 9)
            cigar = [(L << 4) | 0] if k % 2 else []
            if k % 4 == 0:
                cigar = [(3 << 4) | 4, (L << 4) | 0, (2 << 4) | 4][:1 + k % 3]
            tags = (b"NMC\x03", b"", b"RGZgroup1\0MMZC+m,1;\0", b"qsi\x09\0\0\0")[k % 4]
            out.append(forge_record(name, seq, qual, flag=rev | (0x4 if not cigar else 0), cigar=cigar, tags=tags,
                                    ref_id=-1 if not cigar else k % 2, pos=-1 if not cigar else 100 * k, pad=k % 3))
            if k % 4 == 1:
                out.append(forge_record(_name(rng, 7), b"ACGTAC", b"\x1e" * 6, flag=SECONDARY | rev, cigar=[(6 << 4)]))
            if k % 6 == 2:
                out.append(forge_record(_name(rng, 9), b"GGCC", None, flag=SUPPLEMENTARY))
            if k % 5 == 3:
                out.append(forge_record(_name(rng, 6), b"", b"", flag=0x4))
    out.append(forge_record(b"last one  with blanks", b"ACGTN", bytes([40, 30, 20, 10, 0])))
    return out


def corpus_stream(seed=5):
    return forge_header(b"@HD\tVN:1.6\n@SQ\tSN:chrT\tLN:5000\n@SQ\tSN:chrU\tLN:70000\n", [(b"chrT", 5000), (b"chrU", 70000)]) + \
        b"".join(corpus_records(seed))
