"""BAM output in plain Python: the specification of NH_CODEC_BAM (nohuman_amd/csrc/nh_bamout.hip and the run around it).  Nothing
here calls the library.

  header_bytes     the header of an inflated BAM stream, byte for byte: magic, l_text, text, n_ref, references
  select           the inflated stream of one BAM output: the header, then the chosen records, each as it lies in the input
  selected_bytes   the same without the header: what the kernels alone (nh_bam_select_device) leave in their buffer
  kernel_table     the table the kernels take for the kept records of a stream
  parse            an output's inflated stream -> (header, records): every output must still be a BAM stream

The rules: the records of a BAM output are the KEPT records of the input (tests/bam_model.kept: not secondary, not
supplementary, with bases) whose host flag is `want`, in input order, each copied byte for byte with its block_size field -- tags,
CIGAR, flags and a reverse-strand record's orientation untouched.  The records the reader skips are written nowhere.  No @PG line
is added to the header, nothing is added to a record.  An empty selection is the header alone."""
import numpy as np

from tests import bam_model as bm


def header_bytes(stream):
    """the bytes in front of the first record"""
    recs = bm.records(stream)
    if recs:
        return stream[:recs[0].offset]
    return stream  # (a stream without records is its header: records() has walked it)


def kept_records(stream):
    return [r for r in bm.records(stream) if bm.kept(r)]


def record_bytes(stream, rec):
    return stream[rec.offset:rec.offset + 4 + rec.block_size]


def selected_bytes(stream, host_flags, want):
    """host_flags: one truth value per KEPT record, in order; want: False selects the records whose flag is false"""
    keep = kept_records(stream)
    assert len(host_flags) == len(keep), (len(host_flags), len(keep))
    return b"".join(record_bytes(stream, r) for r, h in zip(keep, host_flags) if bool(h) == bool(want))


def select(stream, host_flags, want):
    return header_bytes(stream) + selected_bytes(stream, host_flags, want)


def kernel_table(stream, base=0):
    """(n, 2) uint64 for the kept records: the offset of block_size less `base`; the second word is the reader's text offset, which
    the builder does not read (here: all ones)"""
    keep = kept_records(stream)
    t = np.full((len(keep), 2), np.uint64(2 ** 64 - 1), np.uint64)
    for i, r in enumerate(keep):
        t[i, 0] = r.offset - base
    return t


def parse(out_stream):
    """-> (the header's bytes, [the bytes of each record]); BamError where the output is no BAM stream"""
    recs = bm.records(out_stream)
    return header_bytes(out_stream), [record_bytes(out_stream, r) for r in recs]
