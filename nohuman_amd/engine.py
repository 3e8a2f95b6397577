"""Engine: Python view of the C ABI (include/nohuman_engine.h).  numpy in, numpy out."""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

from . import _lib

RESULT_DTYPE = np.dtype([("call", "<u4"), ("total_kmers", "<u4"), ("clade_hits", "<u4"),
                         ("hit_groups", "<u4")])
TAXON_AMBIGUOUS = 0xFFFFFFFF
TAXON_MATE_BORDER = 0xFFFFFFFE
FLAG_PAIRED = 1
FLAG_LONG = 2
# nh_codec of include/nohuman_engine.h: what out_codec takes
CODEC_NONE, CODEC_BZIP2, CODEC_GZIP, CODEC_XZ, CODEC_ZSTD, CODEC_BGZF, CODEC_BAM = 0, 1, 2, 3, 4, 5, 6


class EngineError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("nohuman engine error %d: %s" % (code, message))
        self.code = code
        self.message = message


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib.lib().nh_last_error().decode(errors="replace"))


def probe() -> str:
    """`nohuman --check` counterpart (/root/reference/src/lib.rs:50-57): raises if unusable."""
    buf = C.create_string_buffer(256)
    rc = _lib.lib().nh_probe(buf, 256)
    if rc != 0:
        raise EngineError(rc, buf.value.decode(errors="replace"))
    return buf.value.decode()


def run(db_dir, in1, out1, in2=None, out2=None, kraken_output=None, report=None, confidence: float = 0.0,
        threads: int = 1, keep_human: bool = False, device_ids=None, out_codec: int = 0,
        codec_threads: int = 0, human_out1=None, human_out2=None, mask: bool = False, calls=None,
        human_ids=None, min_base_quality: int = 0, read_stats=None, taxon_outs=None, report_minimizer_data: bool = False,
        minimizer_table=None, minimizer_data=None, host_taxids=None, keep_taxids=None, dust_reads: bool = False,
        host_intervals=None, host_bases_only: bool = False, host_gap: int = 0, host_cut: bool = False,
        host_min_piece: int = 35) -> "_lib.nh_stats":
    """nh_run: whole run, database loaded into every listed device (default: all visible).  human_out1 (and, paired,
    human_out2) given: nh_run_split -- the non-human reads go to out1 / out2 and, in the same pass, the human reads to
    human_out1 / human_out2 exactly as a keep_human run would write them.  mask: nh_run_mask -- every read goes to
    out1 / out2 in input order, a human read's bases replaced by N (with human_out1 / human_out2 as well, if given).
    out_codec: the container of every output, one of the CODEC_* numbers (CODEC_BGZF: gzip in bgzip's blocked form).
    CODEC_BAM (in1 a BAM file, alone; not with mask or taxon_outs): out1 and human_out1 are BAM files -- the input's header (no
    @PG line added) and the selected records of the input copied byte for byte, tags intact, BGZF framed; the records the
    reader skips (secondary, supplementary, without bases) are written nowhere, and no call is added to a record (it is in
    calls and kraken_output).  Every other output is what the same run with a FASTQ codec writes.
    calls / human_ids (nh_run_ex; any kind of run): two plain-text read lists built on the GPU in the same pass -- calls: a
    line per fragment, C/U, id, taxid, length(s), total_kmers, clade_hits, hit_groups, tab-separated (clade_hits /
    total_kmers is the confidence that `confidence` thresholds); human_ids: the id of every human fragment.
    min_base_quality (nh_run_minq; kraken2's --minimum-base-quality, 0..93): a base of a FASTQ record with a Phred+33 quality
    below it is classified as an ambiguous base; every record written keeps its bases.  0: exactly the run without it.
    read_stats (nh_run_rstats; any kind of run): a path, or a ReadStats -- the QC summary of all, non-human and human reads per
    mate (reads, bases, lengths, N50, GC, quality histogram), counted on the GPU in the same pass; the table goes to the path,
    the numbers into the ReadStats.
    taxon_outs (nh_run_taxa; not with keep_human): up to 8 selectors [(taxid or "other", out1, out2 or None), ...] -- the
    classified reads sorted by clade on the GPU in the same pass, each to the deepest selected taxon that is its call or an
    ancestor of it ("other": in no selector's clade), written as a keep_human run writes them.  The stats returned then carry
    taxon_fragments: the selectors' fragment counts, in the order given.
    report_minimizer_data / minimizer_table / minimizer_data (nh_run_mdata; any kind of run): kraken2's --report-minimizer-data --
    per taxon, the minimizer hit groups of the run's reads and how many DISTINCT database minimizers they were, counted exactly
    on the GPU by a pass behind the classifier.  report_minimizer_data puts the two clade numbers into columns 4 and 5 of
    `report`; minimizer_table is the path of the project's own table (with the cells of the table per taxon and the coverage);
    minimizer_data is a list that receives a dict per node of the taxonomy, in internal-id order from the root (taxid,
    reads_clade, reads_own, minimizers_clade, minimizers_own, distinct_clade, distinct_own, db_cells_clade, db_cells_own).
    host_taxids / keep_taxids (nh_run_host; any kind of run): the host selection -- two lists of taxids, 16 together at most.  A
    classified fragment is a HOST fragment iff the deepest listed taxon that is its call or an ancestor of its call is a host
    taxid; a classified fragment that is not is SPARED and every output treats it as it treats an unclassified one: out1 / out2,
    the human outputs, the mask, human_ids and the classes of read_stats follow the selection, while calls, kraken_output,
    report, taxon_outs, the minimizer data and the stats' three totals keep the true calls.  host_taxids=[1] is the run without a
    selection; [9606] on a standard database removes only human reads; [1] with keep_taxids=[10239] everything but viruses.  The
    stats returned then carry host_fragments and spared_fragments (their sum is `classified`).
    dust_reads (nh_run_dust; any kind of run): every sequence, both mates, FASTA as FASTQ, is classified with its low-complexity
    stretches (symmetric DUST, window 64, level 20, each sequence on its own) as ambiguous bases -- what cures the false positives
    of a database built without low-complexity masking; every record written keeps its bases.  With min_base_quality the
    classifier sees the union of the two masks.  The stats returned then carry dust_masked_bases.
    host_intervals (nh_run_intervals; any kind of run): a BED file, plain text, of where in each read the host k-mers lie -- a line
    `id, start, end, mate (1|2), taxid of the call` for every maximal run of bases that host k-mers cover (0-based, half-open), in
    input order; a k-mer is host when its minimizer is found in the table and, with host_taxids / keep_taxids, its value lies in
    the host clades.  Nothing else the run writes changes.  A BAM input's coordinates are those of the FASTQ text the reader
    transcodes to: a reverse-strand record is counted on its reverse complement.  The stats returned then carry
    interval_fragments, intervals and covered_bases.
    host_bases_only (nh_run_hostbases; implies mask): a masked run that writes N only over the bases that host k-mers cover -- the
    coverage of host_intervals, on the copy the classifier read -- of a host fragment and keeps the input's own bases elsewhere;
    every other byte of every output is the masked run's.  host_gap (0..4096, needs host_bases_only): an uncovered run of at most
    so many bases between two covered ones of the same sequence is masked as well (mates apart, never a run that touches an end);
    34 (k - 1) is the recommendation for noisy long reads.  The stats returned then carry host_bases, masked_bases and closed_bases.
    host_cut (nh_run_hostcut; implies mask; single-end only, not with host_bases_only): a masked run that cuts the closed coverage
    (host_gap as above) out of a host fragment and writes every uncovered run of at least host_min_piece bases (1..2^31-1, default
    35 = k) as a record of its own, `<id>:<start>-<end>` (0-based, half-open) in front of the rest of the header, the input's own
    bases and qualities of the run; a host fragment with no such run is not written, every other fragment is written whole.  Every
    other output is the masked run's.  The stats returned then carry host_bases, pieces, piece_bases, cut_bases, short_bases,
    dropped_reads and closed_bases (host_bases = piece_bases + cut_bases + short_bases)."""
    a = _lib.nh_run_args()
    a.db_dir = os.fsencode(db_dir)
    a.in1 = os.fsencode(in1)
    a.in2 = os.fsencode(in2) if in2 else None
    a.out1 = os.fsencode(out1)
    a.out2 = os.fsencode(out2) if out2 else None
    a.kraken_output = os.fsencode(kraken_output) if kraken_output else None
    a.report = os.fsencode(report) if report else None
    a.confidence = float(confidence)
    a.threads = int(threads)
    a.keep_human = int(bool(keep_human))
    a.out_codec = int(out_codec)
    a.codec_threads = int(codec_threads)
    ids = None
    if device_ids:
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        a.n_devices = len(device_ids)
        a.device_ids = ids
    else:
        a.n_devices = 0
        a.device_ids = None
    return _run_entry("nh_run", (), lambda: _taxo_nodes(os.fspath(db_dir)), a, human_out1, human_out2, mask, calls, human_ids,
                      min_base_quality, read_stats, taxon_outs, report_minimizer_data, minimizer_table, minimizer_data, host_taxids,
                      keep_taxids, dust_reads, host_intervals, host_bases_only, host_gap, host_cut, host_min_piece)


def _run_entry(prefix, lead, nodes, a, human_out1, human_out2, mask, calls, human_ids, min_base_quality, read_stats, taxon_outs,
               report_minimizer_data, minimizer_table, minimizer_data, host_taxids, keep_taxids, dust_reads=False,
               host_intervals=None, host_bases_only=False, host_gap=0, host_cut=False, host_min_piece=35) -> "_lib.nh_stats":
    """run() and Engine.run(): the entry of the family `prefix` (nh_run / nh_run_engine, behind the arguments `lead`: none / the
    handle) that the options ask for -- the first of hostcut, hostbases, intervals, dust, host, mdata, taxa, rstats, minq, ex, mask, split, none that has one -- and
    what it hands back, on the stats.  nodes(): the nodes of the taxonomy, asked only where minimizer data wants a list."""
    fn = lambda suffix: getattr(_lib.lib(), prefix + suffix)
    s = _lib.nh_stats()
    head = tuple(lead) + (C.byref(a),)
    want_md = report_minimizer_data or minimizer_table is not None or minimizer_data is not None
    host_gap = int(host_gap)
    if host_gap < 0 or (host_gap and not host_bases_only and not host_cut):
        raise EngineError(-1, "host_gap %d: it is 0..%d and needs host_bases_only" % (host_gap, _lib.NH_HOST_GAP_MAX))
    host_min_piece = int(host_min_piece)
    if host_min_piece != 35 and not host_cut:
        raise EngineError(-1, "host_min_piece %d: it needs host_cut" % host_min_piece)
    if host_cut and not 1 <= host_min_piece <= 0x7FFFFFFF:
        raise EngineError(-1, "host_min_piece %d: it is 1..2147483647" % host_min_piece)
    mask = mask or bool(host_bases_only) or bool(host_cut)
    if host_cut or host_bases_only or host_intervals is not None or dust_reads or host_taxids or keep_taxids or want_md or taxon_outs or read_stats is not None or min_base_quality:
        # the entries that take nh_run_minq's list and, each, one thing more: every one gets the list as far as its own last argument
        x = _extras_or_none(mask, human_out1, human_out2, calls, human_ids)
        rs = _read_stats(read_stats) if read_stats is not None else None
        t = _taxon_outs(taxon_outs or [])
        md = _minimizer_data(report_minimizer_data, minimizer_table, minimizer_data, nodes()) if want_md else None
        hf = _host_filter(host_taxids, keep_taxids) if host_taxids or keep_taxids else None
        rd = _lib.nh_read_dust(C.sizeof(_lib.nh_read_dust), 1, 0) if dust_reads else None
        hi = (_lib.nh_host_intervals(C.sizeof(_lib.nh_host_intervals), 0, os.fsencode(host_intervals), 0, 0, 0)
              if host_intervals is not None else None)
        hb = (_lib.nh_host_bases(C.sizeof(_lib.nh_host_bases), 1, min(host_gap, 0xFFFFFFFF), 0, 0, 0, 0) if host_bases_only else None)
        hc = (_lib.nh_host_cut(C.sizeof(_lib.nh_host_cut), 1, min(host_gap, 0xFFFFFFFF), host_min_piece) if host_cut else None)
        tail = [x, _minq(min_base_quality), _path_or_none(rs.path) if rs else None, C.byref(rs.raw) if rs else None,
                t if len(t) else None, len(t), C.byref(md) if md is not None else None, C.byref(hf) if hf is not None else None,
                C.byref(rd) if rd is not None else None, C.byref(hi) if hi is not None else None, C.byref(hb) if hb is not None else None,
                C.byref(hc) if hc is not None else None]
        suffix, n = (("_hostcut", 12) if hc is not None else ("_hostbases", 11) if hb is not None else ("_intervals", 10) if hi is not None else ("_dust", 9) if rd is not None else ("_host", 8) if hf is not None else ("_mdata", 7) if want_md else ("_taxa", 6) if taxon_outs else
                     ("_rstats", 4) if rs is not None else ("_minq", 2))
        _check(fn(suffix)(*head, *tail[:n], C.byref(s)))
        if md is not None:
            _minimizer_data_out(md, minimizer_data)
        if taxon_outs:
            s.taxon_fragments = [int(o.fragments) for o in t]
        if hf is not None:
            s.host_fragments, s.spared_fragments = int(hf.host_fragments), int(hf.spared_fragments)
        if rd is not None:
            s.dust_masked_bases = int(rd.masked_bases)
        if hi is not None:
            s.interval_fragments, s.intervals, s.covered_bases = int(hi.fragments), int(hi.intervals), int(hi.covered_bases)
        if hb is not None:
            s.host_bases, s.masked_bases, s.closed_bases = int(hb.host_bases), int(hb.masked_bases), int(hb.closed_bases)
        if hc is not None:
            for k in _lib.HOST_CUT_COUNTS + ("closed_bases",):
                setattr(s, k, int(getattr(hc, k)))
    elif calls is not None or human_ids is not None:
        x = _extras(mask, human_out1, human_out2, calls, human_ids)
        _check(fn("_ex")(*head, C.byref(x), C.byref(s)))
    elif mask:
        _check(fn("_mask")(*head, _path_or_none(human_out1), _path_or_none(human_out2), C.byref(s)))
    elif human_out1 is not None or human_out2 is not None:
        _check(fn("_split")(*head, _path_or_none(human_out1), _path_or_none(human_out2), C.byref(s)))
    else:
        _check(fn("")(*head, C.byref(s)))
    return s


def _path_or_none(p):
    return os.fsencode(p) if p is not None else None


def _taxon_outs(sel):
    """run(taxon_outs=...): the nh_taxon_out array of [(taxid or "other", out1, out2 or None), ...]"""
    sel = list(sel)
    t = (_lib.nh_taxon_out * len(sel))()
    for x, (taxid, out1, out2) in zip(t, sel):
        if isinstance(taxid, str) and taxid != "other":
            raise EngineError(-1, "taxon_outs: a selector is a taxid or \"other\", not %r" % (taxid,))
        x.taxid = _lib.NH_TAXON_OTHER if taxid == "other" else int(taxid)
        x.out1 = _path_or_none(out1)
        x.out2 = _path_or_none(out2)
    return t


def _taxo_nodes(db_dir) -> int:
    """nodes of the taxonomy in db_dir (or its db subdirectory), from taxo.k2d's header; 0 where it cannot be read"""
    for d in (db_dir, os.path.join(db_dir, "db")):
        try:
            with open(os.path.join(d, "taxo.k2d"), "rb") as f:
                head = f.read(16)
            if len(head) == 16 and head[:8] == b"K2TAXDAT":
                return int.from_bytes(head[8:16], "little")
        except OSError:
            pass
    return 0


def _minimizer_data(in_report, table, want_list, nodes) -> "_lib.nh_minimizer_data":
    """run(report_minimizer_data=, minimizer_table=, minimizer_data=): the nh_minimizer_data of a run on a taxonomy of `nodes`"""
    md = _lib.nh_minimizer_data()
    md.struct_size = C.sizeof(_lib.nh_minimizer_data)
    md.in_report = int(bool(in_report))
    md.table = _path_or_none(table)
    if want_list is not None:
        cap = max(int(nodes), 1)
        md._keep = (_lib.nh_taxon_minimizers * cap)()
        md.taxa = md._keep
        md.taxa_cap = cap
    return md


def _minimizer_data_out(md, want_list):
    if want_list is None:
        return
    del want_list[:]
    for i in range(min(int(md.n_taxa), int(md.taxa_cap))):
        want_list.append({name: int(getattr(md.taxa[i], name)) for name, _ in _lib.nh_taxon_minimizers._fields_})


def _host_filter(host_taxids, keep_taxids) -> "_lib.nh_host_filter":
    """run(host_taxids=, keep_taxids=): the nh_host_filter of two lists of taxids (the library checks them)"""
    hf = _lib.nh_host_filter()
    hf.struct_size = C.sizeof(_lib.nh_host_filter)
    for name, ids in (("host", host_taxids), ("keep", keep_taxids)):
        ids = [int(x) for x in (ids or [])]
        if any(x < 0 or x >= 2 ** 64 for x in ids):
            raise EngineError(-1, "%s_taxids: a taxid is a number in 0 .. 2^64 - 1" % name)
        arr = (C.c_uint64 * max(len(ids), 1))(*ids)
        setattr(hf, "_keep_" + name, arr)  # (the struct borrows the arrays)
        setattr(hf, "n_" + name, len(ids))
        setattr(hf, name + "_taxids", arr)
    return hf


def host_table(taxo_bytes, host_taxids=None, keep_taxids=None) -> bytes:
    """nh_host_table_image: the host-node table of a selection on a taxo.k2d image, one byte per node in internal-id order (entry
    0 is 0): 1 where the deepest listed taxon that is the node or an ancestor of it is a host taxid.  No GPU needed."""
    taxo_bytes = bytes(taxo_bytes)
    hf = _host_filter(host_taxids, keep_taxids)
    n = C.c_uint64(0)
    cap = int.from_bytes(taxo_bytes[8:16], "little") if len(taxo_bytes) >= 16 else 0
    cap = min(max(cap, 1), max(len(taxo_bytes), 1))  # (a node takes 56 bytes: a count above the image's bytes is refused anyway)
    buf = (C.c_uint8 * cap)()
    _check(_lib.lib().nh_host_table_image(taxo_bytes, len(taxo_bytes), C.byref(hf), buf, cap, C.byref(n)))
    return bytes(buf[:int(n.value)])


def _extras(mask, human_out1, human_out2, calls, human_ids) -> "_lib.nh_run_extras":
    x = _lib.nh_run_extras()
    x.struct_size = C.sizeof(_lib.nh_run_extras)
    x.mask = int(bool(mask))
    x.human_out1 = _path_or_none(human_out1)
    x.human_out2 = _path_or_none(human_out2)
    x.calls = _path_or_none(calls)
    x.human_ids = _path_or_none(human_ids)
    return x


def _extras_or_none(mask, human_out1, human_out2, calls, human_ids):
    """nh_run_minq's extras: NULL for a plain run"""
    if not mask and human_out1 is None and human_out2 is None and calls is None and human_ids is None:
        return None
    return C.byref(_extras(mask, human_out1, human_out2, calls, human_ids))


def _minq(q) -> int:
    q = int(q)
    if q < 0:
        raise EngineError(-1, "minimum base quality %d is not in 0..93 (Phred+33)" % q)
    return min(q, 0xFFFFFFFF)


class ReadStats:
    """What a run with read statistics counted (nh_read_stats): `raw` is the C struct -- raw.cls[class][mate] with class 0
    non-human, 1 human (reads, bases, min_len, max_len, gc, other, qual_reads, qual_bases, qhist[94]), raw.median_len[set][mate]
    and raw.n50[set][mate] with set 0 input, 1 non-human, 2 human, raw.mates.  `path`: where the run also writes the table (None:
    nowhere).  The definitions are the project's own (include/nohuman_engine.h), not seqkit's."""

    def __init__(self, path=None):
        self.path = path
        self.raw = _lib.nh_read_stats()

    def write(self, path):
        """the table of these numbers (nh_read_stats_write; no GPU needed)"""
        _check(_lib.lib().nh_read_stats_write(C.byref(self.raw), os.fsencode(path)))


def _read_stats(v) -> "ReadStats":
    """run(read_stats=...): a ReadStats as it is, a path as a ReadStats that writes there"""
    return v if isinstance(v, ReadStats) else ReadStats(v)


MAX_TAXA_NODES = 4096  # nodes of a taxa manifest with the root (include/nohuman_engine.h)


def _build_args(fasta_paths, out_dir, taxa, taxid, taxon_name, load_factor, capacity, piece_kmers, device, threads, force,
                mask_low_complexity):
    """build_db and extend_db: their nh_build_args (present layout) and the per-node array it points to, which the caller keeps
    (the library refuses taxa together with fasta_paths, taxid or taxon_name, and neither of them)"""
    if fasta_paths is None:
        fasta_paths = []
    if isinstance(fasta_paths, (str, bytes, os.PathLike)):
        fasta_paths = [fasta_paths]
    paths = [os.fsencode(p) for p in fasta_paths]
    a = _lib.nh_build_args_v3()
    a.struct_size = C.sizeof(_lib.nh_build_args_v3)
    a.mask_low_complexity = int(bool(mask_low_complexity))
    a.n_fasta = len(paths)
    if paths or taxa is None:
        a.fasta = (C.c_char_p * max(len(paths), 1))(*paths)
    if taxa is not None:
        a.taxa_file = os.fsencode(taxa)
    per_node = (_lib.nh_build_taxon_stats * MAX_TAXA_NODES)()
    a.taxon_stats = per_node
    a.taxon_stats_cap = MAX_TAXA_NODES
    a.out_dir = os.fsencode(out_dir) if out_dir is not None else None
    a.taxid = int(taxid)
    a.taxon_name = taxon_name.encode() if isinstance(taxon_name, str) else taxon_name
    a.load_factor = float(load_factor)
    a.capacity = int(capacity)
    a.piece_kmers = int(piece_kmers)
    a.device = int(device)
    a.threads = int(threads)
    a.force = int(bool(force))
    return a, per_node


def _build_stats_dict(s) -> dict:
    """nh_build_stats (present layout) as a dict, in the struct's order"""
    return {name: getattr(s, name) for name, _ in _lib.nh_build_stats._fields_ + _lib.nh_build_stats_v2._fields_ + _lib.nh_build_stats_v3._fields_}


def _taxon_stats(s, per_node) -> list:
    """the per-node array of a call that gave the stats s: a dict a node"""
    return [{name: getattr(per_node[i], name) for name, _ in _lib.nh_build_taxon_stats._fields_}
            for i in range(min(int(s.taxa), MAX_TAXA_NODES))]


def build_db(fasta_paths=None, out_dir=None, *, taxid: int = 0, taxon_name=None, load_factor: float = 0.0, capacity: int = 0,
             piece_kmers: int = 0, device: int = 0, threads: int = 1, force: bool = False,
             mask_low_complexity: bool = False, taxa=None, exclude=None) -> dict:
    """nh_build_db: a kraken2 database directory (hash.k2d, opts.k2d, taxo.k2d) built on the GPU from FASTA files (plain or
    gzip, wrapped lines, any number of records; one path or a list).  One taxon (taxid, 0 = 9606; taxon_name), or several:
    taxa is the path of a manifest with a line `taxid <TAB> parent taxid <TAB> name [<TAB> FASTA path]...` per taxon (parent 1
    is the root; the library parses it), and excludes fasta_paths, taxid and taxon_name -- a minimizer found in two taxa is
    stored as their lowest common ancestor.  The default geometry (k = 35, l = 31) only.  load_factor 0 = 0.7; capacity 0 =
    ceil(distinct minimizers / load_factor), counted on the device -- a capacity given is used as it is and the counting pass
    skipped; piece_kmers: k-mers per piece a wave scans (0 = default); force: replace a database already in out_dir;
    mask_low_complexity: mask low-complexity sequence on the GPU before the minimizers are taken (symmetric DUST, window 64,
    threshold 2.0 -- what kraken2-build's dustmasker step is for; see dust_mask).  Returns nh_build_stats as a dict
    (sequences, bases, kmers, ambiguous_kmers, distinct_minimizers, capacity, size, seconds_read / _count / _insert / _write,
    masked_bases, seconds_mask, taxa) with taxon_stats, a list of dicts (taxid, sequences, bases, kmers, cells), one a node
    in internal-id order from the root on; Engine.open(out_dir) and run(out_dir, ...) work on the result.
    exclude: a path or a list of paths (FASTA or FASTQ, plain or gzip) whose minimizers are left out of the database
    (nh_build_db_exclude): the table is built from the host's distinct minimizers that none of these sequences carries, nothing
    of them is stored, the counting pass runs even with a capacity given, and the dict gains exclude_sequences, exclude_bases,
    exclude_kmers, exclude_ambiguous_kmers, exclude_lookups, excluded_minimizers, kept_minimizers, seconds_exclude_read and
    seconds_exclude.  None or an empty list is a build without the feature."""
    if exclude is None:
        exclude = []
    if isinstance(exclude, (str, bytes, os.PathLike)):
        exclude = [exclude]
    x_paths = [os.fsencode(p) for p in exclude]
    a, per_node = _build_args(fasta_paths, out_dir, taxa, taxid, taxon_name, load_factor, capacity, piece_kmers, device, threads, force,
                              mask_low_complexity)
    s = _lib.nh_build_stats_v3()
    if x_paths:
        x = _lib.nh_exclude_args()
        x.struct_size = C.sizeof(_lib.nh_exclude_args)
        x.n_fasta = len(x_paths)
        x_arr = (C.c_char_p * len(x_paths))(*x_paths)
        x.fasta = x_arr
        xs = _lib.nh_exclude_stats()
        xs.struct_size = C.sizeof(_lib.nh_exclude_stats)
        _check(_lib.lib().nh_build_db_exclude(C.byref(a), C.byref(x), C.byref(s), C.byref(xs)))
    else:
        _check(_lib.lib().nh_build_db(C.byref(a), C.byref(s)))
    out = _build_stats_dict(s)
    if x_paths:
        out.update(exclude_sequences=xs.sequences, exclude_bases=xs.bases, exclude_kmers=xs.kmers,
                   exclude_ambiguous_kmers=xs.ambiguous_kmers, exclude_lookups=xs.lookups,
                   excluded_minimizers=xs.excluded_minimizers, kept_minimizers=xs.kept_minimizers,
                   seconds_exclude_read=xs.seconds_read, seconds_exclude=xs.seconds_exclude)
    out["taxon_stats"] = _taxon_stats(s, per_node)
    return out


def extend_db(base_dir, out_dir, fasta_paths=None, *, taxa=None, taxid: int = 0, taxon_name=None, max_load: float = 0.0,
              mask_low_complexity: bool = False, force: bool = False, device: int = 0, threads: int = 1, piece_kmers: int = 0) -> dict:
    """nh_extend_db: the database in base_dir with taxa added, written to out_dir -- only the three .k2d files of the base are
    needed, not the sequences it was made from.  The taxa are one taxon (fasta_paths, taxid, taxon_name: a child of the root, or
    the base's node of that taxid) or a manifest as build_db(taxa=...) reads it, whose parents may also be taxids of the base and
    whose lines may name a taxon of the base to add sequences to it.  The table keeps the capacity of the base (its free cells
    are the room there is); max_load is the highest load the result may have (0 = 0.95) -- EngineError with code -6
    (NH_ECAPACITY) and nothing written where the addition does not fit.  Returns nh_build_stats and nh_extend_stats as one
    dict (base_size, base_nodes, base_value_bits, nodes_added, cells_added, shadowed_cells, load, seconds_load, seconds_rekey
    beside build_db's keys) with taxon_stats, a list of dicts (taxid, sequences, bases, kmers, cells, base_cells: the cells
    the node held in the base, after renumbering) a node of the merged taxonomy in internal-id order from the root on."""
    a, per_node = _build_args(fasta_paths, out_dir, taxa, taxid, taxon_name, max_load, 0, piece_kmers, device, threads, force,
                              mask_low_complexity)
    x = _lib.nh_extend_args()
    x.struct_size = C.sizeof(_lib.nh_extend_args)
    x.base_dir = os.fsencode(base_dir) if base_dir is not None else None
    base_cells = (C.c_uint64 * MAX_TAXA_NODES)()
    x.base_cells = base_cells
    x.base_cells_cap = MAX_TAXA_NODES
    s = _lib.nh_build_stats_v3()
    xs = _lib.nh_extend_stats()
    xs.struct_size = C.sizeof(_lib.nh_extend_stats)
    _check(_lib.lib().nh_extend_db(C.byref(a), C.byref(x), C.byref(s), C.byref(xs)))
    out = _build_stats_dict(s)
    out.update({name: getattr(xs, name) for name, _ in _lib.nh_extend_stats._fields_ if name not in ("struct_size", "reserved")})
    out["taxon_stats"] = [dict(node, base_cells=int(base_cells[i])) for i, node in enumerate(_taxon_stats(s, per_node))]
    return out


def dust_mask(seqs, device: int = 0):
    """nh_dust_mask: low-complexity masking of sequences on the GPU -- symmetric DUST at dustmasker's defaults (window 64,
    threshold 2.0), the kernel build_db(mask_low_complexity=True) runs.  seqs: bytes objects (one alone is taken as a list of
    one), each masked on its own: no triplet spans two of them.  Returns (the sequences with every masked base as N, the number
    of masked bases).  Bytes other than ACGTacgt end a run and stay as they are."""
    if isinstance(seqs, (bytes, bytearray, memoryview)):
        seqs = [seqs]
    seqs = [bytes(s) for s in seqs]
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    starts = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs) > 1:
        starts[1:] = np.cumsum(lens)[:-1]
    total = int(lens.sum())
    buf = C.create_string_buffer(b"".join(seqs), max(total, 1))
    u64p = C.POINTER(C.c_uint64)
    masked = C.c_uint64(0)
    _check(_lib.lib().nh_dust_mask(int(device), C.cast(buf, C.c_void_p), total, starts.ctypes.data_as(u64p),
                                   lens.ctypes.data_as(u64p), len(seqs), C.byref(masked)))
    raw = buf.raw
    return [raw[int(a):int(a) + int(n)] for a, n in zip(starts, lens)], int(masked.value)


BamInfo = collections.namedtuple("BamInfo", "records reads bases skipped_secondary skipped_empty reverse_complemented missing_qualities digest")


def bam_scan(path, threads: int = 1) -> BamInfo:
    """nh_bam_scan: the counts of a BAM file and the digest (nh_fastx_scan's) of the FASTQ it transcodes to -- the host side of the
    BAM reader alone, no GPU.  EngineError -1 for a file that is no BAM, -2 for a malformed one (the message names the record)."""
    info = _lib.nh_bam_info()
    info.struct_size = C.sizeof(info)
    _check(_lib.lib().nh_bam_scan(os.fsencode(path), int(threads), C.byref(info)))
    return BamInfo(*(int(getattr(info, f)) for f in BamInfo._fields))


BamPairInfo = collections.namedtuple("BamPairInfo", "paired pairs bases1 bases2 digest1 digest2")


def bam_scan_pairs(path, threads: int = 1):
    """nh_bam_scan_pairs: bam_scan's pass and what a paired BAM has besides -> (BamInfo, BamPairInfo): whether the file is paired
    (its first kept record has flag 0x1), its pairs, each mate's bases and the digest (nh_fastx_scan's) of each mate's FASTQ.  A
    file whose pairs do not chain -- an orphan, two names, two records of one mate -- is EngineError -2 naming the record."""
    info, pinfo = _lib.nh_bam_info(), _lib.nh_bam_pair_info()
    info.struct_size, pinfo.struct_size = C.sizeof(info), C.sizeof(pinfo)
    _check(_lib.lib().nh_bam_scan_pairs(os.fsencode(path), int(threads), C.byref(info), C.byref(pinfo)))
    return (BamInfo(*(int(getattr(info, f)) for f in BamInfo._fields)),
            BamPairInfo(bool(pinfo.paired), *(int(getattr(pinfo, f)) for f in BamPairInfo._fields[1:])))


def bam_paired(path) -> bool:
    """nh_bam_paired: is the file a paired BAM -- a BAM whose first kept record has flag 0x1 (False for anything else)"""
    return bool(_lib.lib().nh_bam_paired(os.fsencode(path)))


def device_count() -> int:
    n = C.c_int(0)
    _check(_lib.lib().nh_device_count(C.byref(n)))
    return n.value


class Engine:
    """A kraken2 database resident in one GPU's HBM plus the classify entry points."""

    def __init__(self, handle):
        self._L = _lib.lib()
        self._h = handle

    # -- constructors -------------------------------------------------------------------------
    @classmethod
    def open(cls, db_dir, device: int = 0) -> "Engine":
        L = _lib.lib()
        h = C.c_void_p()
        _check(L.nh_open(os.fsencode(db_dir), device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_images(cls, opts: bytes, taxo: bytes, hashb, device: int = 0) -> "Engine":
        L = _lib.lib()
        h = C.c_void_p()
        hb = np.frombuffer(hashb, dtype=np.uint8) if isinstance(hashb, (bytes, bytearray)) \
            else np.ascontiguousarray(hashb).view(np.uint8)
        _check(L.nh_open_images(opts, len(opts), taxo, len(taxo), hb.ctypes.data, hb.nbytes, device,
                                C.byref(h)))
        return cls(h)

    @classmethod
    def synthetic(cls, capacity: int, n_keys: int, depth: int = 30, seed: int = 1,
                  device: int = 0) -> "Engine":
        L = _lib.lib()
        h = C.c_void_p()
        _check(L.nh_open_synthetic(capacity, n_keys, depth, seed, device, C.byref(h)))
        return cls(h)

    def close(self):
        if self._h is not None:
            self._L.nh_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- database ------------------------------------------------------------------------------
    @property
    def info(self) -> _lib.nh_db_info:
        i = _lib.nh_db_info()
        _check(self._L.nh_db_info_get(self._h, C.byref(i)))
        return i

    def db_check(self) -> _lib.nh_db_check:
        """What the content check of nh_open* found: non-empty cells, largest value, load factor, seconds."""
        c = _lib.nh_db_check()
        _check(self._L.nh_db_check_get(self._h, C.byref(c)))
        return c

    def reload_launch_knobs(self):
        """Tuning / test hook: NOHUMAN_FRAG_CHUNK / NOHUMAN_SEG_CAP / NOHUMAN_SCHED are read when an engine is opened;
        this reads them again (no launch may be in flight)."""
        fn = self._L.nh_debug_reload_knobs
        fn.restype = None
        fn.argtypes = [C.c_void_p]
        fn(self._h)

    def options(self) -> _lib.nh_options:
        o = _lib.nh_options()
        _check(self._L.nh_options_get(self._h, C.byref(o)))
        return o

    def set_options(self, *, minimum_hit_groups=None, linear_probing=None, reset_per_mate=None,
                    ambiguity_rule=None):
        o = self.options()
        if ambiguity_rule is not None:
            # the rule as a plain index (0 = last l-mer, 1 = mmscanner.h is_ambiguous()); the C ABI keeps 0 for
            # "the engine's default" (include/nohuman_engine.h: NH_AMBIGUITY_LAST_LMER 1, NH_AMBIGUITY_QUEUE 2)
            if int(ambiguity_rule) not in (0, 1):
                raise EngineError(-1, "ambiguity_rule must be 0 (last l-mer) or 1 (queue)")
            o.ambiguity_rule = int(ambiguity_rule) + 1
        if minimum_hit_groups is not None:
            o.minimum_hit_groups = int(minimum_hit_groups)
        if linear_probing is not None:
            o.linear_probing = int(linear_probing)
        if reset_per_mate is not None:
            o.reset_per_mate = int(reset_per_mate)
        _check(self._L.nh_options_set(self._h, C.byref(o)))

    def ambiguity_rule(self) -> int:
        """The rule in force as a plain index (0 = last l-mer, 1 = queue)"""
        return int(self.options().ambiguity_rule) - 1

    def external_id(self, internal: int) -> int:
        v = C.c_uint64(0)
        _check(self._L.nh_taxon_external(self._h, internal, C.byref(v)))
        return v.value

    def download_table(self) -> np.ndarray:
        cells = np.empty(self.info.capacity, dtype=np.uint32)
        _check(self._L.nh_table_download(self._h, cells.ctypes.data, cells.size))
        return cells

    def taxonomy_image(self) -> bytes:
        n = C.c_size_t(0)
        _check(self._L.nh_taxonomy_image(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(self._L.nh_taxonomy_image(self._h, buf, n.value, C.byref(n)))
        return buf.raw

    def opts_image(self) -> bytes:
        n = C.c_size_t(0)
        _check(self._L.nh_opts_image(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(self._L.nh_opts_image(self._h, buf, n.value, C.byref(n)))
        return buf.raw

    # -- classify ------------------------------------------------------------------------------
    def classify(self, bases: np.ndarray, seq_offsets: np.ndarray, paired: bool = False,
                 confidence: float = 0.0, want_taxa: bool = False, long_reads: bool = False):
        """Host buffers in, result records (RESULT_DTYPE) out; optional per-k-mer taxa list.  long_reads:
        NH_FLAG_LONG (the library sets it itself for batches of more than 2000 bases per fragment)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        mates = 2 if paired else 1
        n_seq = seq_offsets.size - 1
        if n_seq % mates:
            raise ValueError("paired input needs an even number of sequences")
        n_frag = n_seq // mates
        flags = (FLAG_PAIRED if paired else 0) | (FLAG_LONG if long_reads else 0)
        out = np.zeros(n_frag, dtype=RESULT_DTYPE)
        bptr = bases.ctypes.data if bases.size else None
        if not want_taxa:
            _check(self._L.nh_classify_batch(self._h, bptr, seq_offsets.ctypes.data, n_frag, flags,
                                             float(confidence), out.ctypes.data, None, None, 0))
            return out
        cap = int(self._L.nh_kmer_taxa_entries(self._h, seq_offsets.ctypes.data, n_frag, flags))
        taxa = np.zeros(cap + 1, dtype=np.uint32)
        toff = np.zeros(n_frag + 1, dtype=np.uint64)
        _check(self._L.nh_classify_batch(self._h, bptr, seq_offsets.ctypes.data, n_frag, flags,
                                         float(confidence), out.ctypes.data, taxa.ctypes.data,
                                         toff.ctypes.data, cap + 1))
        return out, taxa[:cap], toff

    def classify_device(self, d_bases: int, d_seq_offsets: int, n_frag: int, paired: bool,
                        confidence: float, d_results: int, d_counters: int = 0, stream: int = 0,
                        d_kmer_taxa: int = 0, d_kmer_taxa_offsets: int = 0, long_reads: bool = False):
        """Device pointers in (ints), asynchronous on `stream` (a hipStream_t as int)."""
        _check(self._L.nh_classify_batch_device(
            self._h, d_bases, d_seq_offsets, n_frag,
            (FLAG_PAIRED if paired else 0) | (FLAG_LONG if long_reads else 0),
            float(confidence), d_results, d_kmer_taxa or None, d_kmer_taxa_offsets or None,
            d_counters or None, stream or None))

    def classify_records_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_frag: int,
                                paired: bool, confidence: float, d_results: int, d_counters: int = 0,
                                stream: int = 0, d_kmer_taxa: int = 0, d_kmer_taxa_offsets: int = 0,
                                long_reads: bool = False):
        """Sequences in place inside a device buffer of record text: (start, length) per sequence."""
        _check(self._L.nh_classify_records_device(
            self._h, d_text, text_len, d_seq_starts, d_seq_lens, n_frag,
            (FLAG_PAIRED if paired else 0) | (FLAG_LONG if long_reads else 0), float(confidence), d_results,
            d_kmer_taxa or None, d_kmer_taxa_offsets or None, d_counters or None, stream or None))

    def quality_mask_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, d_qual_starts: int,
                            n_seq: int, min_base_quality: int, d_out: int, d_masked: int = 0, stream: int = 0):
        """kraken2's --minimum-base-quality as a pass in front of classify_records_device: d_out (text_len + 8 bytes, the
        layout of d_text) receives every sequence's bases, N where the Phred+33 quality at d_qual_starts[i] + j is below
        min_base_quality (an all-ones quality start: copied); nothing else of d_out is written.  d_masked: one uint64 the
        kernel adds its masked bases to.  Asynchronous on `stream`."""
        _check(self._L.nh_quality_mask_device(self._h, d_text, text_len, d_seq_starts, d_seq_lens, d_qual_starts, n_seq,
                                              _minq(min_base_quality), d_out, d_masked or None, stream or None))

    def dust_reads_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_seq: int, d_out: int,
                          d_masked: int = 0, stream: int = 0):
        """--dust-reads as a pass in front of classify_records_device (nh_dust_reads_device): d_out (text_len bytes, the layout
        of d_text) already holds the sequences -- a copy of the text, or quality_mask_device's output -- and gets N at every base
        that symmetric DUST (window 64, level 20) masks in the sequence d_text[start, +len) taken on its own; nothing else of d_out
        is written.  d_masked: one uint64 the kernel adds its masked bases to.  A sequence that leaves the text is skipped and
        fails the engine's next blocking call.  Waits for `stream`."""
        _check(self._L.nh_dust_reads_device(self._h, d_text or None, int(text_len), d_seq_starts or None, d_seq_lens or None, int(n_seq),
                                            d_out or None, d_masked or None, stream or None))

    def host_cover_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_seq: int, d_cover: int,
                          d_host_of: int = 0, n_nodes: int = 0, stream: int = 0):
        """--host-intervals' mark pass behind classify_records_device (nh_host_cover_device): d_cover, ceil(text_len / 32) uint32
        zeroed by the caller, gets a bit set for every byte of d_text (4-byte aligned) that a host k-mer of the sequences
        d_text[start, +len) covers; a k-mer is host when its minimizer is found with a non-zero value v and -- d_host_of given,
        n_nodes bytes -- d_host_of[v] is not 0.  A word without a new bit is not written.  A sequence that leaves the text is
        skipped and fails the engine's next blocking call.  Waits for `stream`."""
        _check(self._L.nh_host_cover_device(self._h, d_text or None, int(text_len), d_seq_starts or None, d_seq_lens or None, int(n_seq),
                                            d_host_of or None, int(n_nodes), d_cover or None, stream or None))

    def cover_close_device(self, d_cover: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_seq: int, gap: int,
                           d_closed_bases: int = 0, stream: int = 0) -> None:
        """--host-bases-only's closing on host_cover_device's bitmap (nh_cover_close_device): an uncovered run of at most `gap` bases
        with a covered base on each side in the same sequence becomes covered.  d_closed_bases: 0, or a uint64 in device memory the
        kernel adds the bases it sets to.  A sequence outside the text is skipped and sets the sticky error bit 1024."""
        _check(self._L.nh_cover_close_device(self._h, d_cover or None, int(text_len), d_seq_starts or None, d_seq_lens or None, int(n_seq),
                                             int(gap), d_closed_bases or None, stream or None))

    def host_cut_device(self, d_text: int, text_len: int, d_records: int, d_seq_starts: int, d_seq_lens: int, d_idlen: int, d_results: int,
                        n: int, fastq: bool, d_cover: int, min_piece: int, d_out: int, cap: int, d_total: int, d_error_bits: int,
                        d_counts: int = 0, stream: int = 0) -> None:
        """--host-cut's item list and text builder on a bitmap laid out as host_cover_device leaves it (nh_host_cut_device): fragment
        i (sequence d_text[start, +len), record d_records[i] = {header start, header length, qualities start, length} uint32, id
        length d_idlen[i]) is written to d_out whole where d_results[i].call is 0, and as its uncovered runs of at least min_piece
        bases, `<id>:<a>-<b>` records, where it is not.  d_total (uint64): the bytes; d_counts: 0, or six uint64 the kernels add to
        (_lib.HOST_CUT_COUNTS).  d_error_bits (int32): 4096 a sequence or a field outside the text or an id longer than its header,
        16384 a FASTQ host record whose quality line is not as long as its sequence (such a record writes nothing), 8192 a text
        above cap (total 0, nothing written).  A bit outside a sequence changes nothing.  Waits for `stream`."""
        _check(self._L.nh_host_cut_device(self._h, d_text or None, int(text_len), d_records or None, d_seq_starts or None, d_seq_lens or None,
                                          d_idlen or None, d_results or None, int(n), int(bool(fastq)), d_cover or None, int(min_piece),
                                          d_out or None, int(cap), d_total or None, d_counts or None, d_error_bits or None, stream or None))

    def cover_intervals_device(self, d_cover: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_seq: int, d_intervals: int,
                               cap_records: int, d_total: int, d_error_bits: int, stream: int = 0):
        """host_cover_device's bitmap into records (nh_cover_intervals_device): d_intervals receives {uint32 seq, start, end} for
        every maximal run of set bits inside a sequence, in the order of the sequence table, then by start; d_total (uint64) their
        number.  More than cap_records: bit 2048 in d_error_bits (int32), total 0, nothing written; a sequence outside the text:
        bit 1024 there and no record.  Waits for `stream`."""
        _check(self._L.nh_cover_intervals_device(self._h, d_cover or None, int(text_len), d_seq_starts or None, d_seq_lens or None, int(n_seq),
                                                 d_intervals or None, int(cap_records), d_total or None, d_error_bits or None, stream or None))

    def bam_to_fastq_device(self, d_bam: int, bam_len: int, d_table: int, n_records: int, d_text: int, text_cap: int, text_len: int,
                            d_error_bits: int, stream: int = 0):
        """The BAM reader's kernel alone (nh_bam_to_fastq_device): the records of d_bam (bam_len bytes, 4-byte aligned) that
        d_table names -- two uint64 a record: where its block_size field lies in d_bam, where its '@' lies in d_text, ascending --
        are written as "@name\\nSEQ\\n+\\nQUAL\\n" into d_text[0, text_len) (text_cap bytes, 4-byte aligned).  d_error_bits: one
        int32 the caller zeroed; bit 1: a record outside d_bam, bit 2: a record's text outside the text -- such a record is not
        written, the others are.  Asynchronous on `stream`."""
        _check(self._L.nh_bam_to_fastq_device(self._h, d_bam or None, int(bam_len), d_table or None, int(n_records), d_text or None,
                                              int(text_cap), int(text_len), d_error_bits or None, stream or None))

    def bam_select_device(self, d_bam: int, bam_len: int, d_table: int, n_records: int, d_results: int, want: int, d_out: int, out_cap: int,
                          d_total: int, d_error_bits: int, stream: int = 0):
        """BAM output's kernels alone (nh_bam_select_device): of the records of d_bam (bam_len bytes, 4-byte aligned) that d_table
        names -- the reader's table, two uint64 a record, the first where its block_size field lies in d_bam -- those whose
        d_results[i].call is 0 (want 0) or not 0 (want 1) are copied whole, 4 + block_size bytes each, contiguous and in table
        order, into d_out (out_cap bytes, 4-byte aligned); d_total (one uint64 in device memory) receives their bytes.
        d_error_bits: one int32 the caller zeroed; bit 1: a record outside d_bam -- not written, the others are; bit 4: the
        total is above out_cap -- nothing is written, the total is 0.  Waits for `stream`."""
        _check(self._L.nh_bam_select_device(self._h, d_bam or None, int(bam_len), d_table or None, int(n_records), d_results or None,
                                            int(want), d_out or None, int(out_cap), d_total or None, d_error_bits or None, stream or None))

    def bam_select_pairs_device(self, d_bam: int, bam_len: int, d_table: int, n_pairs: int, d_results: int, want: int, d_out: int, out_cap: int,
                                d_total: int, d_error_bits: int, stream: int = 0):
        """bam_select_device on the pairs of a paired BAM (nh_bam_select_pairs_device): d_table is the paired reader's, two uint64
        a PAIR -- where its two records lie in d_bam, in file order --, d_results one nh_result a pair.  Both records of a
        selected pair are written, in table order; a record outside d_bam sets bit 1 and is written nowhere, and neither is its
        mate.  Everything else as bam_select_device."""
        _check(self._L.nh_bam_select_pairs_device(self._h, d_bam or None, int(bam_len), d_table or None, int(n_pairs), d_results or None,
                                                  int(want), d_out or None, int(out_cap), d_total or None, d_error_bits or None, stream or None))

    def read_stats_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, d_qual_starts: int,
                          d_results: int, n_frag: int, d_acc: int, paired: bool = False, max_workgroups: int = 0, stream: int = 0):
        """The read statistics' counting pass behind classify_records_device (nh_read_stats_device): every sequence adds its
        reads, bases, length extrema, GC, other bases and quality histogram to d_acc[class][mate] -- four nh_read_class (102
        uint64 each) the caller zeroed, min_len all-ones -- class 1 where d_results[i / mates].call != 0.  The arrays are those of
        quality_mask_device.  Asynchronous on `stream`."""
        _check(self._L.nh_read_stats_device(self._h, d_text, text_len, d_seq_starts, d_seq_lens, d_qual_starts, d_results, n_frag,
                                            FLAG_PAIRED if paired else 0, d_acc, int(max_workgroups), stream or None))

    def host_filter_device(self, d_res_in: int, d_res_out: int, n: int, d_host_of: int, n_nodes: int, d_counts: int = 0, stream: int = 0):
        """The host selection's pass behind classify_*_device (nh_host_filter_device): d_res_out[i] = d_res_in[i] (n nh_result, 16-byte
        aligned; the same array is allowed) with call = 0 where d_host_of[call] is 0 (n_nodes bytes, what host_table() returns).
        d_counts: two uint64 {host, spared} the kernel adds to.  A call >= n_nodes becomes 0 and fails the engine's next blocking
        call.  Asynchronous on `stream`."""
        _check(self._L.nh_host_filter_device(self._h, d_res_in or None, d_res_out or None, int(n), d_host_of or None, int(n_nodes),
                                             d_counts or None, stream or None))

    def minimizer_marks_bytes(self) -> int:
        """bytes of the bitmap minimizer_mark_device writes: one bit a cell of the table, 4 * ceil(capacity / 32)"""
        n = C.c_uint64(0)
        _check(self._L.nh_minimizer_marks_bytes(self._h, C.byref(n)))
        return int(n.value)

    def minimizer_mark_device(self, d_text: int, text_len: int, d_seq_starts: int, d_seq_lens: int, n_frag: int, d_marks: int,
                              d_groups: int, paired: bool = False, stream: int = 0):
        """The minimizer data's marking pass (nh_minimizer_mark_device), on the arrays of classify_records_device: every hit
        group sets the bit of the cell where its key was found in d_marks (minimizer_marks_bytes() bytes) and adds 1 to
        d_groups[taxon] (node_count uint64); the caller zeroes both.  Asynchronous on `stream`."""
        _check(self._L.nh_minimizer_mark_device(self._h, d_text, text_len, d_seq_starts, d_seq_lens, n_frag,
                                                FLAG_PAIRED if paired else 0, d_marks, d_groups, stream or None))

    def minimizer_count_device(self, d_marks: int, d_counts: int, stream: int = 0):
        """nh_minimizer_count_device: d_counts[taxon] (node_count uint64, zeroed by the caller) grows by the marked cells of
        that taxon; d_marks 0: by all its cells.  Asynchronous on `stream`."""
        _check(self._L.nh_minimizer_count_device(self._h, d_marks or None, d_counts, stream or None))

    def add_sequences(self, d_bases: int, d_seq_offsets: int, n_seq: int, value: int, stream: int = 0):
        """Bench/test support: insert the minimizers of device-resident sequences into the table."""
        _check(self._L.nh_synthetic_add_sequences(self._h, d_bases, d_seq_offsets, n_seq, value,
                                                  stream or None))

    def stats(self) -> _lib.nh_stats:
        s = _lib.nh_stats()
        _check(self._L.nh_stats_get(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        _check(self._L.nh_stats_reset(self._h))

    # -- whole run -----------------------------------------------------------------------------
    def run(self, in1, out1, in2=None, out2=None, kraken_output=None, report=None,
            confidence: float = 0.0, threads: int = 1, keep_human: bool = False, out_codec: int = 0,
            codec_threads: int = 0, human_out1=None, human_out2=None, mask: bool = False, calls=None,
            human_ids=None, min_base_quality: int = 0, read_stats=None, taxon_outs=None, report_minimizer_data: bool = False,
            minimizer_table=None, minimizer_data=None, host_taxids=None, keep_taxids=None, dust_reads: bool = False,
            host_intervals=None, host_bases_only: bool = False, host_gap: int = 0, host_cut: bool = False,
            host_min_piece: int = 35) -> _lib.nh_stats:
        """nh_run_engine; with human_out1 (and, paired, human_out2): nh_run_engine_split; mask: nh_run_engine_mask; with
        calls / human_ids: nh_run_engine_ex; with min_base_quality: nh_run_engine_minq; with read_stats:
        nh_run_engine_rstats; with taxon_outs: nh_run_engine_taxa; with report_minimizer_data / minimizer_table / minimizer_data:
        nh_run_engine_mdata; with host_taxids / keep_taxids: nh_run_engine_host; with dust_reads: nh_run_engine_dust; with host_intervals:
        nh_run_engine_intervals; with host_bases_only (and host_gap): nh_run_engine_hostbases; with host_cut (host_gap, host_min_piece): nh_run_engine_hostcut -- as run() above."""
        a = _lib.nh_run_args()
        a.db_dir = None
        a.in1 = os.fsencode(in1)
        a.in2 = os.fsencode(in2) if in2 else None
        a.out1 = os.fsencode(out1)
        a.out2 = os.fsencode(out2) if out2 else None
        a.kraken_output = os.fsencode(kraken_output) if kraken_output else None
        a.report = os.fsencode(report) if report else None
        a.confidence = float(confidence)
        a.threads = int(threads)
        a.keep_human = int(bool(keep_human))
        a.n_devices = 1
        a.device_ids = None
        a.out_codec = int(out_codec)
        a.codec_threads = int(codec_threads)
        return _run_entry("nh_run_engine", (self._h,), lambda: self.info.node_count, a, human_out1, human_out2, mask, calls, human_ids,
                          min_base_quality, read_stats, taxon_outs, report_minimizer_data, minimizer_table, minimizer_data, host_taxids,
                          keep_taxids, dust_reads, host_intervals, host_bases_only, host_gap, host_cut, host_min_piece)
