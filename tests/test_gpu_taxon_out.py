"""Per-taxon outputs on the GPU (nh_run_taxa, `--taxon-out`): the classified records sorted by clade in HBM behind the
classifier (nohuman_amd/csrc/nh_split.hip, k_tout_*).  Every case compares a run with selectors against (a) the partition, by
tests/taxout_model.py, of a keep_human = 1 run of the same inputs and (b) a run without selectors for every other output and
the stats.  The toy database: taxonomy 1 -> {10 -> {11 -> {111, 112}, 12}, 20 -> {21, 9606}}."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import synth
from tests import taxout_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
PARENT = dict(synth.TOY_EDGES)
EXT = {0: ".fq", 2: ".fq.gz", 4: ".fq.zst", 5: ".fq.gz"}
TRACE = re.compile(r"taxon-out: (\d+) records, (\d+) bytes built on device; (\d+) fetched to host; kernel")
SEL4 = [10, 11, 9606, tm.OTHER]
HB_FRAGS = 1024  # fragments of one block of the builder


def _read(path, codec):
    raw = open(path, "rb").read()
    if codec in (2, 5):
        assert raw[:2] == b"\x1f\x8b", path
        if codec == 5:
            assert raw[-28:] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]), path
        return gzip.decompress(raw)
    if codec == 4:
        from tests.test_codec import _zstd_decompress
        assert raw[:4] == b"\x28\xb5\x2f\xfd", path
        return _zstd_decompress(raw, 64 << 20)
    return raw


def _stats(st):
    return (st.total_sequences, st.classified, st.unclassified, st.total_bases, st.table_lookups)


class Env:
    def __init__(self, env):
        self.env = dict(env or {}, NOHUMAN_TRACE="1")

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(errf, db=DB, **kw):
    """one engine.run on the database directory `db` with fd 2 (the library's trace lines) in errf"""
    from nohuman_amd import engine
    saved = os.dup(2)
    fd = os.open(str(errf), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    os.close(fd)
    try:
        return engine.run(db, **kw)
    finally:
        os.dup2(saved, 2)
        os.close(saved)


class Case:
    """the two reference runs of an input (keep_human = 1; the run without selectors), made once, then any number of selector
    lists against them.  extra: further keyword arguments of every run but the keep_human one (mask, calls, ...), whose values
    that start with '@' are file names inside the run's directory.  db, parent: the database directory and the parent map of
    its taxonomy (the toy database's by default)."""

    def __init__(self, tmp, name, in1, in2=None, codec=0, env=None, device_ids=(0,), extra=None, fasta=False, minq=0, db=DB,
                 parent=PARENT):
        self.tmp, self.name, self.in1, self.in2, self.codec, self.env = tmp, name, in1, in2, codec, env
        self.db, self.parent = str(db), parent
        self.device_ids, self.extra, self.fastq, self.minq = list(device_ids), dict(extra or {}), not fasta, minq
        self.mates = ("1", "2") if in2 else ("1",)
        self.runs = 0
        with Env(env):
            self.ref_dir, self.ref, _ = self._one("ref", None)
            d = tmp / (name + "_keep")
            d.mkdir()
            kw = dict(in1=in1, out1=str(d / ("o1" + EXT[codec])), in2=in2, out2=str(d / ("o2" + EXT[codec])) if in2 else None, threads=4,
                      out_codec=codec, keep_human=True, min_base_quality=minq, device_ids=self.device_ids)
            self.keep_stats = _run(tmp / (name + "_keep.stderr"), db=self.db, **kw)
            self.keep = [_read(d / ("o%s%s" % (m, EXT[codec])), codec) for m in self.mates]

    def _one(self, tag, sel):
        d = self.tmp / ("%s_%s" % (self.name, tag))
        d.mkdir()
        kw = dict(in1=self.in1, out1=str(d / ("o1" + EXT[self.codec])), in2=self.in2, out2=str(d / ("o2" + EXT[self.codec])) if self.in2 else None,
                  kraken_output=str(d / "k.txt"), report=str(d / "r.txt"), threads=4, out_codec=self.codec, min_base_quality=self.minq,
                  device_ids=self.device_ids)
        for k, v in self.extra.items():
            kw[k] = str(d / v[1:]) if isinstance(v, str) and v.startswith("@") else v
        if sel is not None:
            kw["taxon_outs"] = [(s, str(d / ("t%d_1%s" % (i, EXT[self.codec]))), str(d / ("t%d_2%s" % (i, EXT[self.codec]))) if self.in2 else None)
                                for i, s in enumerate(sel)]
        errf = self.tmp / ("%s_%s.stderr" % (self.name, tag))
        st = _run(errf, db=self.db, **kw)
        return d, st, errf.read_bytes().decode(errors="replace")

    def check(self, sel):
        """a run with the selectors `sel`: its per-taxon files are the model's, everything else the reference run's"""
        self.runs += 1
        with Env(self.env):
            d, st, err = self._one("s%d" % self.runs, sel)
        want_counts = None
        built = 0
        for mi, m in enumerate(self.mates):
            files, counts = tm.partition(self.keep[mi], self.fastq, self.parent, sel)
            assert want_counts in (None, counts)
            want_counts = counts
            for i in range(len(sel)):
                got = _read(d / ("t%d_%s%s" % (i, m, EXT[self.codec])), self.codec)
                assert got == files[i], (self.name, sel, "selector", i, "mate", m, len(got), len(files[i]))
                built += len(got)
        assert st.taxon_fragments == want_counts, (self.name, sel)
        theirs = {p.name for p in d.iterdir() if not re.match(r"t\d_[12]\.", p.name)}
        assert theirs == {p.name for p in self.ref_dir.iterdir()}, (self.name, sel)
        for f in sorted(theirs):
            a, b = (d / f).read_bytes(), (self.ref_dir / f).read_bytes()
            if f.endswith((".gz", ".zst")):
                a, b = _read(d / f, self.codec), _read(self.ref_dir / f, self.codec)
            assert a == b, (self.name, sel, f)
        assert _stats(st) == _stats(self.ref) == _stats(self.keep_stats), (self.name, sel)
        m = TRACE.findall(err)
        assert len(m) == 1, err[-3000:]
        trace = tuple(int(x) for x in m[0])
        assert trace[0] == sum(want_counts) and trace[1] == built, (self.name, sel, trace, want_counts, built)
        return want_counts, trace


def _golden(paired):
    if paired:
        return os.path.join(GOLD, "reads_pe_1.fq"), os.path.join(GOLD, "reads_pe_2.fq")
    return os.path.join(GOLD, "reads_se.fq"), None


# ---- 1. the goldens

@pytest.mark.parametrize("paired", [False, True])
def test_golden_reads_with_and_without_other(tmp_path, paired):
    in1, in2 = _golden(paired)
    c = Case(tmp_path, "g", in1, in2)
    counts, _ = c.check(SEL4)
    assert all(counts) and sum(counts) == c.ref.classified
    if not paired:
        assert counts == [78, 51, 10, 112]
    assert c.check(SEL4[:3])[0] == counts[:3]
    assert c.check([1])[0] == [c.ref.classified]  # the root alone takes every classified read


# ---- 2. block and scan borders

@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    """reads drawn from the toy genomes with the taxid of their call (0: unclassified), classified once through the calls table"""
    from nohuman_amd import engine
    d = tmp_path_factory.mktemp("pool")
    rng = np.random.default_rng(20)
    reads = synth.sample_reads(rng, synth.toy_db()[3], 6000, length=60, len_jitter=12)
    (d / "pool.fq").write_bytes(b"".join(b"@p%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    engine.run(DB, str(d / "pool.fq"), str(d / "o.fq"), calls=str(d / "calls.tsv"), threads=4)
    calls = [int(ln.split(b"\t")[2]) for ln in (d / "calls.tsv").read_bytes().splitlines()]
    assert len(calls) == len(reads)
    by = {}
    for r, c in zip(reads, calls):
        by.setdefault(c, []).append(r)
    for c in (0, 1, 10, 11, 12, 20, 21, 9606, 111):
        assert len(by.get(c, [])) >= 20, (c, {k: len(v) for k, v in by.items()})
    return by


def _designed(pool, n):
    """n reads: clade 10 without 11 / clade 11 / unclassified / root and 20 in turn, no call at 112; the only read at 9606 is the
    last of block 0, the only one at 21 the first of block 1"""
    turn = [pool[10] + pool[12], pool[11] + pool[111], pool[0], pool[1] + pool[20]]
    out = []
    for i in range(n):
        src = pool[9606] if i == HB_FRAGS - 1 else pool[21] if i == HB_FRAGS else turn[i % 4]
        r = src[(i // 4) % len(src)]
        out.append(b"@d%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)))
    return b"".join(out)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_block_and_scan_borders(tmp_path, pool, n):
    p = tmp_path / "d.fq"
    p.write_bytes(_designed(pool, n))
    c = Case(tmp_path, "b", str(p))
    cls = c.ref.classified
    assert c.check([1])[0] == [cls]  # every classified read in one bin
    assert c.check([tm.OTHER])[0] == [cls]
    counts, _ = c.check([10, 11, tm.OTHER])  # bins alternating read by read
    assert sum(counts) == cls and (n < 8 or all(counts))
    counts, _ = c.check([9606, 21, 112, 10])  # one read at a block's end, one at the next block's start, a selector without reads
    assert counts[:3] == [int(n >= HB_FRAGS), int(n > HB_FRAGS), 0]


def test_no_classified_read_at_all(tmp_path, pool):
    p = tmp_path / "u.fq"
    p.write_bytes(b"".join(b"@u%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)) for i, r in enumerate((pool[0] * 4)[:1025])))
    for codec in (0, 2, 5, 4):
        c = Case(tmp_path, "u%d" % codec, str(p), codec=codec)
        counts, trace = c.check(SEL4)  # (every file is decoded by _read: empty and valid in its codec)
        assert counts == [0, 0, 0, 0] and trace[:2] == (0, 0) and c.ref.classified == 0


# ---- 3. alignment

def _aligned(fasta, kinds):
    """ids of 1..9 bytes x sequences of 35..43 bases cut from the toy genomes; kinds: the record shapes in turn"""
    g = synth.toy_db()[3]
    keys = sorted(g)
    out = []
    i = 0
    for idlen in range(1, 10):
        for slen in range(35, 44):
            genome = g[keys[i % len(keys)]]
            st = 401 * (i % 3) + 7 * (i % 40)  # inside one segment of the genome (segments of 400 bases and an N between)
            s = genome[st:st + slen]
            assert len(s) == slen and b"N" not in s
            name = (b"%d" % i).rjust(idlen, b"x")[-idlen:]
            kind = kinds[i % len(kinds)]
            nl = b"\r\n" if kind == "crlf" else b"\n"
            if fasta:
                out.append(b">" + name + nl + s + nl)
            else:
                out.append(b"@" + name + nl + s + nl + (b"+" + name if kind == "plusid" else b"+") + nl + b"G" * slen + nl)
            i += 1
    return b"".join(out)


@pytest.mark.parametrize("fasta", [False, True])
def test_every_alignment_of_record_start_and_fields(tmp_path, fasta):
    """minimum_hit_groups 1, so that reads of one to nine k-mers are classified"""
    p = tmp_path / ("al.fa" if fasta else "al.fq")
    p.write_bytes(_aligned(fasta, ("plain", "crlf") if fasta else ("plain", "crlf", "plusid")))
    c = Case(tmp_path, "al", str(p), fasta=fasta, env={"NOHUMAN_OPT_MIN_HIT_GROUPS": "1"})
    assert c.ref.classified >= 60, c.ref.classified
    for sel in ([1], [10, 20], [11, 12, 21, 9606, tm.OTHER]):
        c.check(sel)
    # the starts of the records inside the one bin of [1]: every alignment, and the text as the keep_human run normalised it
    starts, at = set(), 0
    for rec in tm.records(c.keep[0], not fasta):
        starts.add(at % 4)
        at += len(rec)
    assert starts == {0, 1, 2, 3} and b"\r" not in c.keep[0] and (fasta or b"\n+\n" in c.keep[0])


# ---- 4. several batches and slots

def test_several_batches(tmp_path, pool):
    p = tmp_path / "d.fq"
    p.write_bytes(_designed(pool, 2049))
    c = Case(tmp_path, "bt", str(p), env={"NOHUMAN_BATCH_FRAGS": "400"})  # six batches
    counts, _ = c.check([10, 11, 9606, 21, tm.OTHER])
    assert all(counts)
    c = Case(tmp_path, "bt2", str(p), codec=2, env={"NOHUMAN_BATCH_FRAGS": "400"})
    c.check([10, 11, 9606, 21, tm.OTHER])


def bins_end(sizes):
    """where the last bin that has bytes ends in a mate's buffer of one batch: every bin starts at the next multiple of 256 bytes
    behind the end of the bin before it (k_tout_scan).  With a host codec that is what the run fetches of the buffer"""
    at = end = 0
    for n in sizes:
        at = (at + 255) & ~255
        if n:
            end = at + n
        at += n
    return end


def test_more_than_256_blocks_with_eight_selectors(tmp_path, pool):
    """258 blocks in one batch and the largest number of selectors: scan_block_sums takes 256 block sums a round, so every bin's
    second round starts with the sum carried over from its first (the size of test_gpu_builders.py's
    test_more_than_256_blocks_in_one_batch; the one case here that takes more than a few seconds)"""
    n = 262144 + 1025
    p = tmp_path / "d.fq"
    p.write_bytes(_designed(pool, n))
    c = Case(tmp_path, "wide", str(p), env={"NOHUMAN_BATCH_FRAGS": "270000"})
    sel = [10, 11, 12, 111, 20, 21, 9606, tm.OTHER]
    counts, trace = c.check(sel)
    assert counts[5] == counts[6] == 1 and all(counts) and sum(counts) == c.ref.classified
    files, _ = tm.partition(c.keep[0], True, PARENT, sel)
    assert trace[2] == bins_end([len(f) for f in files])  # the eight bins' starts in the one batch's buffer
    assert (n + HB_FRAGS - 1) // HB_FRAGS == 258


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.argv = ["x"]
import pathlib
from tests import test_gpu_taxon_out as t
tmp = pathlib.Path(%(tmp)r)
for codec in (0, 2):
    c = t.Case(tmp, "two_%%d" %% codec, %(in1)r, None, codec=codec, device_ids=(0, 1))
    print("COUNTS", codec, c.check([10, 11, 9606, 21, "other"]))
print("CHILD OK")
"""


def test_two_logical_devices(tmp_path, pool):
    p = tmp_path / "d.fq"
    p.write_bytes(_designed(pool, 2049))
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="400")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), in1=str(p))
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "CHILD OK" in out.stdout
    assert "DEVICE DISCIPLINE" not in out.stderr


# ---- 5. codecs

@pytest.mark.parametrize("codec", [0, 2, 5, 4])
@pytest.mark.parametrize("paired", [False, True])
def test_codecs(tmp_path, codec, paired):
    in1, in2 = _golden(paired)
    c = Case(tmp_path, "c", in1, in2, codec=codec)
    _, trace = c.check(SEL4)
    if codec in (2, 5):
        assert trace[2] == 0  # the GPU encoders take the bins' spans from HBM
    else:
        assert trace[2] >= trace[1] > 0  # host codecs: the built text is fetched (with the gaps between the bins)


# ---- 6. one long read

def test_one_long_read_beside_short_ones(tmp_path, pool):
    g = synth.toy_db()[3]
    long_read = (g[111] * (300_000 // len(g[111]) + 1))[:300_000]
    recs = [b"@s%d\n%s\n+\n%s\n" % (i, r, b"F" * len(r)) for i, r in enumerate((pool[111] + pool[11] + pool[12])[:60])]
    recs.insert(30, b"@long\n%s\n+\n%s\n" % (long_read, b"5" * len(long_read)))
    p = tmp_path / "long.fq"
    p.write_bytes(b"".join(recs))
    for codec in (0, 2):
        c = Case(tmp_path, "l%d" % codec, str(p), codec=codec)
        counts, trace = c.check([11, 12])
        assert trace[1] > 300_000 and counts[0] >= 2


# ---- 7. everything at once

def test_everything_at_once(tmp_path):
    in1, in2 = _golden(True)
    extra = dict(mask=True, human_out1="@h1.fq", human_out2="@h2.fq", calls="@calls.tsv", human_ids="@ids.txt", read_stats="@rs.tsv")
    c = Case(tmp_path, "all", in1, in2, extra=extra, minq=10)
    counts, _ = c.check(SEL4)
    assert all(counts)
    for f in ("h1.fq", "h2.fq", "calls.tsv", "ids.txt", "rs.tsv", "k.txt", "r.txt", "o1.fq", "o2.fq"):
        assert (c.ref_dir / f).exists(), f


# ---- 8. a taxid the taxonomy does not hold

def test_unknown_taxid_is_refused_before_anything_is_written(tmp_path):
    from nohuman_amd import engine
    in1, in2 = _golden(True)
    d = tmp_path / "bad"
    d.mkdir()
    with pytest.raises(engine.EngineError) as ei:
        engine.run(DB, in1, str(d / "o1.fq"), in2=in2, out2=str(d / "o2.fq"), kraken_output=str(d / "k.txt"), report=str(d / "r.txt"),
                   calls=str(d / "c.tsv"), taxon_outs=[(10, str(d / "a1.fq"), str(d / "a2.fq")), (4242, str(d / "b1.fq"), str(d / "b2.fq"))])
    assert ei.value.code == -1 and "4242" in str(ei.value)
    assert list(d.iterdir()) == []


# ---- 9. the CLI

@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_end_to_end(tmp_path):
    in1, in2 = _golden(True)
    d = tmp_path
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)

    def cli(args):
        r = subprocess.run([BIN, "--db", DB, "-t", "4"] + args, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stderr
    cli(["-H", "-o", str(d / "h_1.fq"), "-O", str(d / "h_2.fq"), in1, in2])
    cli(["-o", str(d / "n_1.fq"), "-O", str(d / "n_2.fq"), in1, in2])
    err = cli(["-o", str(d / "s_1.fq"), "-O", str(d / "s_2.fq"), "--taxon-out", "10:" + str(d / "a#.fq"), "--taxon-out", "other:" + str(d / "o#.fq"),
               in1, in2])
    for m in ("1", "2"):
        files, counts = tm.partition((d / ("h_%s.fq" % m)).read_bytes(), True, PARENT, [10, tm.OTHER])
        assert (d / ("a_%s.fq" % m)).read_bytes() == files[0] and (d / ("o_%s.fq" % m)).read_bytes() == files[1]
        assert (d / ("s_%s.fq" % m)).read_bytes() == (d / ("n_%s.fq" % m)).read_bytes()
    assert all(counts)
    assert 'Taxon 10 (' in err and '): %d reads written to: "%s" "%s"' % (counts[0], d / "a_1.fq", d / "a_2.fq") in err
    assert 'Taxon other' in err and ': %d reads written to: "%s" "%s"' % (counts[1], d / "o_1.fq", d / "o_2.fq") in err
    assert not any(p.name.endswith(".partial") for p in d.iterdir())
