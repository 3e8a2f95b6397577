"""Whole runs with BAM output (out_codec = NH_CODEC_BAM) on a forged BAM of toy-database reads -- tags of several kinds on most
records (a B array, a Z tag of a few hundred bytes), reverse-strand records, absent qualities, secondary, supplementary and empty
records in between, a header with @PG and @RG lines and two references -- against tests/bamout_model.py: the inflated outputs are
the model's streams for the host flags of the SAME input's FASTQ-codec run (its --calls file), every other output is byte for byte
that run's.  Batches of 100 fragments, the input in BGZF members of 4000 bytes, every configuration in a child process."""
import gzip
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_model as bm
from tests import bamout_model as bo
from tests import bgzf_util
from tests import host_model as hm
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
N_READS = 700
OTHERS = ("calls", "ids", "rs", "k", "r")  # the outputs that are no record outputs
HEADER_TEXT = (b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:run1\tPL:ONT\tDS:basecall_model=sup@v5\n@RG\tID:run2\tPL:ONT\n"
               b"@PG\tID:basecaller\tPN:dorado\tVN:0.9\n@SQ\tSN:chrT\tLN:5000\n@SQ\tSN:chrU\tLN:70000\n")

CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
spec = json.load(open(sys.argv[1]))
res = {}
for r in spec["runs"]:
    d = r["dir"]
    os.mkdir(d)
    p = lambda x: os.path.join(d, x)
    kw = dict(calls=p("calls"), human_ids=p("ids"), read_stats=p("rs"), kraken_output=p("k"), report=p("r"), threads=4,
              device_ids=spec["ids"], out_codec=r["codec"], codec_threads=2, keep_human=bool(r.get("keep_human")))
    if r.get("split"):
        kw["human_out1"] = p("h")
    if r.get("host"):
        kw["host_taxids"] = r["host"]
    st = engine.run(%(db)r, r["in1"], p("o"), **kw)
    res[r["name"]] = [st.total_sequences, st.classified, st.unclassified]
print("RESULT " + json.dumps(res))
"""


def forged_stream(genomes, n=N_READS, seed=3, only=None):
    """-> (the BAM stream of n toy-database reads with what a BAM may hold in between; only: the indices of the reads that are kept in)"""
    rng = np.random.default_rng(seed)
    reads = synth.sample_reads(rng, genomes, n, lower_rate=0.0, len_jitter=60)
    recs = []
    for i, s in enumerate(reads):
        s = s or b"A"
        flag = bm.REVERSE if i % 3 == 1 else 0
        qual = None if i % 11 == 5 else rng.integers(2, 42, len(s), dtype=np.uint8).tobytes()
        ml = rng.integers(0, 256, 3 + i % 40, dtype=np.uint8).tobytes()
        mv = rng.integers(0, 2, 10 + 3 * (i % 90), dtype=np.uint8).tobytes()
        tags = [b"qsi" + struct.pack("<i", 9 + i % 20),
                b"RGZrun%d\0" % (1 + i % 2) + b"chi" + struct.pack("<i", i % 512),
                b"MMZC+m," + b",".join(b"%d" % (j % 7) for j in range(3 + i % 40)) + b";\0MLBC" + struct.pack("<I", len(ml)) + ml,
                b"mvBc" + struct.pack("<I", len(mv)) + mv + b"stZ2026-01-01T00:00:%02d.000+00:00\0" % (i % 60),
                b"duf" + struct.pack("<f", 0.25 * i) + b"XZZ" + bytes(65 + (j * 7 + i) % 26 for j in range(200 + i % 150)) + b"\0"]
        chosen_tags = b"".join(t for k, t in enumerate(tags) if (i >> k) & 1 or i % 5 == k) if i % 8 else b""
        rec = bm.forge_record(b"read%d/%d ch=%d" % (i, i % 7, i % 512) if i % 2 else b"r%d" % i, s, qual, flag=flag | 0x4, tags=chosen_tags, pad=0)
        if only is None or i in only:
            recs.append(rec)
        if i % 9 == 0:
            recs.append(bm.forge_record(b"sec%d" % i, s[:50], None, flag=bm.SECONDARY, cigar=[(len(s[:50]) << 4)], tags=b"NMC\x02"))
        if i % 13 == 0:
            recs.append(bm.forge_record(b"sup%d" % i, s[:30], bytes(len(s[:30])), flag=bm.SUPPLEMENTARY | bm.REVERSE))
        if i % 17 == 0:
            recs.append(bm.forge_record(b"empty%d" % i, b"", b"", tags=b"qsi\x01\0\0\0"))
    return bm.forge_header(HEADER_TEXT, [(b"chrT", 5000), (b"chrU", 70000)]) + b"".join(recs)


def child(tmp, tag, runs, ids=(0,), env=None):
    """the runs in one child process -> ({name: [total, classified, unclassified]}, the child's stderr)"""
    for r in runs:
        r["dir"] = str(tmp / (tag + "_" + r["name"]))
    spec = tmp / (tag + ".json")
    spec.write_text(json.dumps(dict(runs=runs, ids=list(ids))))
    e = dict(os.environ, NOHUMAN_BATCH_FRAGS="100", NOHUMAN_RCCL="0", NOHUMAN_TRACE="1", **(env or {}))
    for k in ("NOHUMAN_GZ_READER", "NOHUMAN_BAM_SPAN"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, db=DB), str(spec)], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.split("RESULT ")[1]), out.stderr


def rd(tmp, tag, name, f):
    return (tmp / (tag + "_" + name) / f).read_bytes()


def host_flags(calls_file, hostmap=None):
    """the host flag of every fragment from a --calls table: classified, or -- a selection -- classified into a host clade"""
    rows = [ln.split(b"\t") for ln in calls_file.splitlines()]
    return [int(r[2]) != 0 if hostmap is None else hm.is_host(int(r[2]), hostmap) for r in rows]


def check_bam(raw, want_stream):
    """a written BAM file: BGZF framing with consistent sizes, the EOF member last, the inflated stream"""
    bgzf_util.check_bgzf(raw, want_stream)
    assert raw[-28:] == bgzf_util.EOF_MEMBER
    assert gzip.decompress(raw) == want_stream


SPLIT = dict(split=True)
RUNS = [dict(name="fq_split", codec=0, **SPLIT), dict(name="fq_keep", codec=0, keep_human=True), dict(name="fq_plain", codec=0),
        dict(name="bam_split", codec=6, **SPLIT), dict(name="bam_keep", codec=6, keep_human=True), dict(name="bam_plain", codec=6),
        dict(name="fq_sel", codec=2, host=[9606], **SPLIT), dict(name="bam_sel", codec=6, host=[9606], **SPLIT)]


@pytest.fixture(scope="module")
def base(tmp_path_factory, toy):
    """the input, and the default configuration's runs on it, made once: FASTQ-codec and BAM-codec, split / keep_human / plain, and
    a split run with a host selection; then the round trip of the non-host BAM"""
    tmp = tmp_path_factory.mktemp("bamout_run")
    stream = forged_stream(toy[3])
    _, counts, _, keep = bm.to_fastq(stream)
    assert counts.reads == N_READS and counts.skipped_secondary > 50 and counts.skipped_empty > 20
    assert counts.reverse_complemented > 200 and counts.missing_qualities > 40
    sizes = [4 + r.block_size for r in keep]
    assert max(sizes) > 700 and {s % 4 for s in sizes} == {0, 1, 2, 3}
    assert sum(1 for r in keep if b"MLBC" in stream[r.offset:r.offset + 4 + r.block_size]) > 200
    bam = tmp / "reads.bam"
    bam.write_bytes(bm.bgzf(stream, 4000))
    runs = [dict(r, in1=str(bam)) for r in RUNS]
    runs.append(dict(name="round_trip", codec=0, in1=str(tmp / "d_bam_split" / "o")))
    stats, err = child(tmp, "d", runs)
    return dict(tmp=tmp, stream=stream, bam=str(bam), stats=stats, err=err, counts=counts)


def check_against_fastq_run(base, tmp, tag, stats, sel=False):
    """the BAM-codec runs of a configuration (made by `tag`'s child) against the model and the default configuration's FASTQ runs"""
    stream, ref = base["stream"], base["tmp"]
    flags = host_flags(rd(ref, "d", "fq_split", "calls"))
    assert 100 < sum(flags) < N_READS - 100
    for name, fq, outs in (("bam_split", "fq_split", (("o", False), ("h", True))), ("bam_keep", "fq_keep", (("o", True),)),
                           ("bam_plain", "fq_plain", (("o", False),))):
        for f, want in outs:
            check_bam(rd(tmp, tag, name, f), bo.select(stream, flags, want))
        for f in OTHERS:
            assert rd(tmp, tag, name, f) == rd(ref, "d", fq, f), (tag, name, f)
        assert stats[name] == base["stats"][fq] and stats[name][0] == N_READS
    if sel:
        hostmap = hm.host_of(dict(synth.TOY_EDGES), [9606])
        every, chosen = host_flags(rd(ref, "d", "fq_sel", "calls")), host_flags(rd(ref, "d", "fq_sel", "calls"), hostmap)
        assert every == flags and 0 < sum(chosen) < sum(every)  # (the selection spares classified reads)
        check_bam(rd(tmp, tag, "bam_sel", "o"), bo.select(stream, chosen, False))  # the spared records land in out1
        check_bam(rd(tmp, tag, "bam_sel", "h"), bo.select(stream, chosen, True))
        for f in OTHERS:
            assert rd(tmp, tag, "bam_sel", f) == rd(ref, "d", "fq_sel", f), (tag, f)
        assert stats["bam_sel"] == base["stats"]["fq_sel"]


def test_split_keep_human_and_plain_runs_and_a_host_selection(base):
    check_against_fastq_run(base, base["tmp"], "d", base["stats"], sel=True)
    # the two outputs of the split run are a partition of the kept records, the skipped ones are in neither
    o, h = (bm.records(gzip.decompress(rd(base["tmp"], "d", "bam_split", f))) for f in ("o", "h"))
    assert len(o) + len(h) == N_READS and all(bm.kept(r) for r in o + h)
    assert "bam-out: " in base["err"] and "DEVICE DISCIPLINE" not in base["err"]


def test_only_runs_with_bam_output_trace_the_builder(base):
    """the builder's trace line: one a BAM-codec run, none for the FASTQ-codec runs of the same input (nothing of it runs there)"""
    n_bam = sum(1 for r in RUNS if r["codec"] == 6)
    assert base["err"].count("[nohuman trace] bam-out: ") == n_bam
    assert base["err"].count("[nohuman trace] wall ") == len(RUNS) + 1


def test_round_trip_the_written_bam_is_read_again(base):
    import nohuman_amd
    tmp, stream = base["tmp"], base["stream"]
    flags = host_flags(rd(tmp, "d", "fq_split", "calls"))
    for f, want in (("o", False), ("h", True)):
        info = nohuman_amd.bam_scan(str(tmp / "d_bam_split" / f))
        c = bm.to_fastq(bo.select(stream, flags, want))[1]
        assert tuple(info[:7]) == tuple(c), (f, info, c)
        assert info.skipped_secondary == info.skipped_empty == 0 and info.records == info.reads == sum(1 for x in flags if x == want)
    # the non-host file as in1: every call unclassified, every read written again
    n = flags.count(False)
    assert base["stats"]["round_trip"] == [n, 0, n]
    rows = rd(tmp, "d", "round_trip", "calls").splitlines()
    assert len(rows) == n and all(r.startswith(b"U\t") for r in rows)
    assert rd(tmp, "d", "round_trip", "o") == bm.to_fastq(bo.select(stream, flags, False))[0]


def test_nothing_selected_is_header_and_eof(base, toy):
    tmp = base["tmp"]
    flags = host_flags(rd(tmp, "d", "fq_split", "calls"))
    runs = []
    streams = {}
    for name, want in (("all_host", True), ("no_host", False)):
        streams[name] = forged_stream(toy[3], only={i for i, h in enumerate(flags) if h == want})
        p = tmp / (name + ".bam")
        p.write_bytes(bm.bgzf(streams[name], 4000))
        runs.append(dict(name=name, codec=6, in1=str(p), keep_human=not want, split=False))
        runs.append(dict(name=name + "_split", codec=6, in1=str(p), split=True))
    stats, _ = child(tmp, "n", runs)
    for name, want in (("all_host", True), ("no_host", False)):
        s = streams[name]
        n = flags.count(want)
        assert stats[name] == [n, n if want else 0, 0 if want else n]
        raw = rd(tmp, "n", name, "o")
        check_bam(raw, bo.header_bytes(s))  # the one output of the run: nothing selected
        assert len(bgzf_util.members(raw)) == 2 and bm.records(gzip.decompress(raw)) == []
        # the split run of the same input: one side everything, the other the header and the EOF member
        full, empty = ("h", "o") if want else ("o", "h")
        check_bam(rd(tmp, "n", name + "_split", empty), bo.header_bytes(s))
        check_bam(rd(tmp, "n", name + "_split", full), bo.select(s, [want] * n, want))


@pytest.mark.parametrize("tag,env,ids", [("host_gzip", {"NOHUMAN_GZIP": "host"}, (0,)), ("chunk7", {"NOHUMAN_BAM_CHUNK": "7"}, (0,)),
                                         ("two_devices", {"NOHUMAN_FAKE_DEVICES": "2", "NOHUMAN_DEBUG_DEVICE": "1"}, (0, 1))])
def test_the_same_bytes_under_other_configurations(base, tag, env, ids):
    """the host's BGZF encoder; a reader window that refills inside records; two logical devices under the discipline checker"""
    runs = [dict(r, in1=base["bam"]) for r in RUNS if r["name"] in ("bam_split", "bam_keep", "bam_plain", "bam_sel")]
    stats, err = child(base["tmp"], tag, runs, ids=ids, env=env)
    check_against_fastq_run(base, base["tmp"], tag, stats, sel=True)
    assert "DEVICE DISCIPLINE" not in err, [ln for ln in err.splitlines() if "DISCIPLINE" in ln][:3]


def test_cli(base, tmp_path):
    assert os.path.exists(BIN), "the CLI host is not built"
    stream = base["stream"]
    flags = host_flags(rd(base["tmp"], "d", "fq_split", "calls"))
    e = dict(os.environ, NOHUMAN_DEVICES="0")
    work = tmp_path / "w"
    work.mkdir()
    (work / "calls.bam").write_bytes(open(base["bam"], "rb").read())
    # the default name
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--bam-out", str(work / "calls.bam")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(work)) == ["calls.bam", "calls.nohuman.bam"]
    check_bam((work / "calls.nohuman.bam").read_bytes(), bo.select(stream, flags, False))
    # -o and --human-out1 together
    o, h = tmp_path / "kept.bam", tmp_path / "human.bam"
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--bam-out", "-o", str(o), "--human-out1", str(h), str(work / "calls.bam")], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    check_bam(o.read_bytes(), bo.select(stream, flags, False))
    check_bam(h.read_bytes(), bo.select(stream, flags, True))
    # without the flag the default name and the FASTQ stay (tests/test_gpu_bam_run.py pins them); --help mentions the flag
    hlp = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert "--bam-out" in hlp.stdout and "tags" in hlp.stdout
