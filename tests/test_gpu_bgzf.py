"""BGZF output on the GPU (NH_CODEC_BGZF = 5; the BGZF mode of the encoder in nohuman_amd/csrc/nh_deflate.hip): every file is
walked member by member by the parser of tests/bgzf_util.py, compared with the host encoder's member boundaries, read back by
this repo's own GPU reader, and every kind of run is compared with its plain-text twin."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

from nohuman_amd import _lib
from tests import bgzf_util, deflate_pins
from tests.test_bgzf_host import NAMES, host_bgzf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DB = os.path.join(GOLD, "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
BGZF = 5


@pytest.fixture(scope="module")
def texts(tmp_path_factory, toy):
    return bgzf_util.corpus(tmp_path_factory.mktemp("bgzf_corpus"), toy[3])


def gpu_bgzf(data, path):
    L = _lib.lib()
    stats = (C.c_uint64 * 2)()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    rc = L.nh_bgzf_gpu_file(0, buf, len(data), os.fsencode(str(path)), stats)
    assert rc == 0, L.nh_last_error().decode()
    assert os.path.getsize(path) == stats[0]
    raw = open(path, "rb").read()
    # the file is the one the encoder's host model writes in its BGZF mode (ways, price choice and chunk size from the environment)
    deflate_pins.assert_equals_model(raw, data, os.environ.get("PYTEST_CURRENT_TEST", str(path)), "the environment's, BGZF",
                                     **deflate_pins.encoder_options(bgzf=True))
    return raw


@pytest.mark.parametrize("name", NAMES)
def test_gpu_encoder_writes_what_bgzip_writes(tmp_path, texts, name):
    data = texts[name]
    raw = gpu_bgzf(data, tmp_path / "g.gz")
    sizes = bgzf_util.check_bgzf(raw, data)
    if not data:
        assert raw == bgzf_util.EOF_MEMBER
    # the same member boundaries as the host encoder's
    assert sizes == bgzf_util.check_bgzf(host_bgzf(tmp_path, data, 2), data)
    if name == "random":
        # stored blocks: two a member (5 bytes each), the closing block (5), a byte of padding, 26 of framing; the EOF member
        assert len(raw) <= len(data) + len(sizes) * (2 * 5 + 5 + 1 + 26) + 28, len(raw) - len(data)


def test_chunk_boundary_makes_no_short_member(tmp_path, monkeypatch, texts):
    """Two chunks (NOHUMAN_GZIP_CHUNK_MB=64, the smallest): the chunk is cut down to whole regions, so the member that ends the
    first chunk is a full one."""
    monkeypatch.setenv("NOHUMAN_GZIP_CHUNK_MB", "64")
    n = (64 << 20) + 100_000
    fq = texts["fastq"]
    data = (fq * (n // len(fq) + 1))[:n]
    raw = gpu_bgzf(data, tmp_path / "big.gz")
    sizes = bgzf_util.check_bgzf(raw, data)  # (no short member before the last, text equal)
    assert len(sizes) + 1 == -(-n // 65280) + 1 == len(bgzf_util.members(raw))


def test_own_gpu_reader_takes_the_file_by_its_headers(tmp_path, texts):
    """The encoder's members hold several deflate blocks (bgzip's hold one): the reader's header-driven path decodes them with no
    chunk decoded again and no piece left to the host decoder."""
    data = texts["fastq"]
    raw = gpu_bgzf(data, tmp_path / "g.gz")
    n_members = len(bgzf_util.members(raw))
    st = (C.c_uint64 * 8)()
    L = _lib.lib()
    rc = L.nh_gunzip_device_file(os.fsencode(str(tmp_path / "g.gz")), os.fsencode(str(tmp_path / "g.txt")), 0, 0, 0, st)
    assert rc == 0, L.nh_last_error().decode()
    assert (tmp_path / "g.txt").read_bytes() == data
    assert (st[4], st[2], st[3]) == (n_members, 0, 0), list(st)  # members, chunks decoded again, pieces by the host decoder
    assert st[1] > 1  # more than one chunk: the starts did come from the headers
    # several pieces: a piece's end falls among the blocks of a member; the text and the members' checks stay the same
    for seg, stretch in ((200_000, 8192), (64_000, 32768)):
        rc = L.nh_gunzip_device_file(os.fsencode(str(tmp_path / "g.gz")), os.fsencode(str(tmp_path / "g.txt")), 0, seg, stretch, st)
        assert rc == 0, L.nh_last_error().decode()
        assert (tmp_path / "g.txt").read_bytes() == data and (st[4], st[5]) == (n_members, len(data)), list(st)


# ---- whole runs ---------------------------------------------------------------------------------------------------------
KINDS = {  # name: (keywords of the run, human outputs?)
    "normal": (dict(), False),
    "keep_human": (dict(keep_human=True), False),
    "split": (dict(), True),
    "mask": (dict(mask=True), False),
    "mask_human": (dict(mask=True), True),
}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_inputs")
    out = {}
    for m in ("1", "2"):
        raw = open(os.path.join(GOLD, "reads_pe_%s.fq" % m), "rb").read() * 12
        (d / ("r_%s.fq" % m)).write_bytes(raw)
        (d / ("r_%s.fq.gz" % m)).write_bytes(gzip.compress(raw, 6))
        out["plain" + m] = str(d / ("r_%s.fq" % m))
        out["gz" + m] = str(d / ("r_%s.fq.gz" % m))
    return out


def _stats(st):
    return (st.total_sequences, st.classified, st.unclassified, st.total_bases, st.table_lookups)


def _one_run(eng, d, in1, in2, codec, kw, human, want_k):
    d.mkdir()
    ext = ".fq.gz" if codec == BGZF else ".fq"
    p = {x: str(d / (x + ext)) for x in ("o1", "o2") + (("h1", "h2") if human else ())}
    k, r = str(d / "k.txt"), str(d / "r.txt")
    extra = dict(human_out1=p["h1"], human_out2=p["h2"]) if human else {}
    st = eng.run(in1, p["o1"], in2=in2, out2=p["o2"], kraken_output=k if want_k else None, report=r, threads=4, out_codec=codec,
                 codec_threads=2, **kw, **extra)
    files = {x: open(f, "rb").read() for x, f in p.items()}
    return files, _stats(st), open(k, "rb").read() if want_k else b"", open(r, "rb").read()


def _both_codecs(tmp_path, in1, in2, kind, want_k=True):
    """the run with BGZF outputs and with plain ones: every BGZF file well-formed and the plain file's bytes inside"""
    from nohuman_amd import Engine
    kw, human = KINDS[kind]
    with Engine.open(DB) as eng:
        plain = _one_run(eng, tmp_path / "plain", in1, in2, 0, kw, human, want_k)
        blocked = _one_run(eng, tmp_path / "bgzf", in1, in2, BGZF, kw, human, want_k)
    assert sorted(plain[0]) == sorted(blocked[0])
    for x, raw in blocked[0].items():
        bgzf_util.check_bgzf(raw, plain[0][x])
    assert blocked[1:] == plain[1:], kind  # stats, -k lines, report
    assert 0 < plain[1][1] < plain[1][0]
    assert sum(len(t) for t in plain[0].values()) > 100_000
    return blocked[0]


@pytest.mark.parametrize("kind", list(KINDS))
def test_runs_with_bgzf_outputs_equal_plain_runs(tmp_path, monkeypatch, inputs, kind):
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "1000")
    _both_codecs(tmp_path, inputs["plain1"], inputs["plain2"], kind)


@pytest.mark.parametrize("kind", list(KINDS))
def test_runs_fed_by_the_gpu_readers_device_only_batches(tmp_path, monkeypatch, capfd, inputs, kind):
    """gzip inputs through the reader on the GPU, no -k file: the batches' text exists in HBM only and the encoder takes its
    spans from there"""
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "1000")
    monkeypatch.setenv("NOHUMAN_GZ_READER", "device")
    monkeypatch.setenv("NOHUMAN_TRACE", "1")
    _both_codecs(tmp_path, inputs["gz1"], inputs["gz2"], kind, want_k=False)
    assert "gzip reader on GPU" in capfd.readouterr().err


@pytest.mark.parametrize("kind", list(KINDS))
def test_runs_with_the_host_encoder(tmp_path, monkeypatch, inputs, kind):
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "1000")
    monkeypatch.setenv("NOHUMAN_GZIP", "host")
    _both_codecs(tmp_path, inputs["plain1"], inputs["plain2"], kind)


def test_bgzf_outputs_of_a_human_run_come_back_as_inputs(tmp_path, monkeypatch, capfd, inputs):
    """-H with BGZF outputs, then those files as the inputs of a second run (through the reader on the GPU): the same records and
    counters as from the plain-text outputs of the same -H run"""
    from nohuman_amd import Engine
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "1000")
    first = {}
    with Engine.open(DB) as eng:
        for codec, ext in ((0, ".fq"), (BGZF, ".fq.gz")):
            o1, o2 = str(tmp_path / ("h_1" + ext)), str(tmp_path / ("h_2" + ext))
            eng.run(inputs["plain1"], o1, in2=inputs["plain2"], out2=o2, keep_human=True, threads=4, out_codec=codec)
            first[codec] = (o1, o2)
        for o, want in zip(first[BGZF], first[0]):
            bgzf_util.check_bgzf(open(o, "rb").read(), open(want, "rb").read())
        second = {}
        for codec in (0, BGZF):
            d = tmp_path / ("second_%d" % codec)
            d.mkdir()
            if codec == BGZF:
                monkeypatch.setenv("NOHUMAN_GZ_READER", "device")
                monkeypatch.setenv("NOHUMAN_TRACE", "1")
                capfd.readouterr()
            st = eng.run(first[codec][0], str(d / "o1.fq"), in2=first[codec][1], out2=str(d / "o2.fq"), kraken_output=str(d / "k.txt"),
                         report=str(d / "r.txt"), keep_human=True, threads=4)
            second[codec] = (_stats(st),) + tuple((d / f).read_bytes() for f in ("o1.fq", "o2.fq", "k.txt", "r.txt"))
        err = capfd.readouterr().err
    assert "gzip reader on GPU" in err and "0 pieces by the host decoder" in err, err[-1500:]
    assert second[BGZF] == second[0]
    assert second[0][0][1] > 0 and len(second[0][1]) > 100_000


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_bgzf_on_gzip_inputs(tmp_path, inputs):
    """`nohuman --bgzf` with the format resolved from the gzip inputs: default names, .gz extension, BGZF inside"""
    for m in ("1", "2"):  # (the fixtures' text twice: the kept reads of one copy fill a member and a half, short of the size asked for below)
        (tmp_path / ("s_%s.fq.gz" % m)).write_bytes(gzip.compress(open(inputs["plain" + m], "rb").read() * 2, 6))
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    base = ["-D", DB, "-t", "4", str(tmp_path / "s_1.fq.gz"), str(tmp_path / "s_2.fq.gz")]
    r = subprocess.run([BIN, "--bgzf"] + base, cwd=tmp_path, env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([BIN, "-F", "u", "-o", str(tmp_path / "p_1.fq"), "-O", str(tmp_path / "p_2.fq")] + base, cwd=tmp_path, env=e,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for m in ("1", "2"):
        want = (tmp_path / ("p_%s.fq" % m)).read_bytes()
        assert len(want) > 100_000
        bgzf_util.check_bgzf((tmp_path / ("s_%s.nohuman.fq.gz" % m)).read_bytes(), want)
