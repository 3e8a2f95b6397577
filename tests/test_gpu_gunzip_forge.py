"""The gzip READER on the GPU (nh_gunzip_device_file / nohuman_amd/csrc/nh_gunzip.hip) on hand-forged DEFLATE streams
(tests/deflate_forge.py): the dialects zlib never writes, which reach what no zlib-made FASTQ stream is known to reach in
k_inflate3 -- the canonical walk for codes beyond the root tables on either side and on both, the fifth far match of a
window, long overlapping matches, far matches out of the markers, stored blocks of 0 and 65535 bytes, member headers with
names beyond 64 bytes -- and the malformed ones.  The forge keeps its valid cases inside the decoder's room (16 : 1 a
stretch), so no piece may go to the host decoder: a test that quietly lets the host do the work proves nothing.  And the
GPU ENCODER's streams (nh_deflate.hip), a third dialect, through the GPU reader."""
import gzip
import zlib

import numpy as np
import pytest

from tests import deflate_forge as forge
from tests.test_gpu_deflate import _mixture, fastq_text, gpu_gzip
from tests.test_gpu_gunzip import gunzip_dev
from tests.test_gpu_run import DB

pytestmark = pytest.mark.gpu

CORPUS = forge.corpus()
VALID = [c for c in CORPUS if c.text is not None]
INVALID = [c for c in CORPUS if c.text is None]
SHAPES = [(0, 0), (40_000, 2048), (64_000, 4096)]
# A distance that reaches before its member's first byte: the chunk the member starts in sees it (k_inflate3: fresh_member); a
# chunk that starts further on reports how far before its start it reached (ChunkDesc::reach) and the host holds that
# against the member's text so far.  These cases carry the CRC-32 of the text a reader produces that takes the window for
# granted, so nothing but that check refuses them.  The last one lies in a piece that the host decoder takes over (text beyond
# 16 : 1 follows it) at pieces of 40 KiB: host_piece() hands it no more window than the member has text.
REACH_BEFORE_MEMBER = ("distance_before_first_member", "distance_before_later_member", "distance_32768_at_32767_of_later_member",
                       "distance_before_member_behind_dense_text")


def run_case(tmp_path, case, seg, stretch):
    src, dst = tmp_path / "x.gz", tmp_path / "x.out"
    src.write_bytes(case.gz)
    st = gunzip_dev(src, dst, seg, stretch)
    return st, dst.read_bytes()


@pytest.mark.parametrize("seg,stretch", SHAPES)
@pytest.mark.parametrize("case", VALID, ids=lambda c: c.name)
def test_valid_forged_streams_on_the_device_alone(tmp_path, case, seg, stretch):
    st, got = run_case(tmp_path, case, seg, stretch)
    print(case.name, seg, stretch, st)
    assert len(got) == len(case.text), (len(got), len(case.text), st)
    if got != case.text:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(case.text, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%d bytes differ, first at %d (%s)" % (bad.size, bad[0], st))
    assert st["text"] == len(case.text)
    assert st["members"] == case.members
    assert st["host_pieces"] == 0, st


@pytest.mark.parametrize("seg,stretch", SHAPES)
@pytest.mark.parametrize("case", [c for c in INVALID if c.name not in REACH_BEFORE_MEMBER], ids=lambda c: c.name)
def test_invalid_forged_streams_are_refused(tmp_path, case, seg, stretch):
    with pytest.raises(RuntimeError):
        run_case(tmp_path, case, seg, stretch)


@pytest.mark.parametrize("seg,stretch", SHAPES)
@pytest.mark.parametrize("name", REACH_BEFORE_MEMBER)
def test_a_distance_before_the_members_first_byte_is_refused(tmp_path, name, seg, stretch):
    case = [c for c in INVALID if c.name == name][0]
    with pytest.raises(RuntimeError):
        run_case(tmp_path, case, seg, stretch)


def _run_readers(tmp_path, monkeypatch, name, gz):
    """_run_both_readers of tests/test_gpu_run.py for a stream that is given, not made by gzip.compress"""
    from nohuman_amd import Engine
    outs = {}
    p1 = tmp_path / (name + ".fq.gz")
    p1.write_bytes(gz)
    for reader in ("device", "device-text", "host"):
        monkeypatch.setenv("NOHUMAN_GZ_READER", reader)
        o1, k = tmp_path / ("o1_" + reader), tmp_path / ("k_" + reader)
        with Engine.open(DB) as eng:
            st = eng.run(str(p1), str(o1), kraken_output=str(k), out_codec=0, threads=4)
        outs[reader] = (o1.read_bytes(), k.read_bytes(), (st.total_sequences, st.classified, st.total_bases))
    assert outs["device"] == outs["host"], name
    assert outs["device-text"] == outs["host"], name
    return outs["host"]


def test_fastq_relaid_through_the_run_with_every_reader(tmp_path, monkeypatch):
    case = [c for c in VALID if c.name == "fastq_relaid"][0]
    monkeypatch.setenv("NOHUMAN_GZDEV_SEG", "16384")
    monkeypatch.setenv("NOHUMAN_GZDEV_STRETCH", "2048")
    monkeypatch.setenv("NOHUMAN_BATCH_FRAGS", "100")
    got = _run_readers(tmp_path, monkeypatch, "relaid", case.gz)
    monkeypatch.setenv("NOHUMAN_GZ_READER", "host")
    want = _run_readers(tmp_path, monkeypatch, "zlib", gzip.compress(case.text, 6))  # the same text as zlib writes it
    assert got == want and got[2][0] > 100


def beyond_16_to_1(data):
    """does some 16 KiB of the text, with the window before it for a dictionary, deflate beyond 16 : 1?  (Decided from the
    input with zlib -9: there the reader's slots may overflow and a piece go to the host decoder.)"""
    for i in range(0, len(data), 8192):
        w = data[i:i + 16384]
        if i:
            co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, data[max(0, i - 32768):i])
        else:
            co = zlib.compressobj(9, zlib.DEFLATED, -15)
        if len(w) > 16 * len(co.compress(w) + co.flush()):
            return True
    return False


def _encoder_inputs():
    ins = [("fastq_1MB", fastq_text(2800, 5))]
    ins += [("mixture_%d" % s, _mixture(s)) for s in (0, 3, 7, 11, 19)]
    for period in (32767, 32768, 32769):
        unit = np.random.default_rng(period).integers(0, 256, period, dtype=np.uint8).tobytes()
        ins.append(("period_%d" % period, unit * 5 + unit[:1000]))
    text = fastq_text(200, 9)
    ins += [("size_%d" % n, (text * (n // len(text) + 1))[:n]) for n in (0, 1, 65537)]
    return ins


ENCODER_INPUTS = _encoder_inputs()


@pytest.mark.parametrize("name,data", ENCODER_INPUTS, ids=[n for n, _ in ENCODER_INPUTS])
def test_the_gpu_encoders_streams_through_the_gpu_reader(tmp_path, name, data):
    gz = tmp_path / "enc.gz"
    gpu_gzip(data, str(gz))
    dense = beyond_16_to_1(data)
    for seg, stretch in ((0, 0), (40_000, 2048)):
        st = gunzip_dev(gz, tmp_path / "enc.out", seg, stretch)
        assert (tmp_path / "enc.out").read_bytes() == data, (name, seg, stretch, st)
        assert st["text"] == len(data)
        assert dense or st["host_pieces"] == 0, (name, seg, stretch, st)
