"""The host model of the GPU gzip / BGZF encoder (nh_gzip_model_file, nohuman_amd/csrc/nh_deflate_model.h) on a CPU: its files are
well-formed under zlib for every variant the GPU tests run, the bytes do not depend on the thread count, the price hand-over from
chunk to chunk and the pilot do what the encoder's host side does -- and the pin set (tests/deflate_pins.py) SEPARATES the encoder's
variants: a set on which 4, 6 and 8 ways, the two price sets or the region sizes gave the same bytes would pin nothing."""
import ctypes as C
import zlib

import pytest

from nohuman_amd import _lib
from tests import bgzf_util
from tests import deflate_pins as P


def _variant_options(knobs, bgzf):
    return P.encoder_options(dict(knobs, NOHUMAN_GZIP_CHUNK_MB="64"), bgzf)


@pytest.fixture(scope="module")
def modelled():
    """{variant: {input: (file, stats)}}: the whole pin set under every variant, computed once"""
    out = {}
    for name, knobs, bgzf in P.VARIANTS:
        if name == "pageable_staging":
            continue   # (the same options as ways4_gzip)
        opts = _variant_options(knobs, bgzf)
        out[name] = {pin: P.model(text, **opts)[:2] for pin, text in P.pin_set()}
    return out


def _one_gzip_member(raw, text):
    d = zlib.decompressobj(31)
    assert d.decompress(raw) == text and d.eof and d.unused_data == b""   # content, CRC-32, ISIZE; nothing behind the member


@pytest.mark.parametrize("variant", [v[0] for v in P.VARIANTS if v[0] != "pageable_staging"])
def test_every_file_is_well_formed(modelled, variant):
    bgzf = dict((v[0], v[2]) for v in P.VARIANTS)[variant]
    for pin, text in P.pin_set():
        raw = modelled[variant][pin][0]
        if bgzf:
            bgzf_util.check_bgzf(raw, text)   # every member on its own: BSIZE, CRC-32, ISIZE; the EOF member last
            if not text:
                assert raw == bgzf_util.EOF_MEMBER
        else:
            assert raw[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])
            _one_gzip_member(raw, text)


def test_bytes_do_not_depend_on_threads_or_on_the_call():
    pins = dict(P.pin_set())
    for pin, opts in (("mixture_0", dict()), ("mixture_1", dict(region=4096, ways=6)), ("pilot_forty_17_regions", dict(region=4096)),
                      ("size_65281_fastq", dict(bgzf=True)), ("mixture_2", dict(region=4096, chunk=16384, ways=8))):
        one = P.model(pins[pin], threads=1, **opts)
        many = P.model(pins[pin], threads=16, **opts)
        again = P.model(pins[pin], threads=16, **opts)
        assert one == many == again, pin


def test_prices_are_handed_from_chunk_to_chunk():
    """Chunks of four small regions: every region of chunk k + 1 starts from the lengths region 0 of chunk k ended with, so a text
    whose statistics change behind chunk 0 comes out differently than from one chunk -- and both are the text."""
    text = P.fastq_text(50, 3)[:16384] + P.reads_with_qualities("spread", 100, 5)[:20000] + bytes(range(256)) * 40 + b"ACGT" * 3000
    whole, st_whole, sizes_whole = P.model(text, region=4096, chunk=128 << 20, prices=1)
    cut, st_cut, sizes_cut = P.model(text, region=4096, chunk=4 * 4096, prices=1)
    _one_gzip_member(whole, text)
    _one_gzip_member(cut, text)
    assert st_cut["regions"] == st_whole["regions"] == -(-len(text) // 4096) > 12
    assert sizes_cut[:4] == sizes_whole[:4]          # chunk 0: the same starting prices, the same streams
    assert sizes_cut[4:] != sizes_whole[4:] and cut != whole
    assert len(text) > 3 * 4 * 4096                  # (more than one hand-over)
    # the pilot sees the regions of chunk 0 only, sixteen at the most: four here
    assert P.model(text, region=4096, chunk=4 * 4096)[1]["price_set"] == P.model(text[:4 * 4096], region=4096)[1]["price_set"]
    # forcing the set the pilot chose reproduces the pilot's file byte for byte; the other set gives another file
    for chunk in (128 << 20, 4 * 4096):
        piloted, st, _ = P.model(text, region=4096, chunk=chunk)
        assert P.model(text, region=4096, chunk=chunk, prices=st["price_set"])[0] == piloted
        assert P.model(text, region=4096, chunk=chunk, prices=1 - st["price_set"])[0] != piloted


def test_pilot_reads_sixteen_regions_and_a_tie_goes_to_set_one():
    # a text without A C G T N prices the same under both sets: a tie, set 1
    assert P.model(b"hello, world! " * 300)[1]["price_set"] == 1
    assert P.model(b"")[1]["price_set"] == 0 and P.model(b"", prices=1)[1]["price_set"] == 0   # (no chunk, no pilot: nothing chosen)
    # what lies behind the sixteenth region does not reach the pilot: set 0 wins on the first sixteen, whatever follows
    pins = dict(P.pin_set())
    head = pins["pilot_spread_16_regions"] + b"\n" * 7   # exactly sixteen regions of 4096
    assert len(head) == 16 * 4096 and P.model(head, region=4096)[1]["price_set"] == 0
    tail = P.reads_with_qualities("forty", 600, 9)    # alone, in regions this small, this text wants set 1
    assert P.model(tail, region=4096)[1]["price_set"] == 1
    assert P.model(head + tail, region=4096)[1]["price_set"] == 0


def test_the_pin_set_discriminates(modelled):
    """Conditions on the model alone: the pinned bytes must move when a variant's rule moves."""
    pins = [p for p, _ in P.pin_set()]

    def differ(a, b):
        return [p for p in pins if modelled[a][p][0] != modelled[b][p][0]]

    report = {}
    for a, b in (("ways4_gzip", "ways6_gzip"), ("ways6_gzip", "ways8_gzip"), ("ways4_gzip", "ways8_gzip"),
                 ("ways4_bgzf", "ways6_bgzf"), ("ways6_bgzf", "ways8_bgzf"), ("ways4_bgzf", "ways8_bgzf"),
                 ("ways4_region4096_prices0", "ways4_region4096_prices1"), ("ways8_region4096_prices0", "ways8_region4096_prices1"),
                 ("ways4_gzip", "ways4_region4096_pilot"), ("ways8_gzip", "ways8_region4096_pilot")):
        report[a, b] = differ(a, b)
        assert report[a, b], "no pinned input separates %s from %s" % (a, b)
    assert "bucket_pressure" in report["ways4_gzip", "ways6_gzip"] and "bucket_pressure" in report["ways6_gzip", "ways8_gzip"]
    for v in ("ways4_region4096_pilot", "ways8_region4096_pilot", "ways4_gzip", "ways6_bgzf"):
        assert {modelled[v][p][1]["price_set"] for p in pins if not p.startswith("size_0_")} == {0, 1}, v   # (an empty text has no pilot)
    small = modelled["ways4_region4096_pilot"]   # the pilot texts of 15, 16 and 17 small regions: both sets chosen among them
    assert {small[p][1]["price_set"] for p in pins if p.startswith("pilot_")} == {0, 1}
    # a tie in the pilot: set 1 goes on, and the reads behind the sixteen regions come out differently under set 0
    for v, pin, region in (("ways4_gzip", "pilot_tie", 65536), ("ways4_region4096_pilot", "pilot_tie_small_regions", 4096)):
        text = dict(P.pin_set())[pin]
        assert modelled[v][pin][1]["price_set"] == 1
        assert P.model(text[:16 * region], region=region, prices=0)[0] == P.model(text[:16 * region], region=region, prices=1)[0]
        assert P.model(text, region=region, prices=0)[0] != modelled[v][pin][0] == P.model(text, region=region, prices=1)[0]
    for v in modelled:
        total = {k: [modelled[v][p][1][k] for p in pins] for k in P.STAT_NAMES}
        assert sum(total["stored_blocks"]) > 0 and sum(total["dynamic_blocks"]) > 0, v
        assert max(total["longest_match"]) == 258 and sum(total["extended"]) > 0, v
        assert sum(total["repaired7"]) > 0, v
        if "region4096" not in v:
            assert max(total["longest_dist"]) == 32768, v       # exactly the window, never more
            assert modelled[v]["distance_32768"][1]["longest_dist"] == 32768 and modelled[v]["distance_32769"][1]["longest_dist"] < 32768
            assert modelled[v]["distance_32767"][1]["longest_dist"] == 32767
            assert sum(total["repaired15"]) > 0 and modelled[v]["steep_counts"][1]["repaired15"] == 1, v
        else:
            assert max(total["longest_dist"]) <= 4095, v        # a region of 4096 bytes has no longer distance
        assert modelled[v]["skewed_code_lengths"][1]["repaired7"] == 1, v
        assert modelled[v]["no_match"][1]["matches"] == 0 and modelled[v]["no_match"][1]["dynamic_blocks"] >= 1, v
        assert modelled[v]["all_values_equally_often"][1]["matches"] == 0
        assert modelled[v]["almost_only_matches"][1]["tokens"] * 40 < 37000, v   # (literals: the unit's 37 bytes at a region's start)
        assert modelled[v]["distance_across_regions"][1]["longest_dist"] < 32768
    # the match that would cross a region's end is cut there: region 0 alone holds a match of the 200 bytes before its end
    text = dict(P.pin_set())["match_cut_by_region_end"]
    for end in (4096, 65536):
        assert P.model(text[end - 1000:end])[1]["longest_match"] == 200
        assert P.model(text[end - 1000:end + 100])[1]["longest_match"] == 258   # (uncut, it is a longest match)
    assert modelled["ways4_region4096_pilot"]["match_cut_by_region_end"][1]["longest_match"] == 200   # (both are ends of small regions)


def test_refusals_and_the_environment_reader():
    L = _lib.lib()
    for bad in (dict(ways=5), dict(ways=16), dict(prices=2), dict(prices=-2), dict(chunk_bytes=100)):
        kw = dict(ways=4, region_bytes=65536, chunk_bytes=64 << 20, prices=-1, bgzf=0, threads=1)
        kw.update(bad)
        opts = _lib.nh_gzip_model_opts(**kw)
        assert L.nh_gzip_model_file(b"abc", 3, b"/dev/null", C.byref(opts), None) == -1, bad   # NH_EINVAL
    assert P.encoder_options({}) == dict(ways=4, region=65536, chunk=128 << 20, prices=-1, bgzf=False)
    env = {"NOHUMAN_GZIP_WAYS": "6", "NOHUMAN_GZIP_REGION": "5000", "NOHUMAN_GZIP_CHUNK_MB": "1", "NOHUMAN_GZIP_PRICES": "0x"}
    assert P.encoder_options(env, True) == dict(ways=6, region=5000, chunk=64 << 20, prices=0, bgzf=True)
    assert P.encoder_options({"NOHUMAN_GZIP_WAYS": "7", "NOHUMAN_GZIP_CHUNK_MB": "9999", "NOHUMAN_GZIP_PRICES": "2"})["ways"] == 4
    # the region is rounded as the encoder rounds it: 5000 -> 4992, below 4096 -> 4096, above 65536 -> 65536
    text = dict(P.pin_set())["size_65537_fastq"]
    assert P.model(text, region=5000)[1]["regions"] == -(-65537 // 4992)
    assert P.model(text, region=1)[0] == P.model(text, region=4096)[0]
    assert P.model(text, region=1 << 20)[0] == P.model(text, region=65536)[0]


def test_a_mismatch_is_located():
    """assert_equals_model names the input, the variant, the region and the offset, and says whether the streams agree as text"""
    text = dict(P.pin_set())["pilot_bins_17_regions"]
    raw, _, sizes = P.model(text, region=4096)
    assert P.assert_equals_model(raw, text, "x", "v", region=4096)["regions"] == 17
    at = 10 + sum(sizes[:3]) + 5
    broken = raw[:at] + bytes([raw[at] ^ 0x10]) + raw[at + 1:]
    with pytest.raises(AssertionError) as ei:
        P.assert_equals_model(broken, text, "pilot_bins_17_regions", "ways4", region=4096)
    msg = str(ei.value)
    assert "'pilot_bins_17_regions'" in msg and "'ways4'" in msg and "region 3 of 17" in msg and "offset 5 of" in msg and msg.endswith("NO")
    other = P.model(text, region=4096, ways=8)[0]   # another valid encoding of the same text
    with pytest.raises(AssertionError) as ei:
        P.assert_equals_model(other, text, "pilot_bins_17_regions", "ways4", region=4096)
    assert "region 0 of 17" in str(ei.value) and str(ei.value).endswith("yes")
    for bgzf_raw in (P.model(text, bgzf=True, ways=8)[0],):
        with pytest.raises(AssertionError) as ei:
            P.assert_equals_model(bgzf_raw, text, "t", "bgzf", bgzf=True)
        assert "region 0 of 2" in str(ei.value)
