"""--mask-low-complexity / mask_low_complexity / nh_dust_mask without a device: the CLI's usage error and help, the bindings'
layouts, and what nh_dust_mask refuses before any device is touched.  tests/test_gpu_dust.py and test_gpu_build_db_dust.py mask."""
import ctypes as C
import os
import subprocess

import nohuman_amd
from nohuman_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
NO_DEVICE = 1 << 20  # a device id no machine has


def _cli(*args):
    p = subprocess.run([BIN] + list(args), capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


def test_cli_flag_needs_build_db(tmp_path):
    reads = tmp_path / "reads.fq"
    reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for args in (("--mask-low-complexity", str(reads)), ("--mask-low-complexity", "--mask", str(reads), "-o", str(tmp_path / "o.fq")),
                 ("--mask-low-complexity",)):
        rc, _, err = _cli(*args)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err, (args, rc, err)
        assert "'--mask-low-complexity' needs '--build-db <DIR>'" in err, err
    assert os.listdir(tmp_path) == ["reads.fq"]


def test_cli_help_lists_the_flag():
    rc, out, _ = _cli("--help")
    assert rc == 0 and "--mask-low-complexity" in out


def test_cli_flag_passes_the_argument_checks(tmp_path):
    """with --build-db the flag is no usage error: the call gets as far as the input (which is not there)"""
    rc, _, err = _cli("--build-db", str(tmp_path / "db"), "--reference", str(tmp_path / "none.fa"), "--mask-low-complexity")
    assert rc == 2 and "none.fa" in err and not (tmp_path / "db").exists()


def test_bindings_match_the_header():
    """the first layout stays (80 and 88 bytes); the present structs add their fields behind it"""
    assert C.sizeof(_lib.nh_build_args) == 80 and C.sizeof(_lib.nh_build_stats) == 88
    assert C.sizeof(_lib.nh_build_args_v2) == 88 and _lib.nh_build_args_v2.mask_low_complexity.offset == 80
    assert C.sizeof(_lib.nh_build_stats_v2) == 104
    assert (_lib.nh_build_stats_v2.masked_bases.offset, _lib.nh_build_stats_v2.seconds_mask.offset) == (88, 96)
    src = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    assert "#define NH_BUILD_ARGS_SIZE_V1 80u" in src and "#define NH_BUILD_STATS_SIZE_V1 88u" in src
    assert "nh_dust_mask" in _lib.SYMBOLS and nohuman_amd.dust_mask is not None


def test_struct_sizes_the_builder_accepts(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">chr1\n" + b"ACGTTGCAAGGCTTAACCGGTTACGATCGATTGCA" * 4 + b"\n")
    paths = (C.c_char_p * 1)(os.fsencode(str(fa)))
    for size, want in ((76, -1), (79, -1), (80, -4), (84, -4), (88, -4), (96, -4)):  # (-4: it got as far as the device check)
        a = _lib.nh_build_args_v2()
        a.struct_size, a.n_fasta, a.fasta, a.out_dir, a.device = size, 1, paths, os.fsencode(str(tmp_path / "db")), NO_DEVICE
        a.mask_low_complexity = 1
        s = _lib.nh_build_stats_v2()
        C.memset(C.byref(s), 0xA5, C.sizeof(s))
        assert _lib.lib().nh_build_db(C.byref(a), C.byref(s)) == want, size
        # the stats are zeroed as far as the caller's layout goes, and no further
        assert bytes(s)[:88] == bytes(88) and bytes(s)[88:] == (bytes(16) if size >= 88 else b"\xa5" * 16), size
        assert not (tmp_path / "db").exists()


def _dust(buf, starts, lens, device=NO_DEVICE, text=True, lists=True):
    cbuf = (C.c_char * max(len(buf), 1)).from_buffer(buf)
    st = (C.c_uint64 * max(len(starts), 1))(*starts)
    ln = (C.c_uint64 * max(len(lens), 1))(*lens)
    masked = C.c_uint64(7)
    rc = _lib.lib().nh_dust_mask(device, C.cast(cbuf, C.c_void_p) if text else None, len(buf), st if lists else None,
                                 ln if lists else None, len(starts), C.byref(masked))
    return rc, masked.value


def test_dust_mask_refuses_before_any_device():
    text = b"A" * 64
    buf = bytearray(text)
    for starts, lens in (([60], [5]), ([65], [0]), ([0, 0], [64, 65]), ([1 << 63], [1 << 63])):
        assert _dust(buf, starts, lens) == (-1, 0), (starts, lens)
        assert _lib.lib().nh_last_error().decode().startswith("nh_dust_mask:")
    assert _dust(buf, [0], [64], text=False)[0] == -1 and _dust(buf, [0], [64], lists=False)[0] == -1
    # nothing to mask: no device is asked for
    assert _dust(buf, [], []) == (0, 0) and _dust(buf, [0, 64], [0, 0]) == (0, 0)
    # and what passes ends at the device check (no fallback to the CPU)
    assert _dust(buf, [0], [64]) == (-4, 0)
    assert buf == text
