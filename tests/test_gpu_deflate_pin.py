"""Every variant of the GPU gzip / BGZF encoder against its host model, byte for byte, on the pin set (tests/deflate_pins.py).

The encoder reads its knobs once per process (NOHUMAN_GZIP_WAYS, NOHUMAN_GZIP_REGION, NOHUMAN_GZIP_PRICES, NOHUMAN_NO_PINNED), so a
variant is a fresh child process that encodes the whole pin set; the parent compares every file with nh_gzip_model_file under the same
options.  Together the variants run all six k_deflate instantiations (4, 6, 8 ways, with and without the final block of BGZF), the small
regions with both forced price sets and with the pilot, and the pageable staging buffers.  The children run one after another, each
under its own time limit; once one has died or failed, the remaining variants fail without starting anything on the GPU."""
import os
import subprocess
import sys

import pytest

from tests import deflate_pins as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 240   # a child sets up some hundred encoders (its buffers and streams each time); a healthy one takes a fraction of this
_stopped = []         # why no further child may start

CHILD = ("import sys, os, ctypes as C; sys.path.insert(0, %r)\n"
         "from nohuman_amd import _lib\n"
         "L = _lib.lib()\n"
         "d, entry = sys.argv[1], getattr(L, sys.argv[2])\n"
         "for f in sorted(os.listdir(d)):\n"
         "    if not f.endswith('.bin'): continue\n"
         "    data = open(os.path.join(d, f), 'rb').read()\n"
         "    rc = entry(0, data, len(data), os.path.join(sys.argv[3], f[:-4] + '.gz').encode(), None)\n"
         "    if rc != 0:\n"
         "        print(f, rc, L.nh_last_error().decode())\n"
         "        sys.exit(3)\n") % ROOT


@pytest.fixture(scope="module")
def pin_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_pins")
    for i, (name, text) in enumerate(P.pin_set()):
        (d / ("%03d.bin" % i)).write_bytes(text)
    return d


@pytest.mark.parametrize("variant", [v[0] for v in P.VARIANTS])
def test_variant_equals_the_model_on_the_pin_set(tmp_path, pin_files, variant):
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    knobs, bgzf = next((k, b) for n, k, b in P.VARIANTS if n == variant)
    env = {k: v for k, v in os.environ.items() if not k.startswith("NOHUMAN_GZIP") and k != "NOHUMAN_NO_PINNED"}
    env.update(knobs, NOHUMAN_GZIP_CHUNK_MB="64")   # (the smallest chunks: the buffers of an encoder are sized by them)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, str(pin_files), "nh_bgzf_gpu_file" if bgzf else "nh_gzip_gpu_file", str(tmp_path)],
                           env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        _stopped.append("the child of variant %s did not end within %d s" % (variant, CHILD_SECONDS))
        pytest.fail(_stopped[0])
    if r.returncode != 0:
        _stopped.append("the child of variant %s ended with status %d: %s" % (variant, r.returncode, (r.stdout + r.stderr)[-1500:]))
        pytest.fail(_stopped[0])
    opts = P.encoder_options(env, bgzf)
    for i, (name, text) in enumerate(P.pin_set()):
        raw = (tmp_path / ("%03d.gz" % i)).read_bytes()
        P.assert_equals_model(raw, text, name, variant, **opts)
