"""GPU: examples/batch_multiband.c builds against the public headers and the library and shows what the band split is
for: three bands with a dynamics object each, every band's compressor at work on the tone that lies in it, no clip
counter moved, and the programme under the limiter's threshold."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_multiband_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_multiband"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_multiband.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert "3 bands at 300 and 3000 Hz, 255 taps, delay 127 -> dynamics per band: delay 63" in out[0], out
    gains = []
    for k in range(3):
        m = re.match(r"band %d: threshold=-\d+ dBFS ratio=\d:1 detector=\d+ frames min_gain=(\d+) clips=(\d+)$" % k, out[1 + k])
        assert m, out
        gains.append(int(m.group(1)))
        assert int(m.group(2)) == 0, out                         # the bands added up exactly
    # every band holds one tone above its threshold (half of 16000, 9000, 6000 against -24, -18, -30 dBFS): each
    # compressor worked, none of them by more than the 12 dB its ratio can take from these levels
    assert all(32768 // 4 < g < 32768 for g in gains), gains
    m = re.match(r"programme: frames=24000 rate=48000 channels=1 peak=(-?\d+) power=(-?[\d.]+) lim_min_gain=(\d+)$", out[4])
    assert m, out
    assert 1000 < abs(int(m.group(1))) <= 29204, out
