"""GPU: examples/batch_leveller.c builds against the public headers and the library and shows what the leveller is for:
a talker at -40 dBFS and one at -6 dBFS both end at the gain their level asks for, 20 dB up and 14 dB down, and the
limiter behind holds its ceiling through the cough that the raised gain drives into the clamp."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_leveller_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_leveller"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_leveller.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(out) == 5, out
    # the designed parameters: -20 and -60 dB re 32768, +-24 dB re 4096, 6 and 20 dB/s at 1024 frames of 48 kHz
    assert out[0] == ("2 microphones -> leveller: window 1024 frames, target 3277, gate 33, gain 258..64917, rise 973, "
                      "fall 3141 -> limiter: threshold 29204"), out
    mics = []
    for s in range(2):
        m = re.match(r"mic %d: gain 4096 -> (\d+) \(wanted (\d+) at level (\d+)\), within a step: yes, clips (\d+)$" % s,
                     out[1 + s])
        assert m, out
        mics.append([int(v) for v in m.groups()])
    for (gain, wanted, level, _), rms, rate in zip(mics, (327.68, 16422.8), (973, 3141)):
        assert abs(level - rms) <= 2, out                                  # the tone's RMS: 32768 * 10^(dB / 20)
        assert wanted == (3277 << 12) // level, out
        assert abs(gain - wanted) <= max(1, (gain * rate) >> 16), out
    assert mics[0][0] > 9 * 4096 and mics[1][0] < 4096 // 4, out            # about +20 dB and -14 dB
    assert mics[0][3] > 0 and mics[1][3] == 0, out                         # the cough met the clamp, the loud talker never
    for s in range(2):
        m = re.match(r"programme %d: frames=240000 rate=48000 channels=1 peak=(-?\d+) power=(-?[\d.]+) lim_min_gain=(\d+)$" % s,
                     out[3 + s])
        assert m, out
        assert abs(int(m.group(1))) <= 29204, out                          # the limiter's ceiling
    assert abs(int(re.search(r"peak=(-?\d+)", out[3]).group(1))) > 29000, out     # ... reached by the cough alone
    assert int(re.search(r"lim_min_gain=(\d+)", out[3]).group(1)) < 32768, out
    assert int(re.search(r"lim_min_gain=(\d+)", out[4]).group(1)) == 32768, out
