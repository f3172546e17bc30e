"""GPU: examples/batch_parallel.c builds against the public headers and the library and shows what the delay stage is
for: a dry path exactly as late as the compressor beside it.  With the unity curve the program finds the bus output equal
to the delayed input bit for bit; with a curve the loud part comes out lower than it went in and the quiet part stays."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_parallel_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_parallel"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_parallel.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert "dynamics: delay 63, delay line: 63 of at most 63 frames" in out[0], out
    assert out[1] == "unity curve: bus output equals the input delayed by 63 frames: yes", out
    m = re.match(r"parallel compression: dyn_min_gain=(\d+) quiet_peak=(\d+) loud_peak=(\d+) \(dry (\d+) (\d+)\)$", out[2])
    assert m, out
    gain, quiet, loud, dry_quiet, dry_loud = (int(v) for v in m.groups())
    assert 32768 // 16 < gain < 32768 // 2, out              # the compressor worked hard on the loud part
    # half the dry signal is always there: the loud part loses less than 6 dB and more than 2, the quiet part next to nothing
    assert dry_loud // 2 <= loud < dry_loud * 4 // 5, out
    assert dry_quiet * 9 // 10 <= quiet <= dry_quiet, out
    m = re.match(r"programme: frames=24000 rate=48000 channels=1 peak=(-?\d+) power=(-?[\d.]+) lim_min_gain=(\d+)$", out[3])
    assert m, out
    assert 1000 < abs(int(m.group(1))) <= 29204, out
