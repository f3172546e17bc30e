"""GPU: examples/batch_drift.c builds against the public headers and the library and shows what the drift stage is for:
a source that delivers 1000 ppm more frames than the batch consumes stays inside its elastic buffer, the servo settles
at the source's offset, and the signal watch behind the bus finds no dead air and no clipped sample."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
SERVO_RESIDUAL_PPM = 2 * 73.9                  # tests/test_drift_host.py: the settled delta's measured residual, times two


def test_batch_drift_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_drift"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_drift.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == 12 + 2, out
    rows = [re.fullmatch(r"block +(\d+): fill +(\d+), delta +([-+][\d.]+) ppm, (\d+) frames in, (\d+) out", l) for l in out[:12]]
    assert all(rows), out
    assert [int(m.group(1)) for m in rows] == list(range(250, 3001, 250))
    assert [int(m.group(5)) for m in rows] == [512 * n for n in range(250, 3001, 250)]
    # what went in is what came out, stretched by the steps in force: about 1000 ppm more in the settled part
    grown = (int(rows[-1].group(4)) - int(rows[-5].group(4))) / (int(rows[-1].group(5)) - int(rows[-5].group(5)))
    assert abs((grown - 1.0) * 1e6 - 1000.0) < 20.0, grown
    m = re.fullmatch(r"fill stayed in (\d+)\.\.(\d+) of 2048; settled at ([-\d.]+) ppm", out[12])
    assert m, out[12]
    assert 0 <= int(m.group(1)) <= int(m.group(2)) <= 2048
    assert abs(float(m.group(3)) - 1000.0) <= SERVO_RESIDUAL_PPM
    assert out[13] == "dead air 0 frames, clipped samples 0"
