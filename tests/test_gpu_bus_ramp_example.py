"""GPU: examples/batch_fader.c builds against the public headers and the library and shows what the send ramps are
for: the faded programme's positions as cmhip_bus_ramp_state reports them, and a largest sample-to-sample jump below
the stepped programme's."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_fader_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_fader"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_fader.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    blocks = [ln for ln in out if ln.startswith("block ")]
    assert [ln.split()[2:] for ln in blocks] == [
        ["frames=1208", "at=1208", "send0=0/0", "send1=0/0"], ["frames=240", "at=1448", "send0=240/480", "send1=240/480"],
        ["frames=240", "at=1688", "send0=0/0", "send1=0/0"], ["frames=712", "at=2400", "send0=0/0", "send1=0/0"]], out
    assert any(ln.startswith("faded: ") for ln in out) and any(ln.startswith("stepped: ") for ln in out)
    m = re.match(r"largest jump, left channel: faded=(\d+) stepped=(\d+) click-free=yes$", out[-1])
    assert m, out
    faded, stepped = int(m.group(1)), int(m.group(2))
    # a full-scale sine of 48 samples moves by at most 32767 * 2 pi / 48 = 4290 a sample, and the left channel never
    # carries more than full scale; the step takes half of microphone 0 away near its crest
    assert faded <= 4400 and stepped > 2 * faded, (faded, stepped)
