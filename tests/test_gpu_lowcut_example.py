"""GPU: examples/batch_lowcut.c builds against the public headers and the library and shows what the filter is for: a
microphone with a DC offset holds a gate open through the pauses; behind a 40 Hz high-pass whose zero lies on z = 1
exactly the gate closes, and the voice passes both ways."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_lowcut_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_lowcut"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_lowcut.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(out) == 5, out
    sec = gpu.iir_design(gpu.IIR_HIGHPASS, 48000.0, 40.0)
    m = re.match(r"low cut: HIGHPASS 40 Hz at 48000: b (-?\d+) (-?\d+) (-?\d+) a (-?\d+) (-?\d+) \(units of 2\^-26\), "
                 r"b0 \+ b1 \+ b2 = 0; -inf dB at 0 Hz, (-?[\d.]+) dB at 500 Hz$", out[0])
    assert m, out
    assert tuple(int(v) for v in m.groups()[:5]) == sec.as_tuple()
    assert -0.01 < float(m.group(6)) <= 0.0, out                           # the voice passes
    assert out[1] == "voice: gate gain without the filter 32768, behind the low cut 32768", out
    m = re.match(r"pause: gate gain without the filter 32768, behind the low cut (\d+)$", out[2])
    assert m and int(m.group(1)) < 400, out                                # the gate's range is 40 dB: 328
    peaks = []
    for s in range(2):
        m = re.match(r"programme %d: frames=\d+ rate=48000 channels=1 peak=(-?\d+) power=(-?[\d.]+) filter clips=0 overs=0$" % s,
                     out[3 + s])
        assert m, out
        peaks.append(abs(int(m.group(1))))
    # offset + voice; behind the filter the first frames still carry the offset's step, which then decays
    assert 2690 <= peaks[0] <= 2700 and 1200 <= peaks[1] <= 2700, out
