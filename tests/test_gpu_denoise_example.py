"""GPU: examples/batch_denoise.c builds against the public headers and the library and shows what the noise suppressor
is for: a quiet talker is levelled 12 dB up, and the room's noise with the talker -- unless the suppressor stands in front; then
the noise floor of the programme is no higher than at the microphone.  The printed reduction lies in the range
tests/test_denoise_host.py holds the arithmetic to."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_denoise_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_denoise"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_denoise.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(out) == 3, out
    # the designed parameters: 18 dB of reduction, 6 dB of over-subtraction, 10.7 and 21.4 ms at hops of 256 frames
    assert out[0] == ("2 microphones -> noise suppressor: blocks of 512 frames, delay 511, floor 4125, over 64, shifts 1 and 2 "
                      "-> leveller: target 3277, gate 164 -> limiter: threshold 29204"), out
    m = re.match(r"noise floor: microphone (-[\d.]+) dBFS, programme without suppression (-[\d.]+) dBFS, with (-[\d.]+) dBFS$",
                 out[1])
    assert m, out
    mic, without, with_ = (float(v) for v in m.groups())
    assert abs(mic + 56.0) < 0.5, out
    assert 10.0 < without - mic < 14.0, out                              # the leveller lifted the noise with the talker
    assert with_ <= mic, out                                             # ... and with the suppressor it no longer does
    m = re.match(r"reduction ([\d.]+) dB, leveller gains (\d+) and (\d+), learned blocks (\d+), clips 0, sat 0, "
                 r"noise lifted: no$", out[2])
    assert m, out
    assert 12.0 <= float(m.group(1)) <= 18.0, out
    assert abs(float(m.group(1)) - (without - with_)) < 0.11, out
    assert all(13000 < int(g) < 20000 for g in m.group(2, 3)), out       # about +12 dB re 4096
    assert int(m.group(4)) == (24000 - 512) // 256 + 1, out
