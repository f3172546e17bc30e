"""GPU: examples/batch_automix.c builds against the public headers and the library and shows what the automixer is for:
one talker passes at unity, two equal talkers at -3 dB each, four at -6 dB each, silent microphones sink to their floor,
and the bus behind carries the sum."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_automix_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_automix"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_automix.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0] == "4 microphones in one group -> automixer: window 256 frames -> bus at unity; 1024 frames a phase", out
    # isqrt(2^24 / n) for n = 1, 2, 4 talkers; the peak is the talkers' sum: n * ((8000 * gain + 2048) >> 12)
    assert out[1:] == ["phase 1: gains 4096 0 0 0, programme peak 8000",
                       "phase 2: gains 2896 2896 0 0, programme peak 11312",
                       "phase 3: gains 2048 2048 2048 2048, programme peak 16000"], out
