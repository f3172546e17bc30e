"""GPU: examples/batch_sweep.c builds against the public headers and the library and moves a low cut from 40 to 160 Hz
under a tone on a DC offset, once with a step and once with a ramp over 50 ms.  Every figure it prints is held against
the numpy model of tests/test_gpu_iir_ramp.py on the same signal; the ramp bends the tone no more than the step does,
and neither leaves any of the offset behind."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
BLOCK, BLOCKS, MOVE, RAMP, TAIL = 960, 30, 15, 2400, 4800


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_sweep", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_batch_sweep_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_sweep"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_sweep.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(out) == 8, out
    # the same signal through the model
    TR = _load("test_gpu_iir_ramp")
    lo = gpu.iir_design(gpu.IIR_HIGHPASS, 48000.0, 40.0).as_tuple()
    hi = gpu.iir_design(gpu.IIR_HIGHPASS, 48000.0, 160.0).as_tuple()
    n = np.arange(BLOCKS * BLOCK)
    x = (3000 + np.rint(8000.0 * np.sin(2.0 * np.pi * n / 480.0))).astype(np.int16)[:, None]
    m = TR.RampModel(2, 1, 1)
    m.set(-1, 0, lo)
    y, mirror = [[], []], []
    for k in range(BLOCKS):
        if k == MOVE:
            m.set(0, 0, hi)
            m.ramp(1, 0, hi, RAMP)
        got = m.run([x[k * BLOCK:(k + 1) * BLOCK]] * 2)
        for s in range(2):
            y[s].append(got[s][:, 0].astype(np.int64))
        mirror.append((m.ramp_state(1, 0), m.now(1, 0)))
    y = [np.concatenate(v) for v in y]
    at = MOVE * BLOCK

    def worst(s, a, b, order):
        return int(np.abs(np.diff(y[s][a:b], n=order)).max())

    assert out[0] == ("low cut: HIGHPASS 40 Hz: b %d %d %d a %d %d -> 160 Hz: b %d %d %d a %d %d (units of 2^-26)" % (lo + hi)), out
    for i, k in enumerate((MOVE, MOVE + 1, MOVE + 2)):
        (done, frames), now = mirror[k]
        assert out[1 + i] == ("after block %d: stream 1's ramp at %d of %d, in force b %d %d %d a %d %d, b0 + b1 + b2 = 0"
                              % ((k, done, frames) + now)), out
    assert [mirror[k][0] for k in (MOVE, MOVE + 1, MOVE + 2)] == [(960, RAMP), (1920, RAMP), (0, 0)] and mirror[MOVE + 2][1] == hi
    bends = []
    for s, who in enumerate(("stream 0 (step): ", "stream 1 (ramp over 2400 frames): ")):
        want = who + "largest jump %d, largest second difference %d (%d before the move)" % (
            worst(s, at - 480, at + 2880, 1), worst(s, at - 480, at + 2880, 2), worst(s, at - 960, at - 480, 2))
        assert out[4 + s] == want, out
        bends.append(worst(s, at - 480, at + 2880, 2))
    assert bends[1] <= bends[0]
    for s in range(2):
        last = y[s][-TAIL:]
        m_ = re.match(r"stream %d: last 100 ms mean (-?[\d.]+) peak (\d+), filter clips=0 overs=0$" % s, out[6 + s])
        assert m_, out
        assert float(m_.group(1)) == round(float(last.mean()), 3) and int(m_.group(2)) == int(np.abs(last).max())
        assert abs(float(m_.group(1))) < 0.5                             # nothing of the offset's 3000 is left
    assert np.abs(y[0][-TAIL:] - y[1][-TAIL:]).max() <= 1               # both have arrived at the same filter
