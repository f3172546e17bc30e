"""GPU: the mixer's matrix ramps (cmhip_mix_ramp_matrix, csrc/k_mixramp.hip) against a numpy model of the arithmetic
include/coolmic_hip.h states ("matrix ramps"), bit for bit: both kernel forms with tiles inside, across and behind a
ramp and positions carried over runs, cuts and retargets, set_matrix cancelling, the order of ramp_matrix with the runs,
the extremes of the int32 bound and the rounding, a long ramp, transparency, refusals that change nothing, and the C
example.  Output slots are pre-filled with a sentinel; every sample past a stream's count must still hold it after a
run.  (tests/test_mix_ramp_host.py takes the model from here; the noise, the dense matrices and the rig come from
tests/test_gpu_mix.py.)"""
import ctypes as C
import importlib.util
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def _mix_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_mix_model", os.path.join(ROOT, "tests", "test_gpu_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _mix_test_module()
noise, dense_matrix, model_mix, SENTINEL, SATURATED_MAX = (TG.noise, TG.dense_matrix, TG.model_mix, TG.SENTINEL,
                                                           TG.SATURATED_MAX)
RAMP_MAX = 1 << 20


# ---------------------------------------------------------------------------
# the specification in numpy

def ramp_position(n, R):
    """p(n) = min(32768, (n * ceil(2^32 / R)) >> 17) for n = 0..R (an array or a number); n above R counts as R"""
    assert 2 <= R <= RAMP_MAX
    inc = -(-(1 << 32) // R)
    n = np.minimum(np.asarray(n, dtype=np.int64), R)
    return np.minimum(32768, (n * inc) >> 17)


def ramp_weight(w0, w1, p):
    """sgn(N) * (|N| >> 15), N = w0 (32768 - p) + w1 p: the division by 32768 truncated towards zero"""
    w0, w1, p = np.asarray(w0, dtype=np.int64), np.asarray(w1, dtype=np.int64), np.asarray(p, dtype=np.int64)
    N = w0 * (32768 - p) + w1 * p
    assert N.size == 0 or np.abs(N).max() <= 1 << 30
    return np.sign(N) * (np.abs(N) >> 15)


class RampModel:
    """one stream's matrix over time: W0, W1, done, R as the header's section has them"""

    def __init__(self, W):
        self.w0 = self.w1 = np.asarray(W, dtype=np.int64).copy()
        self.done = self.R = 0

    def ramping(self):
        return self.done < self.R

    def now(self):
        return ramp_weight(self.w0, self.w1, ramp_position(self.done, self.R)) if self.ramping() else self.w1

    def state(self):
        """what cmhip_mix_ramp_state answers"""
        return (self.done, self.R, self.now()) if self.ramping() else (0, 0, self.w1)

    def set(self, W):
        self.w0 = self.w1 = np.asarray(W, dtype=np.int64).reshape(self.w1.shape).copy()
        self.done = self.R = 0

    def ramp(self, W, R):
        if R < 2:
            return self.set(W)
        self.w0 = self.now()
        self.w1 = np.asarray(W, dtype=np.int64).reshape(self.w1.shape).copy()
        self.done, self.R = 0, R

    def run(self, x):
        """x int16 [F][C_in] -> int16 [F][C_out], and the position moves on by F"""
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.w1.shape[1])
        F = x.shape[0]
        if self.ramping():
            p = ramp_position(self.done + 1 + np.arange(F), self.R)
            W = ramp_weight(self.w0[None], self.w1[None], p[:, None, None])          # [F][C_out][C_in]
            assert F == 0 or np.abs(W).sum(axis=2).max() <= 65535                    # the row bound, every frame
            acc = np.einsum("foc,fc->fo", W, x)
            self.done = min(self.R, self.done + F)
        else:
            acc = x @ self.w1.T
        assert acc.size == 0 or np.abs(acc + 8192).max() < 2 ** 31                   # int32 never overflows
        return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)


class Rig(TG.Rig):
    """tests/test_gpu_mix.py's rig with a RampModel per stream beside the mixer"""

    def __init__(self, cm, streams, ci, co, max_frames, matrices=None):
        super().__init__(cm, streams, ci, co, max_frames, matrices)
        self.models = [RampModel(w) for w in self.W]

    def ramp(self, stream, w, R):
        self.m.ramp_matrix(stream, w, R)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].ramp(w, R)
            assert np.array_equal(self.m.get_matrix(s), np.asarray(w).reshape(self.CO, self.CI))      # the target

    def step(self, stream, w):
        self.m.set_matrix(stream, w)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].set(w)

    def check_state(self):
        for s, mod in enumerate(self.models):
            done, total, w = self.m.ramp_state(s)
            d, r, wm = mod.state()
            assert (done, total) == (d, r), ("stream", s, (done, total), (d, r))
            assert np.array_equal(w, wm), ("stream", s)

    def play(self, xs, frames=None, uniform=False):
        """a run of the device and of the models, compared; then the states compared -> the models' outputs"""
        wants = [mod.run(x) for mod, x in zip(self.models, xs)]
        self.run(xs, frames=frames, uniform=uniform, wants=wants)
        self.check_state()
        return wants


def saturated_share(ys):
    return sum(TG.saturated(y) for y in ys) / max(1, sum(y.size for y in ys))


# ---------------------------------------------------------------------------
# 1. both forms: tiles inside, across and behind a ramp, positions carried from run to run

PAIRS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (6, 2), (5, 3), (7, 5), (16, 16)]


@pytest.mark.parametrize("ci,co", PAIRS)
def test_forms(gpu, ci, co):
    cm = gpu
    t = cm.plan_mix(5, ci, co, 1).tile_frames
    counts = [2 * t + 13, t, t - 1, 1, 0]
    ramps = [t + 300, 7, 2, 50, 9]
    assert t < ramps[0] < 2 * t          # stream 0: a tile inside the ramp, one in which it ends, one behind it
    seeds = [1000 * ci + 10 * co + s for s in range(5)]
    W0 = [dense_matrix(ci, co, seed) for seed in seeds]
    W1 = [dense_matrix(ci, co, seed + 500) for seed in seeds]
    xs = [noise(100 * ci + co + 7 * s, 2 * t + 13, ci) for s in range(5)]
    rig = Rig(cm, 5, ci, co, counts[0], W0)
    for s in range(5):
        rig.ramp(s, W1[s], ramps[s])
    ys = rig.play([x[:n] for x, n in zip(xs, counts)])
    assert [mod.done for mod in rig.models] == [ramps[0], 7, 2, 1, 0]
    ys += rig.play([x[::-1][:n] for x, n in zip(xs, counts)])    # no new call: stream 1 is at n = t + 1, stream 4 at 0
    assert rig.models[3].state()[:2] == (2, 50) and rig.models[4].state()[:2] == (0, 9)
    ys += rig.play([x[:50] for x in xs], uniform=True)           # the two short streams reach their ends as well
    share = saturated_share(ys)
    print("mix ramp forms %2d -> %2d: tile_frames %d, saturated outputs in the model %.2f %%" % (ci, co, t, 100 * share))
    assert share < SATURATED_MAX
    # every ramp has ended: the plain kernels with the targets
    assert all(rig.m.ramp_state(s)[:2] == (0, 0) for s in range(5))
    wants = [model_mix(x[:n], w) for x, n, w in zip(xs, counts, W1)]
    rig.run([x[:n] for x, n in zip(xs, counts)], wants=wants)
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts and retargeting: the output does not depend on how the stream was cut into runs

CUTS = ([400, 2600], [1, 7, 8, 384, 100, 900, 1, 599, 1000])


@pytest.mark.parametrize("ci,co", [(2, 2), (6, 2)])
def test_cuts_and_retargeting(gpu, ci, co):
    cm = gpu
    A, B, Cm = (dense_matrix(ci, co, 40 * ci + co + i) for i in range(3))
    x = noise(2000 + ci, 3000, ci)
    whole = RampModel(A)
    whole.ramp(B, 700)
    want = [whole.run(x[:400])]
    assert whole.state()[:2] == (400, 700)
    whole.ramp(Cm, 1000)
    want.append(whole.run(x[400:]))
    want = np.concatenate(want)
    assert TG.saturated(want) < SATURATED_MAX * want.size
    outs = []
    for cuts in CUTS:
        assert sum(cuts) == 3000
        rig = Rig(cm, 1, ci, co, max(cuts), [A])
        rig.ramp(0, B, 700)
        got, at = [], 0
        for n in cuts:
            if at == 400:
                rig.ramp(0, Cm, 1000)
                rig.check_state()
            rig.play([x[at:at + n]])
            got.append(rig.dst.array[0, :n * co].reshape(-1, co).copy())
            at += n
        rig.close()
        outs.append(np.concatenate(got))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want)


# ---------------------------------------------------------------------------
# 3. set_matrix cancels a ramp; a ramp of 0 or 1 frames is set_matrix

def test_set_matrix_cancels_and_short_ramps_step(gpu):
    cm = gpu
    for ci, co in ((2, 1), (3, 2)):
        A, B, D = (dense_matrix(ci, co, 70 + 5 * ci + i) for i in range(3))
        xs = [noise(2100 + s, 500, ci) for s in range(2)]
        rig = Rig(cm, 2, ci, co, 500, [A, A])
        for R in (0, 1):                                         # (on a mixer that has never ramped)
            rig.ramp(0, [B, D][R], R)
            assert rig.m.ramp_state(0)[:2] == (0, 0)
            rig.run([x[:300] for x in xs], wants=[model_mix(xs[0][:300], [B, D][R]), model_mix(xs[1][:300], A)])
        rig.ramp(-1, B, 1000)
        rig.play([x[:300] for x in xs])
        assert rig.m.ramp_state(0)[:2] == (300, 1000)
        rig.step(0, D)                                           # stream 0 steps, stream 1 ramps on
        assert rig.m.ramp_state(0)[:2] == (0, 0) and rig.m.ramp_state(1)[:2] == (300, 1000)
        assert np.array_equal(rig.m.get_matrix(0), D)
        ys = rig.play(xs)
        assert np.array_equal(ys[0], model_mix(xs[0], D))
        rig.ramp(1, A, 1)                                        # R = 1 during a ramp: a step as well
        assert rig.m.ramp_state(1)[:2] == (0, 0)
        rig.run(xs, wants=[model_mix(xs[0], D), model_mix(xs[1], A)])
        rig.close()


# ---------------------------------------------------------------------------
# 4. ramp_matrix is ordered with the runs by the stream alone

def test_ordering_without_synchronisation(gpu):
    cm = gpu
    S = 300
    counts = [s % 65 for s in range(S)]
    W = [np.array([[8192 + s, -(4096 + 3 * s)]], dtype=np.int16) for s in range(S)]        # names its stream
    xs = [noise(500 + s, n, 2) for s, n in enumerate(counts)]
    rig = Rig(cm, S, 2, 1, 64, W)
    A, B = np.array([[12000, -3000]], dtype=np.int16), np.array([[-7000, 9000]], dtype=np.int16)
    second = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    rig.src.array[:] = 0x5a5a
    for s, x in enumerate(xs):
        rig.src.array[s, :counts[s] * 2] = x.reshape(-1)
    rig.dst.array[:] = SENTINEL
    second.array[:] = SENTINEL
    m = rig.m
    m.ramp_matrix(-1, A, 100)                                    # no synchronisation anywhere: ramp, run, ramp, run
    m.run(rig.src.dev, rig.in_stride, 64, rig.dst.dev, rig.out_stride, counts)
    m.ramp_matrix(7, B, 40)
    m.run(rig.src.dev, rig.in_stride, 64, second.dev, rig.out_stride, counts)
    m.sync()
    for mod in rig.models:
        mod.ramp(A, 100)
    first = [mod.run(x) for mod, x in zip(rig.models, xs)]
    rig.models[7].ramp(B, 40)
    rig.check(rig.dst.array, first)
    rig.check(second.array, [mod.run(x) for mod, x in zip(rig.models, xs)])
    rig.check_state()
    assert np.array_equal(m.get_matrix(7), B) and np.array_equal(m.get_matrix(8), A)
    second.free()
    rig.close()


# ---------------------------------------------------------------------------
# 5. the extremes of the int32 bound, and the rounding

def test_extremes_and_rounding(gpu):
    cm = gpu
    w16 = np.full(16, 4096, dtype=np.int64) * np.where(np.arange(16) % 3 == 0, -1, 1)
    w16[5] = -(65535 - 15 * 4096)
    for ci, w0, w1 in ((16, w16, -w16), (2, np.array([-32768, 32767]), np.array([32767, -32768]))):
        assert np.abs(w0).sum() == 65535 == np.abs(w1).sum() and (np.sign(w0) == -np.sign(w1)).all()
        kinds = np.array([np.where(w0 < 0, -32768, 32767), np.where(w0 < 0, 32767, -32768), [-32768] * ci, [32767] * ci])
        x = kinds[np.arange(4096) % 4].astype(np.int16)          # full scale, both sign patterns, all along the ramp
        rig = Rig(cm, 1, ci, 1, 4096, [w0.reshape(1, ci).astype(np.int16)])
        rig.ramp(0, w1.reshape(1, ci).astype(np.int16), 4096)
        y = rig.play([x])[0].reshape(-1)                         # (the model asserts its int32 and the row bound)
        assert y[0] == 32767 and y[1] == -32768 and y[4092] == -32768 and y[4093] == 32767
        assert rig.m.ramp_state(0)[:2] == (0, 0)
        rig.close()
    # halves round towards +inf (tests/test_gpu_mix.py's vectors), with {8192, 8192} met at p = 16384: frame 1 of 2
    vec = np.array([[1, 0], [-1, 0], [-1, -2], [32767, 32767], [-32768, -32768]], dtype=np.int16)
    assert ramp_position(1, 2) == 16384 and ramp_weight([0, 16384], [16384, 0], 16384).tolist() == [8192, 8192]
    rig = Rig(cm, 5, 2, 1, 8, [[[0, 16384]]] * 5)
    rig.ramp(-1, [[16384, 0]], 2)
    ys = rig.play([np.array([v, v]) for v in vec])
    assert [y[0, 0] for y in ys] == [1, 0, -1, 32767, -32768] and [y[1, 0] for y in ys] == vec[:, 0].tolist()
    rig.close()


# ---------------------------------------------------------------------------
# 6. a long ramp: positions that repeat, and that leave floor(32768 n / R)

def test_a_long_ramp(gpu):
    cm = gpu
    R = 100000
    n = np.arange(R + 1)
    p = ramp_position(n, R)
    dev = p - (32768 * n) // R
    assert np.abs(dev).max() == 1 and (np.diff(p) == 0).any() and p[R] == 32768
    x = noise(2600, 4 * 32768, 1)
    rig = Rig(cm, 1, 1, 1, 32768, [[[16384]]])
    rig.ramp(0, [[-12000]], R)
    for i in range(4):
        rig.play([x[i * 32768:(i + 1) * 32768]])
        assert rig.m.ramp_state(0)[0] == ((i + 1) * 32768 if i < 3 else 0)
    rig.close()


# ---------------------------------------------------------------------------
# 7. transparency

@pytest.mark.parametrize("channels", [1, 2, 6])
def test_a_ramp_between_identities_is_transparent(gpu, channels):
    cm = gpu
    t = cm.plan_mix(1, channels, channels, 1).tile_frames
    eye = 16384 * np.eye(channels, dtype=np.int16)
    x = noise(2700 + channels, t + 11, channels)
    rig = Rig(cm, 1, channels, channels, t + 11)
    rig.ramp(0, eye, t + 100)
    assert rig.m.ramp_state(0)[:2] == (0, t + 100)
    rig.run([x], wants=[x])
    rig.run([x[:200]], wants=[x[:200]])
    rig.close()


def test_ended_ramps_leave_a_plain_mixer(gpu):
    cm = gpu
    W = [dense_matrix(2, 2, 2800 + s) for s in range(3)]
    xs = [noise(2810 + s, 2500, 2) for s in range(3)]
    plain = Rig(cm, 3, 2, 2, 2500, W)
    ramped = Rig(cm, 3, 2, 2, 2500)
    for s in range(3):
        ramped.ramp(s, W[s], 100 + s)
    ramped.play([x[:300] for x in xs])
    assert all(ramped.m.ramp_state(s)[:2] == (0, 0) for s in range(3))
    a = plain.run(xs)
    ramped.run(xs, wants=a)
    assert np.array_equal(plain.dst.array, ramped.dst.array)
    plain.close()
    ramped.close()


# ---------------------------------------------------------------------------
# 8. refusals change nothing and launch nothing

def test_refusals(gpu):
    cm = gpu
    A, B = np.array([[9000, -5000]], dtype=np.int16), np.array([[-3000, 12000]], dtype=np.int16)
    xs = [noise(2900 + s, 600, 2) for s in range(2)]
    for started in (False, True):                # (before the ramps' state exists, and while a ramp runs)
        rig = Rig(cm, 2, 2, 1, 600, [A, A])
        m = rig.m
        if started:
            rig.ramp(-1, B, 500)
            rig.play([x[:100] for x in xs])
        rig.dst.array[:] = SENTINEL
        before = [m.ramp_state(s) for s in range(2)]
        assert m.ramp_matrix_rc(0, A, RAMP_MAX + 1) == cm.ERROR_INVAL
        assert m.ramp_matrix_rc(0, [[-32768, -32768]], 100) == cm.ERROR_INVAL
        assert m.ramp_matrix_rc(0, [[-32768, -32768]], 1) == cm.ERROR_INVAL
        assert m.ramp_matrix_rc(2, A, 100) == cm.ERROR_INVAL and m.ramp_matrix_rc(-2, A, 100) == cm.ERROR_INVAL
        assert cm.lib.cmhip_mix_ramp_matrix(m.h, 0, None, 100) == cm.ERROR_FAULT
        assert cm.lib.cmhip_mix_ramp_matrix(None, 0, A.ctypes.data, 100) == cm.ERROR_FAULT
        a, b = C.c_uint32(77), C.c_uint32(77)
        assert cm.lib.cmhip_mix_ramp_state(m.h, 2, C.byref(a), C.byref(b), None) == cm.ERROR_INVAL
        assert (a.value, b.value) == (77, 77)
        assert cm.lib.cmhip_mix_ramp_state(m.h, 0, None, None, None) == cm.ERROR_FAULT
        m.sync()
        assert (rig.dst.array == SENTINEL).all()
        for s in range(2):
            now = m.ramp_state(s)
            assert now[:2] == before[s][:2] == ((100, 500) if started else (0, 0))
            assert np.array_equal(now[2], before[s][2])
            assert np.array_equal(m.get_matrix(s), B if started else A)
        rig.play(xs)                             # the running ramp continues unharmed
        assert m.ramp_matrix_rc(1, A, RAMP_MAX) == 0 and m.ramp_state(1)[:2] == (0, RAMP_MAX)
        rig.close()


# ---------------------------------------------------------------------------
# 9. the example

def test_batch_fade_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_fade"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_fade.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    rows = {}
    for ln in out:
        if ln.startswith("block "):
            f = dict(kv.split("=") for kv in ln.split()[2:])
            rows.setdefault(f["phase"], []).append(float(f["power"]))
    assert set(rows) == {"fade-in", "steady", "crossfade", "swapped", "fade-out"}, out
    fade_in, steady, fade_out = rows["fade-in"], rows["steady"], rows["fade-out"]
    assert len(fade_in) >= 4 and all(b > a for a, b in zip(fade_in, fade_in[1:])), fade_in
    assert all(abs(p - steady[-1]) < 0.1 for p in steady + rows["swapped"]), (steady, rows["swapped"])
    assert fade_in[-1] < steady[0] + 0.1
    assert len(fade_out) >= 4 and all(b < a for a, b in zip(fade_out, fade_out[1:])), fade_out
