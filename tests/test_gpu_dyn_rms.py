"""GPU: the RMS detector of the dynamics stage (cmhip_dyn_new_detector, csrc/k_dyn.h) against the RMS model -- the
keyed model of tests/test_gpu_dyn_key.py with the one line L = isqrt(sum(e^2 over A) >> a) in int64 -- bit for bit, the
sentinel past every count and the meter included: dense cases over five geometries and both kernel forms, plain and
with a key map of every kind, the edges of the root on a curve that turns every level's parity into a gain, cuts queued
without a synchronisation, the mean detector through the new constructor, bursts, reset, refusals that launch nothing,
the chain bus -> RMS dynamics with a key -> limiter -> batch, and the C example.  (tests/test_dyn_rms_host.py takes the
model and the cases from here.)"""
import ctypes
import functools
import importlib.util
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def _load(name):
    spec = importlib.util.spec_from_file_location("dynrms_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TK = _load("test_gpu_dyn_key")                    # the keyed model, its rig and its dense cases
TG = TK.TG                                        # the unkeyed model, the signal, the dense curve, the rig
geometry, signal, design, DENSE_CURVE, dense_seed = TG.geometry, TG.signal, TG.design, TG.DENSE_CURVE, TG.dense_seed
SETS, SENTINEL, UNITY = TG.SETS, TG.SENTINEL, TG.UNITY
MEAN, RMS, isqrt = TK.MEAN, TK.RMS, TK.isqrt      # CMHIP_DYN_DETECT_*; the model's root
CHANNELS = [1, 2, 3, 6, 16]
DIFFER_MEAN = 0.25                                # of the long streams' frames whose output differs from the mean detector's
DIFFER_OWN_KEYED = 0.50                           # of a follower's frames whose output differs from its own RMS detector's
DIFFER_MEAN_KEYED = 0.20                          # ... and from the keyed mean detector's


# ---------------------------------------------------------------------------
# the model: TK.model_dyn_keyed with detector = RMS (include/coolmic_hip.h, "dynamics", "RMS detector")

def model_rms(x, hist, T, a, b, H, root=isqrt):
    return TK.model_dyn_keyed(x, hist, x, hist, T, a, b, H, RMS, root)


class RmsRig(TK.KeyRig):
    """TK.KeyRig over a stage made by cmhip_dyn_new_detector and the model of that detector"""

    def __init__(self, cm, streams, channels, a, b, H, max_frames, curve=None, detector=RMS):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Dynamics(streams, channels, a, b, H, max_frames, detector=detector)
        self.model = TK.KeyModel(streams, channels, a, b, H, detector=detector)
        assert self.m.delay() == self.model.D and self.m.detector() == detector
        self.stride = (max_frames * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        if curve is not None:
            self.set(-1, curve)


# ---------------------------------------------------------------------------
# 1. dense cases: five geometries, both forms, ragged and uniform counts

@functools.lru_cache(maxsize=None)
def dense_rms_case(a, b, H, channels, t):
    """TG.dense_case's streams, counts and curve under the RMS model: the outputs of the ragged run and of the uniform
    run that follows it on one stage, the meter, and the figures of the dense conditions -- computed once, never changed"""
    xs, counts, T = TG.dense_case(a, b, H, channels, t)[:3]
    hist = geometry(a, b, H)[4]
    model = TK.KeyModel(len(counts), channels, a, b, H, detector=RMS)
    model.set(-1, T)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    s_all = [sg for per in model.s for sg in per]
    frames = sum(sg.size for sg in s_all)
    unity = sum(int((sg == UNITY).sum()) for sg in s_all) / frames
    change = sum(int((np.diff(sg) != 0).sum()) for sg in s_all) / max(sum(sg.size - 1 for sg in s_all if sg.size), 1)
    smallest = min(int(sg.min()) for sg in s_all)
    # what the mean detector gives for the two longest streams, from silence: a kernel that ignores the detector gives this
    zero = np.zeros((hist, channels), dtype=np.int16)
    differ = min(float((TG.model_dyn(xs[s][:counts[s]], zero, T, a, b, H)[0] != ragged[s]).any(axis=1).mean())
                 for s in range(2))
    return xs, counts, T, ragged, full, unity, change, smallest, list(model.gmin), differ


def assert_dense_rms(a, b, H, unity, change, smallest, differ):
    """held on the MODEL before anything is compared: the gain moves, the gate closes, and the detector matters"""
    TG.assert_dense(a, b, H, unity, change, smallest)
    assert differ >= DIFFER_MEAN, (a, b, H, differ)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("a,b,H", SETS)
def test_dense(gpu, a, b, H, channels):
    cm = gpu
    plan = cm.plan_dynrms(8, channels, a, b, H, 1)
    mean = cm.plan_dyn(8, channels, a, b, H, 1)
    assert plan.fast == (1 if channels <= 2 else 0) and plan.passes == mean.passes + a
    assert (plan.tile_frames, plan.halo, plan.lds_bytes, plan.grid) == (mean.tile_frames, mean.halo, mean.lds_bytes, mean.grid)
    t = plan.tile_frames
    xs, counts, T, ragged, full, unity, change, smallest, gmin, differ = dense_rms_case(a, b, H, channels, t)
    print("dyn rms dense a %2d b %d H %4d C %2d: tile %d, unity %.1f %%, changing %.1f %%, min s %d, differing from the "
          "mean detector %.1f %%" % (a, b, H, channels, t, 100 * unity, 100 * change, smallest, 100 * differ))
    assert_dense_rms(a, b, H, unity, change, smallest, differ)
    rig = RmsRig(cm, len(counts), channels, a, b, H, counts[0], T)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. dense keyed cases: the key map and the groups of TK.dense_key_case

@functools.lru_cache(maxsize=None)
def dense_rms_key_case(a, b, H, channels, t):
    """TK.dense_key_case's streams, counts, map and curve under the RMS model, with the shares of the followers' frames
    (the two long groups, from silence) that differ from their own RMS detector's and from the keyed mean detector's"""
    xs, counts, keys, T, mean_ragged = TK.dense_key_case(a, b, H, channels, t)[:5]
    hist = geometry(a, b, H)[4]
    model = TK.KeyModel(len(counts), channels, a, b, H, detector=RMS)
    model.set(-1, T)
    for s, k in enumerate(keys):
        model.set_key(s, k)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    zero = np.zeros((hist, channels), dtype=np.int16)
    own, mean = [], []
    for s in range(2 * TK.GROUP):
        if keys[s] != s:
            alone = model_rms(xs[s][:counts[s]], zero, T, a, b, H)[0]
            own.append(float((alone != ragged[s]).any(axis=1).mean()))
            mean.append(float((mean_ragged[s] != ragged[s]).any(axis=1).mean()))
    followers = [s for s in range(len(counts)) if keys[s] != s]
    s_all = [sg for s in followers for sg in model.s[s]]
    change = sum(int((np.diff(sg) != 0).sum()) for sg in s_all) / sum(sg.size - 1 for sg in s_all)
    smallest = min(int(sg.min()) for sg in s_all)
    return xs, counts, keys, T, ragged, full, list(model.gmin), min(own), min(mean), change, smallest


def assert_dense_rms_key(own, mean, change, smallest):
    """held on the MODEL before anything is compared: a kernel that ignores the key or the detector cannot pass"""
    assert own >= DIFFER_OWN_KEYED and mean >= DIFFER_MEAN_KEYED and change >= TG.CHANGE_SHARE and smallest < TG.MIN_S, \
        (own, mean, change, smallest)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("a,b,H", SETS)
def test_dense_keyed(gpu, a, b, H, channels):
    cm = gpu
    t = cm.plan_dynrms(8, channels, a, b, H, 1).tile_frames
    xs, counts, keys, T, ragged, full, gmin, own, mean, change, smallest = dense_rms_key_case(a, b, H, channels, t)
    print("dyn rms keyed dense a %2d b %d H %4d C %2d: tile %d, differing from the own detector %.1f %%, from the keyed "
          "mean detector %.1f %%, changing %.1f %%, min s %d" % (a, b, H, channels, t, 100 * own, 100 * mean, 100 * change,
                                                                  smallest))
    assert_dense_rms_key(own, mean, change, smallest)
    rig = RmsRig(cm, len(counts), channels, a, b, H, counts[0], T)
    rig.set_map(keys)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream, the same map
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 3. the edges of the root: constant magnitudes r, then the same with every A-th frame at r - 1 (M just below r * r)

ROOT_EDGES = [1, 2, 3, 8, 181, 182, 4095, 4096, 23170, 23171, 32767, 32768]
ROOT_SETS = [(10, 3, 0), (3, 3, 0), (6, 6, 0)]


def sawtooth():
    """T[k] = 32768 for even k, 0 for odd k: a level one off lands on another line between two knots, or another knot"""
    T = np.zeros(TG.CURVE, dtype=np.uint16)
    T[0:TG.USED:2] = UNITY
    return T


def root_edge_signal(a, b, H):
    """mono int16 [n][1]: per r of ROOT_EDGES a stretch of magnitude r with alternating sign (-32768 for 32768), then a
    stretch of the same length in which every A-th frame has magnitude r - 1; a stretch outlasts the history and a
    window, and is a multiple of A"""
    A, B, D, W, hist = geometry(a, b, H)
    n = -(-(max(2 * A, hist + A) + A) // A) * A
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    parts = []
    for r in ROOT_EDGES:
        flat_ = np.full(n, r, dtype=np.int64)
        dip = flat_.copy()
        dip[A - 1::A] = r - 1
        for m in (flat_, dip):
            parts.append(np.where(m == 32768, -32768, m * sign))
    x = np.concatenate(parts)
    assert x.min() >= -32768 and x.max() <= 32767
    return x.astype(np.int16)[:, None], n


def root_float32(v):
    """a root taken as a truncated single-precision sqrt of the mean square"""
    return np.sqrt(np.asarray(v).astype(np.float32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def root_edge_case(a, b, H):
    x, n = root_edge_signal(a, b, H)
    hist = geometry(a, b, H)[4]
    zero = np.zeros((hist, 1), dtype=np.int16)
    T = sawtooth()
    want = model_rms(x, zero, T, a, b, H)
    wrong = {name: float((model_rms(x, zero, T, a, b, H, root)[0] != want[0]).any(axis=1).mean())
             for name, root in (("plus one", lambda v: isqrt(v) + 1), ("minus one", lambda v: np.maximum(isqrt(v) - 1, 0)))}
    f32 = int((model_rms(x, zero, T, a, b, H, root_float32)[0] != want[0]).any(axis=1).sum())
    return x, n, T, want, wrong, f32


@pytest.mark.parametrize("a,b,H", ROOT_SETS)
def test_root_edges(gpu, a, b, H):
    cm = gpu
    x, n, T, want, wrong, f32 = root_edge_case(a, b, H)
    print("dyn rms root edges a %2d b %d H %d: %d frames, a root one too large changes %.1f %% of them, one too small "
          "%.1f %%, a truncated float32 sqrt %d frames" % (a, b, H, x.shape[0], 100 * wrong["plus one"],
                                                          100 * wrong["minus one"], f32))
    assert x.shape[0] == 2 * len(ROOT_EDGES) * n and (a != 10 or x.shape[0] == 98304)
    assert wrong["plus one"] >= 0.5 and wrong["minus one"] >= 0.5          # held on the MODEL: the test separates both
    assert a != 10 or f32 > 0                                    # ... and a root that rests on single-precision rounding
    rig = RmsRig(cm, 1, 1, a, b, H, x.shape[0], T)
    got = rig.run([x])
    assert np.array_equal(got[0], want[0])
    rig.close()


# ---------------------------------------------------------------------------
# 4. cuts: TG.test_cuts' and TK.test_cuts_keyed's chunkings on RMS stages, queued without a synchronisation

CUT_SETS = [(1, 6, 6, 0), (2, 8, 5, 100), (6, 5, 9, 7), (2, 9, 9, 1024)]


@pytest.mark.parametrize("channels,a,b,H", CUT_SETS)
def test_cuts(gpu, channels, a, b, H):
    cm = gpu
    t = cm.plan_dynrms(2, channels, a, b, H, 1).tile_frames
    hist = geometry(a, b, H)[4]
    T = design(**DENSE_CURVE)
    x = [signal(7000 + 10 * channels + s, 3 * t, channels) for s in range(2)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [model_rms(v, zero, T, a, b, H) for v in x]
    assert all((w[0] != TG.model_dyn(v, zero, T, a, b, H)[0]).any(axis=1).mean() >= DIFFER_MEAN for v, w in zip(x, want))
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    for starve in (False, True):
        # stream 0 is cut as the list says; stream 1 in the same runs, or with 0 frames in alternate runs
        dyn = cm.Dynamics(2, channels, a, b, H, 3 * t, curve=T, detector=RMS)
        chunks, pos = [], [0, 0]
        for r, n in enumerate(cuts):
            n1 = 0 if starve and r % 2 else n
            chunks.append([x[0][pos[0]:pos[0] + n], x[1][pos[1]:pos[1] + n1]])
            pos = [pos[0] + n, pos[1] + n1]
        outs = TG.run_chunks(cm, dyn, channels, chunks)
        for s in range(2):
            got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
            assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), (starve, s)
            for arr, counts in outs:
                assert (arr[s, counts[s] * channels:] == SENTINEL).all()
        assert dyn.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(2)]
        dyn.close()


@pytest.mark.parametrize("channels,a,b,H", CUT_SETS)
def test_cuts_keyed(gpu, channels, a, b, H):
    cm = gpu
    keys = TK.CUT_KEYS
    t = cm.plan_dynrms(6, channels, a, b, H, 1).tile_frames
    hist = geometry(a, b, H)[4]
    T = design(**DENSE_CURVE)
    S = len(keys)
    x = [signal(9000 + 10 * channels + s, 3 * t, channels) for s in range(S)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [TK.model_dyn_keyed(x[s], zero, x[k], zero, T, a, b, H, RMS) for s, k in enumerate(keys)]
    for s, k in enumerate(keys):
        assert k == s or (want[s][0] != model_rms(x[s], zero, T, a, b, H)[0]).any(axis=1).mean() >= DIFFER_OWN_KEYED, s
        mean = TK.model_dyn_keyed(x[s], zero, x[k], zero, T, a, b, H)[0]
        assert (want[s][0] != mean).any(axis=1).mean() >= DIFFER_MEAN_KEYED, s
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    dyn = cm.Dynamics(S, channels, a, b, H, 3 * t, curve=T, detector=RMS)
    for s, k in enumerate(keys):
        dyn.set_key(s, k)
    chunks, pos = [], [0] * S
    for r, n in enumerate(cuts):
        ns = [n] * 4 + [0 if r % 2 else n] * 2                   # the pair 4 -> 5 gets 0 frames in alternate runs
        chunks.append([x[s][pos[s]:pos[s] + ns[s]] for s in range(S)])
        pos = [p + m for p, m in zip(pos, ns)]
    outs = TG.run_chunks(cm, dyn, channels, chunks)
    for s in range(S):
        got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
        assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), s
        for arr, counts in outs:
            assert (arr[s, counts[s] * channels:] == SENTINEL).all()
    assert pos[:4] == [3 * t] * 4 and 0 < pos[4] == pos[5] < 3 * t
    assert dyn.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(S)]
    dyn.close()


# ---------------------------------------------------------------------------
# 5. the mean detector through the new constructor; an RMS stage without a key

def test_detector_zero_is_the_old_stage(gpu):
    cm = gpu
    a, b, H, ch = 6, 6, 0, 2
    t = cm.plan_dyn(8, ch, a, b, H, 1).tile_frames
    xs, counts, T, ragged, full = TG.dense_case(a, b, H, ch, t)[:5]
    outs = []
    for detector in (None, MEAN):
        m = cm.Dynamics(len(counts), ch, a, b, H, counts[0], curve=T, detector=detector)
        assert m.delay() == (1 << b) - 1 and m.detector() == MEAN
        m.close()
        rig = RmsRig(cm, len(counts), ch, a, b, H, counts[0], T, detector=MEAN) if detector == MEAN else \
            TG.Rig(cm, len(counts), ch, a, b, H, counts[0], T)
        got = rig.run([x[:n] for x, n in zip(xs, counts)])           # (compared with the mean model inside)
        assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
        got = rig.run(xs, uniform=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, full))
        outs.append(rig.dst.array.copy())
        rig.close()
    assert np.array_equal(outs[0], outs[1])                      # bit-identical arrays, the sentinel included


def test_rms_without_a_key(gpu):
    cm = gpu
    a, b, H, ch = 6, 6, 0, 2
    t = cm.plan_dynrms(4, ch, a, b, H, 1).tile_frames
    xs = [signal(1700 + s, t + 77, ch) for s in range(4)]
    T = design(**DENSE_CURVE)
    zero = np.zeros((geometry(a, b, H)[4], ch), dtype=np.int16)
    plain = [model_rms(x, zero, T, a, b, H)[0] for x in xs]
    rig = RmsRig(cm, 4, ch, a, b, H, t + 77, T)
    got = rig.run(xs)
    assert all(np.array_equal(g, w) for g, w in zip(got, plain))
    rig.reset()
    rig.set_key(0, 3)
    rig.m.set_key(-1, -1)
    rig.model.set_key(-1, -1)
    assert [rig.m.get_key(s) for s in range(4)] == [-1] * 4
    got = rig.run(xs)
    assert all(np.array_equal(g, w) for g, w in zip(got, plain))
    rig.run([x[:100] for x in xs])
    rig.close()


# ---------------------------------------------------------------------------
# 6. literal edges, state and refusals

@pytest.mark.parametrize("channels", [1, 2, 6])
def test_bursts_at_a_tile_edge_and_at_the_history_length(gpu, channels):
    """TG's bursts on an RMS stage: one straddles a tile edge, the last frame of the other lies exactly HIST frames before
    the second run begins -- that run's first output still sees it through the history, the next one does not"""
    cm = gpu
    a, b, H = 6, 5, 100
    A, B, D, W, hist = geometry(a, b, H)
    t = cm.plan_dynrms(1, channels, a, b, H, 1).tile_frames
    T = TG.steps()
    base = int(TG.curve_at(T, np.array([300]))[0])               # constant magnitude: the level is 300 under both detectors
    n = t + 500
    x = np.full((n, channels), 300, dtype=np.int16)
    x[t - 10:t + 10, channels - 1] = -32768
    x[n - hist - 49:n - hist + 1] = 30000                        # its last frame is frame n - hist
    rig = RmsRig(cm, 1, channels, a, b, H, n, T)
    rig.run([x])
    s = rig.model.s[0][0]
    assert s[t - B] == base and s[t - 1] != base and s[t] != base
    rig.run([np.full((n, channels), 300, dtype=np.int16)])
    s2 = rig.model.s[0][1]
    assert s2[0] != base and s2[1] == base                       # frame n - hist is the oldest that frame n depends on
    rig.close()


def test_reset_and_the_meter(gpu):
    cm = gpu
    a, b, H = 5, 4, 20
    T = design(**DENSE_CURVE)
    xs = [signal(600 + s, 700, 1) for s in range(3)]
    rig = RmsRig(cm, 3, 1, a, b, H, 700, T)
    rig.run(xs)
    assert all(g < UNITY for g in rig.model.gmin)
    assert rig.m.min_gain(reset=True).tolist() == rig.model.gmin
    assert rig.m.min_gain().tolist() == [UNITY] * 3              # re-armed, the history kept
    rig.model.gmin = [UNITY] * 3
    rig.run([np.full((50, 1), 20000, dtype=np.int16)] * 3)
    rig.reset(1)                                                 # stream 1 starts again from silence, 0 and 2 go on
    ys = rig.run(xs)
    zero = np.zeros((geometry(a, b, H)[4], 1), dtype=np.int16)
    assert np.array_equal(ys[1], model_rms(xs[1], zero, T, a, b, H)[0])
    assert not np.array_equal(ys[0][:40], model_rms(xs[0], zero, T, a, b, H)[0][:40])
    rig.close()


def test_refusals(gpu):
    cm = gpu
    lib = cm.lib
    for detector in (2, 0xffffffff):
        d = cm.DynDesc(0, 2, 2, 6, 6, 0, 256, None)
        assert lib.cmhip_dyn_new_detector(ctypes.byref(d), detector) is None and b"dyn_new:" in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Dynamics(2, 2, 6, 6, 0, 256, detector=detector)
    rig = RmsRig(cm, 4, 2, 6, 6, 0, 256, design(**DENSE_CURVE))
    m, src, dst, st = rig.m, rig.src.dev, rig.dst.dev, rig.stride
    assert st == 520
    rig.set_key(0, 1)
    xs = [signal(700 + s, 256, 2) for s in range(4)]
    rig.run(xs)                                                  # a history that a launch would change
    rig.dst.array[:] = SENTINEL
    rig.src.array[:] = SENTINEL
    cases = {
        "misaligned in": (src + 2, st, 256, dst, st, None),
        "misaligned out": (src, st, 256, dst + 8, st, None),
        "in stride not a multiple of 8": (src, st + 4, 256, dst, st, None),
        "out stride not a multiple of 8": (src, st, 256, dst, st - 4, None),
        "in stride too small": (src, 504, 256, dst, st, None),
        "out stride too small": (src, st, 256, dst, 504, None),
        "frames above max_frames": (src, st, 257, dst, st, None),
        "a count above frames": (src, st, 100, dst, st, [100, 100, 100, 101]),
        "a keyed stream and its key with different counts": (src, st, 256, dst, st, [100, 101, 100, 7]),
        "in == out": (src, st, 256, src, st, None),
        "out inside in": (src, st, 256, src + 16, st, None),
        "in begins inside out": (dst + 2 * st, st, 256, dst, st, None),
    }
    for name, (i, ist, n, o, ost, fps) in cases.items():
        assert m.run_rc(i, ist, n, o, ost, fps) == cm.ERROR_INVAL, name
    assert lib.cmhip_dyn_run(m.h, None, st, 256, None, dst, st) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_run(m.h, src, st, 256, None, None, st) == cm.ERROR_FAULT
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.run(xs)                                                  # the history and the parity are what the first run left
    rig.close()


# ---------------------------------------------------------------------------
# 7. composition: bus -> RMS dynamics with one key -> limiter -> the slots of a batch, five ragged blocks on one stream

CHAIN_BLOCKS = TG.CHAIN_BLOCKS                    # per programme: the counts of its bed and its voice, block by block


def test_chain_with_an_rms_stage_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    tb = _load("test_gpu_bus")
    TL = TG.TL
    cm = gpu
    P, F = 2, 4100                                               # programmes; bus outputs 2p (bed), 2p + 1 (voice)
    S, B1 = 4 * P, 2 * P                                         # two sources per sum
    a, b, H, la, lh, T_lim, drive = 6, 6, 30, 6, 30, 29204, 6144
    duck = cm.dyn_design_duck(threshold_db=-36.0, depth_db=14.0, knee_db=8.0)
    comp = design(**DENSE_CURVE)
    sum_of = [s // 2 for s in range(S)]
    prog_of = [q // 2 for q in sum_of]
    total = [sum(CHAIN_BLOCKS[prog_of[s]]) for s in range(S)]
    xs = [TG.bursts(2000 + s, total[s], 1) for s in range(S)]
    for s in range(S):
        if sum_of[s] % 2:                                        # the presenters pause: the bed comes back up
            xs[s][1000:2500] = 0
    table = (sum_of, list(range(S)), np.full((S, 1, 1), 8192, dtype=np.int16))
    dyn_m, lim_m = TK.KeyModel(B1, 1, a, b, H, detector=RMS), TL.Model(B1, 1, la, lh)
    for p in range(P):
        dyn_m.set(2 * p, duck)
        dyn_m.set(2 * p + 1, comp)
        dyn_m.set_key(2 * p, 2 * p + 1)
    lim_m.set(-1, T_lim, drive)
    objects, arrays = [], []
    try:
        batch = cm.Batch(B1, 1, F, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, rate=48000)
        objects.append(batch)
        st = batch.hip_stream()
        bus = cm.Bus(S, B1, 1, 1, F, 16, hip_stream=st)
        objects.append(bus)
        dyn = cm.Dynamics(B1, 1, a, b, H, F, hip_stream=st, detector=RMS)
        objects.append(dyn)
        lim = cm.Limiter(B1, 1, la, lh, F, threshold=T_lim, drive=drive, hip_stream=st)
        objects.append(lim)
        assert bus.hip_stream() == dyn.hip_stream() == lim.hip_stream() == st and dyn.detector() == RMS
        bus.set_routing(*table)
        for p in range(P):
            dyn.set_curve(2 * p, duck)
            dyn.set_curve(2 * p + 1, comp)
            dyn.set_key(2 * p, 2 * p + 1)
        stride = (F + 7) // 8 * 8 + 8
        d_sum, d_dyn, d_lim = (cm.DeviceWords((B1 * s_ * 2 + 7) // 8) for s_ in (stride, stride, batch.stride))
        arrays += [d_sum, d_dyn, d_lim]
        wants, results, pos = [], [], [0] * S
        for r in range(len(CHAIN_BLOCKS[0])):
            counts = [CHAIN_BLOCKS[prog_of[s]][r] for s in range(S)]
            ins = [xs[s][pos[s]:pos[s] + counts[s]] for s in range(S)]
            pos = [p + n for p, n in zip(pos, counts)]
            outs = lim_m.run(dyn_m.run(tb.model_bus(ins, table, B1, 1)))
            wants.append(outs)
            feed = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride))
            res = cm.MappedPcm(batch)
            feed.array[:] = 0x5a5a
            res.array[:] = SENTINEL
            for s, x in enumerate(ins):
                feed.array[s, :x.size] = x.reshape(-1)
            results.append(res)
            arrays += [feed, res]
            # (no wait anywhere: the order is the stream's)
            kb = bus.run(feed.dev, stride, max(counts), d_sum.dev, stride, counts)
            assert kb.tolist() == [CHAIN_BLOCKS[q // 2][r] for q in range(B1)]    # equal within a keyed pair
            dyn.run(d_sum.dev, stride, int(kb.max()), d_dyn.dev, stride, kb)
            lim.run(d_dyn.dev, stride, int(kb.max()), d_lim.dev, batch.stride, kb)
            batch.run_slots(int(kb.max()), d_lim.dev, res.dev, kb)
        batch.sync()                                             # (the only synchronisation)
        for r, outs in enumerate(wants):
            for q in range(B1):
                want = outs[q].reshape(-1)
                have = results[r].array[q, :want.size]
                bad = np.flatnonzero(have != want)
                assert bad.size == 0, ("block", r, "stream", q, "first mismatch at frame", int(bad[0]), "of", want.size)
                assert (results[r].array[q, want.size:] == SENTINEL).all(), ("block", r, "stream", q)
        assert dyn.min_gain().tolist() == dyn_m.gmin and lim.min_gain().tolist() == lim_m.gmin
        floor = int(duck[:123].min())
        for p in range(P):                                       # the bed was ducked all the way, and came back up
            assert dyn_m.gmin[2 * p] == floor < 8000 and max(int(sg.max()) for sg in dyn_m.s[2 * p]) == UNITY
        vu, rcs = batch.vu_results()
        for q in range(B1):
            y = np.concatenate([outs[q].reshape(-1) for outs in wants])
            v = oracle.vu_new(1)
            oracle.vu_accumulate(v, y)
            _, vr = oracle.vu_result(v)
            assert rcs[q] == 0 and oracle_ffi.vu_result_dict(vr) == vu[q].as_dict(), q
            assert vu[q].frames == sum(CHAIN_BLOCKS[q // 2]) and abs(vu[q].global_peak) <= T_lim
    finally:                                 # (the stages that borrow the batch's stream go before the batch, whatever the outcome)
        for o in reversed(objects):
            o.close()
        for o in arrays:
            o.free()


# ---------------------------------------------------------------------------
# 8. the example

SINE_AMPLITUDE, EXAMPLE_FRAMES, EXAMPLE_RATE, EXAMPLE_HZ = 23170, 48000, 48000, 997
EXAMPLE_SET = (10, 6, 0)
EXAMPLE_CURVE = dict(ct=-12.0, R=4.0, K=0.0, gt=-96.0, Re=1.0, rng=0.0)


def example_figures(T):
    """the model's meters for the example's two streams, a 997 Hz sine of amplitude 23170 and a square wave of equal
    power (amplitude 16384 = round(23170 / sqrt 2)), over the last 4096 frames (the steady state), under both detectors
    -> {detector: [sine, square]}"""
    a, b, H = EXAMPLE_SET
    n = np.arange(EXAMPLE_FRAMES)
    sine = np.floor(SINE_AMPLITUDE * np.sin(2 * np.pi * EXAMPLE_HZ * n / EXAMPLE_RATE) + 0.5).astype(np.int16)[:, None]
    square = np.where((n // 24) % 2 == 0, 16384, -16384).astype(np.int16)[:, None]
    zero = np.zeros((geometry(a, b, H)[4], 1), dtype=np.int16)
    out = {}
    for name, f in (("mean", lambda x: TG.model_dyn(x, zero, T, a, b, H)), ("rms", lambda x: model_rms(x, zero, T, a, b, H))):
        out[name] = [int(f(x)[1][-4096:].min()) for x in (sine, square)]
    return out


def test_batch_rmscomp_in_c(gpu, tmp_path):
    cm = gpu
    exe = tmp_path / "batch_rmscomp"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_rmscomp.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(out) == 3 and out[0].startswith("a 997 Hz sine and a square wave of equal power -> compressor: delay 63")
    f = {ln.split(":")[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in out[1:]}
    T = cm.dyn_design(comp_threshold_db=-12.0, comp_ratio=4.0)
    assert np.array_equal(T, design(**EXAMPLE_CURVE))
    want = example_figures(T)
    for name in ("mean", "rms"):
        assert [int(f[name]["sine_gain"]), int(f[name]["square_gain"])] == want[name], (name, f[name], want[name])
    # equal power, equal gain: 1024 frames are 21.27 periods, so a window's mean square ripples by at most 1 / (2 pi 21.27)
    # = 0.75 %, the level by half of that, 0.03 dB, and the gain, at 3/4 dB per dB, by 0.3 % of about 19500 -- below 100
    # units -- while the mean detector reads the sine 0.91 dB lower and lets it through 0.68 dB (8 %) louder
    assert abs(want["rms"][0] - want["rms"][1]) <= 100 and want["mean"][0] - want["mean"][1] >= 1000
    assert f["rms"]["sine_db"] == f["rms"]["square_db"] == "-4.5" and f["mean"]["sine_db"] == "-3.8"
