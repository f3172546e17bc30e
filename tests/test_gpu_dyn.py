"""GPU: the dynamics stage (cmhip_dyn_*, csrc/k_dyn.hip) against a numpy model of the arithmetic include/coolmic_hip.h
states, bit for bit: both kernel forms over five geometries on a signal of bursts with a designed compressor / gate
curve, ragged and uniform counts around the tile and the history length, a stream cut into runs without a
synchronisation, literal edges of the curve's index, per-stream curves and their order with the runs, reset and the gain
meter, refusals that launch nothing, the chain bus -> dynamics -> limiter -> batch on one stream block by block, and the
C example.  Output slots are pre-filled with a sentinel; every sample past a stream's count must still hold it after a
run.  (tests/test_dyn_host.py takes the model, the signal and the dense cases from here.)"""
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
SENTINEL = -21555                                 # what the output slots hold before a run
UNITY = 32768
CURVE = 128                                       # CMHIP_DYN_CURVE
USED = 123                                        # entries 0..122 are read


def _load(name):
    spec = importlib.util.spec_from_file_location("dyn_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TL = _load("test_gpu_lim")                        # the limiter's tests: the bursts signal and the limiter's model
bursts = TL.bursts


# ---------------------------------------------------------------------------
# the model: include/coolmic_hip.h, "dynamics", in numpy

def geometry(a, b, H):
    """-> A, B, D, W, HIST"""
    A, B = 1 << a, 1 << b
    return A, B, B - 1, B + H, (A - 1) + (B + H - 1) + (B - 1)


def curve_index(l):
    """l int64 [n] in 0..32768 -> idx, frac, sh as the header states them, case by case"""
    l = np.asarray(l, dtype=np.int64)
    E = np.searchsorted(2 ** np.arange(1, 17), l, side="right")          # floor(log2 l) for l >= 1
    hi = E >= 3
    up, dn = np.maximum(E - 3, 0), np.maximum(3 - E, 0)
    idx = 1 + 8 * E + np.where(hi, (l >> up) & 7, (l << dn) & 7)
    frac = np.where(hi, l & ((1 << up) - 1), 0)
    sh = np.where(hi, E - 3, 0)
    zero = l == 0
    return np.where(zero, 0, idx), np.where(zero, 0, frac), np.where(zero, 0, sh)


def curve_at(T, l):
    T = np.asarray(T, dtype=np.int64)
    idx, frac, sh = curve_index(l)
    return T[idx] + (((T[idx + 1] - T[idx]) * frac) >> sh)


def _sums(v, n):
    """sliding sums of n: entry i is sum(v[i .. i + n - 1])"""
    c = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    return c[n:] - c[:-n]


def model_dyn(x, hist, T, a, b, H):
    """x int16 [F][C]; hist int16 [HIST][C], oldest first; T the curve -> y int16 [F][C], s int64 [F]"""
    A, B, D, W, HIST = geometry(a, b, H)
    F = x.shape[0]
    if F == 0:
        return x.copy(), np.zeros(0, np.int64)
    z = np.concatenate([hist, x]).astype(np.int64)
    e = np.abs(z).max(axis=1)
    L = _sums(e, A) >> a
    l = np.lib.stride_tricks.sliding_window_view(L.astype(np.int32), W).max(axis=1).astype(np.int64)
    g = curve_at(T, l)
    s = _sums(g, B) >> b                                                 # F entries
    assert s.size == F and L.max() <= UNITY and s.max() <= UNITY and s.min() >= 0
    xd = z[HIST - D: HIST - D + F]
    y = (xd * s[:, None] + (1 << 14)) >> 15
    assert (np.abs(y) <= np.abs(xd)).all()
    return y.astype(np.int16), s


def next_hist(hist, x):
    """the history after a run: the last HIST frames of (hist, x)"""
    return np.concatenate([hist, x])[-hist.shape[0]:]


def design(ct=0.0, R=1.0, K=0.0, gt=-96.0, Re=1.0, rng=0.0):
    """the designer's formula in numpy doubles -> int64 [128]"""
    k = np.arange(1, USED)
    v = (8 + (k - 1) % 8) * 2.0 ** ((k - 1) // 8 - 3)
    x = 20 * np.log10(v / 32768.0)
    d = x - ct
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = (1 / R - 1) * (d + K / 2) ** 2 / (2 * K) if K > 0 else np.zeros_like(d)
    comp = np.where(2 * d < -K, 0.0, np.where((2 * np.abs(d) <= K) & (K > 0), knee, (1 / R - 1) * d))
    gate = np.where((x < gt) & (rng > 0), np.maximum(-rng, (x - gt) * (Re - 1)), 0.0)
    out = np.zeros(CURVE, dtype=np.int64)
    out[1:USED] = np.minimum(32768, np.floor(32768 * 10 ** ((comp + gate) / 20) + 0.5))
    out[0] = min(32768, int(np.floor(32768 * 10 ** (-rng / 20) + 0.5)))
    return out


DENSE_CURVE = dict(ct=-18.0, R=4.0, K=6.0, gt=-45.0, Re=2.0, rng=40.0)


def flat(value):
    return np.full(CURVE, value, dtype=np.uint16)


def signal(seed, frames, channels):
    """the limiter tests' bursts with one near-silent stretch, frames 300..363 within +-2: the level falls to the E < 3
    knots and, at the shortest geometry too, the gate closes all the way (without it the smallest s of (3, 3, 0) is the
    ramp out of the silent history, 3354)"""
    x = bursts(seed, frames, channels).copy()
    if frames > 300:
        n = min(64, frames - 300)
        x[300:300 + n] = np.random.default_rng(seed + 77).integers(-2, 3, size=(n, channels))
    return x


class Model:
    """the streams of a dynamics stage as the header states them: raw history, curves, the meter"""

    def __init__(self, streams, channels, a, b, H):
        self.S, self.C, self.a, self.b, self.H = streams, channels, a, b, H
        self.A, self.B, self.D, self.W, self.HIST = geometry(a, b, H)
        self.hist = [np.zeros((self.HIST, channels), dtype=np.int16) for _ in range(streams)]
        self.curve = [flat(UNITY).astype(np.int64)] * streams
        self.gmin = [UNITY] * streams
        self.s = [[] for _ in range(streams)]        # every s a run gave, for the dense conditions

    def set(self, stream, T):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.curve[s] = np.asarray(T, dtype=np.int64)

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.hist[s] = np.zeros((self.HIST, self.C), dtype=np.int16)
            self.gmin[s] = UNITY

    def run(self, xs):
        ys = []
        for s, x in enumerate(xs):
            x = np.asarray(x, dtype=np.int16).reshape(-1, self.C)
            y, sg = model_dyn(x, self.hist[s], self.curve[s], self.a, self.b, self.H)
            self.hist[s] = next_hist(self.hist[s], x)
            if sg.size:
                self.gmin[s] = min(self.gmin[s], int(sg.min()))
                self.s[s].append(sg)
            ys.append(y)
        return ys


class Rig:
    """a dynamics stage between two arrays of pinned, device-mapped host memory, and its model"""

    def __init__(self, cm, streams, channels, a, b, H, max_frames, curve=None):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Dynamics(streams, channels, a, b, H, max_frames)
        self.model = Model(streams, channels, a, b, H)
        assert self.m.delay() == self.model.D
        self.stride = (max_frames * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        if curve is not None:
            self.set(-1, curve)

    def set(self, stream, T):
        self.m.set_curve(stream, T)
        self.model.set(stream, T)
        for s in (range(self.S) if stream < 0 else [stream]):
            assert np.array_equal(self.m.get_curve(s), np.asarray(T))

    def reset(self, stream=-1):
        self.m.reset(stream)
        self.model.reset(stream)

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def fill(self, xs):
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        self.src.array[:] = 0x5a5a
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        return counts

    def run(self, xs, frames=None, uniform=False):
        """xs: per stream int16 [F_s][C]; runs the device and the model, compares outputs, the untouched rest and the
        meter; -> the model's outputs"""
        counts = self.fill(xs)
        frames = max(counts) if frames is None else frames
        assert not uniform or all(n == frames for n in counts)
        self.dst.array[:] = SENTINEL
        self.m.run(self.src.dev, self.stride, frames, self.dst.dev, self.stride, None if uniform else counts)
        self.m.sync()
        wants = self.model.run(xs)
        self.check(self.dst.array, wants)
        assert self.m.min_gain().tolist() == self.model.gmin
        return wants

    def check(self, array, wants):
        for s, want in enumerate(wants):
            n = want.size
            have = array[s, :n].reshape(-1, self.C)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(),
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (array[s, n:] == SENTINEL).all(), ("stream", s, "written past its count")


# ---------------------------------------------------------------------------
# 1. dense cases: five geometries, both forms, ragged and uniform counts

SETS = [(3, 3, 0), (6, 6, 0), (8, 5, 100), (10, 9, 1536), (5, 9, 7)]
CHANNELS = [1, 2, 3, 6, 16]
CHANGE_SHARE = 0.25                               # of adjacent frames of the model whose s differs, at least
MIN_S = 1000                                      # the model's smallest s lies below
UNITY_SHARE = {(3, 3, 0): 0.20, (6, 6, 0): 0.20}  # of the model's frames with s = 32768, at least


def dense_counts(t, hist):
    return [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 1, 0]


def dense_seed(a, b, H, channels, stream):
    return 100000 * a + 7000 * b + 10 * H + 1000 * channels + stream + 1


@functools.lru_cache(maxsize=None)
def dense_case(a, b, H, channels, t):
    """the streams' full-length inputs, the curve, and over the ragged run followed by the uniform run on one stage: the
    model's outputs of both and the figures of the dense condition -- computed once, never changed"""
    hist = geometry(a, b, H)[4]
    counts = dense_counts(t, hist)
    xs = [signal(dense_seed(a, b, H, channels, s), counts[0], channels) for s in range(len(counts))]
    T = design(**DENSE_CURVE)
    model = Model(len(counts), channels, a, b, H)
    model.set(-1, T)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    s_all = [sg for per in model.s for sg in per]
    frames = sum(sg.size for sg in s_all)
    unity = sum(int((sg == UNITY).sum()) for sg in s_all) / frames
    change = sum(int((np.diff(sg) != 0).sum()) for sg in s_all) / max(sum(sg.size - 1 for sg in s_all if sg.size), 1)
    smallest = min(int(sg.min()) for sg in s_all)
    return xs, counts, T, ragged, full, unity, change, smallest, list(model.gmin)


def assert_dense(a, b, H, unity, change, smallest):
    """a test must not pass on a signal that leaves the gain flat: held on the MODEL, before anything is compared"""
    assert change >= CHANGE_SHARE and smallest < MIN_S and unity >= UNITY_SHARE.get((a, b, H), 0.0), \
        (a, b, H, unity, change, smallest)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("a,b,H", SETS)
def test_dense(gpu, a, b, H, channels):
    cm = gpu
    plan = cm.plan_dyn(8, channels, a, b, H, 1)
    assert plan.fast == (1 if channels <= 2 else 0)
    t = plan.tile_frames
    xs, counts, T, ragged, full, unity, change, smallest, gmin = dense_case(a, b, H, channels, t)
    print("dyn dense a %2d b %d H %4d C %2d: tile %d, unity %.1f %%, changing %.1f %%, min s %d"
          % (a, b, H, channels, t, 100 * unity, 100 * change, smallest))
    assert_dense(a, b, H, unity, change, smallest)
    assert np.array_equal(cm.dyn_design(comp_threshold_db=-18, comp_ratio=4, comp_knee_db=6, gate_threshold_db=-45,
                                        gate_ratio=2, gate_range_db=40), T)      # the library's designer gives this curve
    rig = Rig(cm, len(counts), channels, a, b, H, counts[0], T)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts: one run equals the same stream in many, queued without a synchronisation

def run_chunks(cm, dyn, channels, chunks):
    """chunks: per run a list of per-stream int16 [F][C]; queues every run on buffers of its own, synchronises once
    -> per run the output array [S][stride] and the counts"""
    S = len(chunks[0])
    bufs = []
    for xs in chunks:
        counts = [x.shape[0] for x in xs]
        frames = max(counts)
        stride = (frames * channels + 7) // 8 * 8 + 8
        src = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride))
        dst = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride))
        src.array[:] = 0x5a5a
        dst.array[:] = SENTINEL
        for s, x in enumerate(xs):
            src.array[s, :counts[s] * channels] = x.reshape(-1)
        dyn.run(src.dev, stride, frames, dst.dev, stride, counts)
        bufs.append((src, dst, counts))
    dyn.sync()                                                   # (the only synchronisation)
    outs = [(dst.array.copy(), counts) for _, dst, counts in bufs]
    for src, dst, _ in bufs:
        src.free()
        dst.free()
    return outs


# (the last geometry is the longest history whose cuts still leave a rest inside 3 tiles: HIST = 2557)
@pytest.mark.parametrize("channels,a,b,H", [(1, 6, 6, 0), (2, 8, 5, 100), (6, 5, 9, 7), (2, 9, 9, 1024)])
def test_cuts(gpu, channels, a, b, H):
    cm = gpu
    t = cm.plan_dyn(2, channels, a, b, H, 1).tile_frames
    hist = geometry(a, b, H)[4]
    T = design(**DENSE_CURVE)
    x = [signal(7000 + 10 * channels + s, 3 * t, channels) for s in range(2)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [model_dyn(v, zero, T, a, b, H) for v in x]
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    for starve in (False, True):
        # stream 0 is cut as the list says; stream 1 in the same runs, or with 0 frames in alternate runs
        dyn = cm.Dynamics(2, channels, a, b, H, 3 * t, curve=T)
        chunks, pos = [], [0, 0]
        for r, n in enumerate(cuts):
            n1 = 0 if starve and r % 2 else n
            chunks.append([x[0][pos[0]:pos[0] + n], x[1][pos[1]:pos[1] + n1]])
            pos = [pos[0] + n, pos[1] + n1]
        outs = run_chunks(cm, dyn, channels, chunks)
        for s in range(2):
            got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
            assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), (starve, s)
            for arr, counts in outs:
                assert (arr[s, counts[s] * channels:] == SENTINEL).all()
        assert dyn.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(2)]
        dyn.close()


# ---------------------------------------------------------------------------
# 3. literal edges

def test_single_full_scale_sample_under_the_unity_curve(gpu):
    cm = gpu
    rig = Rig(cm, 1, 1, 6, 6, 0, 1000)                           # the curve of creation: a pure delay
    x = np.zeros((1000, 1), dtype=np.int16)
    x[500] = -32768
    y = rig.run([x])[0]
    want = np.zeros((1000, 1), dtype=np.int16)
    want[500 + 63] = -32768
    assert np.array_equal(y, want) and rig.m.min_gain().tolist() == [UNITY]
    rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_zero_curve_and_silence_knot(gpu, channels):
    """a curve of zeros gives zeros; a curve that is unity at knot 0 only, over silence and then full-scale square waves,
    moves between idx 0 and idx 121"""
    cm = gpu
    a, b, H = 4, 3, 3
    t = cm.plan_dyn(1, channels, a, b, H, 1).tile_frames
    n = t + 300
    sq = np.where((np.arange(n) // 5) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
    rig = Rig(cm, 1, channels, a, b, H, n, flat(0))
    y = rig.run([sq])[0]
    assert not y.any() and rig.m.min_gain().tolist() == [0]
    rig.close()
    only0 = flat(0)
    only0[0] = UNITY
    x = sq.copy()
    x[:200] = 0
    x[600:700] = -32768                                          # level 32768 exactly: knot 121, and knot 122 times 0
    x[t - 40:t + 60] = 0                                         # silence across the tile edge: back to knot 0
    rig = Rig(cm, 1, channels, a, b, H, n, only0)
    y = rig.run([x])[0]
    s = rig.model.s[0][0]
    assert s[0] == UNITY and s[150] == UNITY and s[400] == 0 and s[t + 40] == UNITY and s[-1] == 0
    assert curve_index(np.array([0, 32768]))[0].tolist() == [0, 121]
    assert rig.m.min_gain().tolist() == [0]
    rig.close()


def test_levels_below_eight(gpu):
    """constant inputs of magnitude 1..7 (and 0, 8, 9): the E < 3 knots, each with a gain of its own"""
    cm = gpu
    a, b, H = 3, 3, 0
    T = steps()
    levels = list(range(10))
    xs = [np.full((200, 2), v, dtype=np.int16) * np.array([1, -1], dtype=np.int16) for v in levels]
    rig = Rig(cm, len(levels), 2, a, b, H, 200, T)
    rig.run(xs)
    idx = [0, 1, 9, 13, 17, 19, 21, 23, 25, 26]                  # the header's knots of levels 0..9
    for v, k in zip(levels, idx):
        assert int(rig.model.s[v][0][-1]) == int(T[k]), (v, k)
    assert np.array_equal(curve_index(np.array(levels))[0], idx)
    rig.close()


def steps():
    """every knot another gain: whatever moves the level moves the output"""
    return (UNITY - 257 * np.arange(CURVE)).astype(np.uint16)


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_bursts_at_a_tile_edge_and_at_the_history_length(gpu, channels):
    """a burst that straddles a tile edge, and one whose last frame lies exactly HIST frames before the second run
    begins: that run's first output still sees it through the history, the next one does not"""
    cm = gpu
    a, b, H = 6, 5, 100
    A, B, D, W, hist = geometry(a, b, H)
    t = cm.plan_dyn(1, channels, a, b, H, 1).tile_frames
    T = steps()
    base = int(curve_at(T, np.array([300]))[0])
    n = t + 500
    x = np.full((n, channels), 300, dtype=np.int16)
    x[t - 10:t + 10, channels - 1] = -32768
    x[n - hist - 49:n - hist + 1] = 30000                        # its last frame is frame n - hist
    rig = Rig(cm, 1, channels, a, b, H, n, T)
    rig.run([x])
    s = rig.model.s[0][0]
    assert s[t - B] == base and s[t - 1] != base and s[t] != base
    rig.run([np.full((n, channels), 300, dtype=np.int16)])
    s2 = rig.model.s[0][1]
    assert s2[0] != base and s2[1] == base                       # frame n - hist is the oldest that frame n depends on
    rig.close()


# ---------------------------------------------------------------------------
# 4. curves and state

def test_per_stream_curves_and_ordering(gpu):
    cm = gpu
    S, a, b, H = 300, 4, 3, 5
    counts = [40 + s % 65 for s in range(S)]
    xs = [bursts(500 + s, n, 2) for s, n in enumerate(counts)]
    rig = Rig(cm, S, 2, a, b, H, 104)
    second = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.stride))
    rig.fill(xs)
    rig.dst.array[:] = SENTINEL
    second.array[:] = SENTINEL
    m = rig.m
    # no synchronisation anywhere: 300 sets, run, set(-1), run; the second run sees the first one's frames with the new curve
    for s in range(S):
        m.set_curve(s, flat(UNITY - s))                          # names its stream
    m.run(rig.src.dev, rig.stride, 104, rig.dst.dev, rig.stride, counts)
    m.set_curve(-1, flat(12345))
    m.run(rig.src.dev, rig.stride, 104, second.dev, rig.stride, counts)
    m.sync()
    for s in range(S):
        rig.model.set(s, flat(UNITY - s))
    first = rig.model.run(xs)
    rig.check(rig.dst.array, first)
    rig.model.set(-1, flat(12345))
    then = rig.model.run(xs)
    rig.check(second.array, then)
    assert not np.array_equal(first[299], then[299]) and np.array_equal(m.get_curve(299), flat(12345))
    assert m.min_gain().tolist() == rig.model.gmin == [12345] * S
    second.free()
    rig.close()


def test_reset_and_the_meter(gpu):
    cm = gpu
    a, b, H = 5, 4, 20
    T = design(**DENSE_CURVE)
    xs = [signal(600 + s, 700, 1) for s in range(3)]
    rig = Rig(cm, 3, 1, a, b, H, 700, T)
    rig.run(xs)
    assert all(g < UNITY for g in rig.model.gmin)
    assert rig.m.min_gain(reset=True).tolist() == rig.model.gmin
    assert rig.m.min_gain().tolist() == [UNITY] * 3                          # re-armed, the history kept
    rig.model.gmin = [UNITY] * 3
    loud = [np.full((50, 1), 20000, dtype=np.int16)] * 3
    rig.run(loud)
    rig.reset(1)                                                 # stream 1 starts again from silence, 0 and 2 go on
    ys = rig.run(xs)
    zero = np.zeros((geometry(a, b, H)[4], 1), dtype=np.int16)
    assert np.array_equal(ys[1], model_dyn(xs[1], zero, T, a, b, H)[0])
    assert not np.array_equal(ys[0][:40], model_dyn(xs[0], zero, T, a, b, H)[0][:40])
    # a bad table is refused and the old curve stays
    for k in (0, 57, 122):
        bad = np.asarray(T, dtype=np.uint16).copy()
        bad[k] = 32769
        assert rig.m.set_curve_rc(0, bad) == cm.ERROR_INVAL, k
    assert rig.m.set_curve_rc(3, flat(1)) == cm.ERROR_INVAL and rig.m.set_curve_rc(-2, flat(1)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_dyn_set_curve(rig.m.h, 0, None) == cm.ERROR_FAULT
    assert np.array_equal(rig.m.get_curve(0), T)
    ok = np.asarray(T, dtype=np.uint16).copy()
    ok[123:] = 65535                                             # ignored entries may hold anything
    rig.set(0, ok)
    rig.reset()
    rig.run(xs)
    rig.close()


# ---------------------------------------------------------------------------
# 5. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    rig = Rig(cm, 2, 2, 6, 6, 0, 256, design(**DENSE_CURVE))
    m, src, dst, st = rig.m, rig.src.dev, rig.dst.dev, rig.stride
    assert st == 520
    xs = [signal(700 + s, 256, 2) for s in range(2)]
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
        "a count above frames": (src, st, 100, dst, st, [100, 101]),
        "in == out": (src, st, 256, src, st, None),
        "out inside in": (src, st, 256, src + 16, st, None),
        "out begins in the last slot of in": (src, st, 256, src + 2 * (st + 256), st, None),
        "in begins inside out": (dst + 2 * st, st, 256, dst, st, None),
    }
    for name, (a, ast, n, o, ost, fps) in cases.items():
        assert m.run_rc(a, ast, n, o, ost, fps) == cm.ERROR_INVAL, name
    assert cm.lib.cmhip_dyn_run(m.h, None, st, 256, None, dst, st) == cm.ERROR_FAULT
    assert cm.lib.cmhip_dyn_run(m.h, src, st, 256, None, None, st) == cm.ERROR_FAULT
    assert cm.lib.cmhip_dyn_min_gain(m.h, None, 0) == cm.ERROR_FAULT
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.run(xs)                                                  # the history is what the first run left
    rig.close()


# ---------------------------------------------------------------------------
# 6. composition: bus -> dynamics -> limiter -> the slots of a batch, all on the batch's stream, block by block

CHAIN_BLOCKS = ([3000, 1, 0, 4097, 700], [2999, 7, 4100, 0, 1234])      # per bus: its streams' counts, block by block


def test_chain_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    tb = _load("test_gpu_bus")
    cm = gpu
    S, B, F = 4, 2, 4100
    a, b, H, la, lh, T_lim, drive = 6, 6, 30, 6, 30, 29204, 16384
    curve = design(**DENSE_CURVE)
    bus_of = [0, 0, 1, 1]
    total = [sum(CHAIN_BLOCKS[bus_of[s]]) for s in range(S)]
    # microphones 0 and 2 speak, 1 and 3 are room noise within +-60
    xs = [bursts(800 + s, total[s], 1) if s % 2 == 0
          else np.random.default_rng(810 + s).integers(-60, 61, size=(total[s], 1)).astype(np.int16) for s in range(S)]
    for s in (0, 2):
        xs[s][1000:2500] = 0                                     # ... and pause: only the room is left, the gate closes
    table = (bus_of, [0, 1, 2, 3], np.full((4, 1, 1), 8192, dtype=np.int16))
    dyn_m, lim_m = Model(B, 1, a, b, H), TL.Model(B, 1, la, lh)
    dyn_m.set(-1, curve)
    lim_m.set(-1, T_lim, drive)
    objects, arrays = [], []
    try:
        batch = cm.Batch(B, 1, F, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, rate=48000)
        objects.append(batch)
        st = batch.hip_stream()
        bus = cm.Bus(S, B, 1, 1, F, 8, hip_stream=st)
        objects.append(bus)
        dyn = cm.Dynamics(B, 1, a, b, H, F, curve=curve, hip_stream=st)
        objects.append(dyn)
        lim = cm.Limiter(B, 1, la, lh, F, threshold=T_lim, drive=drive, hip_stream=st)
        objects.append(lim)
        assert bus.hip_stream() == dyn.hip_stream() == lim.hip_stream() == st
        bus.set_routing(*table)
        stride = (F + 7) // 8 * 8 + 8
        d_sum, d_dyn, d_lim = (cm.DeviceWords((B * s_ * 2 + 7) // 8) for s_ in (stride, stride, batch.stride))
        arrays += [d_sum, d_dyn, d_lim]
        wants, feeds, results, pos = [], [], [], [0] * S
        for r in range(len(CHAIN_BLOCKS[0])):
            counts = [CHAIN_BLOCKS[bus_of[s]][r] for s in range(S)]
            ins = [xs[s][pos[s]:pos[s] + counts[s]] for s in range(S)]
            pos = [p + n for p, n in zip(pos, counts)]
            outs = lim_m.run(dyn_m.run(tb.model_bus(ins, table, B, 1)))
            wants.append(outs)
            feed = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride))
            res = cm.MappedPcm(batch)
            feed.array[:] = 0x5a5a
            res.array[:] = SENTINEL
            for s, x in enumerate(ins):
                feed.array[s, :x.size] = x.reshape(-1)
            feeds.append(feed)
            results.append(res)
            arrays += [feed, res]
            # (no wait anywhere: the order is the stream's)
            kb = bus.run(feed.dev, stride, max(counts), d_sum.dev, stride, counts)
            assert kb.tolist() == [CHAIN_BLOCKS[0][r], CHAIN_BLOCKS[1][r]]
            dyn.run(d_sum.dev, stride, int(kb.max()), d_dyn.dev, stride, kb)
            lim.run(d_dyn.dev, stride, int(kb.max()), d_lim.dev, batch.stride, kb)
            batch.run_slots(int(kb.max()), d_lim.dev, res.dev, kb)
        batch.sync()                                             # (the only synchronisation)
        for r, outs in enumerate(wants):
            for q in range(B):
                want = outs[q].reshape(-1)
                have = results[r].array[q, :want.size]
                bad = np.flatnonzero(have != want)
                assert bad.size == 0, ("block", r, "bus", q, "first mismatch at frame", int(bad[0]), "of", want.size)
                assert (results[r].array[q, want.size:] == SENTINEL).all(), ("block", r, "bus", q)
        assert dyn.min_gain().tolist() == dyn_m.gmin and lim.min_gain().tolist() == lim_m.gmin
        assert all(g < 1000 for g in dyn_m.gmin) and all(g < UNITY for g in lim_m.gmin)       # the gate closed, the limiter worked
        vu, rcs = batch.vu_results()
        for q in range(B):
            y = np.concatenate([outs[q].reshape(-1) for outs in wants])
            v = oracle.vu_new(1)
            oracle.vu_accumulate(v, y)
            _, vr = oracle.vu_result(v)
            assert rcs[q] == 0 and oracle_ffi.vu_result_dict(vr) == vu[q].as_dict(), q
            assert vu[q].frames == sum(CHAIN_BLOCKS[q]) and abs(vu[q].global_peak) <= T_lim
    finally:                                 # (the three that borrow the batch's stream go before the batch, whatever the outcome)
        for o in reversed(objects):
            o.close()
        for o in arrays:
            o.free()


# ---------------------------------------------------------------------------
# 7. the example

def test_batch_dynamics_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_dynamics"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_dynamics.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("4 microphones (2 idle) -> bus -> dynamics: delay 63")
    assert len(out) == 2 and out[1].startswith("programme: ")
    f = dict(kv.split("=") for kv in out[1].split()[1:])
    assert int(f["frames"]) == 24000 and int(f["channels"]) == 1
    assert 20000 <= abs(int(f["peak"])) <= 29204                 # driven up and held under -1 dBFS
    assert int(f["dyn_min_gain"]) < 1000                         # the gate closed on the idle stretch: about -40 dB
    assert int(f["lim_min_gain"]) <= 32768
