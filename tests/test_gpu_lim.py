"""GPU: the peak limiter (cmhip_lim_*, csrc/k_lim.hip) against a numpy model of the arithmetic include/coolmic_hip.h
states, bit for bit: both kernel forms over five parameter sets on a signal of bursts, ragged and uniform counts around
the tile and the history length, a stream cut into runs without a synchronisation, literal edges, the ceiling on the
device's own output, per-stream parameters and their order with the runs, reset and the gain-reduction meter, refusals
that launch nothing, the chain bus -> limiter -> batch on one stream, and the C example.  Output slots are pre-filled
with a sentinel; every sample past a stream's count must still hold it after a run.  (tests/test_lim_host.py takes the
model, the signal and the dense cases from here.)"""
import functools
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


def model_lim(x, hist, T, drive, a, H):
    """x int16 [F][C]; hist int16 [HIST][C], oldest first -> y int16 [F][C], s int64 [F]"""
    A = 1 << a; D = A - 1; W = A + H; HIST = A + W - 2
    F = x.shape[0]
    if F == 0: return x.copy(), np.zeros(0, np.int64)
    z = np.concatenate([hist, x]).astype(np.int64)
    pr = (np.abs(z).max(axis=1) * drive + 4095) >> 12
    g = np.where(pr <= T, 32768, (T * 32768) // np.maximum(pr, 1))
    m = np.lib.stride_tricks.sliding_window_view(g, W).min(axis=1)
    s = np.lib.stride_tricks.sliding_window_view(m, A).sum(axis=1) >> a      # F entries
    y = (z[HIST - D: HIST - D + F] * (drive * s)[:, None] + (1 << 26)) >> 27
    assert np.abs(y).max(initial=0) <= T
    return y.astype(np.int16), s


def geometry(a, H):
    """-> A, D, W, HIST"""
    A = 1 << a
    return A, A - 1, A + H, 2 * A + H - 2


def next_hist(hist, x):
    """the history after a run: the last HIST frames of (hist, x)"""
    return np.concatenate([hist, x])[-hist.shape[0]:] if hist.shape[0] else hist


def bursts(seed, frames, channels):
    """quiet uniform noise within +-2000 with bursts of 1..199 frames at a random level in 4000..32768 every 1..399
    frames"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2000, 2001, size=(frames, channels))
    pos = 0
    while True:
        pos += int(rng.integers(1, 400))
        n, level = int(rng.integers(1, 200)), int(rng.integers(4000, 32769))
        if pos >= frames:
            break
        n = min(n, frames - pos)
        x[pos:pos + n] = rng.integers(-level, level + 1, size=(n, channels))
        x[pos + int(rng.integers(0, n)), int(rng.integers(0, channels))] = -level      # the level is reached
        pos += n
    return np.clip(x, -32768, 32767).astype(np.int16)


class Model:
    """the streams of a limiter as the header states them: raw history, parameters, the meter"""

    def __init__(self, streams, channels, a, H):
        self.S, self.C, self.a, self.H = streams, channels, a, H
        self.A, self.D, self.W, self.HIST = geometry(a, H)
        self.hist = [np.zeros((self.HIST, channels), dtype=np.int16) for _ in range(streams)]
        self.par = [(32767, 4096)] * streams
        self.gmin = [UNITY] * streams
        self.s = [[] for _ in range(streams)]        # every s a run gave, for the dense conditions

    def set(self, stream, T, drive):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.par[s] = (T, drive)

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.hist[s] = np.zeros((self.HIST, self.C), dtype=np.int16)
            self.gmin[s] = UNITY

    def run(self, xs):
        ys = []
        for s, x in enumerate(xs):
            x = np.asarray(x, dtype=np.int16).reshape(-1, self.C)
            y, sg = model_lim(x, self.hist[s], self.par[s][0], self.par[s][1], self.a, self.H)
            self.hist[s] = next_hist(self.hist[s], x)
            if sg.size:
                self.gmin[s] = min(self.gmin[s], int(sg.min()))
                self.s[s].append(sg)
            ys.append(y)
        return ys


class Rig:
    """a limiter between two arrays of pinned, device-mapped host memory, and its model"""

    def __init__(self, cm, streams, channels, a, H, max_frames, T=None, drive=None):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Limiter(streams, channels, a, H, max_frames)
        self.model = Model(streams, channels, a, H)
        assert self.m.delay() == self.model.D
        self.stride = (max_frames * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        if T is not None:
            self.set(-1, T, drive)

    def set(self, stream, T, drive):
        self.m.set(stream, T, drive)
        self.model.set(stream, T, drive)
        for s in (range(self.S) if stream < 0 else [stream]):
            assert self.m.get(s) == (T, drive)

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
        """xs: per stream int16 [F_s][C]; runs the device and the model, compares outputs, the untouched rest, the
        ceiling on the device's output and the meter; -> the model's outputs"""
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
            assert np.abs(have.astype(np.int64)).max(initial=0) <= self.model.par[s][0], ("stream", s, "above the ceiling")
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(),
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (array[s, n:] == SENTINEL).all(), ("stream", s, "written past its count")


# ---------------------------------------------------------------------------
# 1. dense cases: five parameter sets, both forms, ragged and uniform counts

SETS = [(3, 0, 20000, 4096), (6, 0, 29204, 8192), (6, 100, 12000, 4096), (8, 37, 29204, 16384), (9, 1536, 8000, 4096)]
CHANNELS = [1, 2, 3, 6, 16]
UNITY_SHARE = (0.02, 0.95)                        # of the model's frames with s = 32768
CHANGE_SHARE = 0.05                               # of adjacent frames of the model whose s differs, at least


def dense_counts(t, hist):
    return [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 1, 0]


# The seeds are chosen so that the MODEL alone meets the dense condition, checked without a device: the long hold of the
# fifth set leaves s at unity only before a stream's first burst, about 2 % of the frames, so its seeds were searched
# (the first base of 7919 * 1, 2, ... that gives at least 2.5 %); the other sets pass with the plain seed.
DENSE_SEED_BASE = {(9, 1536, 1): 3 * 7919, (9, 1536, 2): 2 * 7919, (9, 1536, 3): 1 * 7919, (9, 1536, 6): 2 * 7919,
                   (9, 1536, 16): 2 * 7919}


def dense_seed(a, H, channels, stream):
    return 100000 * a + 10 * H + 1000 * channels + stream + DENSE_SEED_BASE.get((a, H, channels), 1)


@functools.lru_cache(maxsize=None)
def dense_case(a, H, T, drive, channels, t):
    """the streams' full-length inputs, and over the ragged run followed by the uniform run on one limiter: the
    model's outputs of both and the two shares of the dense condition -- computed once, never changed"""
    hist = geometry(a, H)[3]
    counts = dense_counts(t, hist)
    xs = [bursts(dense_seed(a, H, channels, s), counts[0], channels) for s in range(len(counts))]
    model = Model(len(counts), channels, a, H)
    model.set(-1, T, drive)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    s_all = [sg for per in model.s for sg in per]
    frames = sum(sg.size for sg in s_all)
    unity = sum(int((sg == UNITY).sum()) for sg in s_all) / frames
    change = sum(int((np.diff(sg) != 0).sum()) for sg in s_all) / max(sum(sg.size - 1 for sg in s_all if sg.size), 1)
    peak = max(int(np.abs(y.astype(np.int64)).max(initial=0)) for y in ragged + full)
    return xs, counts, ragged, full, unity, change, peak, list(model.gmin)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("a,H,T,drive", SETS)
def test_dense(gpu, a, H, T, drive, channels):
    cm = gpu
    plan = cm.plan_lim(8, channels, a, H, 1)
    assert plan.fast == (1 if channels <= 2 else 0)
    t = plan.tile_frames
    xs, counts, ragged, full, unity, change, peak, gmin = dense_case(a, H, T, drive, channels, t)
    print("lim dense a %d H %4d T %5d drive %5d C %2d: tile %d, unity %.1f %%, changing %.1f %%, peak %d"
          % (a, H, T, drive, channels, t, 100 * unity, 100 * change, peak))
    assert UNITY_SHARE[0] <= unity <= UNITY_SHARE[1] and change >= CHANGE_SHARE
    assert peak == T                                             # the ceiling is reached, never passed
    rig = Rig(cm, len(counts), channels, a, H, counts[0], T, drive)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    dev_peak = int(np.abs(rig.dst.array[:, :counts[0] * channels].astype(np.int64)).max())
    assert dev_peak == T                                         # on the device's own output
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts: one run equals the same stream in many, queued without a synchronisation

def run_chunks(cm, lim, channels, chunks):
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
        lim.run(src.dev, stride, frames, dst.dev, stride, counts)
        bufs.append((src, dst, counts))
    lim.sync()                                                   # (the only synchronisation)
    outs = [(dst.array.copy(), counts) for _, dst, counts in bufs]
    for src, dst, _ in bufs:
        src.free()
        dst.free()
    return outs


@pytest.mark.parametrize("channels,a,H,T,drive", [(1, 6, 0, 29204, 8192), (2, 6, 100, 12000, 4096),
                                                  (6, 8, 37, 29204, 16384), (2, 9, 1536, 8000, 4096)])
def test_cuts(gpu, channels, a, H, T, drive):
    cm = gpu
    t = cm.plan_lim(2, channels, a, H, 1).tile_frames
    hist = geometry(a, H)[3]
    x = [bursts(7000 + 10 * channels + s, 3 * t, channels) for s in range(2)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [model_lim(v, zero, T, drive, a, H) for v in x]
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    for starve in (False, True):
        # stream 0 is cut as the list says; stream 1 in the same runs, or with 0 frames in alternate runs
        lim = cm.Limiter(2, channels, a, H, 3 * t, threshold=T, drive=drive)
        chunks, pos = [], [0, 0]
        for r, n in enumerate(cuts):
            n1 = 0 if starve and r % 2 else n
            chunks.append([x[0][pos[0]:pos[0] + n], x[1][pos[1]:pos[1] + n1]])
            pos = [pos[0] + n, pos[1] + n1]
        outs = run_chunks(cm, lim, channels, chunks)
        for s in range(2):
            got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
            assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), (starve, s)
            for arr, counts in outs:
                assert (arr[s, counts[s] * channels:] == SENTINEL).all()
        assert lim.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(2)]
        lim.close()


# ---------------------------------------------------------------------------
# 3. literal edges

def test_single_full_scale_sample(gpu):
    cm = gpu
    rig = Rig(cm, 1, 1, 6, 0, 1000, 32767, 4096)
    x = np.zeros((1000, 1), dtype=np.int16)
    x[500] = -32768
    y = rig.run([x])[0]
    want = np.zeros((1000, 1), dtype=np.int16)
    want[500 + 63] = -32767
    assert np.array_equal(y, want) and rig.m.min_gain().tolist() == [32767]
    rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_square_wave_at_the_extremes(gpu, channels):
    cm = gpu
    t = cm.plan_lim(1, channels, 4, 3, 1).tile_frames
    n = t + 300
    x = np.where((np.arange(n) // 5) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
    for T, drive in ((1, 4096), (32767, 65535), (1, 65535), (32767, 1), (1, 1)):
        rig = Rig(cm, 1, channels, 4, 3, n, T, drive)
        y = rig.run([x])[0]
        peak = int(np.abs(y.astype(np.int64)).max())
        assert peak <= T and ((T, drive) != (1, 4096) or peak == 1)          # g = 1: +-1 is all that is left
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_below_the_threshold_is_a_pure_delay(gpu, channels):
    cm = gpu
    a, H = 5, 9
    t = cm.plan_lim(2, channels, a, H, 1).tile_frames
    n, D = t + 77, 31
    rng = np.random.default_rng(310 + channels)
    xs = [rng.integers(-20000, 20001, size=(n, channels)).astype(np.int16), rng.integers(-20000, 20001, size=(9, channels)).astype(np.int16)]
    rig = Rig(cm, 2, channels, a, H, n, 20000, 4096)
    ys = rig.run(xs)
    assert not ys[0][:D].any() and np.array_equal(ys[0][D:], xs[0][:n - D]) and not ys[1].any()
    assert rig.m.min_gain().tolist() == [UNITY, UNITY]
    ys = rig.run(xs)                                             # the next run starts with the last D frames of this one
    assert np.array_equal(ys[0][:D], xs[0][n - D:]) and np.array_equal(ys[0][D:], xs[0][:n - D])
    assert not ys[1].any()                                       # 18 frames so far: still inside the delay
    rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_bursts_at_a_tile_edge(gpu, channels):
    """a burst that ends exactly W frames before a tile edge, and one that straddles the edge: the hold reaches across"""
    cm = gpu
    a, H, T = 6, 100, 10000
    A, D, W, hist = geometry(a, H)
    t = cm.plan_lim(1, channels, a, H, 1).tile_frames
    n = 2 * t + 500
    x = np.full((n, channels), 300, dtype=np.int16)
    x[t - W - 20:t - W] = 30000                                  # its last frame is frame t - W - 1
    x[2 * t - 10:2 * t + 10, channels - 1] = -32768
    rig = Rig(cm, 1, channels, a, H, n, T, 4096)
    y = rig.run([x])[0]
    s = rig.model.s[0][0]
    assert s[t - 1] < UNITY and s[t + A - 3] < UNITY and s[t + A - 2] == UNITY         # the release crosses the edge
    assert s[2 * t - 1] < UNITY and s[2 * t] < UNITY and np.abs(y).max() == T
    rig.close()


# ---------------------------------------------------------------------------
# 4. parameters and state

def test_per_stream_parameters_and_ordering(gpu):
    cm = gpu
    S, a, H = 300, 4, 5
    counts = [40 + s % 65 for s in range(S)]
    xs = [bursts(500 + s, n, 2) for s, n in enumerate(counts)]
    rig = Rig(cm, S, 2, a, H, 104)
    for s in range(S):
        rig.set(s, 3000 + 90 * s, 4096 + 100 * s)                # names its stream
    rig.run(xs)
    # no synchronisation anywhere: set, run, set, run; the second run sees the first one's frames with the new values
    second = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.stride))
    rig.fill(xs)
    rig.dst.array[:] = SENTINEL
    second.array[:] = SENTINEL
    m = rig.m
    m.set(-1, 9000, 5000)
    m.run(rig.src.dev, rig.stride, 104, rig.dst.dev, rig.stride, counts)
    m.set(7, 2500, 12000)
    m.run(rig.src.dev, rig.stride, 104, second.dev, rig.stride, counts)
    m.sync()
    assert m.get(7) == (2500, 12000) and m.get(8) == (9000, 5000)
    rig.model.set(-1, 9000, 5000)
    first = rig.model.run(xs)
    rig.check(rig.dst.array, first)
    rig.model.set(7, 2500, 12000)
    before = rig.model.hist[7].copy()
    then = rig.model.run(xs)
    rig.check(second.array, then)
    assert not np.array_equal(then[7], model_lim(xs[7], before, 9000, 5000, a, H)[0])
    assert m.min_gain().tolist() == rig.model.gmin
    second.free()
    rig.close()


def test_reset_and_the_meter(gpu):
    cm = gpu
    a, H = 5, 20
    xs = [bursts(600 + s, 700, 1) for s in range(3)]
    rig = Rig(cm, 3, 1, a, H, 700, 8000, 8192)
    rig.run(xs)
    assert all(g < UNITY for g in rig.model.gmin)
    assert rig.m.min_gain(reset=True).tolist() == rig.model.gmin
    assert rig.m.min_gain().tolist() == [UNITY] * 3                          # re-armed, the history kept
    rig.model.gmin = [UNITY] * 3
    quiet = [np.full((50, 1), 10, dtype=np.int16)] * 3
    rig.run(quiet)                                               # the tail of the bursts is still in the window
    rig.reset(1)                                                 # stream 1 starts again from silence, 0 and 2 go on
    ys = rig.run(xs)
    zero = np.zeros((geometry(a, H)[3], 1), dtype=np.int16)
    assert np.array_equal(ys[1], model_lim(xs[1], zero, 8000, 8192, a, H)[0])
    assert not np.array_equal(ys[0][:40], model_lim(xs[0], zero, 8000, 8192, a, H)[0][:40])
    assert rig.m.set_rc(0, 0, 4096) == cm.ERROR_INVAL and rig.m.set_rc(0, 32768, 4096) == cm.ERROR_INVAL
    assert rig.m.set_rc(0, 8000, 0) == cm.ERROR_INVAL and rig.m.set_rc(0, 8000, 65536) == cm.ERROR_INVAL
    assert rig.m.set_rc(3, 8000, 4096) == cm.ERROR_INVAL and rig.m.set_rc(-2, 8000, 4096) == cm.ERROR_INVAL
    assert rig.m.get(0) == (8000, 8192)
    rig.reset()
    rig.run(xs)
    rig.close()


# ---------------------------------------------------------------------------
# 5. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    rig = Rig(cm, 2, 2, 6, 0, 256, 10000, 8192)
    m, src, dst, st = rig.m, rig.src.dev, rig.dst.dev, rig.stride
    assert st == 520
    xs = [bursts(700 + s, 256, 2) for s in range(2)]
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
    assert cm.lib.cmhip_lim_run(m.h, None, st, 256, None, dst, st) == cm.ERROR_FAULT
    assert cm.lib.cmhip_lim_run(m.h, src, st, 256, None, None, st) == cm.ERROR_FAULT
    assert cm.lib.cmhip_lim_min_gain(m.h, None, 0) == cm.ERROR_FAULT
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.run(xs)                                                  # the history is what the first run left
    rig.close()


# ---------------------------------------------------------------------------
# 6. composition: bus -> limiter -> the slots of a batch, all on the batch's stream

def test_chain_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    import importlib.util
    spec = importlib.util.spec_from_file_location("test_gpu_bus_model", os.path.join(ROOT, "tests", "test_gpu_bus.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    cm = gpu
    S, B, F, a, H, T, drive = 4, 2, 3000, 6, 30, 29204, 8192
    fps = [F, F - 1, 1234, 2000]
    xs = [bursts(800 + s, fps[s], 1) for s in range(S)]
    table = ([0, 0, 1, 1, 1], [0, 1, 1, 2, 3], np.full((5, 1, 1), 8192, dtype=np.int16))
    mixed = tb.model_bus(xs, table, B, 1)
    zero = np.zeros((geometry(a, H)[3], 1), dtype=np.int16)
    want = [model_lim(y.reshape(-1, 1), zero, T, drive, a, H)[0] for y in mixed]
    src_b = cm.Batch(S, 1, F, flags=cm.VU, rate=48000)           # (device memory for the sources)
    mid_b = cm.Batch(B, 1, F, flags=cm.VU, rate=48000)           # (... and for the buses' sums)
    for s in range(S):
        src_b.upload(s, xs[s])
    src_b.sync()
    b = cm.Batch(B, 1, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
    bus = cm.Bus(S, B, 1, 1, F, 8, hip_stream=b.hip_stream())
    lim = cm.Limiter(B, 1, a, H, F, threshold=T, drive=drive, hip_stream=b.hip_stream())
    assert bus.hip_stream() == b.hip_stream() == lim.hip_stream()
    bus.set_routing(*table)
    counts = bus.run(src_b.dev_in, src_b.stride, F, mid_b.dev_in, mid_b.stride, fps)
    assert counts.tolist() == [F, F - 1]
    lim.run(mid_b.dev_in, mid_b.stride, int(counts.max()), b.dev_in, b.stride, counts)
    b.run(int(counts.max()), counts)                             # (no sync between the three: the order is the stream's)
    res, rcs = b.vu_results()
    for s, y in enumerate(want):
        pcm = y.reshape(-1)
        v = oracle.vu_new(1)
        oracle.vu_accumulate(v, pcm)
        _, vr = oracle.vu_result(v)
        assert rcs[s] == 0 and oracle_ffi.vu_result_dict(vr) == res[s].as_dict(), s
        assert res[s].frames == counts[s] and abs(res[s].global_peak) <= T
        assert np.array_equal(b.download(s, int(counts[s])), pcm), s
    assert (lim.min_gain() < UNITY).all()
    lim.close()
    bus.close()
    for o in (b, mid_b, src_b):
        o.close()


# ---------------------------------------------------------------------------
# 7. the example

def test_batch_limiter_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_limiter"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_limiter.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("4 microphones at 8192 -> limiter: lookahead 64 frames (delay 63), threshold 29204, drive 8192")
    assert len(out) == 2 and out[1].startswith("programme: ")
    f = dict(kv.split("=") for kv in out[1].split()[1:])
    assert int(f["frames"]) == 24000 and int(f["channels"]) == 1
    assert 29000 <= abs(int(f["peak"])) <= 29204                 # driven into the ceiling, never past it
    assert 15000 < int(f["min_gain"]) < 20000                    # about 29204 / (2 * 0.866 * 32767) in Q15
