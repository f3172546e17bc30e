"""GPU: the limiter's release stage (cmhip_lim_new_release, csrc/k_limrel.hip) against the numpy model of
tests/test_limrel_host.py, bit for bit, for both detectors: every kernel form over five parameter sets on a signal of
bursts, ragged and uniform counts around the tile and the history length (which reaches the whole tile), a stream cut
into runs without a synchronisation, literal edges (the release ramp itself, bursts at and near a tile edge, the corners
of the parameters), per-stream parameters and their order with the runs, reset and the meter, refusals, rho = 0 through
the new constructor against the old constructors, the chain bus -> limiter -> batch over five ragged blocks, and the C
example.  Output slots are pre-filled with a sentinel; every sample past a stream's count must still hold it after a
run.  The limiter's tile, 4096 frames, is the unit of the shapes."""
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


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_gpu_limrel", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RH = _load("test_limrel_host")     # the model, the parameter sets, the dense cases and their conditions
MH, TG = RH.MH, RH.TG              # the true-peak detector's host tests; tests/test_gpu_lim.py: the rig, the signal
SENTINEL, UNITY, TILE = TG.SENTINEL, 32768, RH.TILE
SAMPLE, TRUE_PEAK = RH.SAMPLE, RH.TRUE_PEAK


class Rig(TG.Rig):
    """a limiter with a release stage between two arrays of pinned, device-mapped host memory, and its model"""

    def __init__(self, cm, det, streams, channels, a, H, rho, max_frames, T=None, drive=None):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Limiter(streams, channels, a, H, max_frames, detector=det, release_log2=rho)
        self.model = RH.ModelRel(det, streams, channels, a, H, rho)
        assert self.m.delay() == self.model.D == (1 << a) + (7 if det else -1)       # the stage adds no delay
        assert self.m.detector() == det and self.m.release() == rho
        self.stride = (max_frames * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        if T is not None:
            self.set(-1, T, drive)


def plan_tile(cm, det, streams, channels, a, H, rho):
    p = cm.plan_limrel(det, streams, channels, a, H, rho, 1)
    assert p.fast == (1 if channels <= 2 else 0) and p.tile_frames == TILE
    assert TILE >= p.halo >= RH.geometry_rel(det, a, H, rho)[3]
    return p.tile_frames


# ---------------------------------------------------------------------------
# 1. dense cases: five parameter sets, both detectors, every kernel form, ragged and uniform counts

@pytest.mark.parametrize("channels", RH.CHANNELS)
@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_dense(gpu, det, i, channels):
    cm = gpu
    a, H, rho, T, drive = RH.sets_of(det)[i]
    t = plan_tile(cm, det, 8, channels, a, H, rho)
    xs, counts, ragged, full, stats, gmin = RH.dense_case(det, a, H, rho, T, drive, channels, t)
    hist = RH.geometry_rel(det, a, H, rho)[3]
    assert counts == [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 1, 0] and (i < 4 or hist == t)
    # the conditions on the input, on the model alone: a kernel that skips the release cannot pass
    differ, unity, change = RH.dense_conditions(det, channels, RH.sets_of(det)[i])
    print("limrel dense det %d a %d H %4d rho %2d T %5d drive %5d C %2d: differ %.1f %%; over the sets unity %.1f %%, "
          "changing %.1f %%, peak %d" % (det, a, H, rho, T, drive, channels, 100 * differ, 100 * unity, 100 * change,
                                         stats["peak"]))
    rig = Rig(cm, det, len(counts), channels, a, H, rho, counts[0], T, drive)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    dev_peak = int(np.abs(rig.dst.array[:, :counts[0] * channels].astype(np.int64)).max())
    assert dev_peak <= T and (det == TRUE_PEAK or dev_peak == T)  # on the device's own output
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts: one run equals the same stream in many, queued without a synchronisation

# (det, channels, set, tiles): 3 tiles hold the runs for every set but the last, whose HIST is the tile itself -- its
# runs of HIST - 1, HIST, HIST + 1 and t + 5 frames alone are more than 3 tiles, so that stream has 5
CUTS = [(SAMPLE, 2, 0, 3), (SAMPLE, 1, 1, 3), (SAMPLE, 2, 2, 3), (SAMPLE, 6, 3, 3), (SAMPLE, 2, 4, 5),
        (TRUE_PEAK, 1, 1, 3), (TRUE_PEAK, 3, 3, 3), (TRUE_PEAK, 2, 4, 5)]


@pytest.mark.parametrize("det,channels,i,tiles", CUTS)
def test_cuts(gpu, det, channels, i, tiles):
    cm = gpu
    a, H, rho, T, drive = RH.sets_of(det)[i]
    t = plan_tile(cm, det, 2, channels, a, H, rho)
    hist = RH.geometry_rel(det, a, H, rho)[3]
    n = tiles * t
    x = [TG.bursts(7200 + 100 * det + 10 * channels + s, n, channels) for s in range(2)]
    zero = RH.zero_hist(det, a, H, rho, channels)
    want = [RH.model_limrel(det, v, zero, T, drive, a, H, rho) for v in x]
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    for starve in (False, True):
        # stream 0 is cut as the list says; stream 1 in the same runs, or with 0 frames in alternate runs
        lim = cm.Limiter(2, channels, a, H, n, threshold=T, drive=drive, detector=det, release_log2=rho)
        chunks, pos = [], [0, 0]
        for r, k in enumerate(cuts):
            k1 = 0 if starve and r % 2 else k
            chunks.append([x[0][pos[0]:pos[0] + k], x[1][pos[1]:pos[1] + k1]])
            pos = [pos[0] + k, pos[1] + k1]
        outs = TG.run_chunks(cm, lim, channels, chunks)
        for s in range(2):
            got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
            assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), (starve, s)
            for arr, counts in outs:
                assert (arr[s, counts[s] * channels:] == SENTINEL).all()
        assert lim.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(2)]
        lim.close()


# ---------------------------------------------------------------------------
# 3. literal edges

@pytest.mark.parametrize("a,rho", [(3, 5), (6, 11), (4, 1)])
def test_the_release_ramp_itself(gpu, a, rho):
    """a single -32768 followed by silence, and the same on a floor of 256 that shows the gain in the output: the gain
    drops to T / 32768 over the attack, stays for the look-ahead, and returns at q per frame for R frames, smoothed by
    the boxcar -- stated literally here, not taken from the model"""
    cm = gpu
    A, R, q, T, p = 1 << a, 1 << rho, UNITY >> rho, 4096, 700
    n = p + A + R + 2 * A + 600
    r = np.full(n + A, UNITY, dtype=np.int64)                     # r of frames -A .. n - 1 (H = 0: m = T over p .. p + A - 1)
    k = np.arange(n - p)
    r[A + p:] = np.minimum(UNITY, T + np.maximum(0, k - (A - 1)) * q)
    s = np.lib.stride_tricks.sliding_window_view(r, A).sum(axis=1)[1:] >> a
    assert s.size == n and s[p - 1] == UNITY and s[p + A - 1] == T == s.min()
    back = p + A - 1 + (UNITY - T + q - 1) // q + A - 1           # the first frame at unity again
    assert s[back - 1] < UNITY and (s[back:] == UNITY).all() and np.diff(s).max() <= q + 1
    for floor in (0, 256):
        x = np.full((n, 1), floor, dtype=np.int16)
        x[p] = -32768
        rig = Rig(cm, SAMPLE, 1, 1, a, 0, rho, n, T, 4096)
        y = rig.run([x])[0]                                       # (equal to the model: checked there)
        assert np.array_equal(rig.model.s[0][0], s)
        xd = np.concatenate([np.zeros(A - 1, dtype=np.int64), x[:n - (A - 1), 0].astype(np.int64)])
        want = (xd * (4096 * s) + (1 << 26)) >> 27
        assert np.array_equal(y[:, 0], want) and want[p + A - 1] == -T and rig.m.min_gain().tolist() == [T]
        if floor:                                                 # 256 * s / 32768 = s >> 7, rounded: the ramp is in the output
            assert np.array_equal(rig.dst.array[0, A - 1 + p + A:n], (s[A - 1 + p + A:] + 64) >> 7)
        rig.close()


@pytest.mark.parametrize("det,channels", [(SAMPLE, 1), (SAMPLE, 2), (SAMPLE, 6), (TRUE_PEAK, 1), (TRUE_PEAK, 2), (TRUE_PEAK, 5)])
def test_bursts_at_a_tile_edge(gpu, det, channels):
    """a burst whose last frame is the last of a tile, one that ends R - 1 frames before the next tile edge (the last
    frame its ramp can reach through the release pass alone is the tile's last), and one that straddles an edge: hold,
    release and boxcar reach across"""
    cm = gpu
    a, H, rho, T = 6, 100, 9, 10000
    A, D, W, hist, R, q = RH.geometry_rel(det, a, H, rho)
    t = plan_tile(cm, det, 1, channels, a, H, rho)
    n = 3 * t + 500
    x = np.full((n, channels), 300, dtype=np.int16)
    x[t - 20:t] = 30000                                           # its last frame is frame t - 1
    x[2 * t - (R - 1) - 20:2 * t - (R - 1)] = -30000              # ... frame 2t - R
    x[3 * t - 10:3 * t + 10, channels - 1] = -32768
    rig = Rig(cm, det, 1, channels, a, H, rho, n, T, 4096)
    y = rig.run([x])[0]
    s = rig.model.s[0][0]
    lag = D - (A - 1)                                             # the true-peak detector's 8 frames
    assert s[t - 300] == UNITY and s[t - 1] < UNITY and s[t] < UNITY and s[t + W + R // 2] < UNITY
    assert s[t + lag + W + A + R] == UNITY                        # the release crossed the edge and ended
    assert s[2 * t - 1] < UNITY and s[2 * t] < UNITY and s[2 * t + lag + W + A] == UNITY
    assert s[3 * t - 1] < UNITY and s[3 * t] < UNITY and np.abs(y.astype(np.int64)).max() <= T
    rig.close()


@pytest.mark.parametrize("det,channels", [(SAMPLE, 1), (SAMPLE, 2), (SAMPLE, 5), (TRUE_PEAK, 1), (TRUE_PEAK, 2), (TRUE_PEAK, 5)])
def test_square_wave_at_the_extremes(gpu, det, channels):
    """square waves at the corners of the parameters; T = 1 with drive 65535 gives the smallest gain and the largest pr
    the division sees"""
    cm = gpu
    a, H, rho = 4, 3, 7
    t = plan_tile(cm, det, 1, channels, a, H, rho)
    n = t + 300
    x = np.where((np.arange(n) // 5) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
    x[n - 200:] = 0                                               # ... and a release from the smallest gain
    for T, drive in ((1, 65535), (1, 4096), (32767, 65535), (32767, 1), (1, 1)):
        rig = Rig(cm, det, 1, channels, a, H, rho, n, T, drive)
        y = rig.run([x])[0]
        peak = int(np.abs(y.astype(np.int64)).max())
        assert peak <= T and ((T, drive) != (1, 4096) or peak <= 1)
        if T == 1 and drive >= 4096:
            assert rig.model.gmin[0] <= 1 and rig.model.s[0][0][-1] > rig.model.s[0][0][n - 200]     # on its way back
        rig.close()


@pytest.mark.parametrize("det,channels", [(SAMPLE, 1), (SAMPLE, 3), (TRUE_PEAK, 2)])
def test_below_the_threshold_is_a_pure_delay(gpu, det, channels):
    cm = gpu
    a, H, rho = 5, 9, 8
    t = plan_tile(cm, det, 2, channels, a, H, rho)
    n, D = t + 77, RH.geometry_rel(det, a, H, rho)[1]
    rng = np.random.default_rng(510 + channels)
    amp = 20000 * 8192 // 16571                                  # the filter's gain is at most 16571 / 8192
    xs = [rng.integers(-amp, amp + 1, size=(n, channels)).astype(np.int16), rng.integers(-amp, amp + 1, size=(9, channels)).astype(np.int16)]
    rig = Rig(cm, det, 2, channels, a, H, rho, n, 20000, 4096)
    ys = rig.run(xs)
    assert not ys[0][:D].any() and np.array_equal(ys[0][D:], xs[0][:n - D]) and not ys[1].any()
    assert rig.m.min_gain().tolist() == [UNITY, UNITY]
    ys = rig.run(xs)                                             # the next run starts with the last D frames of this one
    assert np.array_equal(ys[0][:D], xs[0][n - D:]) and np.array_equal(ys[0][D:], xs[0][:n - D])
    assert not ys[1].any()                                       # 18 frames so far: still inside the delay
    rig.close()


# ---------------------------------------------------------------------------
# 4. parameters, reset, the meter, refusals

@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_per_stream_parameters_and_ordering(gpu, det):
    cm = gpu
    S, a, H, rho = 300, 4, 5, 6
    counts = [40 + s % 65 for s in range(S)]
    xs = [TG.bursts(1100 + s, n, 2) for s, n in enumerate(counts)]
    rig = Rig(cm, det, S, 2, a, H, rho, 104)
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
    assert not np.array_equal(then[7], RH.model_limrel(det, xs[7], before, 9000, 5000, a, H, rho)[0])
    assert m.min_gain().tolist() == rig.model.gmin
    second.free()
    rig.close()


@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_reset_and_the_meter(gpu, det):
    cm = gpu
    a, H, rho = 5, 20, 8
    xs = [TG.bursts(600 + s, 700, 1) for s in range(3)]
    rig = Rig(cm, det, 3, 1, a, H, rho, 700, 8000, 8192)
    rig.run(xs)
    assert all(g < UNITY for g in rig.model.gmin)
    assert rig.m.min_gain(reset=True).tolist() == rig.model.gmin
    assert rig.m.min_gain().tolist() == [UNITY] * 3                          # re-armed, the history kept
    rig.model.gmin = [UNITY] * 3
    quiet = [np.full((50, 1), 10, dtype=np.int16)] * 3
    rig.run(quiet)                                               # the release of the bursts is still on its way
    assert all(g < UNITY for g in rig.model.gmin)
    rig.reset(1)                                                 # stream 1 starts again from silence, 0 and 2 go on
    ys = rig.run(xs)
    zero = RH.zero_hist(det, a, H, rho, 1)
    assert np.array_equal(ys[1], RH.model_limrel(det, xs[1], zero, 8000, 8192, a, H, rho)[0])
    assert not np.array_equal(ys[0][:50], RH.model_limrel(det, xs[0], zero, 8000, 8192, a, H, rho)[0][:50])
    assert rig.m.set_rc(0, 0, 4096) == cm.ERROR_INVAL and rig.m.set_rc(0, 32768, 4096) == cm.ERROR_INVAL
    assert rig.m.set_rc(0, 8000, 0) == cm.ERROR_INVAL and rig.m.set_rc(0, 8000, 65536) == cm.ERROR_INVAL
    assert rig.m.set_rc(3, 8000, 4096) == cm.ERROR_INVAL and rig.m.set_rc(-2, 8000, 4096) == cm.ERROR_INVAL
    assert rig.m.get(0) == (8000, 8192)
    rig.reset()
    rig.run(xs)
    rig.close()


def test_refusals(gpu):
    cm = gpu
    for det, a, H, rho in ((0, 6, 0, 12), (0, 9, 1028, 11), (1, 9, 1015, 11), (1, 6, 0, 5), (2, 6, 1, 5)):
        d = cm.LimDesc(0, 2, 2, a, H, 256, None)
        assert cm.lib.cmhip_lim_new_release(C.byref(d), det, rho) is None and b"lim_new: " in cm.lib.cmhip_last_error()
    rig = Rig(cm, SAMPLE, 2, 2, 6, 0, 9, 256, 10000, 8192)
    m, src, dst, st = rig.m, rig.src.dev, rig.dst.dev, rig.stride
    assert st == 520
    xs = [TG.bursts(700 + s, 256, 2) for s in range(2)]
    rig.run(xs)                                                  # a history that a launch would change
    rig.dst.array[:] = SENTINEL
    rig.src.array[:] = SENTINEL
    cases = {
        "misaligned in": (src + 2, st, 256, dst, st, None),
        "misaligned out": (src, st, 256, dst + 8, st, None),
        "in stride not a multiple of 8": (src, st + 4, 256, dst, st, None),
        "out stride too small": (src, st, 256, dst, 504, None),
        "frames above max_frames": (src, st, 257, dst, st, None),
        "a count above frames": (src, st, 100, dst, st, [100, 101]),
        "in == out": (src, st, 256, src, st, None),
        "in begins inside out": (dst + 2 * st, st, 256, dst, st, None),
    }
    for name, (a, ast, n, o, ost, fps) in cases.items():
        assert m.run_rc(a, ast, n, o, ost, fps) == cm.ERROR_INVAL, name
    assert cm.lib.cmhip_lim_run(m.h, None, st, 256, None, dst, st) == cm.ERROR_FAULT
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.run(xs)                                                  # the history is what the first run left
    rig.close()


# ---------------------------------------------------------------------------
# 5. rho = 0 through the new constructor

@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_release_zero_is_the_old_limiter(gpu, det):
    """cmhip_lim_new_release(d, detector, 0) is cmhip_lim_new_detector: the same delay and plan, and bit for bit the same
    output as a limiter created the old way, and as the old model, on one dense case per kernel form"""
    cm = gpu
    a, H, T, drive = (MH.SETS if det else TG.SETS)[2]
    model_of = MH.ModelTp if det else TG.Model
    for channels in (1, 2, 3):
        counts = [2 * TILE + 13, TILE, TILE - 1, 300, 1, 0]
        xs = [TG.bursts(1300 + 10 * channels + s, counts[0], channels) for s in range(len(counts))]
        outs = []
        for new in (False, True):
            rig = TG.Rig(cm, len(counts), channels, a, H, counts[0])                 # (made by cmhip_lim_new)
            rig.m.close()
            rig.m = (cm.Limiter(len(counts), channels, a, H, counts[0], detector=det, release_log2=0) if new else
                     cm.Limiter(len(counts), channels, a, H, counts[0], detector=det))
            rig.model = model_of(len(counts), channels, a, H)
            assert rig.m.delay() == rig.model.D and rig.m.detector() == det and rig.m.release() == 0
            rig.set(-1, T, drive)
            rig.run([x[:n] for x, n in zip(xs, counts)])          # (equal to the old model: checked there)
            first = rig.dst.array.copy()
            rig.run(xs, uniform=True)
            outs.append((first, rig.dst.array.copy(), rig.m.min_gain().tolist()))
            rig.close()
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
        assert min(outs[0][2][:3]) < UNITY


# ---------------------------------------------------------------------------
# 6. composition: bus -> limiter with a release -> the slots of a batch, block by block on the batch's stream

def test_chain_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    tb = _load("test_gpu_bus")
    cm = gpu
    S, B, F, a, H, rho, T, drive = 4, 2, 3000, 6, 30, 10, 29204, 8192
    blocks = [[F, F - 1, 1234, 2000], [5, 0, 0, 0], [2999, 3000, 5, 0], [0, 3, 0, 0], [777, 1500, 1500, 64]]
    table = ([0, 0, 1, 1, 1], [0, 1, 1, 2, 3], np.full((5, 1, 1), 8192, dtype=np.int16))
    model = RH.ModelRel(SAMPLE, B, 1, a, H, rho)
    model.set(-1, T, drive)
    src_b = cm.Batch(S, 1, F, flags=cm.VU, rate=48000)           # (device memory for the sources)
    mid_b = cm.Batch(B, 1, F, flags=cm.VU, rate=48000)           # (... and for the buses' sums)
    b = cm.Batch(B, 1, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
    bus = cm.Bus(S, B, 1, 1, F, 8, hip_stream=b.hip_stream())
    lim = cm.Limiter(B, 1, a, H, F, threshold=T, drive=drive, hip_stream=b.hip_stream(), release_log2=rho)
    assert bus.hip_stream() == b.hip_stream() == lim.hip_stream() and lim.release() == rho
    bus.set_routing(*table)
    pcm = [[] for _ in range(B)]
    for r, fps in enumerate(blocks):
        xs = [TG.bursts(1400 + 10 * r + s, fps[s], 1) for s in range(S)]
        want = model.run([y.reshape(-1, 1) for y in tb.model_bus(xs, table, B, 1)])
        for s in range(S):
            if fps[s]:
                src_b.upload(s, xs[s])
        src_b.sync()
        counts = bus.run(src_b.dev_in, src_b.stride, max(fps), mid_b.dev_in, mid_b.stride, fps)
        assert counts.tolist() == [y.shape[0] for y in want]
        lim.run(mid_b.dev_in, mid_b.stride, int(counts.max()), b.dev_in, b.stride, counts)
        b.run(int(counts.max()), counts)                         # (no sync between the three: the order is the stream's)
        for s, y in enumerate(want):
            if counts[s]:
                assert np.array_equal(b.download(s, int(counts[s])), y.reshape(-1)), (r, s)
            pcm[s].append(y.reshape(-1))
    res, rcs = b.vu_results()
    for s in range(B):
        y = np.concatenate(pcm[s])
        v = oracle.vu_new(1)
        oracle.vu_accumulate(v, y)
        _, vr = oracle.vu_result(v)
        assert rcs[s] == 0 and oracle_ffi.vu_result_dict(vr) == res[s].as_dict(), s
        assert res[s].frames == y.size and abs(res[s].global_peak) <= T
    assert lim.min_gain().tolist() == model.gmin and max(model.gmin) < UNITY
    lim.close()
    bus.close()
    for o in (b, mid_b, src_b):
        o.close()


# ---------------------------------------------------------------------------
# 7. the example

def test_batch_release_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_release"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_release.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert out[0].startswith("50 Hz tone at 29204 (-1 dBFS), drive 8192 (+6 dB) -> limiter: lookahead 64 frames, hold 0, "
                             "threshold 29204")
    assert len(out) == 3 and out[1].startswith("release_log2=0: ") and out[2].startswith("release_log2=11: ")
    # the same programme through the model
    T, drive, frames, period = 29204, 8192, 48000, 960
    x = np.round(29204 * np.sin(2 * np.pi * (np.arange(frames) % period) / period)).astype(np.int16)[:, None]
    ranges = []
    for line, rho in ((out[1], 0), (out[2], 11)):
        f = dict(kv.split("=") for kv in line.split()[1:])
        y, s = RH.model_limrel(SAMPLE, x, RH.zero_hist(SAMPLE, 6, 0, rho, 1), T, drive, 6, 0, rho)
        peak = int(np.abs(y.astype(np.int64)).max())
        assert abs(int(f["peak"])) == peak <= T and int(f["min_gain"]) == int(s.min())
        tail = s[frames - period:] / 32768
        print("batch_release rho %2d: model s over the last period %.4f .. %.4f; the example says %s .. %s"
              % (rho, tail.min(), tail.max(), f["gain_min"], f["gain_max"]))
        # the estimate leaves out the frames around the zero crossings and rounds: inside the model's range, near its floor
        assert tail.min() - 1e-3 <= float(f["gain_min"]) <= tail.min() + 0.02 and float(f["gain_max"]) <= tail.max() + 1e-3
        assert abs(float(f["range"]) - (float(f["gain_max"]) - float(f["gain_min"]))) < 2e-4
        ranges.append(float(f["range"]))
    assert ranges[1] < 0.6 * ranges[0]                           # the gain no longer follows the waveform
