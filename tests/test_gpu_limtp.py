"""GPU: the limiter's true-peak detector (cmhip_lim_new_detector, csrc/k_limtp.hip) against the numpy model of
tests/test_limtp_host.py, bit for bit: both kernel forms over five parameter sets on a signal of bursts, ragged and
uniform counts around the tile, the history length and the filter's 13 frames, a stream cut into runs without a
synchronisation, literal edges, the sample ceiling and the true-peak ceiling on the device's own output (by the numpy
filter and by the batch's true-peak meter), per-stream parameters and their order with the runs, reset and the meter,
refusals, the sample detector through the new constructor, and the C example.  Output slots are pre-filled with a
sentinel; every sample past a stream's count must still hold it after a run.  The limiter's tile, 4096 frames, is the
unit of the shapes."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_limtp", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MH = _load("test_limtp_host")      # the model, the parameter sets, the dense cases and their conditions
TG = MH.TG                         # tests/test_gpu_lim.py: the rig, the signal, the sample detector's model
SENTINEL, UNITY, TILE = TG.SENTINEL, 32768, MH.TILE


class Rig(TG.Rig):
    """a true-peak limiter between two arrays of pinned, device-mapped host memory, and its model"""

    def __init__(self, cm, streams, channels, a, H, max_frames, T=None, drive=None):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Limiter(streams, channels, a, H, max_frames, detector=cm.LIM_DETECT_TRUE_PEAK)
        self.model = MH.ModelTp(streams, channels, a, H)
        assert self.m.delay() == self.model.D == (1 << a) + 7 and self.m.detector() == 1
        self.stride = (max_frames * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.stride))
        if T is not None:
            self.set(-1, T, drive)


def plan_tile(cm, streams, channels, a, H):
    p = cm.plan_limtp(streams, channels, a, H, 1)
    assert p.fast == (1 if channels <= 2 else 0) and p.tile_frames == TILE and p.halo >= MH.geometry_tp(a, H)[3]
    return p.tile_frames


# ---------------------------------------------------------------------------
# 1. dense cases: five parameter sets, both forms, ragged and uniform counts

@pytest.mark.parametrize("channels", MH.CHANNELS)
@pytest.mark.parametrize("a,H,T,drive", MH.SETS)
def test_dense(gpu, a, H, T, drive, channels):
    cm = gpu
    t = plan_tile(cm, 14, channels, a, H)
    xs, counts, ragged, full, stats, gmin = MH.dense_case(a, H, T, drive, channels, t)
    hist = MH.geometry_tp(a, H)[3]
    assert counts == [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 14, 13, 12, 9, 8, 7, 1, 0]
    # the conditions on the input, on the model: a kernel that ignores the FIR, or one that never reduces, cannot pass
    differ, unity, change = MH.dense_shares(channels)
    print("limtp dense a %d H %4d T %5d drive %5d C %2d: differ %.1f %%; over the sets unity %.1f %%, changing %.1f %%"
          % (a, H, T, drive, channels, 100 * stats["differ"] / stats["frames"], 100 * unity, 100 * change))
    assert stats["differ"] >= MH.DIFFER_SHARE * stats["frames"] and min(differ) >= MH.DIFFER_SHARE
    assert unity >= MH.UNITY_SHARE and change >= MH.CHANGE_SHARE
    rig = Rig(cm, len(counts), channels, a, H, counts[0], T, drive)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    dev_peak = int(np.abs(rig.dst.array[:, :counts[0] * channels].astype(np.int64)).max())
    assert dev_peak <= T                                         # on the device's own output
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts: one run equals the same stream in many, queued without a synchronisation

@pytest.mark.parametrize("channels,a,H,T,drive", [(1, *MH.SETS[1]), (2, *MH.SETS[2]), (6, *MH.SETS[3]), (2, *MH.SETS[4]),
                                                  (1, *MH.SETS[0])])
def test_cuts(gpu, channels, a, H, T, drive):
    cm = gpu
    t = plan_tile(cm, 2, channels, a, H)
    hist = MH.geometry_tp(a, H)[3]
    x = [TG.bursts(7100 + 10 * channels + s, 3 * t, channels) for s in range(2)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [MH.model_limtp(v, zero, T, drive, a, H) for v in x]
    cuts = [1, 7, 12, 13, 14, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    for starve in (False, True):
        # stream 0 is cut as the list says; stream 1 in the same runs, or with 0 frames in alternate runs
        lim = cm.Limiter(2, channels, a, H, 3 * t, threshold=T, drive=drive, detector=1)
        chunks, pos = [], [0, 0]
        for r, n in enumerate(cuts):
            n1 = 0 if starve and r % 2 else n
            chunks.append([x[0][pos[0]:pos[0] + n], x[1][pos[1]:pos[1] + n1]])
            pos = [pos[0] + n, pos[1] + n1]
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

def test_single_full_scale_sample(gpu):
    cm = gpu
    rig = Rig(cm, 1, 1, 6, 1, 1000, 32767, 4096)
    x = np.zeros((1000, 1), dtype=np.int16)
    x[500] = -32768
    y = rig.run([x])[0]
    want = np.zeros((1000, 1), dtype=np.int16)
    want[500 + 71] = -32767                                      # the filter's largest tap is below unity: the sample decides
    assert np.array_equal(y, want) and rig.m.min_gain().tolist() == [32767]
    rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_square_wave_at_the_extremes(gpu, channels):
    """square waves, and the signs of the filter's second phase at full scale (the largest filter output int16 allows),
    at the corners of the parameters; T = 1 with drive 65535 gives the largest pr the division sees"""
    cm = gpu
    t = plan_tile(cm, 2, channels, 4, 3)
    n = t + 300
    sq = np.where((np.arange(n) // 5) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
    signs = np.where(MH.TP_H[1][::-1] > 0, 32767, -32768)
    worst = np.zeros((n, channels), dtype=np.int16)
    for pos in (100, t - 6, t + 100):                            # (one across the tile's edge)
        worst[pos:pos + 12, channels - 1] = signs
    assert int(MH.fir_abs(worst.astype(np.int64)).max()) > 16500 * 32767
    for T, drive in ((1, 4096), (32767, 65535), (1, 65535), (32767, 1), (1, 1)):
        rig = Rig(cm, 2, channels, 4, 3, n, T, drive)
        ys = rig.run([sq, worst])
        peak = int(np.abs(ys[0].astype(np.int64)).max())
        assert peak <= T and ((T, drive) != (1, 4096) or peak <= 1)
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_below_the_threshold_is_a_pure_delay(gpu, channels):
    cm = gpu
    a, H = 5, 9
    t = plan_tile(cm, 2, channels, a, H)
    n, D = t + 77, 39
    rng = np.random.default_rng(410 + channels)
    amp = 20000 * 8192 // 16571                                  # the filter's gain is at most 16571 / 8192
    xs = [rng.integers(-amp, amp + 1, size=(n, channels)).astype(np.int16), rng.integers(-amp, amp + 1, size=(9, channels)).astype(np.int16)]
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
    """a burst whose hold and release cross a tile edge, and one that straddles the next edge"""
    cm = gpu
    a, H, T = 6, 100, 10000
    A, D, W, hist = MH.geometry_tp(a, H)
    t = plan_tile(cm, 1, channels, a, H)
    n = 2 * t + 500
    x = np.full((n, channels), 300, dtype=np.int16)
    x[t - 60:t - 40] = 30000
    x[2 * t - 10:2 * t + 10, channels - 1] = -32768
    rig = Rig(cm, 1, channels, a, H, n, T, 4096)
    y = rig.run([x])[0]
    s = rig.model.s[0][0]
    assert s[t - 200] == UNITY and s[t - 1] < UNITY and s[t] < UNITY and s[t + 100] < UNITY and s[t + 400] == UNITY
    assert s[2 * t - 1] < UNITY and s[2 * t] < UNITY and np.abs(y.astype(np.int64)).max() <= T
    rig.close()


# ---------------------------------------------------------------------------
# 4. the ceiling between the samples, on the device's own output

@pytest.mark.parametrize("channels", [1, 2])
def test_true_peak_ceiling_on_the_sine(gpu, channels):
    """the full-scale sine at fs/4, 45 degrees off the grid: samples of +-23170, a true peak of 1.42 x 23170.  At
    T = 23170 the settled output's true peak is at most T * 2^13 + 8286 -- by the numpy filter over the device's output,
    and by a batch with true peak on that the limiter writes into."""
    cm = gpu
    a, H, T = 6, 1, 23170
    A, D, W, hist = MH.geometry_tp(a, H)
    settle = (2 * hist + 7) // 8 * 8
    n = TILE + 808
    x = MH.sine(n, math.pi / 2, math.pi / 4, channels)
    rig = Rig(cm, 1, channels, a, H, n, T, 4096)
    y = rig.run([x])[0]                                          # (equal to the model, |y| <= T: checked there)
    dev = rig.dst.array[0, :n * channels].reshape(-1, channels)
    bound = T * 8192 + MH.TP_ROUND
    tp = MH.true_peak(dev, settle)
    print("limtp sine C %d: true peak of the device's settled output %d = %.5f x T * 2^13" % (channels, tp, tp / (T * 8192)))
    assert 0.99 * T * 8192 <= tp <= bound and np.array_equal(dev, y)
    assert int(rig.model.s[0][0][settle:].min()) == int(rig.model.s[0][0][settle:].max()) == 23051      # the gain is constant
    # the same through the batch's meter: a second limiter writes into the batch's slots, in two runs; the first
    # window (the attack) is closed and dropped
    b = cm.Batch(1, channels, n, flags=cm.VU, rate=48000)
    assert b.set_true_peak(1) == 0
    lim = cm.Limiter(1, channels, a, H, n, threshold=T, drive=4096, hip_stream=b.hip_stream(), detector=1)
    rig.fill([x])
    peaks = []
    for lo, hi in ((0, settle), (settle, n)):
        lim.run(rig.src.dev + lo * channels * 2, rig.stride - lo * channels, hi - lo, b.dev_in, b.stride, [hi - lo])
        b.run(hi - lo, [hi - lo])
        rc, r = b.tp_result(0)
        assert rc == 0 and r.frames == hi - lo
        peaks.append(r.global_peak)
    assert peaks[1] == tp and peaks[1] <= bound and peaks[0] <= T * 8192 * 1.01
    lim.close()
    b.close()
    rig.close()


# ---------------------------------------------------------------------------
# 5. parameters and state

def test_per_stream_parameters_and_ordering(gpu):
    cm = gpu
    S, a, H = 300, 4, 5
    counts = [40 + s % 65 for s in range(S)]
    xs = [TG.bursts(900 + s, n, 2) for s, n in enumerate(counts)]
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
    assert not np.array_equal(then[7], MH.model_limtp(xs[7], before, 9000, 5000, a, H)[0])
    assert m.min_gain().tolist() == rig.model.gmin
    second.free()
    rig.close()


def test_reset_and_the_meter(gpu):
    cm = gpu
    a, H = 5, 20
    xs = [TG.bursts(600 + s, 700, 1) for s in range(3)]
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
    zero = np.zeros((MH.geometry_tp(a, H)[3], 1), dtype=np.int16)
    assert np.array_equal(ys[1], MH.model_limtp(xs[1], zero, 8000, 8192, a, H)[0])
    assert not np.array_equal(ys[0][:50], MH.model_limtp(xs[0], zero, 8000, 8192, a, H)[0][:50])
    assert rig.m.set_rc(0, 0, 4096) == cm.ERROR_INVAL and rig.m.set_rc(0, 32768, 4096) == cm.ERROR_INVAL
    assert rig.m.set_rc(0, 8000, 0) == cm.ERROR_INVAL and rig.m.set_rc(0, 8000, 65536) == cm.ERROR_INVAL
    assert rig.m.set_rc(3, 8000, 4096) == cm.ERROR_INVAL and rig.m.set_rc(-2, 8000, 4096) == cm.ERROR_INVAL
    assert rig.m.get(0) == (8000, 8192)
    rig.reset()
    rig.run(xs)
    rig.close()


# ---------------------------------------------------------------------------
# 6. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    for det, a, H in ((2, 6, 1), (1, 6, 0), (1, 9, 1526), (7, 6, 1)):
        d = cm.LimDesc(0, 2, 2, a, H, 256, None)
        assert cm.lib.cmhip_lim_new_detector(C.byref(d), det) is None and b"lim_new: " in cm.lib.cmhip_last_error()
    rig = Rig(cm, 2, 2, 6, 1, 256, 10000, 8192)
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
# 7. the sample detector through the new constructor

def test_sample_detector_is_unchanged(gpu):
    """cmhip_lim_new_detector(d, 0) is cmhip_lim_new: delay A - 1, and bit for bit the same output as a limiter created
    the old way, and as the sample detector's model, on one dense case"""
    cm = gpu
    a, H, T, drive = TG.SETS[2]
    for channels in (2, 3):
        t = cm.plan_lim(8, channels, a, H, 1).tile_frames
        xs, counts, ragged, full, unity, change, peak, gmin = TG.dense_case(a, H, T, drive, channels, t)
        outs = []
        for new in (False, True):
            rig = TG.Rig(cm, len(counts), channels, a, H, counts[0])                 # (made by cmhip_lim_new)
            if new:
                rig.m.close()
                rig.m = cm.Limiter(len(counts), channels, a, H, counts[0], detector=cm.LIM_DETECT_SAMPLE)
            assert rig.m.delay() == (1 << a) - 1 and rig.m.detector() == 0
            rig.set(-1, T, drive)
            got = rig.run([x[:n] for x, n in zip(xs, counts)])
            assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
            first = rig.dst.array.copy()
            got = rig.run(xs, uniform=True)
            assert all(np.array_equal(g, w) for g, w in zip(got, full))
            outs.append((first, rig.dst.array.copy(), rig.m.min_gain().tolist()))
            rig.close()
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


# ---------------------------------------------------------------------------
# 8. the example

def test_batch_tplimiter_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_tplimiter"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_tplimiter.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert out[0].startswith("sine at fs/4, samples +-23170 -> limiter: true-peak detector, lookahead 64 frames, hold 1 "
                             "(delay 71), threshold 29204 (-1 dBTP), drive 4096")
    assert len(out) == 2 and out[1].startswith("programme: ")
    f = dict(kv.split("=") for kv in out[1].split()[1:])
    T = 29204
    assert int(f["frames"]) == 24000 - 280 and int(f["bound"]) == T * 8192 + 8286
    # the same programme through the model: the sine, the flush of silence, the window opened after `settle` frames
    a, H, frames, settle = 6, 1, 24000, 280
    x = np.zeros((frames + 71, 1), dtype=np.int16)
    x[:frames, 0] = np.where(np.arange(frames) & 2, -23170, 23170)
    y, s = MH.model_limtp(x, np.zeros((MH.geometry_tp(a, H)[3], 1), dtype=np.int16), T, 4096, a, H)
    peak = MH.true_peak(y[:frames], settle)
    print("batch_tplimiter: model peak %d = %.5f x T * 2^13, min s %d" % (peak, peak / (T * 8192), int(s.min())))
    assert int(f["peak"]) == peak <= int(f["bound"]) and peak >= 0.99 * T * 8192      # into the ceiling, not past it
    assert abs(float(f["dbtp"]) - 20 * math.log10(peak / 2 ** 28)) < 1e-3 and float(f["dbtp"]) < -1.0
    assert int(f["min_gain"]) == int(s.min()) < 29054 == int(s[settle:frames].min())  # the meter: the first frames' transient
