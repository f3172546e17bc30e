"""GPU: channel mixing (cmhip_mix_*, csrc/k_mix.hip) against a numpy model of the arithmetic include/coolmic_hip.h
states, bit for bit: both kernel forms over dense per-stream matrices and ragged counts, vector and tile edges, the
extremes of the int32 bound and the rounding, identity and the creation default, per-stream matrices and the order of
set_matrix with the runs, the presets, refusals that launch nothing, the chain resampler -> mixer -> batch on one
stream, and the C example.  Output slots are pre-filled with a sentinel; every sample past a stream's count must still
hold it after a run.  (tests/test_mix_host.py takes the model and the dense matrices from here.)"""
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
SATURATED_MAX = 0.25              # of a dense case's outputs in the MODEL: a saturated output hides a wrong sum


def model_mix(x, W):
    """x int16 [F][C_in], W int16 [C_out][C_in] -> int16 [F][C_out]: sat16((sum_c W[o][c] x[f][c] + 8192) >> 14)"""
    W = np.asarray(W, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64).reshape(-1, W.shape[1])
    acc = x @ W.T
    assert acc.size == 0 or np.abs(acc + 8192).max() < 2 ** 31
    return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)


def noise(seed, frames, channels):
    """full-scale uniform noise with full-scale frames here and there (the kind tests/test_gpu_src.py uses)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(frames, channels)).astype(np.int16)
    x[rng.integers(0, max(frames, 1), size=frames // 16)] = 32767
    x[rng.integers(0, max(frames, 1), size=frames // 16)] = -32768
    return x


def dense_matrix(ci, co, seed):
    """every |w| in [3B/4, B], B = min(65535 // C_in, 8192), random signs: no entry a kernel could skip unnoticed"""
    B = min(65535 // ci, 8192)
    rng = np.random.default_rng(seed)
    w = rng.integers(3 * B // 4, B + 1, size=(co, ci)) * rng.choice([-1, 1], size=(co, ci))
    assert np.abs(w).sum(axis=1).max() <= 65535
    return w.astype(np.int16)


def saturated(y):
    return int(((y == 32767) | (y == -32768)).sum())


class Rig:
    """a mixer between two arrays of pinned, device-mapped host memory"""

    def __init__(self, cm, streams, ci, co, max_frames, matrices=None):
        self.cm, self.S, self.CI, self.CO = cm, streams, ci, co
        self.m = cm.Mixer(streams, ci, co, max_frames)
        self.in_stride = (max_frames * ci + 7) // 8 * 8
        self.out_stride = (max_frames * co + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.W = [self.m.get_matrix(s) for s in range(streams)]
        if matrices is not None:
            for s, w in enumerate(matrices):
                self.set(s, w)

    def set(self, stream, w):
        self.m.set_matrix(stream, w)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.W[s] = np.asarray(w, dtype=np.int16).reshape(self.CO, self.CI)
            assert np.array_equal(self.m.get_matrix(s), self.W[s])

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def run(self, xs, frames=None, uniform=False, wants=None):
        """xs: per stream int16 [F_s][C_in]; runs the device and the model, compares outputs and the untouched rest;
        -> the model's outputs"""
        counts = [np.asarray(x).reshape(-1, self.CI).shape[0] for x in xs]
        frames = max(counts) if frames is None else frames
        assert not uniform or all(n == frames for n in counts)
        self.src.array[:] = 0x5a5a
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.CI] = np.asarray(x, dtype=np.int16).reshape(-1)
        self.dst.array[:] = SENTINEL
        self.m.run(self.src.dev, self.in_stride, frames, self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = [model_mix(x, self.W[s]) for s, x in enumerate(xs)] if wants is None else wants
        self.check(self.dst.array, wants)
        return wants

    def check(self, array, wants):
        for s, want in enumerate(wants):
            n = want.size
            have = array[s, :n].reshape(-1, self.CO)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(),
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (array[s, n:] == SENTINEL).all(), ("stream", s, "written past its count")


# ---------------------------------------------------------------------------
# 1. both forms: dense matrices, a matrix per stream, ragged and uniform counts

PAIRS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (6, 2), (6, 1), (5, 3), (2, 6), (7, 5), (8, 2), (1, 16), (16, 1),
         (16, 16)]
FAST = {(1, 1), (1, 2), (2, 1), (2, 2)}


def forms_counts(t):
    return [2 * t + 13, t, t - 1, 1, 0]


@functools.lru_cache(maxsize=None)
def forms_case(ci, co, t):
    """matrices, full-length inputs and the model's outputs (uniform run) of a pair at tile_frames t, and the share
    of saturated outputs over the ragged and the uniform run -- computed once, never changed"""
    frames = 2 * t + 13
    W = [dense_matrix(ci, co, 1000 * ci + 10 * co + s) for s in range(5)]
    xs = [noise(100 * ci + co + 7 * s, frames, ci) for s in range(5)]
    full = [model_mix(x, w) for x, w in zip(xs, W)]
    ragged = [y[:n] for y, n in zip(full, forms_counts(t))]
    outs = sum(y.size for y in full + ragged)
    share = sum(saturated(y) for y in full + ragged) / outs
    return W, xs, full, ragged, share


@pytest.mark.parametrize("ci,co", PAIRS)
def test_forms(gpu, ci, co):
    cm = gpu
    plan = cm.plan_mix(5, ci, co, 1)
    assert plan.fast == (1 if (ci, co) in FAST else 0)
    t = plan.tile_frames
    W, xs, full, ragged, share = forms_case(ci, co, t)
    print("mix forms %2d -> %2d: tile_frames %d, saturated outputs in the model %.2f %%" % (ci, co, t, 100 * share))
    assert share < SATURATED_MAX
    counts = forms_counts(t)
    rig = Rig(cm, 5, ci, co, counts[0], W)
    rig.run([x[:n] for x, n in zip(xs, counts)], wants=ragged)
    rig.run(xs, uniform=True, wants=full)                        # a second run on the same mixer: there is no state
    rig.close()


def test_the_clamp_is_exercised(gpu):
    """at least one of the cases of test_forms saturates more than 1 % of its outputs"""
    shares = {p: forms_case(p[0], p[1], gpu.plan_mix(5, p[0], p[1], 1).tile_frames)[4] for p in PAIRS}
    print("mix saturated shares:", {p: round(100 * v, 2) for p, v in shares.items()})
    assert max(shares.values()) > 0.01


# ---------------------------------------------------------------------------
# 2. vector and tile edges: one stream per count

@pytest.mark.parametrize("ci,co", sorted(FAST) + [(3, 2), (6, 2)])
def test_vector_and_tile_edges(gpu, ci, co):
    cm = gpu
    t = cm.plan_mix(1, ci, co, 1).tile_frames
    counts = list(range(0, 18)) + list(range(t - 9, t + 10))
    S = len(counts)
    W = [dense_matrix(ci, co, 50 * ci + co + s) for s in range(S)]
    xs = [noise(3000 + 31 * ci + co + s, n, ci) for s, n in enumerate(counts)]
    wants = [model_mix(x, w) for x, w in zip(xs, W)]
    assert sum(saturated(y) for y in wants) < SATURATED_MAX * sum(y.size for y in wants)
    rig = Rig(cm, S, ci, co, max(counts), W)
    rig.run(xs, wants=wants)
    rig.close()


# ---------------------------------------------------------------------------
# 3. extremes of the int32 bound, and the rounding

def test_extremes_and_rounding(gpu):
    cm = gpu
    rig = Rig(cm, 1, 2, 1, 8, [[[-32768, 32767]]])
    x = np.array([[-32768, 32767], [32767, -32768]], dtype=np.int16)
    want = rig.run([x])[0]
    assert want.reshape(-1).tolist() == [32767, -32768]          # acc = +-(65535 * 32768 - 32767): both saturate
    rig.set(0, [[8192, 8192]])
    x = np.array([[1, 0], [-1, 0], [-1, -2], [32767, 32767], [-32768, -32768]], dtype=np.int16)
    want = rig.run([x])[0]
    assert want.reshape(-1).tolist() == [1, 0, -1, 32767, -32768]            # halves round towards +inf
    rig.close()
    # sixteen channels, sum |w| = 65535, full-scale inputs: signs matching the weights' (the largest positive sums
    # there are), opposite to them (the largest negative ones: |acc| = 32768 * sum of the positive weights + 32767 *
    # sum of the others), and every channel at one end
    w = np.full(16, 4096, dtype=np.int64) * np.where(np.arange(16) % 3 == 0, -1, 1)
    w[5] = -(65535 - 15 * 4096)
    assert np.abs(w).sum() == 65535
    x = np.array([np.where(w < 0, -32768, 32767), np.where(w < 0, 32767, -32768), [-32768] * 16, [32767] * 16],
                 dtype=np.int16)
    for co in (1, 2):
        W = np.array([w, -w][:co], dtype=np.int16)
        rig = Rig(cm, 1, 16, co, 8, [W])
        want = rig.run([x])[0]
        assert want[:2].tolist() == [[32767, -32768][:co], [-32768, 32767][:co]]
        rig.close()


# ---------------------------------------------------------------------------
# 4. identity and the matrix at creation

@pytest.mark.parametrize("channels", [1, 2, 6])
def test_identity(gpu, channels):
    cm = gpu
    t = cm.plan_mix(2, channels, channels, 1).tile_frames
    rig = Rig(cm, 2, channels, channels, t + 11)
    assert np.array_equal(rig.W[0], 16384 * np.eye(channels, dtype=np.int16))            # the creation default
    xs = [noise(400 + channels, t + 11, channels), noise(401 + channels, 5, channels)]
    rig.run(xs, wants=xs)
    rig.set(-1, 16384 * np.eye(channels, dtype=np.int16))
    rig.run(xs, wants=xs)
    rig.close()


def test_creation_default(gpu):
    cm = gpu
    x = noise(410, 300, 6)
    rig = Rig(cm, 1, 6, 2, 300)
    assert rig.W[0].tolist() == [[16384, 0, 0, 0, 0, 0], [0, 16384, 0, 0, 0, 0]]
    rig.run([x], wants=[x[:, :2].copy()])
    rig.close()
    x = noise(411, 300, 2)
    rig = Rig(cm, 1, 2, 6, 300)
    assert rig.W[0].tolist() == [[16384, 0], [0, 16384], [0, 0], [0, 0], [0, 0], [0, 0]]
    rig.run([x], wants=[np.concatenate([x, np.zeros((300, 4), dtype=np.int16)], axis=1)])
    rig.close()


# ---------------------------------------------------------------------------
# 5. a matrix per stream beyond one workgroup's worth of streams, and set_matrix in stream order

def test_per_stream_matrices_and_ordering(gpu):
    cm = gpu
    S = 300
    counts = [s % 65 for s in range(S)]
    W = [np.array([[8192 + s, -(4096 + 3 * s)]], dtype=np.int16) for s in range(S)]        # names its stream
    xs = [noise(500 + s, n, 2) for s, n in enumerate(counts)]
    rig = Rig(cm, S, 2, 1, 64, W)
    rig.run(xs)
    # no synchronisation anywhere: set, run, set, run
    A, B = np.array([[12000, -3000]], dtype=np.int16), np.array([[-7000, 9000]], dtype=np.int16)
    second = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    rig.dst.array[:] = SENTINEL
    second.array[:] = SENTINEL
    m = rig.m
    m.set_matrix(-1, A)
    m.run(rig.src.dev, rig.in_stride, 64, rig.dst.dev, rig.out_stride, counts)
    m.set_matrix(7, B)
    m.run(rig.src.dev, rig.in_stride, 64, second.dev, rig.out_stride, counts)
    m.sync()
    assert np.array_equal(m.get_matrix(7), B) and np.array_equal(m.get_matrix(8), A)
    rig.check(rig.dst.array, [model_mix(x, A) for x in xs])
    rig.check(second.array, [model_mix(x, B if s == 7 else A) for s, x in enumerate(xs)])
    assert not np.array_equal(model_mix(xs[7], A), model_mix(xs[7], B))
    second.free()
    rig.close()


# ---------------------------------------------------------------------------
# 6. the presets on the device

def test_presets(gpu):
    cm = gpu
    x = noise(600, 2500, 6)
    full = np.array([[32767] * 6, [-32768] * 6], dtype=np.int16)
    for preset in (cm.MIX_51_TO_STEREO, cm.MIX_51_TO_STEREO_NORM):
        ci, co, W = cm.mix_preset(preset)
        assert (ci, co) == (6, 2)
        rig = Rig(cm, 2, ci, co, 2500, [W, W])
        want = rig.run([x, full])
        raw = [(np.asarray(v, dtype=np.int64) @ W.astype(np.int64).T + 8192) >> 14 for v in (x, full)]
        if preset == cm.MIX_51_TO_STEREO_NORM:
            # rows sum to 16384: no sum leaves int16, nothing is clamped anywhere
            assert all(-32768 <= v.min() and v.max() <= 32767 for v in raw)
        else:
            assert raw[1].max() > 32767 and raw[1].min() < -32768 and saturated(want[0]) > 0
        assert want[1].tolist() == [[32767, 32767], [-32768, -32768]]
        rig.close()
    for preset, pair in ((cm.MIX_MONO_TO_STEREO, (1, 2)), (cm.MIX_STEREO_TO_MONO, (2, 1)), (cm.MIX_STEREO_TO_MS, (2, 2))):
        ci, co, W = cm.mix_preset(preset)
        assert (ci, co) == pair
        rig = Rig(cm, 1, ci, co, 1500, [W])
        rig.run([noise(610 + preset, 1500, ci)])
        rig.close()


# ---------------------------------------------------------------------------
# 7. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    rig = Rig(cm, 2, 2, 1, 256)
    m, src, dst, si, so = rig.m, rig.src.dev, rig.dst.dev, rig.in_stride, rig.out_stride
    assert (si, so) == (512, 264)
    rig.dst.array[:] = SENTINEL
    rig.src.array[:] = SENTINEL
    cases = {
        "misaligned in": (src + 2, si, 256, dst, so, None),
        "misaligned out": (src, si, 256, dst + 8, so, None),
        "in stride not a multiple of 8": (src, si + 4, 256, dst, so, None),
        "out stride not a multiple of 8": (src, si, 256, dst, so - 4, None),
        "in stride too small": (src, 504, 256, dst, so, None),
        "out stride too small": (src, si, 256, dst, 248, None),
        "frames above max_frames": (src, si, 257, dst, so, None),
        "a count above frames": (src, si, 100, dst, so, [100, 101]),
        "in == out": (src, si, 256, src, so, None),
        "out inside in": (src, si, 256, src + 16, so, None),
        "out begins in the last slot of in": (src, si, 256, src + 2 * (si + 256), so, None),
        "in begins inside out": (dst + 2 * so, si, 256, dst, so, None),
    }
    for name, (a, ast, n, o, ost, fps) in cases.items():
        assert m.run_rc(a, ast, n, o, ost, fps) == cm.ERROR_INVAL, name
    assert cm.lib.cmhip_mix_run(m.h, None, si, 256, None, dst, so) == cm.ERROR_FAULT
    assert cm.lib.cmhip_mix_run(m.h, src, si, 256, None, None, so) == cm.ERROR_FAULT
    # matrices: refused ones change nothing
    before = m.get_matrix(1)
    assert m.set_matrix_rc(0, [[32767, 32767]]) == 0 and m.set_matrix_rc(1, [[-32768, -32768]]) == cm.ERROR_INVAL
    assert m.set_matrix_rc(2, [[1, 1]]) == cm.ERROR_INVAL and m.set_matrix_rc(-2, [[1, 1]]) == cm.ERROR_INVAL
    assert cm.lib.cmhip_mix_set_matrix(m.h, 0, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_mix_get_matrix(m.h, 2, before.ctypes.data) == cm.ERROR_INVAL
    assert np.array_equal(m.get_matrix(1), before) and m.get_matrix(0).tolist() == [[32767, 32767]]
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.W[0] = m.get_matrix(0)
    rig.run([noise(700 + s, 256, 2) for s in range(2)])          # and the mixer works as before
    rig.close()


# ---------------------------------------------------------------------------
# 8. composition: resampler -> mixer -> the slots of a mono 48 kHz batch, all on the batch's stream

def test_composition_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    import importlib.util
    spec = importlib.util.spec_from_file_location("test_gpu_src_model", os.path.join(ROOT, "tests", "test_gpu_src.py"))
    tg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tg)
    cm = gpu
    L, M, T, H = cm.src_design(44100, 48000)
    S, F = 4, 3000
    fps = [F, F - 1, 1234, 7]
    xs = [noise(800 + s, fps[s], 2) for s in range(S)]
    _, _, W = cm.mix_preset(cm.MIX_STEREO_TO_MONO)
    want = [model_mix(tg.Model(L, M, H, 2).run(x), W) for x in xs]
    max_out = F * L // M + 1
    src_b = cm.Batch(S, 2, F, flags=cm.VU, rate=44100)           # (device memory for the 44.1 kHz sources)
    mid_b = cm.Batch(S, 2, max_out, flags=cm.VU, rate=48000)     # (... and for the stereo 48 kHz signal)
    for s in range(S):
        src_b.upload(s, xs[s])
    src_b.sync()
    b = cm.Batch(S, 1, max_out, flags=cm.OUT_PCM | cm.VU, rate=48000)
    assert b.set_gain(-1, 1, 1000, [1250]) == 0
    r = cm.Resampler(S, 2, 44100, 48000, F, hip_stream=b.hip_stream())
    m = cm.Mixer(S, 2, 1, max_out, matrix=W, hip_stream=b.hip_stream())
    assert r.hip_stream() == b.hip_stream() == m.hip_stream()
    counts = r.run(src_b.dev_in, src_b.stride, F, mid_b.dev_in, mid_b.stride, fps)
    assert counts.tolist() == [w.shape[0] for w in want]
    m.run(mid_b.dev_in, mid_b.stride, int(counts.max()), b.dev_in, b.stride, counts)
    b.run(int(counts.max()), counts)                             # (no sync between the three: the order is the stream's)
    res, rcs = b.vu_results()
    _, g = oracle.gain(1, 1, 1000, [1250])
    for s, y in enumerate(want):
        pcm = oracle.gain_apply(g, y.reshape(-1), 1)
        v = oracle.vu_new(1)
        oracle.vu_accumulate(v, pcm)
        _, vr = oracle.vu_result(v)
        assert rcs[s] == 0 and oracle_ffi.vu_result_dict(vr) == res[s].as_dict(), s
        assert res[s].frames == counts[s] and res[s].rate == 48000
        assert np.array_equal(b.download(s, int(counts[s])), pcm), s
    m.close()
    r.close()
    for o in (b, mid_b, src_b):
        o.close()


# ---------------------------------------------------------------------------
# 9. the example

def test_batch_downmix_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_downmix"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_downmix.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("44100 -> 48000: L 160 M 147 T 32; 2 -> 1 channels: W = {8192, 8192}")
    assert len(out) == 9 and all(ln.startswith("stream ") for ln in out[1:])
    for ln in out[1:]:
        f = dict(kv.split("=") for kv in ln.split()[2:])
        assert int(f["frames"]) == 24000 and int(f["rate"]) == 48000 and int(f["channels"]) == 1
        # a full-scale sine in both channels comes out as the same sine: -3 dB, and about -3 LUFS near 1 kHz
        assert -3.2 < float(f["power"]) < -2.8 and -4.0 < float(f["momentary"]) < -2.0
