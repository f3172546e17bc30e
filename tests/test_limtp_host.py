"""CPU: the limiter's true-peak detector (cmhip_lim_new_detector, csrc/k_limtp.hip) on the host side.  The header, the
checks at their edges, cmhip_lim_threshold_dbtp, the plan (csrc/lim_plan.h: plan_limtp beside an unchanged plan_lim)
through the library and as a stand-alone C++ program, plainly and under AddressSanitizer + UBSan; the kernels' division
restated in numpy against `//` over every pr up to 2^21; a numpy int64 MODEL of the arithmetic include/coolmic_hip.h
states (tests/test_gpu_limtp.py compares the device against it bit for bit) and the model's own properties: the sample
ceiling, the pure delay, cut-invariance, the true-peak bound where the gain is constant, and the case the detector
exists for -- a sample-peak limiter that lets an inter-sample peak of 1.4 x T through; an emulation of the kernels'
decomposition (the seam, the 13 frames in front of the evaluated range, consecutive vectors per thread, the passes, the
delayed read at A + 8, the history write) at the plan's tile against the model; and the generated assembly.  Nothing
here needs a GPU."""
import ctypes as C
import functools
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "limtp_plan_test.cpp")


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_lim_model", os.path.join(ROOT, "tests", "test_gpu_lim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # model_lim, geometry, bursts of the sample detector's tests
UNITY = 32768
SWV = np.lib.stride_tricks.sliding_window_view

# BS.1770 Annex 2's filter as the engine holds it (cmhip_tp_coefficients(); test_tp_table_is_the_library_s holds this copy
# against the library's): 4 phases of 12 taps, units of 2^-13; phases 2 and 3 are 1 and 0 reversed
_P0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
_P1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
TP_H = np.array([_P0, _P1, _P1[::-1], _P0[::-1]], dtype=np.int64)
TP_ROUND = 8286                    # what rounding each output sample can add to a filter output: sum |h| / 2, rounded up
FRONT = 13                         # frames in front of frame n that g[n] reads


# ---------------------------------------------------------------------------
# The model

def geometry_tp(a, H):
    """-> A, Dtp, W, HISTtp"""
    A = 1 << a
    return A, A + 7, A + H, 2 * A + H - 2 + FRONT


def fir_abs(z):
    """z int64 [n][C] -> int64 [n - 11][C]: max_p |y_p[m]| for m = 11 .. n - 1"""
    win = SWV(z, 12, axis=0)[..., ::-1]                           # [m - 11][C][k] = z[m - k][C]
    return np.abs(np.einsum("mck,pk->mcp", win, TP_H)).max(axis=2)


def detector_tp(z):
    """z int64 [n][C] -> t int64 [n - 13]: t of frames 13 .. n - 1"""
    n = z.shape[0]
    return np.maximum(np.abs(z[FRONT - 8:n - 8]) << 13, fir_abs(z)[:n - FRONT]).max(axis=1)


def model_limtp(x, hist, T, drive, a, H):
    """x int16 [F][C]; hist int16 [HISTtp][C], oldest first -> y int16 [F][C], s int64 [F]"""
    A, D, W, HIST = geometry_tp(a, H)
    F = x.shape[0]
    assert hist.shape[0] == HIST and H >= 1 and A + W <= 2549
    if F == 0: return x.copy(), np.zeros(0, np.int64)
    z = np.concatenate([hist, x]).astype(np.int64)
    t = detector_tp(z)                                            # of frames 13 .. : A + W - 2 + F entries
    assert t.max() <= 16571 * 32768
    pr = (drive * t + (1 << 25) - 1) >> 25
    assert pr.max() <= 1060528
    g = np.where(pr <= T, UNITY, (T * 32768) // np.maximum(pr, 1))
    m = SWV(g, W).min(axis=1)
    s = SWV(m, A).sum(axis=1) >> a                                # F entries
    y = (z[HIST - D: HIST - D + F] * (drive * s)[:, None] + (1 << 26)) >> 27
    assert np.abs(y).max(initial=0) <= T
    return y.astype(np.int16), s


def true_peak(y, start=0):
    """y [F][C] (zeros in front) -> the largest |filter output| over phases, channels and the frames from `start` on,
    units of 2^-13; with start >= 11 only outputs whose 12 taps all lie at or behind frame start - 11 count"""
    z = np.concatenate([np.zeros((11, y.shape[1]), dtype=np.int64), y.astype(np.int64)])
    return int(fir_abs(z)[start:].max())


class ModelTp(TG.Model):
    """the streams of a true-peak limiter as the header states them"""

    def __init__(self, streams, channels, a, H):
        super().__init__(streams, channels, a, H)
        self.A, self.D, self.W, self.HIST = geometry_tp(a, H)
        self.hist = [np.zeros((self.HIST, channels), dtype=np.int16) for _ in range(streams)]

    def run(self, xs):
        ys = []
        for s, x in enumerate(xs):
            x = np.asarray(x, dtype=np.int16).reshape(-1, self.C)
            y, sg = model_limtp(x, self.hist[s], self.par[s][0], self.par[s][1], self.a, self.H)
            self.hist[s] = TG.next_hist(self.hist[s], x)
            if sg.size:
                self.gmin[s] = min(self.gmin[s], int(sg.min()))
                self.s[s].append(sg)
            ys.append(y)
        return ys


def sine(frames, w, phase, channels=1, amp=32767):
    n = np.arange(frames)
    return np.round(amp * np.sin(w * n + phase)).astype(np.int16)[:, None].repeat(channels, axis=1)


# ---------------------------------------------------------------------------
# The dense cases of the GPU tests: (a, H, T, drive); the last one has HISTtp = 2560 exactly

SETS = [(3, 1, 32767, 4096), (6, 1, 23170, 4096), (6, 64, 29204, 8192), (8, 1024, 1000, 65535), (9, 1525, 20000, 5000)]
CHANNELS = [1, 2, 3, 6, 16]
TILE = 4096                        # the limiter's tile; every test holds the plan against it
DIFFER_SHARE = 0.03                # per set: output frames whose s is not the sample detector's s, delayed by 8
UNITY_SHARE = 0.20                 # over the five sets together: frames at unity
CHANGE_SHARE = 0.15                # ... and adjacent frames whose s differs


def dense_counts(t, hist):
    return [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 14, 13, 12, 9, 8, 7, 1, 0]


@functools.lru_cache(maxsize=None)
def dense_case(a, H, T, drive, channels, t=TILE):
    """the streams' full-length inputs (the same signal for every stream, bursts(7, 2t + 13, C): what differs between
    the streams is where it is cut), and over the ragged run followed by the uniform run on one limiter: the model's
    outputs of both, the meters, and of every frame the model put out the three counts of the dense conditions --
    computed once, never changed"""
    hist = geometry_tp(a, H)[3]
    counts = dense_counts(t, hist)
    x = TG.bursts(7, counts[0], channels)
    xs = [x] * len(counts)
    model = ModelTp(len(counts), channels, a, H)
    model.set(-1, T, drive)
    ragged = model.run([v[:n] for v, n in zip(xs, counts)])
    full = model.run(xs)
    # the sample detector on the same frames, its s delayed by 8: stream 0 as one sequence of both runs
    s_tp = np.concatenate(model.s[0])
    both = np.concatenate([x, x])
    s_sm = TG.model_lim(both, np.zeros((TG.geometry(a, H)[3], channels), dtype=np.int16), T, drive, a, H)[1]
    s_sm = np.concatenate([np.full(8, UNITY), s_sm[:-8]])
    stats = {"frames": int(s_tp.size), "differ": int((s_tp != s_sm).sum()), "unity": int((s_tp == UNITY).sum()),
             "change": int((np.diff(s_tp) != 0).sum())}
    return xs, counts, ragged, full, stats, list(model.gmin)


def dense_shares(channels):
    """-> per set the share of differing frames; over the five sets the shares at unity and of changing gain"""
    st = [dense_case(*p, channels)[4] for p in SETS]
    frames = sum(s["frames"] for s in st)
    return ([s["differ"] / s["frames"] for s in st], sum(s["unity"] for s in st) / frames,
            sum(s["change"] for s in st) / frames)


@pytest.mark.parametrize("channels", CHANNELS)
def test_dense_conditions(channels):
    """the conditions on the dense input, on the model alone: a kernel that ignores the FIR cannot pass the device test"""
    differ, unity, change = dense_shares(channels)
    print("limtp dense C %2d: differ %s %%, unity %.1f %%, changing %.1f %%"
          % (channels, " ".join("%.1f" % (100 * d) for d in differ), 100 * unity, 100 * change))
    assert min(differ) >= DIFFER_SHARE and unity >= UNITY_SHARE and change >= CHANGE_SHARE


# ---------------------------------------------------------------------------
# Header, checks, the threshold helper

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_lim_desc_t d; (void)sizeof(d);\n"
           "d.device = 0; d.streams = d.channels = 1; d.lookahead_log2 = 6; d.hold = 1; d.max_frames = 1; d.hip_stream = 0;\n"
           "return cmhip_lim_check_detector(CMHIP_LIM_DETECT_TRUE_PEAK, 6, 1, 32767, 4096)"
           " + (cmhip_lim_new_detector(0, CMHIP_LIM_DETECT_SAMPLE) != 0) + (int)cmhip_lim_detector(0)"
           " + (int)cmhip_lim_threshold_dbtp(-1.0) + (int)cmhip_lim_delay(0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check_detector(cm):
    ok = cm.lim_check_detector
    assert cm.LIM_DETECT_SAMPLE == 0 and cm.LIM_DETECT_TRUE_PEAK == 1
    assert ok(2, 6, 1, 32767, 4096) == cm.ERROR_INVAL and b"lim:" in cm.lib.cmhip_last_error()
    assert ok(0xffffffff, 6, 1, 32767, 4096) == cm.ERROR_INVAL
    assert ok(1, 6, 0, 32767, 4096) == cm.ERROR_INVAL and b"hold" in cm.lib.cmhip_last_error()
    assert ok(0, 6, 0, 32767, 4096) == 0 and ok(1, 6, 1, 32767, 4096) == 0
    assert ok(1, 9, 1525, 1, 1) == 0 and ok(1, 9, 1526, 1, 1) == cm.ERROR_INVAL and ok(0, 9, 1526, 1, 1) == 0
    for a, want in ((2, cm.ERROR_INVAL), (3, 0), (9, 0), (10, cm.ERROR_INVAL)):
        assert ok(1, a, 1, 32767, 4096) == want, a
    for a in range(3, 9):                                         # below a = 9 the old rule is the tighter one
        assert ok(1, a, 2048 - (1 << a), 1, 1) == 0 and ok(1, a, 2049 - (1 << a), 1, 1) == cm.ERROR_INVAL
    for det in (0, 1):
        for T, want in ((0, cm.ERROR_INVAL), (1, 0), (32767, 0), (32768, cm.ERROR_INVAL)):
            assert ok(det, 6, 1, T, 4096) == want, (det, T)
        for drive, want in ((0, cm.ERROR_INVAL), (1, 0), (65535, 0), (65536, cm.ERROR_INVAL)):
            assert ok(det, 6, 1, 20000, drive) == want, (det, drive)
    for a, H, T, drive in ((6, 0, 1, 1), (6, 5, 0, 1), (10, 0, 1, 1), (9, 1536, 32767, 65535), (9, 1537, 1, 1)):
        assert ok(0, a, H, T, drive) == cm.lim_check(a, H, T, drive)              # detector 0 is cmhip_lim_check
    assert ok(1, 6, 0xffffffff, 1, 1) == cm.ERROR_INVAL and ok(1, 0xffffffff, 1, 1, 1) == cm.ERROR_INVAL


def test_threshold_dbtp(cm):
    f = cm.lim_threshold_dbtp
    assert f(-1.0) == 29204 == math.floor(32768 * 10 ** (-1 / 20))
    assert f(0.0) == 32767 and f(3.0) == 32767 and f(-200.0) == 1 and f(float("nan")) == 0
    assert f(float("inf")) == 32767 and f(float("-inf")) == 1
    assert f(-6.0) == math.floor(32768 * 10 ** (-6 / 20)) == 16422


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_lim_new_detector(None, 1) is None and lib.cmhip_lim_detector(None) == 0
    # descriptors are refused before any device is touched
    for det, streams, channels, a, hold, frames in ((2, 1, 2, 6, 1, 1024), (0xffffffff, 1, 2, 6, 1, 1024),
                                                    (1, 1, 2, 6, 0, 1024), (1, 1, 2, 9, 1526, 1024), (1, 1, 2, 3, 2041, 1024),
                                                    (1, 0, 2, 6, 1, 1024), (1, 1, 17, 6, 1, 1024), (1, 1, 2, 2, 1, 1024),
                                                    (1, 1, 2, 6, 1, 0), (1, 1, 2, 6, 1, (1 << 30) + 1),
                                                    (1, 1 << 20, 16, 6, 1, 1024), (0, 1, 2, 9, 1537, 1024)):
        d = cm.LimDesc(0, streams, channels, a, hold, frames, None)
        assert lib.cmhip_lim_new_detector(C.byref(d), det) is None, (det, streams, channels, a, hold, frames)
        assert b"lim_new: " in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Limiter(streams, channels, a, hold, frames, detector=det)


def test_tp_table_is_the_library_s(cm):
    assert np.array_equal(cm.tp_coefficients().astype(np.int64), TP_H)
    assert int(np.abs(TP_H).sum(axis=1).max()) == 16571 and TP_ROUND == (16571 + 1) // 2


# ---------------------------------------------------------------------------
# The launcher's plan

def test_plan(cm):
    for a in range(3, 10):
        A = 1 << a
        top = min(2048 - A, 2549 - 2 * A)
        for H in (1, 2, top):
            hist = geometry_tp(a, H)[3]
            halo = (hist + 7) // 8 * 8
            for ch in range(1, 17):
                p = cm.plan_limtp(5, ch, a, H, 1)                 # a one-frame run: one workgroup per stream
                assert (p.err, p.grid, p.chunks, p.block) == (0, 5, 1, 256), (a, H, ch)
                assert p.fast == (1 if ch <= 2 else 0)
                t = p.tile_frames
                assert t == TILE >= p.halo == halo >= hist and halo <= 2560
                assert p.lds_bytes == (t + halo) * 4 <= 65536
                assert t + halo <= 256 * 26                       # the elements a thread keeps (LIM_R)
                for frames in (1, t - 1, t, t + 1, 100000):
                    q = cm.plan_limtp(3, ch, a, H, frames)
                    assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
                # the old plan unchanged: the sample detector's halo for the same numbers
                o = cm.plan_lim(5, ch, a, H, 1)
                assert (o.err, o.grid, o.chunks, o.block, o.fast, o.tile_frames) == (0, 5, 1, 256, p.fast, t)
                assert o.halo == (TG.geometry(a, H)[3] + 7) // 8 * 8 and o.lds_bytes == (t + o.halo) * 4
        assert cm.plan_limtp(4, 2, a, top + 1, 100).grid == 0 and cm.plan_limtp(4, 2, a, 0, 100).grid == 0
        assert cm.plan_lim(4, 2, a, 0, 100).grid == 4
    assert geometry_tp(9, 1525)[3] == 2560 == cm.plan_limtp(1, 1, 9, 1525, 1).halo
    p = cm.plan_limtp(1 << 20, 2, 6, 1, 1 << 23)                  # no grid of 2^31 workgroups
    assert p.err != 0 and p.grid == 0
    assert cm.plan_limtp(0, 2, 6, 1, 100).grid == 0 and cm.plan_limtp(4, 2, 6, 1, 0).grid == 0
    for ch, a, H in ((0, 6, 1), (17, 6, 1), (2, 2, 1), (2, 10, 1), (2, 6, 1985)):
        p = cm.plan_limtp(4, ch, a, H, 100)
        assert p.grid == 0 and p.err == 0


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_as_a_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "limtp_plan_test", [])               # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"plans ok: \d{5,} geometries", out.stdout), out.stdout + out.stderr


def test_plan_under_address_and_ub_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", str(probe), "-o", str(tmp_path / "probe")] + san, capture_output=True, text=True)
    if r.returncode != 0:                                         # (decided on a program that cannot be wrong)
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    exe, r = _build_plan_test(tmp_path, "limtp_plan_san", san)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "plans ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The division (lim_div, csrc/k_lim.h) with the true-peak detector's range of pr: up to 2^21 (the largest pr is
# 1 060 528).  As tests/test_lim_host.py: the correctly rounded reciprocal and its two float neighbours.

def _lim_div(num, pr, nudge):
    rcp = np.float32(1.0) / pr.astype(np.float32)
    if nudge:
        rcp = np.nextafter(rcp, np.float32(np.inf if nudge > 0 else 0.0), dtype=np.float32)
    q = (np.float32(num) * rcp).astype(np.uint32).astype(np.int64)            # one rounding of the product, truncated
    r = np.int64(num) - q * pr
    assert (np.abs(q * pr) < 2 ** 32).all() and (r > -pr).all() and (r < 2 * pr).all()      # what the u32 code relies on
    return np.where(r < 0, q - 1, np.where(r >= pr, q + 1, q))


@pytest.mark.parametrize("T", [1, 2, 3, 255, 256, 16384, 29204, 32766, 32767])
def test_division_is_exact(T):
    top = 1 << 21
    pr = np.arange(T + 1, top + 1, dtype=np.int64)
    num = T * 32768
    assert float(np.float32(num)) == num and float(np.float32(top)) == top and (pr.astype(np.float32) == pr).all()
    assert (65535 * 16571 * 32768 + (1 << 25) - 1) >> 25 == 1060528 < top     # the largest pr
    want = num // pr
    for nudge in (-1, 0, 1):
        assert np.array_equal(_lim_div(num, pr, nudge), want), (T, nudge)


# ---------------------------------------------------------------------------
# The model's own properties

@pytest.mark.parametrize("a,H,T,drive", SETS)
def test_model_properties(a, H, T, drive):
    A, D, W, hist = geometry_tp(a, H)
    assert D == A + 7 and (D + 1) % 8 == 0 and hist == A + W - 2 + 13
    zero = np.zeros((hist, 2), dtype=np.int16)
    x = TG.bursts(42 + a, 3 * TILE, 2)
    y, s = model_limtp(x, zero, T, drive, a, H)                   # (asserts |y| <= T itself)
    assert np.abs(y.astype(np.int64)).max() <= T and s.min() < UNITY
    # cut-invariance: one run equals the same stream in runs of 1, 7, 12, 13, 14, HIST - 1, HIST, HIST + 1, 0, 1000, rest
    h, pos, parts = zero, 0, []
    for n in (1, 7, 12, 13, 14, hist - 1, hist, hist + 1, 0, 1000, x.shape[0]):
        part = x[pos:pos + n]
        parts.append(model_limtp(part, h, T, drive, a, H)[0])
        h = TG.next_hist(h, part)
        pos += part.shape[0]
    assert pos == x.shape[0] and np.array_equal(np.concatenate(parts), y)
    # below the threshold (the TRUE peak: the filter's gain is at most 16571 / 8192): a pure delay at unity drive, the
    # rounded product otherwise
    amp = T * 8192 // 16571 // 4
    q = (x.astype(np.int64) * amp // 32768).astype(np.int16)      # |q| <= amp: below T also at drive 12345
    y, s = model_limtp(q, zero, T, 4096, a, H)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], q[:-D])
    y, s = model_limtp(q, zero, T, 12345, a, H)
    assert (s == UNITY).all() and np.array_equal(y[D:], ((q[:-D].astype(np.int64) * 12345 + 2048) >> 12))


SINES = [("fs/4 at 45 degrees", math.pi / 2, math.pi / 4), ("fs/8", math.pi / 4, 0.0), ("0.37 pi", 0.37 * math.pi, 0.0)]


@pytest.mark.parametrize("name,w,phase", SINES)
@pytest.mark.parametrize("a,H,T", [(6, 1, 23170), (3, 1, 23170), (6, 64, 29204)])
def test_model_holds_the_true_peak_bound_on_sines(a, H, T, name, w, phase):
    """full-scale sines into a limiter at unity drive: once the attack has settled the gain is constant (or, at 0.37 pi,
    moves by a few units of 2^-15 only), and the true peak of the output is at most T * 2^13 + 8286"""
    A, D, W, hist = geometry_tp(a, H)
    x = sine(2 * hist + 2000, w, phase)
    y, s = model_limtp(x, np.zeros((hist, 1), dtype=np.int16), T, 4096, a, H)
    tp = true_peak(y, 2 * hist)
    print("limtp sine %s a %d H %d T %d: true peak %.5f x T * 2^13, s %d..%d"
          % (name, a, H, T, tp / (T * 8192), s[2 * hist:].min(), s[2 * hist:].max()))
    assert tp <= T * 8192 + TP_ROUND
    assert tp >= 0.99 * T * 8192                                  # and the ceiling is used: no needless reduction


def test_model_overshoot_where_the_gain_moves():
    """NOT a bound, a record (DESIGN 4.10 quotes it): where the gain moves inside the 12 frames of a filter output the
    true-peak ceiling is no guarantee.  Mono bursts, eight seeds of 3 tiles each, T = 20000 at unity drive: the largest
    true peak of the model's output over T * 2^13, beside what the sample detector leaves.  Asserted is only what holds by
    construction -- the sample ceiling -- and that the detector is what makes the difference."""
    T = 20000
    for a, H in ((3, 1), (6, 1), (6, 64), (8, 1024)):
        worst = sample_mode = 0
        for seed in range(8):
            x = TG.bursts(100 + seed, 3 * TILE, 1)
            y, s = model_limtp(x, np.zeros((geometry_tp(a, H)[3], 1), dtype=np.int16), T, 4096, a, H)
            assert np.abs(y.astype(np.int64)).max() <= T
            worst = max(worst, true_peak(y))
            y, s = TG.model_lim(x, np.zeros((TG.geometry(a, H)[3], 1), dtype=np.int16), T, 4096, a, H)
            sample_mode = max(sample_mode, true_peak(y))
        print("limtp overshoot a %d H %4d: true-peak detector %+.3f %%, sample detector %+.1f %%"
              % (a, H, 100 * (worst / (T * 8192) - 1), 100 * (sample_mode / (T * 8192) - 1)))
        assert worst < sample_mode


def test_sample_detector_lets_an_inter_sample_peak_through():
    """the case the feature exists for: a full-scale sine at fs/4, phase 45 degrees, has samples of +-23170 only; the
    sample detector at T = 23170 leaves it alone, and its true peak is 1.42 x T"""
    a, H, T = 6, 1, 23170
    x = sine(3000, math.pi / 2, math.pi / 4)
    assert int(np.abs(x.astype(np.int64)).max()) == 23170
    y, s = TG.model_lim(x, np.zeros((TG.geometry(a, H)[3], 1), dtype=np.int16), T, 4096, a, H)
    assert (s == UNITY).all() and np.abs(y.astype(np.int64)).max() == T
    ratio = true_peak(y, 1000) / (T * 8192)
    assert 1.3 < ratio < 1.45                                      # (1.42 here: the sine's own peak is 1.414 x T)
    y, s = model_limtp(x, np.zeros((geometry_tp(a, H)[3], 1), dtype=np.int16), T, 4096, a, H)
    assert true_peak(y, 1000) <= T * 8192 + TP_ROUND and s[1000:].max() < 0.73 * UNITY


# ---------------------------------------------------------------------------
# The decomposition of the limiter's one tile (csrc/k_lim_tile.h: lim_tile<TP, REL, SLOTS, CT>), step by step in numpy,
# one workgroup per tile.  tests/test_lim_host.py and tests/test_limrel_host.py run it too, each with the slot count and
# the release of its own kernels.

BLOCK = 256
UNWRITTEN = 1 << 40


def _gain_sample(peak, drive, T):
    pr = (peak * drive + 4095) >> 12
    return np.where(pr <= T, UNITY, (T * 32768) // np.maximum(pr, 1))


def _gain(t, drive, T):
    pr = (drive * t + (1 << 25) - 1) >> 25
    return np.where(pr <= T, UNITY, (T * 32768) // np.maximum(pr, 1))


def _pair_dot(loc):
    """loc int64 [n][L] (local frames of one channel per thread) -> max_p |y_p[t]| for t = 11 .. L - 1 in the kernels' pair
    form: y_p[t] = sum_{i<6} dot2(P[t - 2i], K[p][i]), P[t] = (x[t-1], x[t]), K[p][i] = (H[p][2i+1], H[p][2i])"""
    L = loc.shape[1]
    tt = np.arange(11, L)
    y = np.zeros((4, loc.shape[0], tt.size), dtype=np.int64)
    for i in range(6):
        lo, hi = loc[:, tt - 2 * i - 1], loc[:, tt - 2 * i]
        for p in range(4):
            y[p] += lo * TP_H[p, 2 * i + 1] + hi * TP_H[p, 2 * i]
            assert np.abs(y[p]).max() < 2 ** 31                   # every partial sum fits the accumulator
    return np.abs(y).max(axis=0)


def _emulate_run(det, x, slot, T, drive, a, H, rho, ch, tile, halo, slots):
    """one stream of one run of detector det (0 sample, 1 true peak) with a release of 2^rho frames (rho 0: none) and
    `slots` elements per thread: x int16 [F][C], slot int64 [halo * C] (the history slot the run reads)
    -> out int64 [F * C + 8] (UNWRITTEN where nothing was stored), the slot the run writes, min s or None"""
    A, D, W, hist = geometry_tp(a, H) if det else TG.geometry(a, H)
    hist, q = hist + (1 << rho) - 1, UNITY >> rho
    F = x.shape[0]
    ns, hsamp = F * ch, halo * ch
    hv, nfull, ntail = hsamp // 8, ns // 8, ns % 8
    assert hsamp % 8 == 0 and tile >= halo >= hist >= D and (D + 1) % 8 == 0 and rho >= 0
    # the stream as a tile sees it: the slot's vectors below 0, the run's from 0 on, zeros past the count
    seq = np.concatenate([slot, x.astype(np.int64).reshape(-1), np.zeros(16 + 8 * (tile // 8 + 1) * ch, dtype=np.int64)])

    def vec(vv):                                                  # [...] vector indices -> [...][8] samples
        vv = np.asarray(vv)
        assert (vv >= -hv).all()
        return seq[(hsamp + vv * 8)[..., None] + np.arange(8)]

    def sample(qq):
        qq = np.asarray(qq)
        assert (qq >= -hsamp).all() and (qq < ns).all()
        return seq[hsamp + qq]

    out = np.full(ns + 8, UNWRITTEN, dtype=np.int64)
    new_slot = sample(ns - hsamp + np.arange(hsamp))              # 4. (the last tile, or tile 0 of a stream with 0 frames)
    if F == 0:
        assert np.array_equal(new_slot, slot)
        return out, new_slot, None
    gmin = UNITY
    N = halo + tile
    tid, i = np.meshgrid(np.arange(BLOCK), np.arange(slots), indexing="ij")
    own = (tid + BLOCK * i).reshape(-1)                           # thread t keeps elements t + 256 i, i < slots
    own = own[own < N]
    assert N <= BLOCK * slots and np.array_equal(np.sort(own), np.arange(N))  # every element has exactly one thread
    for f0 in range(0, F, tile):
        nt = min(tile, F - f0)
        L = np.full(N, UNWRITTEN, dtype=np.int64)
        vbase = f0 * ch // 8 - hv
        assert f0 == 0 or vbase >= 0                              # only the run's first tile reads the slot: halo <= tile
        # ---- 1. g of frames f0 - halo .. f0 + tile - 1
        if ch <= 2 and not det:
            fpv = 8 // ch
            NV = N // fpv
            assert N % fpv == 0 and NV <= BLOCK * ((slots * ch + 7) // 8)
            v = np.abs(vec(vbase + np.arange(NV)))
            peak = v if ch == 1 else np.maximum(v[:, 0::2], v[:, 1::2])
            L[:] = _gain_sample(peak, drive, T).reshape(-1)
        elif ch <= 2:
            fpv = 8 // ch
            HV = 16 // fpv                                        # vectors in front of a thread's own: 16 frames
            NV = N // fpv
            cnt = -(-NV // BLOCK)                                 # own vectors per thread, consecutive
            assert N % fpv == 0 and cnt <= (slots * ch + 7) // 8
            w = (np.arange(BLOCK) * cnt)[:, None] + np.arange(-HV, cnt)[None, :]         # [thread][local vector]
            vv = vbase + w
            loaded = (w < NV) & (vv >= -hv)                       # the rest are zeros: in front of the slot, past the range
            assert f0 == 0 or (vv >= -hv).all()                   # ... and past the first tile nothing lies in front of it
            d = np.where(loaded[..., None], vec(np.where(loaded, vv, 0)), 0)             # [thread][local vector][8]
            loc = d.reshape(BLOCK, (HV + cnt) * fpv, ch)          # [thread][local frame][channel]
            t = 16 + np.arange(cnt * fpv)                         # the own frames' local indices
            pk = np.zeros((BLOCK, cnt * fpv), dtype=np.int64)
            for c in range(ch):
                fir = _pair_dot(loc[:, :, c])                     # of local frames 11 ..
                pk = np.maximum(pk, np.maximum(np.abs(loc[:, t - 8, c]) << 13, fir[:, t - 2 - 11]))
            j = (w[:, HV:, None] * fpv + np.arange(fpv)).reshape(BLOCK, -1)              # the elements they are
            keep = np.repeat(w[:, HV:] < NV, fpv, axis=1)
            assert np.array_equal(np.sort(j[keep]), np.arange(N))                        # each written once
            L[j[keep]] = _gain(pk[keep], drive, T)
        elif not det:
            p = f0 - halo + np.arange(N)
            peak = np.zeros(N, dtype=np.int64)
            inside = p < F
            peak[inside] = np.abs(sample(p[inside, None] * ch + np.arange(ch))).max(axis=1)
            L[:] = _gain_sample(peak, drive, T)
        else:
            n = f0 - halo + np.arange(N)
            p = n[:, None] - FRONT + np.arange(FRONT)             # frames n - 13 .. n - 1
            inside = (p >= -halo) & (p < F)
            xs = np.where(inside[..., None], sample(np.where(inside, p, 0)[..., None] * ch + np.arange(ch)), 0)
            pk = np.abs(xs[:, FRONT - 8]).max(axis=1) << 13
            for ph in range(4):
                y = sum(TP_H[ph, k] * xs[:, FRONT - 2 - k] for k in range(12))
                pk = np.maximum(pk, np.abs(y).max(axis=1))
            L[:] = _gain(pk, drive, T)
        assert (L != UNWRITTEN).all()
        # ---- 2. the passes: partner from LDS (32768, or 0 for a sum, in front of element 0), own element back
        j = np.arange(N)

        def one_pass(L, dist, kind, add, shift, vreg):
            o = np.where(j >= dist, L[np.maximum(j - dist, 0)], 0 if kind == 2 else UNITY)
            vreg = np.minimum(vreg, o) if kind == 0 else np.minimum(vreg, o + add) if kind == 1 else vreg + o
            assert vreg.max() < 2 ** 32 and (o + add).max() < 2 ** 32
            return vreg >> shift, vreg

        vreg = L.copy()
        P = 1
        while 2 * P <= W:
            L, vreg = one_pass(L, P, 0, 0, 0, vreg)
            P *= 2
        if W > P:
            L, vreg = one_pass(L, W - P, 0, 0, 0, vreg)
        for e in range(rho):
            L, vreg = one_pass(L, 1 << e, 1, q << e, 0, vreg)
        dd = 1
        while dd < A:
            L, vreg = one_pass(L, dd, 2, 0, a if 2 * dd == A else 0, vreg)
            dd *= 2
        Ls = L[halo:]
        gmin = min(gmin, int(Ls[:nt].min()))
        # ---- 3. the tile's output vectors: the delayed samples of vector v lie in vectors v - back and v - back + 1
        vb, nv = f0 * ch // 8, (nt * ch + 7) // 8
        v8 = vb + np.arange(nv)
        if ch <= 2:
            back = (D + 1) * ch // 8                              # A C / 8, or (A + 8) C / 8 for the true-peak detector
            assert (D + 1) * ch % 8 == 0 and (v8 - back >= -hv).all()
            x0, x1 = vec(v8 - back), vec(v8 - back + 1)
            xs = np.concatenate([x0[:, ch:], x1[:, :ch]], axis=1)                 # mono: samples 1..8, stereo: 2..9
            sf = Ls[(np.arange(nv) * (8 // ch))[:, None] + np.arange(8) // ch]
            y = (xs * (drive * sf) + (1 << 26)) >> 27
        else:
            qq = v8[:, None] * 8 + np.arange(8)
            ok = qq < ns
            qq = np.where(ok, qq, 0)
            y = np.where(ok, (sample(qq - D * ch) * (drive * Ls[np.where(ok, qq // ch - f0, 0)]) + (1 << 26)) >> 27, 0)
        for k in range(nv):
            if v8[k] < nfull:
                out[v8[k] * 8:v8[k] * 8 + 8] = y[k]
            elif v8[k] == nfull:
                out[v8[k] * 8:v8[k] * 8 + ntail] = y[k, :ntail]
    return out, new_slot, gmin


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,H,T,drive", SETS)
def test_emulated_decomposition_equals_the_model(cm, a, H, T, drive, channels):
    p = cm.plan_limtp(14, channels, a, H, 1)
    t, halo = p.tile_frames, p.halo
    assert t == TILE
    xs, counts, ragged, full, stats, gmin = dense_case(a, H, T, drive, channels)
    for s in range(len(counts)):
        slot = np.zeros(halo * channels, dtype=np.int64)
        got_min = UNITY
        for x, want in ((xs[s][:counts[s]], ragged[s]), (xs[s], full[s])):
            out, slot, m = _emulate_run(1, x, slot, T, drive, a, H, 0, channels, t, halo, 26)
            w = want.astype(np.int64).reshape(-1)
            assert np.array_equal(out[:w.size], w), (channels, s)
            assert (out[w.size:] == UNWRITTEN).all(), (channels, s)               # nothing past the stream's count
            got_min = min(got_min, UNITY if m is None else m)
        assert got_min == gmin[s]


# ---------------------------------------------------------------------------
# The generated code

def test_kernel_assembly_house_rules():
    """make asm produces build/k_limtp.s: it holds the three kernels, the packed dot product of the FIR, the 64-bit
    multiply-adds and the reciprocal, no scalar load has a register AND an immediate offset (tests/test_abi.py tells
    why; every workgroup indexes the parameter words with its stream), every kernel keeps its registers out of scratch
    memory, and the sources have no build switches."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_limtp.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_mad_i64_i32", text, flags=re.M)
    assert re.search(r"^\s*v_dot2", text, flags=re.M) and re.search(r"^\s*v_mad_u64_u32", text, flags=re.M)
    assert re.search(r"^\s*v_rcp_(iflag_)?f32", text, flags=re.M) and re.search(r"^\s*s_load_dword", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_limtp.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    names = sorted(scratch)
    assert any("k_limtp_fastILi1E" in k for k in names) and any("k_limtp_fastILi2E" in k for k in names), names
    assert any("k_limtp_any" in k for k in names) and len(names) == 3, names
    assert all(v == 0 for v in scratch.values()), scratch
    for name in ("k_limtp.hip", "k_lim.h", "k_lim_tile.h"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        assert "getenv" not in src
        for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
            assert not re.findall(r"\bCMHIP_(?!K_LIM(?:_TILE)?_H\b)\w+", m.group(1)), m.group(0)
