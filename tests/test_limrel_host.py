"""CPU: the limiter's release stage (cmhip_lim_new_release, csrc/k_limrel.hip) on the host side.  The header as C and
C++, cmhip_lim_check_release at its edges, the plan (csrc/lim_plan.h: lim_geom_rel / plan_limrel beside the unchanged
plans) through the library and as a stand-alone C++ program, plainly and under AddressSanitizer + UBSan; a numpy int64
MODEL of the arithmetic include/coolmic_hip.h states for both detectors (tests/test_gpu_limrel.py compares the device
against it bit for bit) and the model's own properties: rho = 0 is the limiter without the stage, the doubling form of
the release equals its definition, the slope, s never above the limiter's without the stage, the ceiling, the pure
delay, cut-invariance; the conditions on the dense inputs of the GPU tests, on the model alone; an emulation of the
kernels' decomposition (32 element slots per thread, every pass with its partner value, the seam and the history write
with a halo of up to the whole tile) at the plan's own tile against the model; and the generated assembly.  Nothing here
needs a GPU."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "limrel_plan_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_limrel", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MH = _load("test_limtp_host")      # the true-peak detector's model and filter
TG = MH.TG                         # tests/test_gpu_lim.py: the sample detector's model, the signal, the rig
UNITY = 32768
SWV = np.lib.stride_tricks.sliding_window_view
SAMPLE, TRUE_PEAK = 0, 1
TILE = 4096                        # the tile of a limiter with a release; every test holds the plan against it


# ---------------------------------------------------------------------------
# The model

def geometry_rel(det, a, H, rho):
    """-> A, D, W, HIST, R, q"""
    A, D, W, hist = MH.geometry_tp(a, H) if det else TG.geometry(a, H)
    R = 1 << rho
    return A, D, W, hist + R - 1, R, UNITY >> rho


def gains(det, z, T, drive):
    """z int64 [n][C] -> g of frames 0 .. n - 1 (sample detector) or 13 .. n - 1 (true-peak detector)"""
    if det:
        pr = (drive * MH.detector_tp(z) + (1 << 25) - 1) >> 25
    else:
        pr = (np.abs(z).max(axis=1) * drive + 4095) >> 12
    return np.where(pr <= T, UNITY, (T * 32768) // np.maximum(pr, 1))


def release_direct(m, rho):
    """the definition: r[n] = min over 0 <= k < R of (m[n-k] + k*q), for n = R - 1 .. (len(m) - R + 1 entries)"""
    R, q = 1 << rho, UNITY >> rho
    n = m.size - R + 1
    r = m[R - 1:].copy()
    for k in range(1, R):
        np.minimum(r, m[R - 1 - k:R - 1 - k + n] + k * q, out=r)
    return r


def release_doubling(m, rho):
    """the same by doubling, a partner in front of the array counting as 32768: v[j] = min(v[j], v[j - 2^k] + (q << k))"""
    R, q = 1 << rho, UNITY >> rho
    v = m.copy()
    for k in range(rho):
        d = 1 << k
        v = np.minimum(v, np.concatenate([np.full(d, UNITY), v[:-d]]) + (q << k))
    return v[R - 1:]


def model_limrel(det, x, hist, T, drive, a, H, rho):
    """x int16 [F][C]; hist int16 [HIST][C], oldest first -> y int16 [F][C], s int64 [F]"""
    A, D, W, HIST, R, q = geometry_rel(det, a, H, rho)
    F = x.shape[0]
    assert hist.shape[0] == HIST <= 4096 and 0 <= rho <= 11
    if F == 0: return x.copy(), np.zeros(0, np.int64)
    z = np.concatenate([hist, x]).astype(np.int64)
    g = gains(det, z, T, drive)
    m = SWV(g, W).min(axis=1)
    r = release_doubling(m, rho)                                  # (test_release_forms holds it against the definition)
    s = SWV(r, A).sum(axis=1) >> a
    assert s.size == F
    y = (z[HIST - D: HIST - D + F] * (drive * s)[:, None] + (1 << 26)) >> 27
    assert np.abs(y).max(initial=0) <= T
    return y.astype(np.int16), s


class ModelRel(TG.Model):
    """the streams of a limiter with a release stage as the header states them"""

    def __init__(self, det, streams, channels, a, H, rho):
        super().__init__(streams, channels, a, H)
        self.det, self.rho = det, rho
        self.A, self.D, self.W, self.HIST = geometry_rel(det, a, H, rho)[:4]
        self.hist = [np.zeros((self.HIST, channels), dtype=np.int16) for _ in range(streams)]

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.hist[s] = np.zeros((self.HIST, self.C), dtype=np.int16)
            self.gmin[s] = UNITY

    def run(self, xs):
        ys = []
        for s, x in enumerate(xs):
            x = np.asarray(x, dtype=np.int16).reshape(-1, self.C)
            y, sg = model_limrel(self.det, x, self.hist[s], self.par[s][0], self.par[s][1], self.a, self.H, self.rho)
            self.hist[s] = TG.next_hist(self.hist[s], x)
            if sg.size:
                self.gmin[s] = min(self.gmin[s], int(sg.min()))
                self.s[s].append(sg)
            ys.append(y)
        return ys


def zero_hist(det, a, H, rho, channels):
    return np.zeros((geometry_rel(det, a, H, rho)[3], channels), dtype=np.int16)


# ---------------------------------------------------------------------------
# The dense cases of the GPU tests: (a, H, rho, T, drive); the last one has HIST = 4096 = the tile.  The true-peak
# detector takes the same sets with the hold raised to at least 1, the last one with hold 1014 (HIST = 4096 again).

SETS = [(3, 0, 5, 20000, 4096), (6, 0, 6, 29204, 8192), (6, 100, 9, 12000, 4096), (8, 37, 11, 29204, 16384),
        (9, 1027, 11, 8000, 4096)]
SETS_TP = [(3, 1, 5, 20000, 4096), (6, 1, 6, 29204, 8192), (6, 100, 9, 12000, 4096), (8, 37, 11, 29204, 16384),
           (9, 1014, 11, 8000, 4096)]
CHANNELS = [1, 2, 3, 6, 16]
DIFFER_SHARE = 0.02                # per set and channel count: frames whose s is not the s of the rho = 0 model
UNITY_SHARE = 0.10                 # over the five sets together: frames at unity
CHANGE_SHARE = 0.15                # ... and adjacent frames whose s differs


def sets_of(det):
    return SETS_TP if det else SETS


def dense_counts(t, hist):
    return [2 * t + 13, t, t - 1, hist + 1, hist, hist - 1, 1, 0]


# The seeds are such that the MODEL alone meets the dense conditions, checked without a device (test_dense_conditions):
# these plain ones do for every set, detector and channel count (per set 2.1 .. 81 % of the frames differ from the
# rho = 0 model's, the tightest being the shortest release on 16 channels; over the sets 25 .. 31 % are at unity and
# 47 .. 56 % of adjacent frames change), so none had to be searched.
def dense_seed(det, a, H, rho, channels, stream):
    return 1000000 * det + 100000 * a + 10 * H + 7 * rho + 1000 * channels + stream + 1


@functools.lru_cache(maxsize=None)
def dense_case(det, a, H, rho, T, drive, channels, t=TILE):
    """the streams' full-length inputs, and over the ragged run followed by the uniform run on one limiter: the model's
    outputs of both, the meters, and the counts of the dense conditions -- computed once, never changed"""
    hist = geometry_rel(det, a, H, rho)[3]
    counts = dense_counts(t, hist)
    xs = [TG.bursts(dense_seed(det, a, H, rho, channels, s), counts[0], channels) for s in range(len(counts))]
    model = ModelRel(det, len(counts), channels, a, H, rho)
    model.set(-1, T, drive)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    stats = {"frames": 0, "pairs": 0, "differ": 0, "unity": 0, "change": 0}
    for s, n in enumerate(counts):
        if not model.s[s]:
            continue
        sg = np.concatenate(model.s[s])                           # the stream as one sequence of both runs
        both = np.concatenate([xs[s][:n], xs[s]])
        s0 = model_limrel(det, both, zero_hist(det, a, H, 0, channels), T, drive, a, H, 0)[1]
        stats["frames"] += int(sg.size)
        stats["pairs"] += int(sg.size - 1)
        stats["differ"] += int((sg != s0).sum())
        stats["unity"] += int((sg == UNITY).sum())
        stats["change"] += int((np.diff(sg) != 0).sum())
        assert (sg <= s0).all()
    stats["peak"] = max(int(np.abs(y.astype(np.int64)).max(initial=0)) for y in ragged + full)
    return xs, counts, ragged, full, stats, list(model.gmin)


def dense_shares(det, channels):
    """-> per set the share of differing frames; over the five sets the shares at unity and of changing gain"""
    st = [dense_case(det, *p, channels)[4] for p in sets_of(det)]
    return ([s["differ"] / s["frames"] for s in st], sum(s["unity"] for s in st) / sum(s["frames"] for s in st),
            sum(s["change"] for s in st) / sum(s["pairs"] for s in st))


def dense_conditions(det, channels, params):
    """the conditions on the dense input, on the model alone, so that a kernel that skips the release (or never
    reduces, or never moves) cannot pass the device test.  The peak: the sample detector's ceiling is reached, never
    passed; the true-peak detector's gain answers to the peaks between the samples, so its samples stay below T by
    whatever the interpolation adds and only the bound is asserted."""
    differ, unity, change = dense_shares(det, channels)
    st = dense_case(det, *params, channels)[4]
    T = params[3]
    assert st["differ"] >= DIFFER_SHARE * st["frames"] and min(differ) >= DIFFER_SHARE, differ
    assert unity >= UNITY_SHARE and change >= CHANGE_SHARE, (unity, change)
    assert st["peak"] <= T and (det == TRUE_PEAK or st["peak"] == T), (st["peak"], T)
    return st["differ"] / st["frames"], unity, change


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_dense_conditions(det, channels):
    for p in sets_of(det):
        differ, unity, change = dense_conditions(det, channels, p)
        print("limrel dense det %d a %d H %4d rho %2d C %2d: differ %.1f %%; over the sets unity %.1f %%, changing %.1f %%"
              % (det, p[0], p[1], p[2], channels, 100 * differ, 100 * unity, 100 * change))


# ---------------------------------------------------------------------------
# Header, checks

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_lim_desc_t d; (void)sizeof(d);\n"
           "d.device = 0; d.streams = d.channels = 1; d.lookahead_log2 = 6; d.hold = 1; d.max_frames = 1; d.hip_stream = 0;\n"
           "return cmhip_lim_check_release(CMHIP_LIM_DETECT_TRUE_PEAK, 6, 1, 11, 32767, 4096)"
           " + (cmhip_lim_new_release(0, CMHIP_LIM_DETECT_SAMPLE, 11) != 0) + (int)cmhip_lim_release(0)"
           " + (int)cmhip_lim_detector(0) + (int)cmhip_lim_delay(0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check_release(cm):
    ok, bad = cm.lim_check_release, cm.ERROR_INVAL
    for det, H in ((0, 0), (0, 1), (1, 1)):
        assert ok(det, 6, H, 0, 32767, 4096) == 0 and ok(det, 6, H, 11, 32767, 4096) == 0
        assert ok(det, 6, H, 12, 32767, 4096) == bad and b"release_log2" in cm.lib.cmhip_last_error()
        assert ok(det, 6, H, 0xffffffff, 32767, 4096) == bad
    # HIST = 4096 and 4097
    assert ok(0, 9, 1027, 11, 1, 1) == 0 and ok(0, 9, 1028, 11, 1, 1) == bad and b"4096" in cm.lib.cmhip_last_error()
    assert ok(1, 9, 1014, 11, 1, 1) == 0 and ok(1, 9, 1015, 11, 1, 1) == bad
    assert geometry_rel(0, 9, 1027, 11)[3] == 4096 == geometry_rel(1, 9, 1014, 11)[3]
    # hold 0 with the true-peak detector, the detector itself, the bounds without the stage
    assert ok(1, 6, 0, 5, 32767, 4096) == bad and b"hold" in cm.lib.cmhip_last_error()
    assert ok(2, 6, 1, 5, 32767, 4096) == bad and ok(0, 2, 0, 5, 1, 1) == bad and ok(0, 10, 0, 5, 1, 1) == bad
    assert ok(0, 6, 1985, 1, 1, 1) == bad and ok(0, 6, 1984, 1, 1, 1) == 0
    for det in (0, 1):
        for a in range(3, 10):
            for H in (0, 1, 2048 - (1 << a), 2049 - (1 << a)):
                for T, drive in ((0, 1), (1, 1), (32767, 65535), (32768, 1), (1, 65536), (1, 0)):
                    assert ok(det, a, H, 0, T, drive) == cm.lim_check_detector(det, a, H, T, drive)     # rho 0 is that
                    assert (ok(det, a, H, 3, T, drive) == 0) == (cm.lim_check_detector(det, a, H, T, drive) == 0)


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_lim_new_release(None, 0, 5) is None and lib.cmhip_lim_release(None) == 0
    # descriptors are refused before any device is touched
    for det, streams, channels, a, hold, rho, frames in ((0, 1, 2, 6, 0, 12, 1024), (0, 1, 2, 6, 0, 0xffffffff, 1024),
                                                         (0, 1, 2, 9, 1028, 11, 1024), (1, 1, 2, 9, 1015, 11, 1024),
                                                         (1, 1, 2, 6, 0, 5, 1024), (2, 1, 2, 6, 1, 5, 1024),
                                                         (0, 0, 2, 6, 0, 5, 1024), (0, 1, 17, 6, 0, 5, 1024),
                                                         (0, 1, 2, 2, 0, 5, 1024), (0, 1, 2, 6, 1985, 5, 1024),
                                                         (0, 1, 2, 6, 0, 5, 0), (0, 1, 2, 6, 0, 5, (1 << 30) + 1),
                                                         (0, 1 << 20, 16, 6, 0, 5, 1024), (1, 1, 2, 6, 0, 0, 1024)):
        d = cm.LimDesc(0, streams, channels, a, hold, frames, None)
        assert lib.cmhip_lim_new_release(C.byref(d), det, rho) is None, (det, streams, channels, a, hold, rho, frames)
        assert b"lim_new: " in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Limiter(streams, channels, a, hold, frames, detector=det, release_log2=rho)


# ---------------------------------------------------------------------------
# The launcher's plan

def _top_hold(det, a, rho):
    A, R = 1 << a, 1 << rho
    return min(2048 - A, 2549 - 2 * A if det else 1 << 30, 4096 - (2 * A - 2 + R - 1 + (13 if det else 0)))


def test_plan(cm):
    for det in (0, 1):
        for a in range(3, 10):
            for rho in range(0, 12):
                top = _top_hold(det, a, rho)
                assert top >= 1
                assert cm.plan_limrel(det, 4, 2, a, top + 1, rho, 100).grid == 0
                for H in (0, 1, top):
                    if det and H == 0:
                        assert cm.plan_limrel(det, 4, 2, a, H, rho, 100).grid == 0
                        continue
                    hist = geometry_rel(det, a, H, rho)[3]
                    halo = (hist + 7) // 8 * 8
                    for ch in range(1, 17):
                        p = cm.plan_limrel(det, 5, ch, a, H, rho, 1)      # a one-frame run: one workgroup per stream
                        assert (p.err, p.grid, p.chunks, p.block) == (0, 5, 1, 256), (det, a, H, rho, ch)
                        assert p.fast == (1 if ch <= 2 else 0)
                        t = p.tile_frames
                        assert t == TILE >= p.halo == halo >= hist
                        assert p.lds_bytes == (t + halo) * 4 <= 32768 and t + halo <= 256 * 32    # 32 slots per thread
                        for frames in (1, t - 1, t, t + 1, 100000):
                            q = cm.plan_limrel(det, 3, ch, a, H, rho, frames)
                            assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
                        # the plans without the stage are what they were, and rho = 0 is they
                        o = (cm.plan_limtp if det else cm.plan_lim)(5, ch, a, H, 1)
                        base = MH.geometry_tp(a, H)[3] if det else TG.geometry(a, H)[3]
                        assert (o.err, o.grid, o.tile_frames, o.halo) == (0, 5, t, (base + 7) // 8 * 8)
                        if rho == 0:
                            assert all(getattr(p, n) == getattr(o, n) for n, _ in cm.LimPlan._fields_)
    assert cm.plan_limrel(0, 1, 1, 9, 1027, 11, 1).halo == 4096 == cm.plan_limrel(1, 1, 1, 9, 1014, 11, 1).halo
    p = cm.plan_limrel(0, 1 << 20, 2, 6, 0, 5, 1 << 23)           # no grid of 2^31 workgroups
    assert p.err != 0 and p.grid == 0
    assert cm.plan_limrel(0, 0, 2, 6, 0, 5, 100).grid == 0 and cm.plan_limrel(0, 4, 2, 6, 0, 5, 0).grid == 0
    for det, ch, a, H, rho in ((0, 0, 6, 0, 5), (0, 17, 6, 0, 5), (0, 2, 2, 0, 5), (0, 2, 10, 0, 5), (0, 2, 6, 1985, 5),
                               (0, 2, 6, 0, 12), (2, 2, 6, 1, 5)):
        p = cm.plan_limrel(det, 4, ch, a, H, rho, 100)
        assert p.grid == 0 and p.err == 0


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_as_a_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "limrel_plan_test", [])              # g++ alone: the header includes no HIP
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
    exe, r = _build_plan_test(tmp_path, "limrel_plan_san", san)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "plans ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The model's own properties

@pytest.mark.parametrize("rho", range(0, 12))
def test_release_forms(rho):
    """the doubling form, with a partner in front of the array counting as 32768, equals the definition -- on random
    gains, on a single dip (the ramp itself) and at the extremes"""
    rng = np.random.default_rng(50 + rho)
    R, q = 1 << rho, UNITY >> rho
    dip = np.full(3 * R + 50, UNITY)
    dip[R + 20] = 0
    sparse = np.where(rng.random(6000 + 2 * R) < 0.003, rng.integers(0, 32769, 6000 + 2 * R), UNITY)
    for m in (rng.integers(0, 32769, 6000 + 2 * R), sparse, dip, np.zeros(2 * R + 5, dtype=np.int64), np.full(2 * R + 5, UNITY)):
        m = m.astype(np.int64)
        r = release_direct(m, rho)
        assert np.array_equal(release_doubling(m, rho), r)
        assert (r <= m[R - 1:]).all() and (np.diff(r) <= q).all() and r.min() >= 0
        if rho == 0:
            assert np.array_equal(r, m)
    r = release_direct(dip, rho)[20:]                             # from the dip on: 0, q, 2q, .. up to unity
    want = np.minimum(np.arange(r.size) * q, UNITY)
    assert np.array_equal(r[1:], want[:-1]) and r[0] == UNITY


@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_rho_zero_is_the_limiter_without_the_stage(det):
    for a, H, rho, T, drive in sets_of(det):
        x = TG.bursts(60 + a, 2 * TILE + 100, 2)
        zero = zero_hist(det, a, H, 0, 2)
        y, s = model_limrel(det, x, zero, T, drive, a, H, 0)
        want = (MH.model_limtp if det else TG.model_lim)(x, zero, T, drive, a, H)
        assert np.array_equal(y, want[0]) and np.array_equal(s, want[1])


@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
@pytest.mark.parametrize("i", range(5))
def test_model_properties(det, i):
    a, H, rho, T, drive = sets_of(det)[i]
    A, D, W, hist, R, q = geometry_rel(det, a, H, rho)
    zero = zero_hist(det, a, H, rho, 2)
    x = TG.bursts(42 + a, 3 * TILE, 2)
    y, s = model_limrel(det, x, zero, T, drive, a, H, rho)        # (asserts |y| <= T itself)
    assert np.abs(y.astype(np.int64)).max() <= T and s.min() < UNITY
    # the slope: S rises by at most A * q per frame, so s by at most q + 1
    assert np.diff(s).max() <= q + 1
    # never above the limiter without the stage
    s0 = model_limrel(det, x, zero_hist(det, a, H, 0, 2), T, drive, a, H, 0)[1]
    assert (s <= s0).all() and (s < s0).any()
    # cut-invariance: one run equals the same stream in runs of 1, 7, HIST - 1, HIST, HIST + 1, 0, 1000 and the rest
    h, pos, parts = zero, 0, []
    for n in (1, 7, 12, 13, 14, hist - 1, hist, hist + 1, 0, 1000, x.shape[0]):
        part = x[pos:pos + n]
        parts.append(model_limrel(det, part, h, T, drive, a, H, rho)[0])
        h = TG.next_hist(h, part)
        pos += part.shape[0]
    assert pos == x.shape[0] and np.array_equal(np.concatenate(parts), y)
    # below the threshold (the true peak's: the filter's gain is at most 16571 / 8192): a pure delay at unity drive
    amp = min(2000, T * 8192 // 16571 // 4)
    z = (x.astype(np.int64) * amp // 32768).astype(np.int16)      # |z| <= amp: below T also at drive 12345
    y, s = model_limrel(det, z, zero, T, 4096, a, H, rho)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], z[:-D])
    y, s = model_limrel(det, z, zero, T, 12345, a, H, rho)
    assert (s == UNITY).all() and np.array_equal(y[D:], ((z[:-D].astype(np.int64) * 12345 + 2048) >> 12))


# ---------------------------------------------------------------------------
# The decomposition of k_limrel_fast<C> / k_limrel_any / k_limtprel_fast<C> / k_limtprel_any (csrc/k_limrel.hip): the one
# emulation of the tile (tests/test_limtp_host.py) with these kernels' 32 slots per thread and their release.

SLOTS = 32
UNWRITTEN = MH.UNWRITTEN


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("det", [SAMPLE, TRUE_PEAK])
def test_emulated_decomposition_equals_the_model(cm, det, i, channels):
    a, H, rho, T, drive = sets_of(det)[i]
    p = cm.plan_limrel(det, 8, channels, a, H, rho, 1)
    t, halo = p.tile_frames, p.halo
    assert t == TILE and halo == (geometry_rel(det, a, H, rho)[3] + 7) // 8 * 8
    xs, counts, ragged, full, stats, gmin = dense_case(det, a, H, rho, T, drive, channels)
    for s in range(len(counts)):
        slot = np.zeros(halo * channels, dtype=np.int64)
        got_min = UNITY
        for x, want in ((xs[s][:counts[s]], ragged[s]), (xs[s], full[s])):
            assert rho >= 1
            out, slot, m = MH._emulate_run(det, x, slot, T, drive, a, H, rho, channels, t, halo, SLOTS)
            w = want.astype(np.int64).reshape(-1)
            assert np.array_equal(out[:w.size], w), (channels, s)
            assert (out[w.size:] == UNWRITTEN).all(), (channels, s)               # nothing past the stream's count
            got_min = min(got_min, UNITY if m is None else m)
        assert got_min == gmin[s]


# ---------------------------------------------------------------------------
# The generated code

def test_kernel_assembly_house_rules():
    """make asm produces build/k_limrel.s: it holds the six kernels, the packed dot product of the true-peak FIR, the
    64-bit multiply-adds and the reciprocal, no scalar load has a register AND an immediate offset (tests/test_abi.py
    tells why; every workgroup indexes the parameter words with its stream), every kernel keeps its registers out of
    scratch memory, and the source has no build switches."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_limrel.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_mad_i64_i32", text, flags=re.M)
    assert re.search(r"^\s*v_dot2", text, flags=re.M) and re.search(r"^\s*v_mad_u64_u32", text, flags=re.M)
    assert re.search(r"^\s*v_rcp_(iflag_)?f32", text, flags=re.M) and re.search(r"^\s*s_load_dword", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_limrel.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    names = sorted(scratch)
    for stem in ("k_limrel_fastILi1E", "k_limrel_fastILi2E", "k_limrel_any", "k_limtprel_fastILi1E", "k_limtprel_fastILi2E",
                 "k_limtprel_any"):
        assert any(stem in k for k in names), (stem, names)
    assert len(names) == 6 and all(v == 0 for v in scratch.values()), scratch
    for name in ("k_limrel.hip", "k_lim.h", "k_lim_tile.h"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        assert "getenv" not in src
        for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
            assert not re.findall(r"\bCMHIP_(?!K_LIM(?:_TILE)?_H\b)\w+", m.group(1)), m.group(0)
