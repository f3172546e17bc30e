"""CPU: the host side of the dynamics stage's RMS detector (cmhip_dyn_new_detector, cmhip_dyn_detector,
cmhip_dyn_check_detector): the header, the refusals, the root and the plan through the library and as a stand-alone C++
program (csrc/dyn_plan.h: the root for every mean square, the two 32-bit sums against a 64-bit one, the plan), plainly
and under AddressSanitizer + UBSan; the RMS model's own properties and what the header says about constant magnitudes
and sines; and tests/test_dyn_host.py's emulation of the kernels' decomposition (csrc/k_dyn.h with DET =
DYN_DETECT_RMS: the squares split at bit 15, each half through the a unguarded add passes, the halves recombined, the
root from a single-precision seed and its integer repair) at the plan's own tile against the RMS model of
tests/test_gpu_dyn_rms.py.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
RMS_SRC = os.path.join(ROOT, "tests", "cpp", "dyn_rms_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location("dynrmshost_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TR = _load("test_gpu_dyn_rms")     # the RMS model and the cases of the GPU tests
TK, TG = TR.TK, TR.TG              # the keyed and the unkeyed model of the mean detector
TD = _load("test_dyn_host")        # the emulation of the kernels' decomposition
UNITY = 32768
MEAN, RMS = 0, 1


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_dyn_desc_t d; cmhip_dyn_t *m;\n"
           "d.device = 0; d.streams = d.channels = 1; d.detector_log2 = 10; d.smooth_log2 = 6; d.hold = 0; d.max_frames = 1;\n"
           "d.hip_stream = 0; m = cmhip_dyn_new_detector(&d, CMHIP_DYN_DETECT_RMS);\n"
           "return (int)cmhip_dyn_detector(m) + cmhip_dyn_check_detector(CMHIP_DYN_DETECT_MEAN, 10, 6, 0)"
           " + (CMHIP_DYN_DETECT_MEAN != 0u) + (CMHIP_DYN_DETECT_RMS != 1u) + (cmhip_dyn_free(m), 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check_detector_and_the_constructors_refusals(cm):
    lib = cm.lib
    assert (cm.DYN_DETECT_MEAN, cm.DYN_DETECT_RMS) == (MEAN, RMS)
    for det in (MEAN, RMS):
        for a, b, H in ((3, 3, 0), (10, 9, 1536), (6, 3, 2040)):
            assert cm.dyn_check_detector(det, a, b, H) == 0 == cm.dyn_check(a, b, H)
        for a, b, H in ((2, 6, 0), (11, 6, 0), (6, 2, 0), (6, 10, 0), (6, 9, 1537), (6, 6, 0xffffffff)):
            assert cm.dyn_check_detector(det, a, b, H) == cm.ERROR_INVAL == cm.dyn_check(a, b, H)
    for det in (2, 0xffffffff):
        assert cm.dyn_check_detector(det, 6, 6, 0) == cm.ERROR_INVAL and b"detector" in lib.cmhip_last_error()
        d = cm.DynDesc(0, 1, 2, 6, 6, 0, 1024, None)             # refused before any device is touched
        assert lib.cmhip_dyn_new_detector(C.byref(d), det) is None
        msg = lib.cmhip_last_error()
        assert msg.startswith(b"dyn_new: ") and b"detector" in msg, msg
        with pytest.raises(cm.CoolmicError):
            cm.Dynamics(1, 2, 6, 6, 0, 1024, detector=det)
    assert lib.cmhip_dyn_new_detector(None, RMS) is None and lib.cmhip_dyn_detector(None) == 0
    # a bad geometry is refused for both detectors, with cmhip_dyn_new's message
    for det in (MEAN, RMS):
        d = cm.DynDesc(0, 1, 2, 11, 6, 0, 1024, None)
        assert lib.cmhip_dyn_new_detector(C.byref(d), det) is None and b"dyn_new" in lib.cmhip_last_error()


def test_root_and_plan_through_the_library(cm):
    r = np.array(TR.ROOT_EDGES + [0, 5, 65535], dtype=np.int64)
    for v in np.concatenate([r * r, r * r - 1, r * r + 1, r * r + 2 * r, [0, 2 ** 32 - 1, 2 ** 30, 2 ** 30 - 1]]):
        v = int(max(v, 0))
        assert cm.dyn_isqrt(v) == int(TR.isqrt(np.array([v]))[0]), v
    for a, b, H in TG.SETS:
        for ch in (1, 2, 3, 16):
            p, m = cm.plan_dynrms(5, ch, a, b, H, 9000), cm.plan_dyn(5, ch, a, b, H, 9000)
            assert (p.err, p.grid, p.chunks, p.block, p.fast) == (0, m.grid, m.chunks, 256, m.fast)
            assert (p.tile_frames, p.halo, p.lds_bytes) == (m.tile_frames, m.halo, m.lds_bytes) and p.lds_bytes <= 30720
            assert p.passes == m.passes + a
    assert cm.plan_dynrms(1 << 20, 2, 6, 6, 0, 1 << 23).err != 0 and cm.plan_dynrms(4, 2, 11, 6, 0, 100).grid == 0


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        RMS_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_root_sums_and_plan_as_a_program(tmp_path):
    exe, r = _build(tmp_path, "dyn_rms_test", [])                # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    m = re.search(r"rms ok: (\d+) roots, 320 sums, 10752 plans", out.stdout)
    assert out.returncode == 0 and m and int(m.group(1)) > 2 ** 30, out.stdout + out.stderr      # every mean square


def test_root_sums_and_plan_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "dyn_rms_san", ["-DDYN_RMS_THIN", "-fsanitize=address,undefined",
                                              "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "rms ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The RMS model's own properties

def levels(x, a):
    """mono int64 [n] -> L of frames A - 1 .. n - 1 under the mean detector and under RMS"""
    e = np.abs(np.asarray(x, dtype=np.int64))
    return TG._sums(e, 1 << a) >> a, TR.isqrt(TG._sums(e * e, 1 << a) >> a)


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_model_properties(a, b, H):
    A, B, D, W, hist = TG.geometry(a, b, H)
    t = 4096
    zero = np.zeros((hist, 2), dtype=np.int16)
    x = TG.signal(42 + a, 3 * t, 2)
    x[5000] = -32768
    # the curve of creation is a pure delay, bit for bit
    y, s = TR.model_rms(x, zero, TG.flat(UNITY), a, b, H)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], x[:-D]) and y[5000 + D, 0] == -32768
    # never louder than the input, sample by sample
    T = TG.design(**TG.DENSE_CURVE)
    y, s = TR.model_rms(x, zero, T, a, b, H)
    xd = np.concatenate([np.zeros((D, 2), dtype=np.int16), x[:-D]]).astype(np.int64)
    assert (np.abs(y.astype(np.int64)) <= np.abs(xd)).all() and s.min() < 1000 and (np.diff(s) != 0).mean() >= 0.25
    assert (y != TG.model_dyn(x, zero, T, a, b, H)[0]).any(axis=1).mean() >= 0.25         # and not the mean detector's
    # cut-invariance: one run equals the same stream in runs of 1, 7, HIST - 1, HIST, HIST + 1, 0, tile + 5 and the rest
    h, pos, parts = zero, 0, []
    for n in (1, 7, hist - 1, hist, hist + 1, 0, t + 5, x.shape[0]):
        part = x[pos:pos + n]
        parts.append(TR.model_rms(part, h, T, a, b, H)[0])
        h = TG.next_hist(h, part)
        pos += part.shape[0]
    assert pos == x.shape[0] and np.array_equal(np.concatenate(parts), y)
    # a stream that is its own key is the unkeyed model; the KeyModel class agrees with the functions
    model = TK.KeyModel(2, 2, a, b, H, detector=RMS)
    model.set(-1, T)
    model.set_key(1, 0)
    k = TG.signal(91 + a, 3 * t, 2)
    ys = model.run([x, k])
    assert np.array_equal(ys[0], y) and np.array_equal(ys[1], TK.model_dyn_keyed(k, zero, x, zero, T, a, b, H, RMS)[0])


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_constant_magnitude_reads_the_same_under_both_detectors(a, b, H):
    """the mean of A equal squares is the square: from frame HIST on the two models agree bit for bit, on every curve"""
    A, B, D, W, hist = TG.geometry(a, b, H)
    zero = np.zeros((hist, 2), dtype=np.int16)
    n = hist + 600
    sign = np.where(np.arange(n) % 3 == 0, -1, 1)
    for r in (1, 7, 181, 182, 300, 23170, 32767):
        x = np.stack([r * sign, -(r // 2) * sign], axis=1).astype(np.int16)      # the loudest channel has magnitude r
        mean, rms = levels(x[:, 0], a)
        assert (mean == r).all() and (rms == r).all()
        for T in (TG.design(**TG.DENSE_CURVE), TG.steps().astype(np.int64)):
            y0, s0 = TG.model_dyn(x, zero, T, a, b, H)
            y1, s1 = TR.model_rms(x, zero, T, a, b, H)
            assert np.array_equal(y0[hist:], y1[hist:]) and np.array_equal(s0[hist:], s1[hist:]), r
    x = np.full((n, 2), -32768, dtype=np.int16)
    mean, rms = levels(x[:, 0], a)
    assert (mean == 32768).all() and (rms == 32768).all()


def test_what_a_sine_reads():
    """a = 10, 997 Hz at 48 kHz.  RMS reads amplitude / sqrt 2 to within the ripple of a window that holds 21.27 periods
    (1 / (2 pi 21.27) = 0.75 % of the mean square, half of it of the level); the mean reads amplitude * 2 / pi, 0.91 dB
    lower, with the ripple of a rectified sine"""
    n = np.arange(48000)
    amp = 20000
    x = np.floor(amp * np.sin(2 * np.pi * 997 * n / 48000) + 0.5).astype(np.int64)
    mean, rms = levels(x, 10)
    print("sine of amplitude %d: RMS reads %d..%d, the mean %d..%d" % (amp, rms.min(), rms.max(), mean.min(), mean.max()))
    assert 14089 <= rms.min() <= rms.max() <= 14194 and abs(amp / np.sqrt(2) - 14142) < 1
    assert 12671 <= mean.min() <= mean.max() <= 12795 and abs(amp * 2 / np.pi - 12732) < 1
    db = 20 * np.log10(rms.astype(np.float64).mean() / mean.astype(np.float64).mean())
    assert 0.88 <= db <= 0.94                                    # 20 log10(pi / (2 sqrt 2)) = 0.912 dB
    # a whole number of periods in the window, full scale: no ripple; the header's 23170 and about 20861 (64 samples per
    # period make the mean of |sin| cot(pi / 64) / 32 = 0.63611 in place of 2 / pi = 0.63662)
    x = np.floor(32767 * np.sin(2 * np.pi * n / 64) + 0.5).astype(np.int64)
    mean, rms = levels(x, 10)
    assert rms.min() == rms.max() == 23169 and mean.min() == mean.max() == int(32767 / np.tan(np.pi / 64) / 32)
    assert int(np.floor(32768 / np.sqrt(2))) == 23170 and int(np.floor(32768 * 2 / np.pi)) == 20860


def test_the_root_separates_a_single_precision_sqrt():
    """the model's own root against Python's integers, and the inputs on which a truncated float32 sqrt is wrong: they
    exist below 2^30 (which is why dyn_isqrt repairs its seed), and the GPU test's signal at a = 10 reaches some"""
    import math
    v = np.concatenate([np.arange(0, 70000), np.arange(2 ** 30 - 70000, 2 ** 30 + 1),
                        np.random.default_rng(3).integers(0, 2 ** 30, size=20000)])
    assert TR.isqrt(v).tolist() == [math.isqrt(int(q)) for q in v]
    r = np.arange(4097, 32769, dtype=np.int64)
    assert (TR.root_float32(r * r - 1) != r - 1).any()           # r * r - 1 rounds to r * r in 24 bits once r > 4096
    x, n, T, want, wrong, f32 = TR.root_edge_case(10, 3, 0)
    assert x.shape[0] == 98304 and wrong["plus one"] >= 0.5 and wrong["minus one"] >= 0.5 and f32 > 0
    for s in ((3, 3, 0), (6, 6, 0)):
        wrong = TR.root_edge_case(*s)[4]
        assert wrong["plus one"] >= 0.5 and wrong["minus one"] >= 0.5, (s, wrong)


# ---------------------------------------------------------------------------
# The RMS decomposition (csrc/k_dyn.h, DET = DYN_DETECT_RMS): tests/test_dyn_host.py's emulation with det = RMS, plain
# (every stream its own key) and keyed.

@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_rms_decomposition_equals_the_model(cm, a, b, H, channels):
    p = cm.plan_dynrms(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    W = (1 << b) + H
    assert p.passes == 2 * a + int(np.log2(W)) + (1 if W & (W - 1) else 0) + b and p.lds_bytes == (t + halo) * 4
    xs, counts, T, ragged, full, unity, change, smallest, gmin, differ = TR.dense_rms_case(a, b, H, channels, t)
    TR.assert_dense_rms(a, b, H, unity, change, smallest, differ)
    TD._hold_emulation_to(list(range(len(counts))), xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo, RMS)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_keyed_rms_decomposition_equals_the_model(cm, a, b, H, channels):
    p = cm.plan_dynrms(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    xs, counts, keys, T, ragged, full, gmin, own, mean, change, smallest = TR.dense_rms_key_case(a, b, H, channels, t)
    TR.assert_dense_rms_key(own, mean, change, smallest)
    TD._hold_emulation_to(keys, xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo, RMS)


def test_emulated_root_on_the_edges():
    """the emulated dyn_isqrt on the root-edge signal's mean squares, and on the values a float32 seed gets wrong"""
    r = np.arange(0, 32769, dtype=np.int64)
    for v in (r * r, np.maximum(r * r - 1, 0), r * r + 2 * r, r * r + 1):
        v = np.minimum(v, 2 ** 32 - 1)
        assert np.array_equal(TD._dyn_isqrt(v), TR.isqrt(v))
    r = np.arange(32769, 65536, dtype=np.int64)
    for v in (r * r, r * r - 1, r * r + 2 * r):
        assert np.array_equal(TD._dyn_isqrt(v), TR.isqrt(v))
    assert TD._dyn_isqrt(np.array([2 ** 32 - 1]))[0] == 65535


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_dense_conditions_hold_on_the_model(a, b, H):
    """mono, stereo and six channels of the GPU test's dense cases, plain and keyed: the gain moves, the gate closes, and
    neither the detector nor the key can be ignored"""
    for channels in (1, 2, 6):
        case = TR.dense_rms_case(a, b, H, channels, 4096)
        TR.assert_dense_rms(a, b, H, *case[5:8], case[9])
        TR.assert_dense_rms_key(*TR.dense_rms_key_case(a, b, H, channels, 4096)[-4:])
