"""CPU: the host side of the dynamics stage's side-chain keys (cmhip_dyn_set_key, cmhip_dyn_get_key,
cmhip_dyn_design_duck): the header, the duck designer against its formula in numpy, the NULL refusals, the keyed model's
own properties, and tests/test_dyn_host.py's emulation of the keyed decomposition (csrc/k_dyn.h with KEYED = true: step
1's vectors from the KEY's slots across the history seam, step 3's two-vector read and the history write from the
stream's own) at the plan's own tile against the keyed model of tests/test_gpu_dyn_key.py.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("dynkeyhost_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TK = _load("test_gpu_dyn_key")     # the keyed model and the dense cases of the GPU tests
TG = TK.TG                         # the unkeyed model (tests/test_gpu_dyn.py)
TD = _load("test_dyn_host")        # the emulation of the kernels' decomposition
UNITY = 32768


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_dyn_duck_desc_t d; uint16_t t[CMHIP_DYN_CURVE]; long k = 0;\n"
           "d.threshold_db = -30; d.depth_db = 12; d.knee_db = 6;\n"
           "return cmhip_dyn_design_duck(&d, t) + cmhip_dyn_set_key(0, -1, -1) + cmhip_dyn_get_key(0, 0u, &k);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


# ---------------------------------------------------------------------------
# The duck designer

def duck(th, depth, K):
    """the designer's formula in numpy doubles -> int64 [128]"""
    k = np.arange(1, TG.USED)
    v = (8 + (k - 1) % 8) * 2.0 ** ((k - 1) // 8 - 3)
    d = 20 * np.log10(v / 32768.0) - th
    g = -depth * np.clip((d + K / 2) / K, 0, 1) if K > 0 else np.where(d >= 0, -depth, 0.0)
    out = np.zeros(TG.CURVE, dtype=np.int64)
    out[1:TG.USED] = np.minimum(32768, np.floor(32768 * 10 ** (g / 20) + 0.5))
    out[0] = 32768
    return out, d


DUCKS = {
    "a bed under speech": (-36.0, 14.0, 8.0),
    "knee 0": (-30.0, 12.0, 0.0),
    "depth 0": (-20.0, 0.0, 6.0),
    "a threshold above 0 dBFS": (3.0, 20.0, 10.0),
    "a threshold below the lowest knot": (-120.0, 9.0, 2.0),
    "a knee wider than the grid": (-50.0, 40.0, 200.0),
    "a deep duck, a hard corner": (-30.05, 90.0, 0.0),
}


@pytest.mark.parametrize("name", list(DUCKS))
def test_design_duck(cm, name):
    th, depth, K = DUCKS[name]
    want, d = duck(th, depth, K)
    rc, got = cm.dyn_design_duck_rc(th, depth, K)
    assert rc == 0
    got = got.astype(np.int64)
    # the doubles are exact far below one unit: only a rounding tie or a last-ulp pow / log10 difference can move an entry
    assert np.abs(got - want).max() <= 1, (name, np.flatnonzero(got != want))
    assert got[0] == UNITY and not got[123:].any() and cm.dyn_curve_ok(got)
    below = 1 + np.flatnonzero(d < -K / 2 - 1e-9)                 # knots below threshold - K/2: exactly unity
    assert (got[below] == UNITY).all()
    assert (np.diff(got[1:123]) <= 0).all()                      # a duck never rises with the key's level
    if name == "depth 0":
        assert (got[:123] == UNITY).all()
    if name == "a threshold above 0 dBFS":                       # 3 dBFS - K/2 = -2 dBFS: only the top of the grid is inside the knee
        assert got[121] < UNITY and (got[:110] == UNITY).all()
    if name == "a threshold below the lowest knot":              # knot 1 is level 1, -90.3 dBFS: every level is ducked all the way
        assert np.abs(got[1:123] - int(np.floor(32768 * 10 ** (-depth / 20) + 0.5))).max() <= 1
    if name == "a deep duck, a hard corner":                     # level 1024 (knot 81) is -30.1 dBFS, level 1152 -29.1 dBFS
        assert (got[1:82] == UNITY).all() and (got[82:123] == 1).all()           # -90 dB: 1.04 -> 1


def test_design_duck_refusals(cm):
    nan, inf = float("nan"), float("inf")
    good = [-30.0, 12.0, 6.0]
    assert cm.dyn_design_duck_rc(*good)[0] == 0
    for k in range(3):
        for bad in (nan, inf, -inf):
            p = list(good)
            p[k] = bad
            assert cm.dyn_design_duck_rc(*p)[0] == cm.ERROR_INVAL, (k, bad)
    for k, bad in ((1, -0.001), (1, -12.0), (2, -0.001)):
        p = list(good)
        p[k] = bad
        assert cm.dyn_design_duck_rc(*p)[0] == cm.ERROR_INVAL, (k, bad)
    assert b"dyn_design_duck" in cm.lib.cmhip_last_error()
    t = np.zeros(128, dtype=np.uint16)
    assert cm.lib.cmhip_dyn_design_duck(None, t.ctypes.data) == cm.ERROR_FAULT
    assert cm.lib.cmhip_dyn_design_duck(C.byref(cm.DynDuckDesc(-30, 12, 6)), None) == cm.ERROR_FAULT
    with pytest.raises(cm.CoolmicError):
        cm.dyn_design_duck(depth_db=-1.0)
    assert cm.dyn_design_duck(threshold_db=-30.0, depth_db=12.0, knee_db=6.0)[0] == UNITY


def test_key_calls_refuse_null(cm):
    lib = cm.lib
    k = C.c_long(77)
    assert lib.cmhip_dyn_set_key(None, -1, -1) == cm.ERROR_FAULT and lib.cmhip_dyn_set_key(None, 0, 5) == cm.ERROR_FAULT
    assert b"dyn_set_key" in lib.cmhip_last_error()
    assert lib.cmhip_dyn_get_key(None, 0, C.byref(k)) == cm.ERROR_FAULT and k.value == 77
    assert lib.cmhip_dyn_get_key(None, 0, None) == cm.ERROR_FAULT
    assert b"dyn_get_key" in lib.cmhip_last_error()


# ---------------------------------------------------------------------------
# The keyed model's own properties

@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_keyed_model_properties(a, b, H):
    A, B, D, W, hist = TG.geometry(a, b, H)
    t = 4096
    zero = np.zeros((hist, 2), dtype=np.int16)
    x, k = TG.signal(52 + a, 3 * t, 2), TG.signal(91 + a, 3 * t, 2)
    x[5000] = -32768
    T = TG.design(**TG.DENSE_CURVE)
    # a stream that is its own key is the unkeyed model, from a history too
    h = x[:hist][::-1].copy()
    for T_ in (T, TG.steps().astype(np.int64)):
        y0, s0 = TG.model_dyn(x, h, T_, a, b, H)
        y1, s1 = TK.model_dyn_keyed(x, h, x, h, T_, a, b, H)
        assert np.array_equal(y0, y1) and np.array_equal(s0, s1)
    # under the unity curve a keyed stream is a pure delay, bit for bit
    y, s = TK.model_dyn_keyed(x, zero, k, zero, TG.flat(UNITY), a, b, H)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], x[:-D]) and y[5000 + D, 0] == -32768
    # never louder than the stream's OWN delayed input, sample by sample, whatever the key does
    y, s = TK.model_dyn_keyed(x, zero, k, zero, T, a, b, H)
    xd = np.concatenate([np.zeros((D, 2), dtype=np.int16), x[:-D]]).astype(np.int64)
    assert (np.abs(y.astype(np.int64)) <= np.abs(xd)).all() and s.min() < 1000 and (np.diff(s) != 0).mean() >= 0.25
    assert np.array_equal(s, TG.model_dyn(k, zero, T, a, b, H)[1])               # the gain is the one the key would get
    assert not np.array_equal(s, TG.model_dyn(x, zero, T, a, b, H)[1])
    # cut-invariance of a follower, its key and a mutual pair: runs of 1, 7, HIST - 1, HIST, HIST + 1, 0, tile + 5 and the rest
    model = TK.KeyModel(4, 2, a, b, H)
    model.set(-1, T)
    keys = [1, 1, 3, 2]
    xs = [x, k, TG.signal(93 + a, 3 * t, 2), TG.signal(94 + a, 3 * t, 2)]
    for s_, k_ in enumerate(keys):
        model.set_key(s_, k_)
    one = [TK.model_dyn_keyed(xs[s_], zero, xs[k_], zero, T, a, b, H)[0] for s_, k_ in enumerate(keys)]
    pos, parts = 0, [[] for _ in keys]
    for n in (1, 7, hist - 1, hist, hist + 1, 0, t + 5, 3 * t):
        ys = model.run([v[pos:pos + n] for v in xs])
        for s_, y_ in enumerate(ys):
            parts[s_].append(y_)
        pos = min(pos + n, 3 * t)
    assert pos == 3 * t and all(np.array_equal(np.concatenate(p), w) for p, w in zip(parts, one))
    # a burst in the KEY lowers the follower's gain B - 1 frames before it comes out and holds it for W frames
    q = np.full((8000, 1), 300, dtype=np.int16)
    q[2000:3600] = 30000
    f = np.full((8000, 1), 20000, dtype=np.int16)
    z1 = np.zeros((hist, 1), dtype=np.int16)
    y, s = TK.model_dyn_keyed(f, z1, q, z1, T, a, b, H)
    full = int(TG.curve_at(T, np.array([30000]))[0])
    assert full < UNITY and s[1999] == UNITY
    assert s[2000 + D] < UNITY
    assert s[2000 + (A - 1) + D] == full and s[2000 + D:2000 + A + D].min() == full
    assert s[3599 + W - 1] == full
    assert s[3599 + W - 1 + A + B] == UNITY
    assert y[2000 + (A - 1) + D, 0] == (20000 * full + (1 << 14)) >> 15


def test_slide_max_is_the_sliding_window_maximum():
    v = np.random.default_rng(5).integers(0, 32769, size=5000).astype(np.int64)
    for n in (1, 2, 3, 8, 107, 132, 2048, 1999):
        want = np.lib.stride_tricks.sliding_window_view(v, n).max(axis=1)
        assert np.array_equal(TK._slide_max(v, n), want), n


# ---------------------------------------------------------------------------
# The keyed decomposition (csrc/k_dyn.h, KEYED = true): tests/test_dyn_host.py's emulation with step 1 on the key's sequence.

@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_keyed_decomposition_equals_the_keyed_model(cm, a, b, H, channels):
    p = cm.plan_dyn(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    xs, counts, keys, T, ragged, full, gmin, differ, change, smallest = TK.dense_key_case(a, b, H, channels, t)
    TK.assert_dense_key(differ, change, smallest)
    TD._hold_emulation_to(keys, xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo, TD.MEAN)


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_keyed_dense_conditions_hold_on_the_model(a, b, H):
    """mono, stereo, six channels of the GPU test's dense cases: the followers' outputs differ from the own detector's in
    at least half of the frames, the gain moves, the gate closes"""
    for channels in (1, 2, 6):
        case = TK.dense_key_case(a, b, H, channels, 4096)
        TK.assert_dense_key(*case[-3:])
