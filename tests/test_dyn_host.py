"""CPU: the host side of the dynamics stage (cmhip_dyn_*): the header, cmhip_dyn_check at its edges, NULL and descriptor
refusals, what a set asks of a table, the curve designer against its formula in numpy, the launcher's plan
(csrc/dyn_plan.h) through the library and, as a stand-alone C++ program with the curve's index over every level, plainly
and under AddressSanitizer + UBSan; the model's own properties; and an emulation of the kernels' decomposition (tiles, the
halo from the history slot or the previous tile, one sequence of 16-byte vectors across the seam, per-thread elements
and every doubling pass, the lookup from the packed table, the delayed samples out of two vectors, the history written
by the last tile) at the plan's own tile against the model of tests/test_gpu_dyn.py.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "dyn_plan_test.cpp")


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_dyn_model", os.path.join(ROOT, "tests", "test_gpu_dyn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # the model, the signal and the dense cases of the GPU tests
UNITY = 32768


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_dyn_desc_t d; cmhip_dyn_curve_desc_t c; uint32_t g[1]; uint16_t t[CMHIP_DYN_CURVE];\n"
           "d.device = 0; d.streams = d.channels = 1; d.detector_log2 = 6; d.smooth_log2 = 6; d.hold = 0; d.max_frames = 1;\n"
           "d.hip_stream = 0; (void)sizeof(d); c.comp_threshold_db = -18; c.comp_ratio = 4; c.comp_knee_db = 6;\n"
           "c.gate_threshold_db = -45; c.gate_ratio = 2; c.gate_range_db = 40;\n"
           "return cmhip_dyn_check(6, 6, 0) + cmhip_dyn_design(&c, t) + (cmhip_dyn_new(0) != 0) + cmhip_dyn_sync(0)"
           " + (cmhip_dyn_hip_stream(0) != 0) + cmhip_dyn_run(0, 0, 0, 0, 0, 0, 0) + cmhip_dyn_set_curve(0, -1, t)"
           " + cmhip_dyn_get_curve(0, 0, t) + cmhip_dyn_reset(0, -1) + cmhip_dyn_min_gain(0, g, 0)"
           " + (int)cmhip_dyn_delay(0) + (cmhip_dyn_free(0), 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check(cm):
    ok = cm.dyn_check
    for a, want in ((2, cm.ERROR_INVAL), (3, 0), (10, 0), (11, cm.ERROR_INVAL)):
        assert ok(a, 6, 0) == want, a
    for b, want in ((2, cm.ERROR_INVAL), (3, 0), (9, 0), (10, cm.ERROR_INVAL)):
        assert ok(6, b, 0) == want, b
    for b in range(3, 10):
        assert ok(6, b, 2048 - (1 << b)) == 0 and ok(6, b, 2049 - (1 << b)) == cm.ERROR_INVAL       # B + H = 2048, 2049
    assert b"dyn:" in cm.lib.cmhip_last_error()
    assert ok(6, 6, 0xffffffff) == cm.ERROR_INVAL and ok(0xffffffff, 6, 0) == cm.ERROR_INVAL
    assert ok(6, 0xffffffff, 0) == cm.ERROR_INVAL


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    t = np.zeros(128, dtype=np.uint16)
    assert lib.cmhip_dyn_new(None) is None
    assert lib.cmhip_dyn_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_set_curve(None, -1, t.ctypes.data) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_get_curve(None, 0, t.ctypes.data) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_min_gain(None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_hip_stream(None) is None and lib.cmhip_dyn_delay(None) == 0
    assert lib.cmhip_dyn_design(None, t.ctypes.data) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_design(C.byref(cm.DynCurveDesc(0, 1, 0, 0, 1, 0)), None) == cm.ERROR_FAULT
    lib.cmhip_dyn_free(None)
    # descriptors are refused before any device is touched
    for streams, channels, a, b, hold, frames in ((0, 2, 6, 6, 0, 1024), (1, 0, 6, 6, 0, 1024), (1, 17, 6, 6, 0, 1024),
                                                  (1, 2, 2, 6, 0, 1024), (1, 2, 11, 6, 0, 1024), (1, 2, 6, 2, 0, 1024),
                                                  (1, 2, 6, 10, 0, 1024), (1, 2, 6, 6, 1985, 1024), (1, 2, 6, 9, 1537, 1024),
                                                  (1, 2, 6, 6, 0, 0), (1, 2, 6, 6, 0, (1 << 30) + 1),
                                                  (1, 16, 6, 6, 0, (1 << 27) + 1), (1 << 20, 16, 6, 6, 0, 1024)):
        d = cm.DynDesc(0, streams, channels, a, b, hold, frames, None)
        assert lib.cmhip_dyn_new(C.byref(d)) is None, (streams, channels, a, b, hold, frames)
        assert b"dyn_new" in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Dynamics(streams, channels, a, b, hold, frames)


def test_what_a_set_asks_of_a_table(cm):
    """cmhip_dyn_set_curve's validation, on the host function it uses (csrc/dyn_plan.h: dyn_curve_ok)"""
    good = np.full(128, UNITY, dtype=np.uint16)
    assert cm.dyn_curve_ok(good) and cm.dyn_curve_ok(np.zeros(128, dtype=np.uint16))
    for k in (0, 57, 122):
        bad = good.copy()
        bad[k] = 32769
        assert not cm.dyn_curve_ok(bad), k
    for k in range(123, 128):
        ok = good.copy()
        ok[k] = 65535                                            # ignored entries
        assert cm.dyn_curve_ok(ok), k
    assert cm.dyn_curve_ok(TG.design(**TG.DENSE_CURVE))


# ---------------------------------------------------------------------------
# The curve designer

DESIGNS = {
    "the dense cases' curve": dict(ct=-18.0, R=4.0, K=6.0, gt=-45.0, Re=2.0, rng=40.0),
    "no gate": dict(ct=-24.0, R=3.0, K=10.0, gt=-50.0, Re=2.0, rng=0.0),
    "hard knee": dict(ct=-12.0, R=8.0, K=0.0, gt=-60.0, Re=1.5, rng=20.0),
    "R = 1": dict(ct=-20.0, R=1.0, K=6.0, gt=-40.0, Re=3.0, rng=60.0),
    "a hard gate": dict(ct=-6.0, R=2.0, K=3.0, gt=-35.0, Re=1000.0, rng=80.0),
    "gate above the compressor": dict(ct=-30.0, R=6.0, K=12.0, gt=-20.0, Re=2.0, rng=30.0),
    "nothing at all": dict(ct=0.0, R=1.0, K=0.0, gt=-96.0, Re=1.0, rng=0.0),
    "a limiter-like ratio, a wide knee": dict(ct=-3.0, R=100.0, K=40.0, gt=-90.0, Re=1.0, rng=12.0),
}


@pytest.mark.parametrize("name", list(DESIGNS))
def test_design(cm, name):
    p = DESIGNS[name]
    want = TG.design(**p)
    rc, got = cm.dyn_design_rc(p["ct"], p["R"], p["K"], p["gt"], p["Re"], p["rng"])
    assert rc == 0
    got = got.astype(np.int64)
    # the doubles are exact far below one unit: only a rounding tie or a last-ulp pow / log10 difference can move an
    # entry, and by one
    assert np.abs(got - want).max() <= 1, (name, np.flatnonzero(got != want))
    assert got[0] == want[0] and not got[123:].any() and not want[123:].any()
    assert got[:123].max() <= UNITY and cm.dyn_curve_ok(got)
    if p["rng"] == 0 and p["R"] == 1:
        assert (got[:123] == UNITY).all()
    if p["rng"] == 0:
        assert got[0] == UNITY and (np.diff(got[1:123]) <= 0).all()          # a compressor alone never rises with the level
    if name == "a hard gate":
        assert got[1] == got[0] == 3 and got[:123].max() == UNITY            # -80 dB: 3.28 -> 3


def test_design_refusals(cm):
    nan, inf = float("nan"), float("inf")
    good = [-18.0, 4.0, 6.0, -45.0, 2.0, 40.0]
    assert cm.dyn_design_rc(*good)[0] == 0
    for k in range(6):
        for bad in (nan, inf, -inf):
            p = list(good)
            p[k] = bad
            assert cm.dyn_design_rc(*p)[0] == cm.ERROR_INVAL, (k, bad)
    for k, bad in ((1, 0.999), (1, 0.0), (1, -2.0), (4, 0.999), (4, -1.0), (2, -0.001), (5, -0.001)):
        p = list(good)
        p[k] = bad
        assert cm.dyn_design_rc(*p)[0] == cm.ERROR_INVAL, (k, bad)
    assert b"dyn_design" in cm.lib.cmhip_last_error()
    with pytest.raises(cm.CoolmicError):
        cm.dyn_design(comp_ratio=0.5)


# ---------------------------------------------------------------------------
# The launcher's plan

def test_plan(cm):
    for a in (3, 6, 10):
        for b in range(3, 10):
            B = 1 << b
            for H in (0, 1, 2048 - B):
                hist = TG.geometry(a, b, H)[4]
                halo = (hist + 7) // 8 * 8
                for ch in (1, 2, 3, 16):
                    p = cm.plan_dyn(5, ch, a, b, H, 1)               # a one-frame run: one workgroup per stream
                    assert (p.err, p.grid, p.chunks, p.block) == (0, 5, 1, 256), (a, b, H, ch)
                    assert p.fast == (1 if ch <= 2 else 0)
                    t = p.tile_frames
                    assert t == 4096 and t >= p.halo == halo >= hist
                    assert p.lds_bytes == (t + halo) * 4 <= 30720    # far inside what a workgroup may use without a raised limit
                    assert t + halo <= 256 * R                       # the elements a thread keeps (k_dyn.hip: DYN_R)
                    assert p.passes == a + int(np.log2(B + H)) + (1 if (B + H) & (B + H - 1) else 0) + b
                    for frames in (1, t - 1, t, t + 1, 100000):
                        q = cm.plan_dyn(3, ch, a, b, H, frames)
                        assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
    # no grid of 2^31 workgroups
    p = cm.plan_dyn(1 << 20, 2, 6, 6, 0, 1 << 23)                    # 2^20 streams x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_dyn(1 << 20, 2, 6, 6, 0, (1 << 23) - 4096)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    assert cm.plan_dyn(0, 2, 6, 6, 0, 100).grid == 0 and cm.plan_dyn(4, 2, 6, 6, 0, 0).grid == 0
    for ch, a, b, H in ((0, 6, 6, 0), (17, 6, 6, 0), (2, 2, 6, 0), (2, 11, 6, 0), (2, 6, 2, 0), (2, 6, 10, 0), (2, 6, 6, 1985)):
        p = cm.plan_dyn(4, ch, a, b, H, 100)
        assert p.grid == 0 and p.err == 0


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_as_a_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "dyn_plan_test", [])                  # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"plans ok: \d{5,} geometries, 32769 levels", out.stdout), out.stdout + out.stderr


def test_plan_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "dyn_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "plans ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The model's own properties

def test_index_of_every_level():
    l = np.arange(0, UNITY + 1)
    idx, frac, sh = TG.curve_index(l)
    assert (np.diff(idx) >= 0).all() and idx.max() == 121 == idx[-1] and idx[0] == 0 and frac[-1] == 0
    assert (frac < (1 << sh)).all() and (frac[l < 8] == 0).all()
    first = np.flatnonzero(np.diff(idx, prepend=-1))             # the first level of every knot
    assert (frac[first] == 0).all() and first.size == 105
    k = idx[first][1:] - 1
    assert np.array_equal(l[first][1:], (8 + k % 8) * 2.0 ** (k // 8 - 3))       # knot k + 1 stands for this level
    # between two knots the lookup is the straight line, rounded down
    T = np.arange(128) * 250
    v = TG.curve_at(T, l)
    assert (np.diff(v) >= 0).all() and v[0] == 0 and v[-1] == 121 * 250
    T = 32768 - np.arange(128) * 250
    v = TG.curve_at(T, l)
    assert (np.diff(v) <= 0).all() and v[0] == 32768 and v[-1] == 32768 - 121 * 250


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_model_properties(a, b, H):
    A, B, D, W, hist = TG.geometry(a, b, H)
    assert hist == (A - 1) + (W - 1) + (B - 1) <= 3581 and D == B - 1
    t = 4096
    zero = np.zeros((hist, 2), dtype=np.int16)
    x = TG.signal(42 + a, 3 * t, 2)
    x[5000] = -32768
    # the curve of creation is a pure delay, bit for bit
    y, s = TG.model_dyn(x, zero, TG.flat(UNITY), a, b, H)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], x[:-D]) and y[5000 + D, 0] == -32768
    # never louder than the input, sample by sample
    T = TG.design(**TG.DENSE_CURVE)
    y, s = TG.model_dyn(x, zero, T, a, b, H)
    xd = np.concatenate([np.zeros((D, 2), dtype=np.int16), x[:-D]]).astype(np.int64)
    assert (np.abs(y.astype(np.int64)) <= np.abs(xd)).all() and s.min() < 1000 and (np.diff(s) != 0).mean() >= 0.25
    # cut-invariance: one run equals the same stream in runs of 1, 7, HIST - 1, HIST, HIST + 1, 0, tile + 5 and the rest
    h, pos, parts = zero, 0, []
    for n in (1, 7, hist - 1, hist, hist + 1, 0, t + 5, x.shape[0]):
        part = x[pos:pos + n]
        parts.append(TG.model_dyn(part, h, T, a, b, H)[0])
        h = TG.next_hist(h, part)
        pos += part.shape[0]
    assert pos == x.shape[0] and np.array_equal(np.concatenate(parts), y)
    # a rising level is met by the gain B - 1 frames before it comes out; a falling one is held for W frames
    q = np.full((8000, 1), 300, dtype=np.int16)
    q[2000:3600] = 30000                                         # (outlasts the longest detector and ramp together)
    y, s = TG.model_dyn(q, np.zeros((hist, 1), dtype=np.int16), T, a, b, H)
    full = int(TG.curve_at(T, np.array([30000]))[0])
    assert full < UNITY and s[1999] == UNITY
    assert s[2000 + D] < UNITY                                   # the reduction has begun when the onset comes out
    assert s[2000 + (A - 1) + D] == full and s[2000 + D:2000 + A + D].min() == full     # ... and ends with the detector's rise
    assert s[3599 + W - 1] == full                               # L[3599] is the last full level: held for W frames
    assert s[3599 + W - 1 + A + B] == UNITY                      # ... then the detector decays and the gain ramps back


# ---------------------------------------------------------------------------
# The decomposition of k_dyn<CT, DET> / k_dynk<CT, DET> (csrc/k_dyn.hip, the body csrc/k_dyn.h's dyn_tile), step by step
# in numpy, one workgroup per tile.  tests/test_dyn_key_host.py and tests/test_dyn_rms_host.py hold their models to it too.

BLOCK, R = 256, 30
UNWRITTEN = 1 << 40
SPLIT = 15                                        # DYN_SQ_SPLIT
MEAN, RMS = 0, 1                                  # DYN_DETECT_*


def _pack(T):
    """the curve as a workgroup holds it in LDS: dword k = T[k] | T[k+1] << 16, k < 123"""
    T = np.asarray(T, dtype=np.int64)
    return T[:123] | T[1:124] << 16


def _lookup(cv, l):
    """dyn_index + dyn_lookup: the index from the leading zeros of l | 1, one select for l == 0, one packed read"""
    assert l.min() >= 0 and l.max() <= UNITY
    lz = 32 - np.floor(np.log2((l | 1).astype(np.float64))).astype(np.int64) - 1     # __builtin_clz(l | 1); exact below 2^53
    E = 31 - lz
    norm = l << (15 - E)
    assert ((norm >> 15) == 1)[l > 0].all() and (norm < 65536).all()
    sh = np.where(E > 3, E - 3, 0)
    frac = l & ((1 << sh) - 1)
    idx = np.where(l != 0, 1 + 8 * E + ((norm >> 12) & 7), 0)
    assert idx.max() <= 121
    w = cv[idx]
    t0, t1 = w & 0xffff, w >> 16
    prod = (t1 - t0) * frac
    assert np.abs(prod).max() < 2 ** 27
    return t0 + (prod >> sh)


def _dyn_isqrt(v):
    """csrc/dyn_plan.h: dyn_isqrt, operation by operation, in 32-bit ranges"""
    assert v.min() >= 0 and v.max() < 2 ** 32
    r = np.sqrt(v.astype(np.float32)).astype(np.int64)           # (float)v rounds to 24 bits; the root is single precision
    r = np.minimum(r, 65535)
    assert (r * r < 2 ** 32).all()
    r = np.where(r * r > v, r - 1, r)
    assert (r >= 0).all() and (v - r * r >= 0).all()             # nothing wraps
    return np.where(v - r * r > 2 * r, r + 1, r)


def _emulate_run(x, slot, xk, slotk, T, a, b, H, ch, tile, halo, det):
    """one stream of one run: x int16 [F][C] and slot int64 [halo * C] (the history slot the run reads) the stream's own,
    xk and slotk the key's (the stream's own where it has no key), det MEAN or RMS
    -> out int64 [F * C + 8] (UNWRITTEN where nothing was stored), the slot the run writes, min s or None"""
    A, B, D, W, hist = TG.geometry(a, b, H)
    F = x.shape[0]
    assert xk.shape[0] == F                                      # (the host refuses a run otherwise)
    ns, hsamp = F * ch, halo * ch
    hv, nfull, ntail = hsamp // 8, ns // 8, ns % 8
    assert hsamp % 8 == 0 and tile >= halo >= hist
    cv = _pack(T)
    # a stream as a tile sees it: the slot's vectors below 0, the run's from 0 on, zeros past the count
    pad = np.zeros(16 + 8 * (tile // 8 + 1) * ch, dtype=np.int64)
    seq = np.concatenate([slot, x.astype(np.int64).reshape(-1), pad])         # the stream itself
    seqk = np.concatenate([slotk, xk.astype(np.int64).reshape(-1), pad])      # ... and the detector's source

    def vec(q, vv):                                               # [n] vector indices -> [n][8] samples
        vv = np.asarray(vv)
        assert (vv >= -hv).all()
        return q[(hsamp + vv * 8)[:, None] + np.arange(8)]

    def sample(q, i):
        i = np.asarray(i)
        assert (i >= -hsamp).all() and (i < ns).all()
        return q[hsamp + i]

    out = np.full(ns + 8, UNWRITTEN, dtype=np.int64)
    new_slot = sample(seq, ns - hsamp + np.arange(hsamp))         # 4. (the last tile, or tile 0 of a stream with 0 frames),
    if F == 0:                                                    # from the stream's OWN slots
        assert np.array_equal(new_slot, slot)
        return out, new_slot, None
    gmin = UNITY
    N = halo + tile
    tid, i = np.meshgrid(np.arange(BLOCK), np.arange(R), indexing="ij")
    own = (tid + BLOCK * i).reshape(-1)                           # the thread-to-element map: j = tid + 256 i
    assert np.array_equal(np.sort(own[own < N]), np.arange(N))    # every element has exactly one thread
    for f0 in range(0, F, tile):
        nt = min(tile, F - f0)
        # ---- 1. e of frames f0 - halo .. f0 + tile - 1, from the KEY's slots, across the seam between history and run
        if ch <= 2:
            fpv = 8 // ch
            NV = N // fpv
            assert NV <= BLOCK * ((R * ch + 7) // 8)
            vbase = f0 * ch // 8 - hv
            assert f0 == 0 or vbase >= 0                          # only the run's first tile reads the (key's) history slot
            v = np.abs(vec(seqk, vbase + np.arange(NV)))
            e = (v if ch == 1 else np.maximum(v[:, 0::2], v[:, 1::2])).reshape(-1)
        else:
            p = f0 - halo + np.arange(N)
            e = np.zeros(N, dtype=np.int64)
            inside = p < F
            e[inside] = np.abs(sample(seqk, p[inside, None] * ch + np.arange(ch))).max(axis=1)
        assert e.size == N and e.max() <= 32768
        # ---- 2. the passes: partner from LDS, own element back, shifted by the last pass of a sum
        j = np.arange(N)
        passes = 0

        def one_pass(L, dist, is_max, shift):
            nonlocal passes
            o = L[np.maximum(j, dist) - dist]                      # (unguarded: an element without a partner takes element 0)
            v = (np.maximum(L, o) if is_max else L + o)
            assert v.max() < 2 ** 32
            passes += 1
            return v >> shift

        def boxcar(L, n, shift):                                  # log2 n add passes, the last one shifts
            d = 1
            while d < n:
                L = one_pass(L, d, False, shift if 2 * d == n else 0)
                d *= 2
            return L

        if det == RMS:
            sq = e * e
            assert sq.max() < 2 ** 32                             # the square itself fits a dword
            lo = boxcar(sq & ((1 << SPLIT) - 1), A, 0)            # the low halves first, e waiting in registers
            hi = boxcar(sq >> SPLIT, A, 0)
            assert lo.max() <= 2 ** 25 and hi.max() <= 2 ** 25
            M = (hi << (SPLIT - a)) + (lo >> a)                   # dyn_mean_square
            assert M.max() <= 2 ** 30                             # also where an element had no partner
            L = _dyn_isqrt(M)
        else:
            L = boxcar(e, A, a)
        P = 1
        while 2 * P <= W:
            L = one_pass(L, P, True, 0)
            P *= 2
        if W > P:
            L = one_pass(L, W - P, True, 0)
        L = boxcar(_lookup(cv, np.minimum(L, UNITY)), B, b)
        assert passes == (2 * a if det == RMS else a) + int(np.log2(W)) + (1 if W & (W - 1) else 0) + b
        Ls = L[halo:]
        gmin = min(gmin, int(Ls[:nt].min()))
        # ---- 3. the tile's output vectors, the delayed samples from the stream's OWN slots
        vb, nv = f0 * ch // 8, (nt * ch + 7) // 8
        v8 = vb + np.arange(nv)
        if ch <= 2:
            back = (D + 1) * ch // 8
            assert (D + 1) * ch % 8 == 0 and back <= hv
            x0, x1 = vec(seq, v8 - back), vec(seq, v8 - back + 1)
            xs = np.concatenate([x0[:, ch:], x1[:, :ch]], axis=1)                 # mono: samples 1..8, stereo: 2..9
            sf = Ls[(np.arange(nv) * (8 // ch))[:, None] + np.arange(8) // ch]
            prod = xs * sf
        else:
            q = v8[:, None] * 8 + np.arange(8)
            ok = q < ns
            qq = np.where(ok, q, 0)
            prod = np.where(ok, sample(seq, qq - D * ch) * Ls[np.where(ok, qq // ch - f0, 0)], 0)
        assert np.abs(prod + (1 << 14)).max() < 2 ** 31           # the kernel multiplies in 32 bits
        y = (prod + (1 << 14)) >> 15
        for w in range(nv):
            if v8[w] < nfull:
                out[v8[w] * 8:v8[w] * 8 + 8] = y[w]
            elif v8[w] == nfull:
                out[v8[w] * 8:v8[w] * 8 + ntail] = y[w, :ntail]
    return out, new_slot, gmin


def _hold_emulation_to(keys, xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo, det):
    """the ragged run, then the uniform run on the slots it left, stream s reading keys[s]: outputs, the untouched rest
    and the meter against the model's"""
    S = len(counts)
    slots = [np.zeros(halo * channels, dtype=np.int64) for _ in range(S)]
    got_min = [UNITY] * S
    for cut, wants in ((counts, ragged), ([counts[0]] * S, full)):
        new = []
        for s in range(S):
            k = keys[s]
            assert cut[k] == cut[s]
            out, slot, m = _emulate_run(xs[s][:cut[s]], slots[s], xs[k][:cut[k]], slots[k], T, a, b, H, channels, t, halo,
                                        det)
            w = wants[s].astype(np.int64).reshape(-1)
            assert np.array_equal(out[:w.size], w), (channels, s)
            assert (out[w.size:] == UNWRITTEN).all(), (channels, s)               # nothing past the stream's count
            got_min[s] = min(got_min[s], UNITY if m is None else m)
            new.append(slot)
        slots = new                                               # the host flips the parity: every tile read the old slots
    assert got_min == gmin


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_decomposition_equals_the_model(cm, a, b, H, channels):
    p = cm.plan_dyn(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    xs, counts, T, ragged, full, unity, change, smallest, gmin = TG.dense_case(a, b, H, channels, t)
    TG.assert_dense(a, b, H, unity, change, smallest)
    assert all(x.shape[0] == counts[0] for x in xs)               # the uniform run takes every stream whole
    _hold_emulation_to(list(range(len(counts))), xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo, MEAN)


def test_emulated_lookup_of_every_level():
    l = np.arange(0, UNITY + 1)
    for T in (TG.design(**TG.DENSE_CURVE), TG.steps().astype(np.int64), np.arange(128) * 258):
        assert np.array_equal(_lookup(_pack(T), l), TG.curve_at(T, l))


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_dense_conditions_hold_on_the_model(a, b, H):
    """mono, stereo and six channels of the GPU test's dense cases: the gain moves, the gate closes, and at the two
    short geometries a fifth of the frames pass untouched"""
    for channels in (1, 2, 6):
        xs, counts, T, ragged, full, unity, change, smallest, gmin = TG.dense_case(a, b, H, channels, 4096)
        TG.assert_dense(a, b, H, unity, change, smallest)
