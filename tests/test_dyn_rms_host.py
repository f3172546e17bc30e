"""CPU: the host side of the dynamics stage's RMS detector (cmhip_dyn_new_detector, cmhip_dyn_detector,
cmhip_dyn_check_detector): the header, the refusals, the root and the plan through the library and as a stand-alone C++
program (csrc/dyn_plan.h: the root for every mean square, the two 32-bit sums against a 64-bit one, the plan), plainly
and under AddressSanitizer + UBSan; the RMS model's own properties and what the header says about constant magnitudes
and sines; and an emulation of the kernels' decomposition (csrc/k_dyn.h with DET = DYN_DETECT_RMS: the squares split at
bit 15, each half through the a unguarded add passes, the halves recombined, the root from a single-precision seed and
its integer repair) at the plan's own tile against the RMS model of tests/test_gpu_dyn_rms.py.  Nothing here needs a GPU."""
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
TD = _load("test_dyn_host")        # the emulation's helpers
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
    # a stream that is its own key is the unkeyed model; the RmsModel class agrees with the functions
    model = TR.RmsModel(2, 2, a, b, H)
    model.set(-1, T)
    model.set_key(1, 0)
    k = TG.signal(91 + a, 3 * t, 2)
    ys = model.run([x, k])
    assert np.array_equal(ys[0], y) and np.array_equal(ys[1], TR.model_rms_keyed(k, zero, x, zero, T, a, b, H)[0])


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
# The RMS decomposition (csrc/k_dyn.h, DET = DYN_DETECT_RMS) step by step in numpy, one workgroup per tile:
# tests/test_dyn_key_host.py's emulation with step 2's first line replaced.

BLOCK, R, UNWRITTEN = TD.BLOCK, TD.R, TD.UNWRITTEN
SPLIT = 15                                        # DYN_SQ_SPLIT


def _dyn_isqrt(v):
    """csrc/dyn_plan.h: dyn_isqrt, operation by operation, in 32-bit ranges"""
    assert v.min() >= 0 and v.max() < 2 ** 32
    r = np.sqrt(v.astype(np.float32)).astype(np.int64)           # (float)v rounds to 24 bits; the root is single precision
    r = np.minimum(r, 65535)
    assert (r * r < 2 ** 32).all()
    r = np.where(r * r > v, r - 1, r)
    assert (r >= 0).all() and (v - r * r >= 0).all()             # nothing wraps
    return np.where(v - r * r > 2 * r, r + 1, r)


def _emulate_rms_run(x, slot, xk, slotk, T, a, b, H, ch, tile, halo):
    """one stream of one run: x int16 [F][C] and slot int64 [halo * C] the stream's own, xk and slotk the key's (the
    stream's own where it has no key) -> out int64 [F * C + 8] (UNWRITTEN where nothing was stored), the slot the run
    writes, min s or None"""
    A, B, D, W, hist = TG.geometry(a, b, H)
    F = x.shape[0]
    assert xk.shape[0] == F
    ns, hsamp = F * ch, halo * ch
    hv, nfull, ntail = hsamp // 8, ns // 8, ns % 8
    assert hsamp % 8 == 0 and tile >= halo >= hist
    cv = TD._pack(T)
    pad = np.zeros(16 + 8 * (tile // 8 + 1) * ch, dtype=np.int64)
    seq = np.concatenate([slot, x.astype(np.int64).reshape(-1), pad])         # the stream as a tile sees it
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
    new_slot = sample(seq, ns - hsamp + np.arange(hsamp))         # 4. from the stream's OWN slots
    if F == 0:
        assert np.array_equal(new_slot, slot)
        return out, new_slot, None
    gmin = UNITY
    N = halo + tile
    tid, i = np.meshgrid(np.arange(BLOCK), np.arange(R), indexing="ij")
    own = (tid + BLOCK * i).reshape(-1)                           # the thread-to-element map: j = tid + 256 i
    assert np.array_equal(np.sort(own[own < N]), np.arange(N))    # every element has exactly one thread
    for f0 in range(0, F, tile):
        nt = min(tile, F - f0)
        # ---- 1. e of frames f0 - halo .. f0 + tile - 1, across the seam between the history slot and the run
        if ch <= 2:
            fpv = 8 // ch
            NV = N // fpv
            assert NV <= BLOCK * ((R * ch + 7) // 8)
            vbase = f0 * ch // 8 - hv
            assert f0 == 0 or vbase >= 0                          # only the run's first tile reads the history slot
            v = np.abs(vec(seqk, vbase + np.arange(NV)))
            e = (v if ch == 1 else np.maximum(v[:, 0::2], v[:, 1::2])).reshape(-1)
        else:
            p = f0 - halo + np.arange(N)
            e = np.zeros(N, dtype=np.int64)
            inside = p < F
            e[inside] = np.abs(sample(seqk, p[inside, None] * ch + np.arange(ch))).max(axis=1)
        assert e.size == N and e.max() <= 32768
        # ---- 2. the passes
        j = np.arange(N)
        passes = 0

        def one_pass(L, dist, is_max, shift):
            o = L[np.maximum(j, dist) - dist]                      # (unguarded: an element without a partner takes element 0)
            v = (np.maximum(L, o) if is_max else L + o)
            assert v.max() < 2 ** 32
            return v >> shift

        sq = e * e
        assert sq.max() < 2 ** 32                                 # the square itself fits a dword
        lo, hi = sq & ((1 << SPLIT) - 1), sq >> SPLIT
        halves = []
        for half in (lo, hi):                                     # the low halves first, e waiting in registers
            d = 1
            while d < A:
                half = one_pass(half, d, False, 0)
                d *= 2
                passes += 1
            assert half.max() <= 2 ** 25
            halves.append(half)
        M = (halves[1] << (SPLIT - a)) + (halves[0] >> a)         # dyn_mean_square
        assert M.max() <= 2 ** 30                                 # also where an element had no partner
        L = _dyn_isqrt(M)
        P = 1
        while 2 * P <= W:
            L = one_pass(L, P, True, 0)
            P *= 2
            passes += 1
        if W > P:
            L = one_pass(L, W - P, True, 0)
            passes += 1
        L = TD._lookup(cv, np.minimum(L, UNITY))
        d = 1
        while d < B:
            L = one_pass(L, d, False, b if 2 * d == B else 0)
            d *= 2
            passes += 1
        assert passes == 2 * a + int(np.log2(W)) + (1 if W & (W - 1) else 0) + b
        Ls = L[halo:]
        gmin = min(gmin, int(Ls[:nt].min()))
        # ---- 3. the tile's output vectors, the delayed samples from the stream's OWN slots
        vb, nv = f0 * ch // 8, (nt * ch + 7) // 8
        v8 = vb + np.arange(nv)
        if ch <= 2:
            back = (D + 1) * ch // 8
            assert (D + 1) * ch % 8 == 0 and back <= hv
            x0, x1 = vec(seq, v8 - back), vec(seq, v8 - back + 1)
            xs = np.concatenate([x0[:, ch:], x1[:, :ch]], axis=1)
            sf = Ls[(np.arange(nv) * (8 // ch))[:, None] + np.arange(8) // ch]
            prod = xs * sf
        else:
            q = v8[:, None] * 8 + np.arange(8)
            ok = q < ns
            qq = np.where(ok, q, 0)
            prod = np.where(ok, sample(seq, qq - D * ch) * Ls[np.where(ok, qq // ch - f0, 0)], 0)
        assert np.abs(prod + (1 << 14)).max() < 2 ** 31
        y = (prod + (1 << 14)) >> 15
        for w in range(nv):
            if v8[w] < nfull:
                out[v8[w] * 8:v8[w] * 8 + 8] = y[w]
            elif v8[w] == nfull:
                out[v8[w] * 8:v8[w] * 8 + ntail] = y[w, :ntail]
    return out, new_slot, gmin


def _hold_emulation_to(case_keys, xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo):
    S = len(counts)
    slots = [np.zeros(halo * channels, dtype=np.int64) for _ in range(S)]
    got_min = [UNITY] * S
    for cut, wants in ((counts, ragged), ([counts[0]] * S, full)):
        new = []
        for s in range(S):
            k = case_keys[s]
            assert cut[k] == cut[s]
            out, slot, m = _emulate_rms_run(xs[s][:cut[s]], slots[s], xs[k][:cut[k]], slots[k], T, a, b, H, channels, t, halo)
            w = wants[s].astype(np.int64).reshape(-1)
            assert np.array_equal(out[:w.size], w), (channels, s)
            assert (out[w.size:] == UNWRITTEN).all(), (channels, s)               # nothing past the stream's count
            got_min[s] = min(got_min[s], UNITY if m is None else m)
            new.append(slot)
        slots = new                                               # the host flips the parity: every tile read the old slots
    assert got_min == gmin


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_rms_decomposition_equals_the_model(cm, a, b, H, channels):
    p = cm.plan_dynrms(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    W = (1 << b) + H
    assert p.passes == 2 * a + int(np.log2(W)) + (1 if W & (W - 1) else 0) + b and p.lds_bytes == (t + halo) * 4
    xs, counts, T, ragged, full, unity, change, smallest, gmin, differ = TR.dense_rms_case(a, b, H, channels, t)
    TR.assert_dense_rms(a, b, H, unity, change, smallest, differ)
    _hold_emulation_to(list(range(len(counts))), xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_emulated_keyed_rms_decomposition_equals_the_model(cm, a, b, H, channels):
    p = cm.plan_dynrms(8, channels, a, b, H, 1)
    t, halo = p.tile_frames, p.halo
    xs, counts, keys, T, ragged, full, gmin, own, mean, change, smallest = TR.dense_rms_key_case(a, b, H, channels, t)
    TR.assert_dense_rms_key(own, mean, change, smallest)
    _hold_emulation_to(keys, xs, counts, ragged, full, gmin, T, a, b, H, channels, t, halo)


def test_emulated_root_on_the_edges():
    """the emulated dyn_isqrt on the root-edge signal's mean squares, and on the values a float32 seed gets wrong"""
    r = np.arange(0, 32769, dtype=np.int64)
    for v in (r * r, np.maximum(r * r - 1, 0), r * r + 2 * r, r * r + 1):
        v = np.minimum(v, 2 ** 32 - 1)
        assert np.array_equal(_dyn_isqrt(v), TR.isqrt(v))
    r = np.arange(32769, 65536, dtype=np.int64)
    for v in (r * r, r * r - 1, r * r + 2 * r):
        assert np.array_equal(_dyn_isqrt(v), TR.isqrt(v))
    assert _dyn_isqrt(np.array([2 ** 32 - 1]))[0] == 65535


@pytest.mark.parametrize("a,b,H", TG.SETS)
def test_dense_conditions_hold_on_the_model(a, b, H):
    """mono, stereo and six channels of the GPU test's dense cases, plain and keyed: the gain moves, the gate closes, and
    neither the detector nor the key can be ignored"""
    for channels in (1, 2, 6):
        case = TR.dense_rms_case(a, b, H, channels, 4096)
        TR.assert_dense_rms(a, b, H, *case[5:8], case[9])
        TR.assert_dense_rms_key(*TR.dense_rms_key_case(a, b, H, channels, 4096)[-4:])
