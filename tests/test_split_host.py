"""CPU: the band split's host side (cmhip_split_design, cmhip_split_check, csrc/split_plan.h) and an emulation of
k_split.hip's decomposition -- tiles, plane copies, lanes of eight frames, tap blocks, groups -- against the int64 model
of tests/test_gpu_split.py, on that file's cases.  No GPU is used."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "split_plan_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_split", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_split")           # the model, the tables and the cases of the GPU tests
RATE = TG.RATE


# ---------------------------------------------------------------------------
# the design

def i0(x):
    s, t, k = 1.0, 1.0, 1
    while True:
        t = t * (x / 2.0) / k
        if s + t * t == s:
            return s
        s += t * t
        k += 1


def restated_h(rate, crossovers, T):
    """the formula of include/coolmic_hip.h in numpy: h[B-1][T] in double"""
    D = (T - 1) // 2
    x = np.arange(T, dtype=np.float64) - D
    w = np.array([i0(7.5 * np.sqrt(max(0.0, 1.0 - (v / (D + 1.0)) ** 2))) for v in x]) / i0(7.5)
    ls = []
    for f in crossovers:
        fc = f / rate
        l = 2.0 * fc * np.sinc(2.0 * fc * x) * w
        ls.append(l / l.sum())
    return np.array([ls[0]] + [ls[j] - ls[j - 1] for j in range(1, len(ls))])


def quantised(h, b, q):
    g = np.rint(h * 2.0 ** q).astype(np.int64)
    g[(len(h) - 1) // 2] += (2 ** q if b == 0 else 0) - g.sum()
    return g


def restated(rate, crossovers, T):
    h = restated_h(rate, crossovers, T)
    gs, qs = [], []
    for b in range(h.shape[0]):
        for q in range(20, 13, -1):
            g = quantised(h[b], b, q)
            if np.abs(g).max() <= 32767:
                break
        gs.append(g)
        qs.append(q)
    return np.array(gs), np.array(qs)


@pytest.mark.parametrize("bands", [2, 3, 8])
@pytest.mark.parametrize("T", [3, 31, 255, 1023])
def test_design_properties(cm, T, bands):
    g, q = cm.split_design(RATE, bands, TG.CROSSOVERS[bands], T)
    assert g.shape == (bands - 1, T) and q.shape == (bands - 1,)
    g64 = g.astype(np.int64)
    assert np.array_equal(g64, g64[:, ::-1])                                   # symmetric: linear phase
    assert np.abs(g64).max() <= 32767
    assert ((q >= 14) & (q <= 20)).all()
    assert g64.sum(axis=1).tolist() == [1 << int(q[0])] + [0] * (bands - 2)
    assert cm.split_check(bands, T, g, q) == 0
    # agreement with the restatement: a tap differs by at most 1, the centre by at most 1 + the number of differing taps
    rg, rq = restated(RATE, TG.CROSSOVERS[bands], T)
    assert np.array_equal(rq, q)
    D = (T - 1) // 2
    for b in range(bands - 1):
        diff = np.abs(g64[b] - rg[b])
        off = np.delete(diff, D)
        assert off.max(initial=0) <= 1 and diff[D] <= 1 + int((off != 0).sum()), (b, diff.max())
    # q_b is maximal: one more bit and a finished tap leaves +-32767
    h = restated_h(RATE, TG.CROSSOVERS[bands], T)
    for b in range(bands - 1):
        if q[b] < 20:
            assert np.abs(quantised(h[b], b, int(q[b]) + 1)).max() > 32767, b


def test_design_refusals_write_nothing(cm):
    lib = cm.lib
    g = np.full((2, 31), 77, dtype=np.int16)
    q = np.full(2, 99, dtype=np.uint8)

    def design(rate, bands, xs, taps, cap=None, gp=True, qp=True):
        f = (C.c_double * len(xs))(*xs)
        return lib.cmhip_split_design(rate, bands, f, taps, g.ctypes.data if gp else None, q.ctypes.data if qp else None,
                                      g.size if cap is None else cap)

    bad = [(48000, 3, [300.0, 300.0], 31), (48000, 3, [3000.0, 300.0], 31), (48000, 3, [0.0, 300.0], 31),
           (48000, 3, [300.0, 24000.0], 31), (48000, 3, [-1.0, 300.0], 31), (48000, 3, [float("nan"), 300.0], 31),
           (0, 3, [300.0, 3000.0], 31), (48000, 1, [300.0, 3000.0], 31), (48000, 9, [300.0, 3000.0], 31),
           (48000, 3, [300.0, 3000.0], 30), (48000, 3, [300.0, 3000.0], 1), (48000, 3, [300.0, 3000.0], 1025)]
    for rate, bands, xs, taps in bad:
        assert design(rate, bands, xs, taps) == cm.ERROR_INVAL, (rate, bands, xs, taps)
    assert design(48000, 3, [300.0, 3000.0], 31, cap=61) == cm.ERROR_INVAL
    assert b"room for 61" in lib.cmhip_last_error()
    assert design(48000, 3, [300.0, 3000.0], 31, qp=False) == cm.ERROR_FAULT
    assert lib.cmhip_split_design(48000, 3, None, 31, g.ctypes.data, q.ctypes.data, g.size) == cm.ERROR_FAULT
    assert (g == 77).all() and (q == 99).all()
    assert design(48000, 3, [300.0, 3000.0], 31, gp=False, qp=False) == 0        # g == NULL: the arguments alone
    assert design(48000, 3, [300.0, 3000.0], 31, gp=False) == 0 and (q == 99).all()
    assert design(48000, 3, [300.0, 3000.0], 31) == 0 and (g != 77).any() and (q <= 20).all()


def test_check_and_null_arguments(cm):
    lib = cm.lib
    g = np.ones((2, 5), dtype=np.int16)
    assert cm.split_check(3, 5, g, [14, 20]) == 0
    assert cm.split_check(3, 5, np.full((2, 5), -32768), [14, 20]) == 0          # any int16 taps are valid
    assert cm.split_check(3, 5, g, [13, 20]) == cm.ERROR_INVAL and b"q[0]" in lib.cmhip_last_error()
    assert cm.split_check(3, 5, g, [14, 21]) == cm.ERROR_INVAL
    for bands, taps in ((1, 5), (9, 5), (3, 4), (3, 1), (3, 1025)):
        assert cm.split_check(bands, taps, g, [14, 14]) == cm.ERROR_INVAL
    assert cm.split_check(3, 5, None, [14, 14]) == cm.ERROR_FAULT
    assert cm.split_check(3, 5, g, None) == cm.ERROR_FAULT
    assert lib.cmhip_split_new(None, 48000, None) is None
    assert lib.cmhip_split_new_table(None, None, None) is None
    assert lib.cmhip_split_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_split_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_split_clips(None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_split_get_table(None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_split_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_split_delay(None) == 0 and lib.cmhip_split_hip_stream(None) is None
    lib.cmhip_split_free(None)
    # descriptors that are refused before any device is touched
    for kw in (dict(streams=0), dict(channels=0), dict(channels=17), dict(max_frames=0), dict(bands=1), dict(taps=4),
               dict(max_frames=2 ** 31 + 1)):
        f = dict(device=0, streams=2, channels=1, bands=3, taps=5, max_frames=64, hip_stream=None)
        f.update(kw)
        d = cm.SplitDesc(**f)
        q = np.array([14, 14], dtype=np.uint8)
        assert lib.cmhip_split_new_table(C.byref(d), g.ctypes.data, q.ctypes.data) is None, kw


def stop_band_db(tables, qs, j, f_edge, n=1 << 16):
    """the largest |H| of the cumulative low-pass sum_{b<=j} g_b / 2^q_b at and above f_edge, in dB"""
    l = sum(tables[b].astype(np.float64) / 2.0 ** int(qs[b]) for b in range(j + 1))
    H = np.abs(np.fft.rfft(l, n))
    f = np.arange(H.size) * RATE / n
    return 20.0 * np.log10(H[f >= f_edge].max() + 1e-300)


@pytest.mark.parametrize("bands", [2, 3, 8])
def test_stop_band_beats_a_fixed_scale(cm, bands):
    """recorded, not guessed: the stop band of each cumulative low-pass beyond f_j + 2.5 rate / (T-1) at T = 1023, for
    the library's tables (a scale per filter) and for the same filters quantised at q = 14 (DESIGN 4.17 quotes them)"""
    T = 1023
    g, q = cm.split_design(RATE, bands, TG.CROSSOVERS[bands], T)
    h = restated_h(RATE, TG.CROSSOVERS[bands], T)
    fixed = np.array([quantised(h[b], b, 14) for b in range(bands - 1)])
    for j, fj in enumerate(TG.CROSSOVERS[bands]):
        edge = fj + 2.5 * RATE / (T - 1)
        own = stop_band_db(g, q, j, edge)
        q14 = stop_band_db(fixed, [14] * (bands - 1), j, edge)
        print("B=%d T=%d low-pass %d (%.0f Hz): stop band %.1f dB with q=%s, %.1f dB at a fixed q=14"
              % (bands, T, j, fj, own, q[:j + 1].tolist(), q14))
        assert own < q14, (j, own, q14)


# ---------------------------------------------------------------------------
# the group compiler and the plan

def groups_of(mask_row, T):
    """group ends (taps) from a filter's mask words"""
    ends = [2 * (4 * j + p + 1) for j, w in enumerate(mask_row) for p in range(4) if (int(w) >> p) & 1]
    return ends + [T]


def test_groups_of_designed_and_extreme_tables(cm):
    tables = [cm.split_design(RATE, b, TG.CROSSOVERS[b], T) for b in (2, 3, 8) for T in (3, 31, 255, 1023)]
    tables += [TG.edge_tables("max", 1023), TG.edge_tables("one-group", 255), TG.edge_tables("one-group", 31)]
    for g, q in tables:
        pairs, masks, qs = cm.split_compile(g, q)
        nf, T = g.shape
        assert np.array_equal(qs, q)
        for b in range(nf):
            ends = groups_of(masks[b], T)
            lo = 0
            for hi in ends:
                assert hi > lo and (hi % 2 == 0 or hi == T)
                assert int(np.abs(g[b, lo:hi].astype(np.int64)).sum()) <= 65535
                lo = hi
            assert lo == T
            taps = np.zeros(pairs.shape[1] * 2, dtype=np.int64)
            taps[0::2] = (pairs[b] >> 16).astype(np.uint16).astype(np.int16)
            taps[1::2] = (pairs[b] & 0xffff).astype(np.uint16).astype(np.int16)
            assert np.array_equal(taps[:T], g[b]) and (taps[T:] == 0).all()
    _, masks, _ = cm.split_compile(*TG.edge_tables("max", 1023))
    assert len(groups_of(masks[0], 1023)) == 512                               # groups of two taps
    _, masks, _ = cm.split_compile(*TG.edge_tables("one-group", 255))
    assert all(len(groups_of(m, 255)) == 1 for m in masks)                     # sum |g| = 65535: one group
    g, q = cm.split_design(RATE, 2, [1000.0], 255)
    if q[0] == 14 and np.abs(g.astype(np.int64)).sum() <= 65535:
        assert len(groups_of(cm.split_compile(g, q)[1][0], 255)) == 1


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_group_compiler_over_random_tables(tmp_path):
    exe, r = _build_plan_test(tmp_path, "split_plan_test", [])                 # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "groups ok:" in out.stdout, out.stdout + out.stderr


def test_group_compiler_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "split_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "groups ok:" in out.stdout, out.stdout + out.stderr[-2000:]


def test_plan(cm):
    for ch in range(1, 17):
        p = cm.plan_split(5, ch, 3, 255, 1)
        assert (p.err, p.grid, p.block, p.chunks) == (0, 5, 256, 1)
        assert p.fast == (1 if ch <= 2 else 0) and p.tile_frames == (2048 // ch if ch <= 2 else 2048)
        assert p.tp == 256 and p.row == p.tile_frames + 256 + 8 and p.lds_bytes <= 64 * 1024
    p = cm.plan_split(7, 2, 8, 1023, 1025)
    assert (p.chunks, p.grid, p.tp) == (2, 14, 1024)
    assert cm.plan_split(1 << 20, 2, 3, 255, 1 << 21).err == 1


# ---------------------------------------------------------------------------
# the kernel's decomposition, emulated

GARBAGE = 23130                       # what LDS holds where nothing was staged


def wrap32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def wide(acc):
    return np.where(acc == -2 ** 31, 2 ** 31, acc)


def emulate_stream(cm, g, q, channels, hist, x, bug=None):
    """one stream's run as k_split.hip cuts it -> (int16 [B][F][C], clips [B], the new history [T-1][C])
    bug: a mistake made on purpose -- 'last_pair', 'first_tap', 'no_flush', 'hist_oldest', 'halo_short'"""
    nf, T = g.shape
    B = nf + 1
    x = np.asarray(x, dtype=np.int64).reshape(-1, channels)
    F = x.shape[0]
    pairs, masks, qs = cm.split_compile(g, q)
    plan = cm.plan_split(1, channels, B, T, max(F, 1))
    tile, Tp, row, HT, D = plan.tile_frames, plan.tp, plan.row, T - 1, (T - 1) // 2
    assert Tp == pairs.shape[1] * 2
    newer = (pairs >> 16).astype(np.uint16).astype(np.int16).astype(np.int64)
    older = (pairs & 0xffff).astype(np.uint16).astype(np.int16).astype(np.int64)
    lanes = tile // 8 if channels <= 2 else 256
    assert lanes * (2 if channels == 2 else 1) == 256
    y = np.zeros((B, F, channels), dtype=np.int64)
    clips = np.zeros(B, dtype=np.int64)
    h = np.array(hist, dtype=np.int64)
    if bug == "hist_oldest":
        h[0] = 0
    j = np.arange(lanes)
    i = np.arange(8)
    for k in range(-(-F // tile)):
        q0 = k * tile
        j_lo, jh = q0 - (Tp - 1), min(q0 + tile, F) - 1
        staged = jh - j_lo + 1
        for c in range(channels):
            P = np.full((2, row), GARBAGE, dtype=np.int64)             # copy A, and copy B one sample later
            fr = j_lo + np.arange(staged)
            val = np.zeros(staged, dtype=np.int64)
            inrun, inhist = fr >= 0, (fr < 0) & (fr >= -HT)
            if bug == "halo_short":
                inhist &= fr > -HT
            val[inrun] = x[fr[inrun], c]
            val[inhist] = h[HT + fr[inhist], c]
            P[0, :staged] = val
            P[1, 1:staged + 1] = val
            f0 = q0 + 8 * j
            valid = (f0[None, :] + i[:, None]) < F                     # [8][lanes]
            sel = np.broadcast_to((i & 1)[:, None], (8, lanes))
            base = (4 * j + Tp // 2 - 1)[None, :] + ((i + 1) // 2)[:, None]
            rsum = np.zeros((8, lanes), dtype=np.int64)

            def emit(b, r):
                yy = np.clip(r, -32768, 32767)
                clips[b] += int(((yy != r) & valid).sum())
                fi = (f0[None, :] + i[:, None])[valid]
                y[b, fi, c] = yy[valid]

            for b in range(nf):
                acc = np.zeros((8, lanes), dtype=np.int64)
                tot = np.zeros((8, lanes), dtype=np.int64)
                for kk in range(Tp // 2):
                    dw = base - kk
                    assert dw.min() >= 0 and 2 * dw.max() + 1 < row
                    lo, hi = P[sel, 2 * dw], P[sel, 2 * dw + 1]
                    t_new, t_old = newer[b, kk], older[b, kk]
                    if bug == "last_pair" and kk == (T - 1) // 2:
                        t_new = 0
                    if bug == "first_tap" and kk == 0:
                        t_new = 0
                    acc = wrap32(acc + lo * t_old + hi * t_new)
                    if (int(masks[b, kk // 4]) >> (kk % 4)) & 1 and bug != "no_flush":
                        tot += wide(acc)
                        acc = np.zeros_like(acc)
                tot += wide(acc)
                r = (tot + (1 << (int(qs[b]) - 1))) >> int(qs[b])
                rsum += r
                emit(b, r)
            at = (8 * j + Tp - 1 - D)[None, :] + i[:, None]
            emit(nf, P[0, at] - rsum)
    z = np.concatenate([np.array(hist, dtype=np.int64), x])
    return y.astype(np.int16), clips, z[z.shape[0] - HT:]


def emulate_case(cm, kind, T, bands, channels, designed=False, bug=None, runs=None):
    """-> True when the emulation equals the model over the case's runs, clip counters included"""
    g, q = (cm.split_design(RATE, bands, TG.CROSSOVERS[bands], T) if designed
            else TG.dense_case(kind, T, bands, 77 + T + bands))
    t = cm.plan_split(TG.S, channels, bands, T, 1).tile_frames
    models = [TG.Model(g, q, channels) for _ in range(TG.S)]
    hist = [np.zeros((T - 1, channels), dtype=np.int64) for _ in range(TG.S)]
    clips = np.zeros((TG.S, bands), dtype=np.int64)
    same = True
    for k, counts in enumerate(runs or TG.runs_for(t, T)):
        for s, n in enumerate(counts):
            x = (TG.noise(1000 * T + 10 * k + s, n, channels, scale=8192) if designed
                 else TG.edge_input(kind, g, 500 + 10 * k + s, n, channels))
            want = models[s].run(x)
            got, c, hist[s] = emulate_stream(cm, g, q, channels, hist[s], x, bug)
            clips[s] += c
            assert np.array_equal(hist[s], models[s].hist)
            same = same and np.array_equal(got, want)
    return same and np.array_equal(clips, np.array([m.clips for m in models]))


@pytest.mark.parametrize("kind,T,bands,channels", TG.DENSE)
def test_emulation_equals_the_model_on_dense_tables(cm, kind, T, bands, channels):
    assert emulate_case(cm, kind, T, bands, channels)


@pytest.mark.parametrize("T,bands,channels", [(3, 2, 1), (31, 8, 2), (255, 3, 1), (1023, 2, 2)])
def test_emulation_equals_the_model_on_designed_tables(cm, T, bands, channels):
    assert emulate_case(cm, None, T, bands, channels, designed=True)


@pytest.mark.parametrize("channels", [3, 16])
def test_emulation_of_the_any_channel_form(cm, channels):
    assert emulate_case(cm, "dense", 63, 3, channels, runs=[[5, 0, 2049]])


@pytest.mark.parametrize("bug", ["last_pair", "first_tap", "hist_oldest", "halo_short"])
def test_dense_tables_notice_mistakes_at_the_filters_ends(cm, bug):
    """... which a designed table whose outermost taps round to zero lets pass (the reason for dense tables)"""
    runs = [[300, 0, 7], [300, 9, 300]]
    assert not emulate_case(cm, "dense", 255, 3, 2, bug=bug, runs=runs)
    g, _ = cm.split_design(RATE, 2, TG.CROSSOVERS[2], 255)
    if (g[:, 0] == 0).all():
        assert emulate_case(cm, None, 255, 2, 2, designed=True, bug=bug, runs=runs)


def test_dense_tables_notice_a_missed_group_boundary(cm):
    runs = [[40, 0, 7], [300, 9, 300]]
    assert emulate_case(cm, "max", 255, 3, 1, runs=runs)
    assert not emulate_case(cm, "max", 255, 3, 1, bug="no_flush", runs=runs)
    assert emulate_case(cm, "min-pairs", 31, 2, 1, runs=runs)
    assert not emulate_case(cm, "min-pairs", 31, 2, 1, bug="no_flush", runs=runs)


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_split_desc_t d; int16_t g[3] = {0, 16384, 0}; uint8_t q[1] = {14}; double f[1] = {1000.0};\n"
           "uint32_t c[2]; d.device = 0; d.streams = d.channels = 1; d.bands = 2; d.taps = 3; d.max_frames = 1; d.hip_stream = 0;\n"
           "return cmhip_split_check(2, 3, g, q) + cmhip_split_design(48000, 2, f, 3, g, q, 3) + (cmhip_split_new(0, 48000, f) != 0)"
           " + (cmhip_split_new_table(0, g, q) != 0) + cmhip_split_run(0, 0, 0, 0, 0, 0, 0) + cmhip_split_reset(0, -1)"
           " + cmhip_split_clips(0, c, 0) + cmhip_split_get_table(0, g, q) + (int)cmhip_split_delay(0) + cmhip_split_sync(0)"
           " + (cmhip_split_hip_stream(0) != 0) + (cmhip_split_free(0), 0) + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_kernel_assembly_house_rules():
    """make asm produces build/k_split.s: it holds the three kernels and the dot instruction, no scalar load has a
    register AND an immediate offset (tests/test_abi.py tells why), and the mono / stereo kernels keep every register
    out of scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_split.s")).read()
    assert text.count(".amdhsa_kernel") == 3 and re.search(r"^\s*v_dot2\w*_i32_i16", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_split.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    fast = [n for n in scratch if "k_split_fast" in n]
    assert len(fast) == 2 and not [n for n in fast if scratch[n]], scratch
