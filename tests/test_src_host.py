"""CPU: the host side of sample-rate conversion (cmhip_src_*): the geometry and the designed tables, the response of
the int16 tables, the output counts, the launcher's plan, NULL and table refusals, the headers, and the generated
assembly of k_src.hip, and an emulation of the kernel's tile and lane decomposition against the model of the GPU
tests: on the designed tables at forced tile sizes, on the case list of tests/test_gpu_src.py at the plan's own, and
with three mistakes at the ends of the filter made on purpose, which the dense tables of the GPU tests notice.  The
reciprocal that replaces the division by L is checked for every L and every t the kernel can give it.  Nothing here
needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")

GEOMETRY = {(44100, 48000): (160, 147, 32), (48000, 44100): (147, 160, 64), (16000, 48000): (3, 1, 32),
            (48000, 16000): (1, 3, 96), (8000, 48000): (6, 1, 32), (48000, 8000): (1, 6, 192),
            (32000, 44100): (441, 320, 32), (44100, 32000): (320, 441, 64)}
# the 14 rate pairs the formula was prototyped on
PAIRS = [(44100, 48000), (48000, 44100), (16000, 48000), (48000, 16000), (8000, 48000), (48000, 8000), (32000, 44100),
         (44100, 32000), (22050, 48000), (11025, 48000), (96000, 48000), (48000, 96000), (32000, 48000), (48000, 32000)]


def _design(cm, rate_in, rate_out, h=None, cap=0):
    L, M, T = C.c_uint(7), C.c_uint(7), C.c_uint(7)
    rc = cm.lib.cmhip_src_design(rate_in, rate_out, C.byref(L), C.byref(M), C.byref(T),
                                 h.ctypes.data if h is not None else None, cap)
    return rc, (L.value, M.value, T.value)


def test_geometry(cm):
    for (ri, ro), want in GEOMETRY.items():
        assert _design(cm, ri, ro) == (0, want), (ri, ro)         # h == NULL: the geometry only
    for ri, ro in ((48000, 48000), (0, 48000), (48000, 0), (44100, 48001)):
        assert _design(cm, ri, ro) == (cm.ERROR_INVAL, (7, 7, 7)), (ri, ro)
    # a cap that is too small: INVAL, and nothing is written
    h = np.full(160 * 32, 77, dtype=np.int16)
    assert _design(cm, 44100, 48000, h, 160 * 32 - 1) == (cm.ERROR_INVAL, (7, 7, 7))
    assert (h == 77).all()
    assert _design(cm, 44100, 48000, h, 160 * 32) == (0, (160, 147, 32))
    assert (h != 77).any()
    assert cm.lib.cmhip_src_design(44100, 48000, None, None, None, None, 0) == 0          # nothing asked for
    L, M, T, H = cm.src_design(44100, 48000)
    assert (L, M, T) == (160, 147, 32) and H.shape == (160, 32) and np.array_equal(H.reshape(-1), h)


@pytest.mark.parametrize("rates", PAIRS)
def test_table_properties_and_response(cm, rates):
    L, M, T, H = cm.src_design(*rates)
    H = H.astype(np.int64)
    assert T == (32 if L > M else 32 * -(-M // L))
    assert (H.sum(axis=1) == 16384).all()                        # every phase sums to exactly unity
    sabs = int(np.abs(H).sum(axis=1).max())
    assert sabs <= 65535 and int(np.abs(H).max()) <= 32767
    # the response of the int16 table: the prototype h[k L + p] = H[p][k], at the high rate rate_in * L
    h = H.T.reshape(-1) / 16384.0 / L
    n = 65536
    assert h.size <= n
    mag = np.abs(np.fft.rfft(h, n))                              # (unity at 0: every phase sums to 16384)
    nyq_low = 0.5 / max(L, M)                                    # the lower rate's Nyquist, in cycles per high-rate sample
    f = np.arange(mag.size) / n
    db = 20 * np.log10(np.maximum(mag, 1e-12))
    pb = db[f <= 0.8 * nyq_low]
    sb = db[f >= 1.2 * nyq_low]
    at = db[int(round(nyq_low * n))]
    print("src table", rates, "L M T", (L, M, T), "max sum|H| %d max|H| %d passband %.4f..%.4f dB at Nyquist %.1f dB "
          "stopband %.1f dB" % (sabs, int(np.abs(H).max()), pb.min(), pb.max(), at, sb.max()))
    assert -0.1 <= pb.min() and pb.max() <= 0.1
    assert sb.max() <= -60.0


def test_out_frames_equal_a_brute_force_count(cm):
    for L, M in ((160, 147), (147, 160), (3, 2), (1, 6), (640, 147)):
        for F in (0, 1, 2, M - 1, M, M + 1, 1000):
            m = np.arange(0, (M + F) * L // M + 3, dtype=np.int64)
            n = m * M // L
            for r in range(M):
                want = int(((n >= r) & (n < r + F)).sum())
                got = cm.src_out_frames(L, M, r, F)
                assert got == want, (L, M, r, F)
                assert got <= F * L // M + 1
    # a whole period gives exactly L
    assert cm.src_out_frames(160, 147, 146, 147) == 160 and cm.src_out_frames(1, 6, 5, 6) == 1


def test_plan(cm):
    shapes = [(1, (160, 147, 32)), (2, (160, 147, 32)), (2, (147, 160, 64)), (6, (160, 147, 32)), (16, (1, 6, 192)),
              (1, (1, 6, 192)), (16, (320, 441, 64)), (2, (640, 1, 192)), (16, (1, 640, 192)), (2, (3, 2, 8)),
              (2, (320, 441, 64)), (2, (321, 441, 64))]
    shapes += sorted({(c.C, (c.L, c.M, c.T)) for c in TG.CASES} - set(shapes))       # what the GPU tests launch
    assert len(shapes) >= 26
    for C_, (L, M, T) in shapes:
        p = cm.plan_src(5, C_, L, M, T, 1)                       # a one-frame run: one workgroup per stream
        assert (p.err, p.grid, p.chunks, p.block) == (0, 5, 1, 256), (C_, L, M, T)
        assert p.fast == (1 if C_ <= 2 else 0)
        assert p.tile_out >= (2 if p.fast else 1) and p.tile_out & (p.tile_out - 1) == 0
        assert p.tile_in == (p.tile_out - 1) * M // L + (T + 7) // 8 * 8 + 1
        assert p.row % 2 == 0 and p.row > p.tile_in
        table = L * ((T + 7) // 8 * 8 + 8) * 2
        assert p.table_lds == (1 if table <= 45 * 1024 else 0)
        assert p.lds_bytes == (table if p.table_lds else 0) + 2 * C_ * p.row * 2
        assert p.lds_bytes <= 64 * 1024                          # what a workgroup may use without a raised limit
        for out in (p.tile_out - 1, p.tile_out, p.tile_out + 1, 100000):
            q = cm.plan_src(3, C_, L, M, T, out)
            assert (q.chunks, q.grid) == (-(-out // p.tile_out), 3 * -(-out // p.tile_out))
    # the bound of a table in LDS itself: 320 phases of 64 + 8 taps are exactly the 46080 bytes, 321 are above
    at, above = cm.plan_src(1, 2, 320, 441, 64, 1), cm.plan_src(1, 2, 321, 441, 64, 1)
    assert 320 * 72 * 2 == 46080 == 45 * 1024 and (at.table_lds, above.table_lds) == (1, 0)
    assert at.lds_bytes == 46080 + 2 * 2 * at.row * 2 and above.lds_bytes == 2 * 2 * above.row * 2
    p = cm.plan_src(8192, 1, 160, 147, 32, 71500)
    assert p.tile_out == 4096 and p.grid == 8192 * 18
    # no grid of 2^31 workgroups
    p = cm.plan_src(1 << 20, 1, 160, 147, 32, 1 << 23)           # 2^20 streams x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_src(1 << 20, 1, 160, 147, 32, (1 << 23) - 4096)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    assert cm.plan_src(0, 2, 160, 147, 32, 100).grid == 0 and cm.plan_src(4, 2, 160, 147, 32, 0).grid == 0
    assert cm.plan_src(0, 2, 160, 147, 32, 100).err == 0


# ---------------------------------------------------------------------------
# The decomposition of csrc/k_src.hip, step by step in Python, against the model of tests/test_gpu_src.py: the run
# counted from r, the tile's staged frames and its two copies of every plane, history before the run, the reciprocal
# division, the choice of copy by the parity of the plane index, the swapped tap pairs of the device table.  It holds
# the index arithmetic (every plane element a lane reads was written and lies inside its plane) where no GPU is.

def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_src_model", os.path.join(ROOT, "tests", "test_gpu_src.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # the model, the dense tables and the case list of the GPU tests
UNWRITTEN = 1 << 40
# in-bounds mistakes a kernel could make at the ends of the filter (the `fault` of _emulate_run)
FAULTS = ("oldest history frame read as zero", "later tiles take their history one frame too old",
          "last tap pair skipped")


def _emulate_run(L, M, T, H, C_, x, hist, r, tile_out, fault=None, trace=None):
    """x int16 [F][C], hist [C][T-1] -> (y [K][C], the next history, the next r), as the kernel computes them: the
    staging element by element, the lanes of a tile side by side.  fault: one of FAULTS.  trace: a list that gets
    (q0, j_lo, npre, staged, the largest t) per tile."""
    Tp = (T + 7) // 8 * 8
    tab = np.zeros((L, Tp + 8), dtype=np.int64)                  # SrcArgs::table
    tab[:, 0:T:2], tab[:, 1:T:2] = H[:, 1::2], H[:, 0::2]
    F = x.shape[0]
    ins = x.reshape(-1).astype(np.int64)
    kb = (r * L + M - 1) // M
    K = ((r + F) * L + M - 1) // M - kb
    tile_in = (tile_out - 1) * M // L + Tp + 1                   # plan_src
    row = (tile_in + 2) & ~1
    inv = 0 if L == 1 else ((1 << 32) + L - 1) // L
    out = np.zeros((K, C_), dtype=np.int64)
    kk = np.arange(Tp // 2, dtype=np.int64)                      # the tap pairs
    if fault == FAULTS[2]:
        kk = kk[kk != T // 2 - 1]
    for q0 in range(0, K, tile_out):                             # one workgroup each
        nq = min(tile_out, K - q0)
        b0, bl = (kb + q0) * M, (kb + q0 + nq - 1) * M
        n0 = b0 // L
        p0 = b0 - n0 * L
        jh = bl // L - r
        j_lo = (n0 - r) - (Tp - 1)
        staged = jh - j_lo + 1
        assert staged <= tile_in and jh < F
        pl = np.full(2 * C_ * row, UNWRITTEN, dtype=np.int64)
        npre = min(staged, -j_lo) if j_lo < 0 else 0
        for idx in range(npre * C_):
            i, c = divmod(idx, C_)
            j = j_lo + i
            at = T - 1 + j
            if fault == FAULTS[1] and q0 > 0:
                at = max(at - 1, 0)
            val = hist[c][at] if j >= -(T - 1) else 0
            if fault == FAULTS[0] and j == -(T - 1):
                val = 0
            pl[c * row + i] = pl[(C_ + c) * row + i + 1] = val
        if staged > npre:
            jb = max(j_lo, 0)
            for v in range((jb * C_) >> 3, ((jh + 1) * C_ + 7) >> 3):
                for i in range(8):
                    e = v * 8 + i
                    j, c = divmod(e, C_)
                    if jb <= j <= jh:
                        assert e < F * C_                        # (never a sample past the stream's count)
                        pos = j - j_lo
                        pl[c * row + pos] = pl[(C_ + c) * row + pos + 1] = ins[e]
        t = p0 + np.arange(nq, dtype=np.int64) * M               # the lanes
        assert t[-1] < 1 << 22
        dn = (t * inv) >> 32 if inv else t
        p = t - dn * L
        assert (dn == t // L).all() and (0 <= p).all() and (p < L).all()
        a0 = dn + Tp - 1
        off = 2 * ((a0 >> 1)[:, None] - kk[None, :])             # [nq][pairs] inside the plane
        assert off.min() >= 0 and off.max() + 1 < row
        klo, khi = tab[p[:, None], 2 * kk[None, :]], tab[p[:, None], 2 * kk[None, :] + 1]
        for c in range(C_):
            at = (np.where(a0 & 1, c, C_ + c) * row)[:, None] + off
            lo, hi = pl[at], pl[at + 1]
            assert (lo != UNWRITTEN).all() and (hi != UNWRITTEN).all(), (q0, c)
            out[q0:q0 + nq, c] = np.clip(((lo * klo + hi * khi).sum(axis=1) + 8192) >> 14, -32768, 32767)
        if trace is not None:
            trace.append((q0, j_lo, npre, staged, int(t[-1])))
    nh = np.zeros((C_, T - 1), dtype=np.int64)                   # src_history
    for c in range(C_):
        for i in range(T - 1):
            nh[c][i] = hist[c][i + F] if F + i < T - 1 else ins[(F - (T - 1) + i) * C_ + c]
    return out, nh, (r + F) % M


@pytest.mark.parametrize("rates,channels,tile_out", [((44100, 48000), 1, 64), ((44100, 48000), 2, 32),
                                                     ((48000, 44100), 2, 16), ((8000, 48000), 3, 256),
                                                     ((48000, 8000), 2, 2), ((48000, 16000), 16, 4)])
def test_emulated_decomposition_equals_the_model(cm, rates, channels, tile_out):
    tg = TG
    L, M, T, H = cm.src_design(*rates)
    H = H.astype(np.int64)
    model = tg.Model(L, M, H, channels)
    hist, r = np.zeros((channels, T - 1), dtype=np.int64), 0
    for F in (0, 1, 5, T - 2, T - 1, T, 150, 0, 333, M, M + 1):
        x = tg.noise(F + channels, F, channels)
        want = model.run(x)
        got, hist, r = _emulate_run(L, M, T, H, channels, x, hist, r, tile_out)
        assert r == model.r and np.array_equal(hist.T, model.hist)
        assert np.array_equal(got, want.astype(np.int64)), (rates, channels, F)


def _emulate_case(cm, case, tile_out, H, fault=None):
    """every stream of a case through the emulation and the model -> (the tiles (run, stream, first, j_lo, t_hi) and
    (npre, staged) of each, the streams' runs that differ from the model, outputs, saturated outputs of the model)"""
    tiles, parts, differ, outputs, saturated = [], [], [], 0, 0
    for s in range(len(case.runs[0])):
        model = TG.Model(case.L, case.M, H, case.C)
        hist, r = np.zeros((case.C, case.T - 1), dtype=np.int64), 0
        for i, counts in enumerate(case.runs):
            x = TG.noise(1000 * i + 10 * case.C + s, counts[s], case.C)
            want = model.run(x).astype(np.int64)
            trace = []
            got, hist, r = _emulate_run(case.L, case.M, case.T, H, case.C, x, hist, r, tile_out, fault, trace)
            assert r == model.r and np.array_equal(hist.T, model.hist)
            if not np.array_equal(got, want):
                differ.append((i, s))
            tiles += [(i, s, q0 == 0, j_lo, t_hi) for q0, j_lo, _, _, t_hi in trace]
            parts += [(q0, npre, staged) for q0, _, npre, staged, _ in trace]
            outputs += want.size
            saturated += int(((want == 32767) | (want == -32768)).sum())
    return tiles, parts, differ, outputs, saturated


@pytest.mark.parametrize("case", TG.CASES, ids=[c.name for c in TG.CASES])
def test_cases_of_the_gpu_tests_emulated(cm, case):
    """the runs tests/test_gpu_src.py launches, at the plan's own tile_out: each reaches what it is there for, every
    plane element read was written and lies inside its plane, and the outputs are the model's"""
    plan, recs = TG.assert_reaches(cm, case)
    H = TG.case_table(cm, case).astype(np.int64)
    tiles, parts, differ, outputs, saturated = _emulate_case(cm, case, plan.tile_out, H)
    assert not differ, differ
    # the emulation met the tiles the host arithmetic of the GPU test announces
    assert sorted(tiles) == sorted((t.run, t.stream, t.first, t.j_lo, t.t_hi) for t in recs)
    if "mix" in case.reach:
        assert any(q0 > 0 and 0 < npre < case.T - 1 and npre < staged for q0, npre, staged in parts)
    if "halo" in case.reach:
        assert any(q0 > 0 and npre > 0 for q0, npre, _ in parts)
    if case.table == "dense":
        assert saturated < TG.SATURATED_MAX * outputs


@pytest.mark.parametrize("geometry,rates,tile_out,counts", [
    ((1, 6, 192), (48000, 8000), 2, (252, 1, 0, 333)), ((147, 160, 64), (48000, 44100), 16, (150, 1, 0, 333)),
    ((160, 1, 32), (300, 48000), None, (60, 1, 0, 60))])
def test_dense_tables_see_what_designed_tables_do_not(cm, geometry, rates, tile_out, counts):
    """Three in-bounds mistakes at the ends of the filter, made in the emulation: with a dense table each of them
    changes the output, so a kernel that made one would fail the GPU tests; whether the designed table of the same
    geometry notices is printed.  (1, 6, 192) and (147, 160, 64) at forced small tiles, so that tiles after a run's
    first stage history at all; (160, 1, 32) at the plan's 4096, where the second tile does.  A run begins at a
    multiple of M after the history has filled, so that its first output meets the oldest history frame."""
    L, M, T = geometry
    tables = {"dense": TG.dense_table(L, T, L + T).astype(np.int64),
              "designed": cm.src_design(*rates)[3].astype(np.int64)}
    assert cm.src_design(*rates)[:3] == geometry
    case = TG._case("faults", geometry, 2, [[n] for n in counts])
    tile_out = tile_out or cm.plan_src(1, 2, L, M, T, 1).tile_out
    for name, H in tables.items():
        tiles, parts, differ, _, _ = _emulate_case(cm, case, tile_out, H)
        assert not differ and any(q0 > 0 and npre > 0 for q0, npre, _ in parts)
        assert any(run > 0 and j_lo == -(T - 1) for run, _, _, j_lo, _ in tiles)       # the oldest history frame, full
        for fault in FAULTS:
            differ = _emulate_case(cm, case, tile_out, H, fault)[2]
            print("src fault", geometry, name, "table:", fault, "->", "noticed" if differ else "NOT noticed")
            if name == "dense":
                assert differ, fault


def test_src_divmod_is_exact_for_every_l_below_2_22():
    """src_divmod's t * inv >> 32 with inv = ceil(2^32 / L), for every L the library takes: right at every multiple
    of L and just below it, and monotone in t -- so right for every t < 2^22"""
    for L in range(2, 641):
        inv = np.uint64(((1 << 32) + L - 1) // L)
        assert int(inv) < 1 << 32                                # (the kernel multiplies 32 bits by 32 bits)
        k = np.arange(1, -(-(1 << 22) // L), dtype=np.uint64)
        t = k * np.uint64(L)
        assert int(t[-1]) < 1 << 22 <= int(t[-1]) + L
        assert np.array_equal((t * inv) >> np.uint64(32), k), L
        assert np.array_equal(((t - np.uint64(1)) * inv) >> np.uint64(32), k - np.uint64(1)), L


def test_headers_compile_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_src_desc_t d; unsigned int L, M, T; int16_t h[64]; (void)sizeof(d);\n"
           "if (cmhip_src_design(8000, 48000, &L, &M, &T, h, 64)) return 1;\n"
           "return (int)cmhip_src_out_frames(L, M, 0, 10) + (cmhip_src_new(0) != 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_null_arguments_and_table_refusals(cm):
    lib = cm.lib
    u = C.c_uint()
    assert lib.cmhip_src_new(None) is None
    assert lib.cmhip_src_new_table(None, 3, 2, 4, None) is None
    assert lib.cmhip_src_geometry(None, C.byref(u), C.byref(u), C.byref(u)) == cm.ERROR_FAULT
    assert lib.cmhip_src_run(None, None, 0, 0, None, None, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_src_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_src_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_src_max_out_frames(None) == 0 and lib.cmhip_src_hip_stream(None) is None
    lib.cmhip_src_free(None)
    assert cm.src_out_frames(0, 0, 0, 10) == 0
    # tables are refused before any device is touched
    d = cm.SrcDesc(0, 1, 1, 44100, 48000, 1024, None)

    def refused(L, M, h):
        h = np.ascontiguousarray(h, dtype=np.int16)
        got = lib.cmhip_src_new_table(C.byref(d), L, M, h.shape[1], h.ctypes.data)
        return got is None and b"src" in lib.cmhip_last_error()

    good = [[32767, -32767, 1, 0], [-32767, 1, 32767, 0], [16384, 16383, -16384, -16384]]
    over = [row[:] for row in good]
    over[1][3] = 1                                               # sum |h| = 65536
    assert refused(3, 2, over)
    assert refused(3, 2, [row[:3] for row in good])              # odd T
    assert refused(3, 2, np.zeros((3, 194)))                     # T = 194
    assert refused(3, 3, good)                                   # L == M
    assert refused(641, 2, np.zeros((641, 4))) and refused(2, 641, np.zeros((2, 4))) and refused(0, 2, np.zeros((1, 4)))
    assert lib.cmhip_src_new_table(C.byref(d), 3, 2, 4, None) is None
    bad = cm.SrcDesc(0, 1, 17, 44100, 48000, 1024, None)
    h = np.asarray(good, dtype=np.int16)
    assert lib.cmhip_src_new_table(C.byref(bad), 3, 2, 4, h.ctypes.data) is None
    bad = cm.SrcDesc(0, 1, 1, 48000, 48000, 1024, None)          # the designed form: equal rates
    assert lib.cmhip_src_new(C.byref(bad)) is None


def test_kernel_assembly_house_rules():
    """make asm produces build/k_src.s: no scalar load with a register AND an immediate offset (tests/test_abi.py
    tells why), the dot instruction is the one the design counts, and the mono / stereo kernels keep every register
    out of scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_src.s")).read()
    assert ".amdhsa_kernel" in text and "v_dot2c_i32_i16" in text
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_src.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_src_fast" in k}
    assert len(fast) == 2 and any("k_src_any" in k for k in scratch), sorted(scratch)
    assert all(v == 0 for v in fast.values()), fast
    src = open(os.path.join(PKG, "csrc", "k_src.hip")).read()
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_\w+", m.group(1)), m.group(0)
