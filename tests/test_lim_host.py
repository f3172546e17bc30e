"""CPU: the host side of the peak limiter (cmhip_lim_*): the header, cmhip_lim_check at its edges, NULL and descriptor
refusals, the launcher's plan (csrc/lim_plan.h) for every lookahead, hold and channel count and, as a stand-alone C++
program, plainly and under AddressSanitizer + UBSan; the kernel's division routine restated in numpy against `//` over
every pr for nine thresholds; an emulation of the kernels' decomposition (tiles, the halo from the history slot or the
previous tile, one sequence of 16-byte vectors across the seam, per-thread elements and the doubling passes, the
delayed samples out of two vectors, the history written by the last tile) at the plan's own tile against the model of
tests/test_gpu_lim.py; the model's own properties; and the generated assembly of k_lim.hip.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "lim_plan_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_lim", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MH = _load("test_limtp_host")      # the emulation of the tile that all three limiter kernel files instantiate
TG = MH.TG                         # tests/test_gpu_lim.py: the model, the signal and the dense cases of the GPU tests
UNITY = 32768


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_lim_desc_t d; uint32_t g[1]; unsigned int t, v; (void)sizeof(d);\n"
           "d.device = 0; d.streams = d.channels = 1; d.lookahead_log2 = 6; d.hold = 0; d.max_frames = 1; d.hip_stream = 0;\n"
           "return cmhip_lim_check(6, 0, 32767, 4096) + (cmhip_lim_new(0) != 0) + cmhip_lim_sync(0)"
           " + (cmhip_lim_hip_stream(0) != 0) + cmhip_lim_run(0, 0, 0, 0, 0, 0, 0) + cmhip_lim_set(0, -1, 1, 1)"
           " + cmhip_lim_get(0, 0, &t, &v) + cmhip_lim_reset(0, -1) + cmhip_lim_min_gain(0, g, 0)"
           " + (int)cmhip_lim_delay(0) + (cmhip_lim_free(0), 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check(cm):
    ok = cm.lim_check
    for a, want in ((2, cm.ERROR_INVAL), (3, 0), (9, 0), (10, cm.ERROR_INVAL)):
        assert ok(a, 0, 32767, 4096) == want, a
    for a in range(3, 10):
        assert ok(a, 2048 - (1 << a), 1, 1) == 0 and ok(a, 2049 - (1 << a), 1, 1) == cm.ERROR_INVAL       # A + H = 2048, 2049
    for T, want in ((0, cm.ERROR_INVAL), (1, 0), (32767, 0), (32768, cm.ERROR_INVAL)):
        assert ok(6, 0, T, 4096) == want, T
    for drive, want in ((0, cm.ERROR_INVAL), (1, 0), (65535, 0), (65536, cm.ERROR_INVAL)):
        assert ok(6, 0, 20000, drive) == want, drive
    assert b"lim:" in cm.lib.cmhip_last_error()
    assert ok(6, 0xffffffff, 1, 1) == cm.ERROR_INVAL and ok(0xffffffff, 0, 1, 1) == cm.ERROR_INVAL


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_lim_new(None) is None
    assert lib.cmhip_lim_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_lim_set(None, -1, 1, 1) == cm.ERROR_FAULT
    assert lib.cmhip_lim_get(None, 0, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_lim_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_lim_min_gain(None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_lim_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_lim_hip_stream(None) is None and lib.cmhip_lim_delay(None) == 0
    lib.cmhip_lim_free(None)
    # descriptors are refused before any device is touched
    for streams, channels, a, hold, frames in ((0, 2, 6, 0, 1024), (1, 0, 6, 0, 1024), (1, 17, 6, 0, 1024),
                                               (1, 2, 2, 0, 1024), (1, 2, 10, 0, 1024), (1, 2, 6, 1985, 1024),
                                               (1, 2, 9, 1537, 1024), (1, 2, 6, 0, 0), (1, 2, 6, 0, (1 << 30) + 1),
                                               (1, 16, 6, 0, (1 << 27) + 1), (1 << 20, 16, 6, 0, 1024)):
        d = cm.LimDesc(0, streams, channels, a, hold, frames, None)
        assert lib.cmhip_lim_new(C.byref(d)) is None, (streams, channels, a, hold, frames)
        assert b"lim_new" in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Limiter(streams, channels, a, hold, frames)


# ---------------------------------------------------------------------------
# The launcher's plan

def test_plan(cm):
    for a in range(3, 10):
        A = 1 << a
        for H in (0, 1, 2048 - A):
            hist = TG.geometry(a, H)[3]
            halo = (hist + 7) // 8 * 8
            for ch in range(1, 17):
                p = cm.plan_lim(5, ch, a, H, 1)                   # a one-frame run: one workgroup per stream
                assert (p.err, p.grid, p.chunks, p.block) == (0, 5, 1, 256), (a, H, ch)
                assert p.fast == (1 if ch <= 2 else 0)
                t = p.tile_frames
                assert t >= hist and t >= p.halo == halo and t <= 4096 and t & (t - 1) == 0
                assert p.lds_bytes == (t + halo) * 4 <= 65536    # what a workgroup may use without a raised limit
                assert t == 4096 or (2 * t + halo) * 4 > 65536   # the largest power of two that fits
                assert t + halo <= 256 * 26                      # the elements a thread keeps (k_lim.h: LIM_R)
                for frames in (1, t - 1, t, t + 1, 100000):
                    q = cm.plan_lim(3, ch, a, H, frames)
                    assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
    # no grid of 2^31 workgroups
    p = cm.plan_lim(1 << 20, 2, 6, 0, 1 << 23)                    # 2^20 streams x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_lim(1 << 20, 2, 6, 0, (1 << 23) - 4096)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    assert cm.plan_lim(0, 2, 6, 0, 100).grid == 0 and cm.plan_lim(4, 2, 6, 0, 0).grid == 0
    for ch, a, H in ((0, 6, 0), (17, 6, 0), (2, 2, 0), (2, 10, 0), (2, 6, 1985)):
        p = cm.plan_lim(4, ch, a, H, 100)
        assert p.grid == 0 and p.err == 0


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_as_a_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "lim_plan_test", [])                  # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"plans ok: \d{5,} geometries", out.stdout), out.stdout + out.stderr


def test_plan_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "lim_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "plans ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The division of k_lim.hip (lim_div) restated: a float estimate from a reciprocal, one correction step each way.
# v_rcp_f32 is within one ulp of the reciprocal; the form is run with the correctly rounded reciprocal and with its two
# float neighbours, which brackets whatever the instruction returns.

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
    pr = np.arange(T + 1, 524288 + 1, dtype=np.int64)
    num = T * 32768
    assert float(np.float32(num)) == num and float(np.float32(524288)) == 524288         # both exact as floats
    want = num // pr
    for nudge in (-1, 0, 1):
        assert np.array_equal(_lim_div(num, pr, nudge), want), (T, nudge)


# ---------------------------------------------------------------------------
# The decomposition of k_lim_fast<C> / k_lim_any (csrc/k_lim.hip): the one emulation of the tile
# (tests/test_limtp_host.py) with the sample detector, no release and these kernels' 26 slots per thread.

SLOTS = 26
UNWRITTEN = MH.UNWRITTEN


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("a,H,T,drive", TG.SETS)
def test_emulated_decomposition_equals_the_model(cm, a, H, T, drive, channels):
    p = cm.plan_lim(8, channels, a, H, 1)
    t, halo = p.tile_frames, p.halo
    xs, counts, ragged, full, unity, change, peak, gmin = TG.dense_case(a, H, T, drive, channels, t)
    assert TG.UNITY_SHARE[0] <= unity <= TG.UNITY_SHARE[1] and change >= TG.CHANGE_SHARE and peak == T
    for s in range(len(counts)):
        slot = np.zeros(halo * channels, dtype=np.int64)
        got_min = UNITY
        for x, want in ((xs[s][:counts[s]], ragged[s]), (xs[s], full[s])):
            out, slot, m = MH._emulate_run(0, x, slot, T, drive, a, H, 0, channels, t, halo, SLOTS)
            w = want.astype(np.int64).reshape(-1)
            assert np.array_equal(out[:w.size], w), (channels, s)
            assert (out[w.size:] == UNWRITTEN).all(), (channels, s)               # nothing past the stream's count
            got_min = min(got_min, UNITY if m is None else m)
        assert got_min == gmin[s]


# ---------------------------------------------------------------------------
# The model's own properties

@pytest.mark.parametrize("a,H,T,drive", TG.SETS)
def test_model_properties(a, H, T, drive):
    A, D, W, hist = TG.geometry(a, H)
    zero = np.zeros((hist, 2), dtype=np.int16)
    x = TG.bursts(42 + a, 3 * 4096, 2)
    y, s = TG.model_lim(x, zero, T, drive, a, H)
    assert np.abs(y.astype(np.int64)).max() == T                  # the ceiling is reached and never passed
    # cut-invariance: one run equals the same stream in runs of 1, 7, HIST - 1, HIST, HIST + 1, 0, 1000 and the rest
    h, pos, parts = zero, 0, []
    for n in (1, 7, hist - 1, hist, hist + 1, 0, 1000, x.shape[0]):
        part = x[pos:pos + n]
        parts.append(TG.model_lim(part, h, T, drive, a, H)[0])
        h = TG.next_hist(h, part)
        pos += part.shape[0]
    assert pos == x.shape[0] and np.array_equal(np.concatenate(parts), y)
    # below the threshold: a pure delay at unity drive, the rounded product otherwise
    q = (x.astype(np.int64) * 2000 // 32768).astype(np.int16)     # |q| <= 2000: below every set's T, also at drive 12345
    y, s = TG.model_lim(q, zero, T, 4096, a, H)
    assert (s == UNITY).all() and not y[:D].any() and np.array_equal(y[D:], q[:-D])
    y, s = TG.model_lim(q, zero, T, 12345, a, H)
    assert (s == UNITY).all() and np.array_equal(y[D:], ((q[:-D].astype(np.int64) * 12345 + 2048) >> 12))


def test_kernel_assembly_house_rules():
    """make asm produces build/k_lim.s: it holds the three kernels, the 64-bit multiply-add and the reciprocal, no
    scalar load has a register AND an immediate offset (tests/test_abi.py tells why; every workgroup indexes the
    parameter words with its stream), every kernel keeps its registers out of scratch memory, and the source has no
    build switches."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_lim.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_mad_i64_i32", text, flags=re.M)
    assert re.search(r"^\s*v_rcp_(iflag_)?f32", text, flags=re.M) and re.search(r"^\s*s_load_dword", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_lim.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    names = sorted(scratch)
    assert any("k_lim_fastILi1E" in k for k in names) and any("k_lim_fastILi2E" in k for k in names), names
    assert any("k_lim_any" in k for k in names) and any("k_lim_set" in k for k in names), names
    assert all(v == 0 for v in scratch.values()), scratch
    for name in ("k_lim.hip", "k_lim.h", "k_lim_tile.h"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        assert "getenv" not in src
        for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
            assert not re.findall(r"\bCMHIP_(?!K_LIM(?:_TILE)?_H\b)\w+", m.group(1)), m.group(0)
