"""CPU: the host side of the mixer's matrix ramps (cmhip_mix_ramp_*): the header, the two specification functions
against the numpy model of tests/test_gpu_mix_ramp.py over whole ramps, the properties the header states (end point,
monotone, distance from the ideal line, truncation is not a floor shift, the row bound), NULL and range refusals
without a device, the mirror (csrc/mix_ramp.h) driven by a stand-alone C++ program plainly and under sanitizers, an
emulation of both kernels' decomposition at the plan's own tile, and the generated assembly of k_mixramp.hip.  Nothing
here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
MIRROR_SRC = os.path.join(ROOT, "tests", "cpp", "mix_ramp_test.cpp")


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_mix_ramp_model",
                                                  os.path.join(ROOT, "tests", "test_gpu_mix_ramp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TR = _gpu_test_module()            # the model of the GPU tests (and, through it, tests/test_gpu_mix.py's helpers)


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){int16_t w[4] = {0, 0, 0, 0}; uint32_t done, of;\n"
           "if (cmhip_mix_ramp_position(1, 2) != 16384u || cmhip_mix_ramp_weight(0, 16384, 16384) != 8192) return 1;\n"
           "return cmhip_mix_ramp_matrix(0, -1, w, 480) + cmhip_mix_ramp_state(0, 0, &done, &of, w)"
           " + cmhip_mix_ramp_state(0, 0, &done, &of, 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


# ---------------------------------------------------------------------------
# the specification as code against the numpy formula

RAMPS = [2, 3, 5, 7, 8, 63, 64, 100, 480, 1000, 4800, 32768, 32769, 48000, 65536, 100000, 1 << 20]


@pytest.mark.parametrize("R", RAMPS)
def test_position_every_frame(cm, R):
    f = cm.lib.cmhip_mix_ramp_position
    n = np.arange(R + 1, dtype=np.int64)
    got = np.fromiter((f(i, R) for i in range(R + 1)), dtype=np.int64, count=R + 1)
    inc = -(-(1 << 32) // R)
    assert inc <= 1 << 31
    assert np.array_equal(got, np.minimum(32768, (n * inc) >> 17))               # the formula, written out again
    assert np.array_equal(got, TR.ramp_position(n, R))
    assert got[0] == 0 and got[R] == 32768                                       # start and end point
    assert (np.diff(got) >= 0).all()                                             # monotone
    assert np.abs(got - (32768 * n) // R).max() <= 1                             # at most 1 from the ideal line
    assert f(R + 1, R) == 32768 and f(0xffffffff, R) == 32768                    # past the ramp: its end


def test_position_outside_the_range(cm):
    f = cm.lib.cmhip_mix_ramp_position
    assert [f(0, 0), f(1, 0), f(0, 1), f(1, 1), f(5, 1)] == [0, 32768, 0, 32768, 32768]       # a step
    assert cm.mix_ramp_position(240, 480) == 16384 and cm.mix_ramp_weight(16384, 0, 16384) == 8192


def _pairs():
    rng = np.random.default_rng(77)
    edge = [32767, -32768, 0, 1, -1, -32767, 16384, -16384]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(-8191, 8000), (8000, -8191), (12345, -12345)]
    pairs += [tuple(int(v) for v in rng.integers(-32768, 32768, size=2)) for _ in range(140)]
    return pairs


def test_weight_every_position(cm):
    f = cm.lib.cmhip_mix_ramp_weight
    p = np.arange(32769, dtype=np.int64)
    pairs = _pairs()
    assert len(pairs) > 200
    for w0, w1 in pairs:
        want = TR.ramp_weight(w0, w1, p)
        N = w0 * (32768 - p) + w1 * p
        assert np.array_equal(want, np.trunc(N / 32768).astype(np.int64))        # towards zero (exact in doubles)
        assert want[0] == w0 and want[-1] == w1                                  # start and end
        d = np.diff(want)
        assert (d >= 0).all() if w1 >= w0 else (d <= 0).all()                    # monotone
        got = np.fromiter((f(w0, w1, i) for i in range(32769)), dtype=np.int64, count=32769)
        assert np.array_equal(got, want), (w0, w1)
        assert f(w0, w1, 32769) == w1 and f(w0, w1, 0xffffffff) == w1
    for w in (32767, -32768, 0, -1234):                                          # constant
        assert (TR.ramp_weight(w, w, p) == w).all()
    # not a floor shift: where N is negative and not a multiple of 32768 the two differ
    N = -8191 * (32768 - p) + 8000 * p
    differ = TR.ramp_weight(-8191, 8000, p) != (N >> 15)
    assert 0.45 < differ.mean() < 0.55 and not differ[N >= 0].any()


def test_the_row_bound():
    """2000 random row pairs at sum |w| = 65535: every position's row stays within it; floor and round-to-nearest do not"""
    rng = np.random.default_rng(78)
    p = np.arange(0, 32769, 7, dtype=np.int64)[:, None]
    worst = {"trunc": 0, "floor": 0, "round": 0}

    def row(ci):
        cut = np.sort(rng.integers(0, 65536, size=ci - 1))
        mag = np.diff(np.concatenate([[0], cut, [65535]]))
        while mag.max() > 32767:                                 # (an int16 entry)
            i, j = mag.argmax(), mag.argmin()
            mag[j] += mag[i] - 32767
            mag[i] = 32767
        return mag * rng.choice([-1, 1], size=ci)

    for _ in range(2000):
        ci = int(rng.integers(3, 17))
        w0, w1 = row(ci), row(ci)
        assert np.abs(w0).sum() == 65535 == np.abs(w1).sum()
        N = w0[None] * (32768 - p) + w1[None] * p
        worst["trunc"] = max(worst["trunc"], int(np.abs(TR.ramp_weight(w0[None], w1[None], p)).sum(axis=1).max()))
        worst["floor"] = max(worst["floor"], int(np.abs(N >> 15).sum(axis=1).max()))
        worst["round"] = max(worst["round"], int(np.abs((N + 16384) >> 15).sum(axis=1).max()))
    print("row sums at most:", worst)
    assert worst["trunc"] <= 65535 < worst["floor"] and worst["round"] > 65535


def test_null_and_range_refusals_without_a_device(cm):
    lib = cm.lib
    w = np.zeros(4, dtype=np.int16)
    a, b = C.c_uint32(77), C.c_uint32(77)
    assert lib.cmhip_mix_ramp_matrix(None, -1, w.ctypes.data, 480) == cm.ERROR_FAULT
    assert lib.cmhip_mix_ramp_matrix(None, -1, None, 480) == cm.ERROR_FAULT
    assert lib.cmhip_mix_ramp_state(None, 0, C.byref(a), C.byref(b), w.ctypes.data) == cm.ERROR_FAULT
    assert (a.value, b.value) == (77, 77) and b"mix_ramp" in lib.cmhip_last_error()
    for name in ("cmhip_mix_ramp_matrix", "cmhip_mix_ramp_state", "cmhip_mix_ramp_position", "cmhip_mix_ramp_weight"):
        assert name in cm.SIGNATURES
    header = open(os.path.join(ROOT, "include", "coolmic_hip.h")).read()
    assert "truncated TOWARDS ZERO" in header and "ceil(2^32 / R)" in header


# ---------------------------------------------------------------------------
# the mirror: csrc/mix_ramp.h under a stand-alone program

def _build_mirror_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        MIRROR_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_mirror_over_random_sequences(tmp_path):
    exe, r = _build_mirror_test(tmp_path, "mix_ramp_test", [])                   # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ramps ok: 2000 sequences" in out.stdout, out.stdout + out.stderr


def test_mirror_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_mirror_test(tmp_path, "mix_ramp_san",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "ramps ok: 2000 sequences" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The decomposition of the two ramp kernels (csrc/k_mixramp.hip), step by step in Python, with the device's own
# integer steps: the position from n clamped to R, a 64-bit product and a shift; an entry by two products and the
# add-32767-to-negatives arithmetic shift; the uniform choice per tile between the ramp path and the plain one with the
# target.  k_mixr_fast: a lane's units and vectors, one dot per output sample on the dword that holds the frame, with
# mono input the frame's weight in the half its frame sits in.  k_mixr_any: 16-byte vectors staged into pair planes, one
# thread per frame computing every weight dword of its frame, the staged output tile.  The rehearsal before GPU time.
# With no ramp running (done = R = 0, both matrices the stream's own) these are the decompositions of k_mix.hip's two
# kernels: tests/test_mix_host.py calls them so.

UNWRITTEN = 1 << 40


def _dev_pos(n, R, inc):
    q = min(n, R) * inc
    assert q < (1 << 32) + R                                     # the shifted product fits 32 bits
    return min(q >> 17, 32768)


def _dev_w(w0, w1, p):
    N = w0 * (32768 - p) + w1 * p
    assert abs(N) <= 1 << 30
    return (N + ((N >> 31) & 32767)) >> 15


def _load_vectors(ins, ns, v, ragged_ok, past_ok):
    vec = np.zeros(8, dtype=np.int64)                            # load_vec: whole, the ragged end zero padded, or zeros
    if v < ns // 8:
        vec[:] = ins[v * 8:v * 8 + 8]
    elif v == ns // 8 and ns % 8:
        assert ragged_ok
        vec[:ns % 8] = ins[v * 8:]
    else:
        assert past_ok                                           # zeros: nothing past the count is read
    return vec


def _kernel_form(W):
    """(low, high) halves of the kernel form's dwords: dword k of row o is W[o][2k] | W[o][2k+1] << 16, an odd C_in
    padded with zero"""
    co, ci = W.shape
    cp = (ci + 1) // 2
    lo, hi = np.zeros((co, cp), dtype=np.int64), np.zeros((co, cp), dtype=np.int64)
    lo[:, :] = W[:, 0::2]
    hi[:, :ci // 2] = W[:, 1::2]
    return lo, hi


def _emulate_fast(x, w0, w1, done, R):
    co, ci = w0.shape
    uf = 8 // min(ci, co)
    vi, vo = uf * ci // 8, uf * co // 8
    nu = 4 // max(vi, vo)
    tile = 64 * nu * uf
    inc = -(-(1 << 32) // R) if R else 0
    F = x.shape[0]
    ins = x.reshape(-1).astype(np.int64)
    ns_in, ns_out = F * ci, F * co
    outs = np.full(F * co + 13, UNWRITTEN, dtype=np.int64)
    paths = set()
    for k in range(-(-F // tile)):                               # one wave each
        full = (k + 1) * tile <= F
        ramp = done + k * tile < R                               # (uniform)
        paths.add(ramp)
        for lane in range(64):
            for j in range(nu):
                u = k * 64 * nu + 64 * j + lane
                dwords = []
                for i in range(vi):
                    vec = _load_vectors(ins, ns_in, u * vi + i, not full, not full)
                    dwords += [(vec[2 * d], vec[2 * d + 1]) for d in range(4)]
                wf = []                                          # per frame and row: (weight of the low, the high half)
                for f in range(uf):
                    p = _dev_pos(done + u * uf + 1 + f, R, inc) if ramp else 32768
                    rows = []
                    for oc in range(co):
                        w = [_dev_w(int(w0[oc, c]), int(w1[oc, c]), p) if ramp else int(w1[oc, c]) for c in range(ci)]
                        rows.append((w[0], w[1]) if ci == 2 else ((0, w[0]) if f & 1 else (w[0], 0)))
                    wf.append(rows)
                for i in range(vo):
                    o8 = np.zeros(8, dtype=np.int64)
                    for e in range(i * 8, i * 8 + 8):            # output sample of the unit
                        f, oc = divmod(e, co)
                        lo, hi = dwords[(f * ci) >> 1]
                        wlo, whi = wf[f][oc]
                        o8[e - i * 8] = min(max((8192 + lo * wlo + hi * whi) >> 14, -32768), 32767)
                    v = u * vo + i
                    if v < ns_out // 8:
                        outs[v * 8:v * 8 + 8] = o8
                    elif v == ns_out // 8 and ns_out % 8:
                        assert not full
                        outs[v * 8:v * 8 + ns_out % 8] = o8[:ns_out % 8]
    return outs, tile, paths


def _emulate_any(x, w0, w1, done, R, tile):
    co, ci = w0.shape
    cp = (ci + 1) // 2
    inc = -(-(1 << 32) // R) if R else 0
    F = x.shape[0]
    ins = x.reshape(-1).astype(np.int64)
    ns_in, ns_out = F * ci, F * co
    k0, k1 = _kernel_form(w0), _kernel_form(w1)
    outs = np.full(F * co + 13, UNWRITTEN, dtype=np.int64)
    paths = set()
    for f0 in range(0, F, tile):                                 # one workgroup each
        nt = min(tile, F - f0)
        ramp = done + f0 < R                                     # (uniform)
        paths.add(ramp)
        plo = np.full((cp, tile), UNWRITTEN, dtype=np.int64)
        phi = np.full((cp, tile), UNWRITTEN, dtype=np.int64)
        assert (f0 * ci) % 8 == 0 and (f0 * co) % 8 == 0
        vb, nv = f0 * ci // 8, (nt * ci + 7) // 8
        for w in range(nv):
            vec = _load_vectors(ins, ns_in, vb + w, True, False)     # whole, or the ragged end: none past it
            if ci % 2 == 0:
                for i in range(4):
                    f, k = divmod(w * 4 + i, cp)
                    if f < nt:
                        plo[k, f], phi[k, f] = vec[2 * i], vec[2 * i + 1]
            else:
                for i in range(8):
                    f, c = divmod(w * 8 + i, ci)
                    if f < nt:
                        (phi if c & 1 else plo)[c >> 1, f] = vec[i]
        ot = np.full(tile * co, UNWRITTEN, dtype=np.int64)
        for f in range(nt):                                      # the threads
            lo, hi = plo[:, f], phi[:, f].copy()
            assert (lo != UNWRITTEN).all()
            if ci % 2:
                assert hi[cp - 1] == UNWRITTEN and not k0[1][:, cp - 1].any() and not k1[1][:, cp - 1].any()
                hi[cp - 1] = 12345                               # whatever LDS held: it meets a zero weight
            assert (hi != UNWRITTEN).all()
            p = _dev_pos(done + f0 + f + 1, R, inc) if ramp else 32768
            for o in range(co):
                acc = 8192
                for kk in range(cp):
                    if ramp:
                        wlo = _dev_w(int(k0[0][o, kk]), int(k1[0][o, kk]), p)
                        whi = _dev_w(int(k0[1][o, kk]), int(k1[1][o, kk]), p)
                    else:
                        wlo, whi = int(k1[0][o, kk]), int(k1[1][o, kk])
                    if ci % 2 and kk == cp - 1:
                        assert whi == 0
                    acc += int(lo[kk]) * wlo + int(hi[kk]) * whi
                ot[f * co + o] = min(max(acc >> 14, -32768), 32767)
        vb, nv = f0 * co // 8, (nt * co + 7) // 8
        for w in range(nv):
            v = vb + w
            if v < ns_out // 8:
                outs[v * 8:v * 8 + 8] = ot[w * 8:w * 8 + 8]
            elif v == ns_out // 8:
                outs[v * 8:v * 8 + ns_out % 8] = ot[w * 8:w * 8 + ns_out % 8]
    return outs, paths


def _cases(t):
    """(frames, done, R): a tile inside the ramp, one in which it ends and one behind it; a ramp that ended inside the
    first tile; one carried from an earlier run; no ramp; ragged counts"""
    return [(2 * t + 13, 0, t + 300), (t - 1, 0, 7), (t + 1, 123, 50000), (9, 0, 2), (t, 0, 0), (1, 6, 7), (0, 3, 9),
            (7, 99, 100)]


@pytest.mark.parametrize("ci,co", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_emulated_fast_forms_equal_the_model(cm, ci, co):
    t = cm.plan_mix(1, ci, co, 1).tile_frames
    seen = set()
    for s, (F, done, R) in enumerate(_cases(t)):
        w0 = TR.dense_matrix(ci, co, 9500 + 10 * ci + co + s).astype(np.int64)
        w1 = TR.dense_matrix(ci, co, 9700 + 10 * ci + co + s).astype(np.int64)
        x = TR.noise(9600 + s, F, ci)
        mod = TR.RampModel(w1)
        mod.w0, mod.done, mod.R = w0, done, R
        want = mod.run(x).astype(np.int64).reshape(-1)
        got, tile, paths = _emulate_fast(x, w0, w1, done, R)
        seen |= paths
        assert tile == t
        assert np.array_equal(got[:want.size], want), (ci, co, F, done, R)
        assert (got[want.size:] == UNWRITTEN).all(), (ci, co, F)                 # nothing past the stream's count
    assert seen == {True, False}


@pytest.mark.parametrize("ci,co", [(3, 2), (6, 2), (5, 3), (16, 16)])
def test_emulated_decomposition_equals_the_model(cm, ci, co):
    p = cm.plan_mix(1, ci, co, 1)
    assert p.fast == 0
    t = p.tile_frames
    seen = set()
    for s, (F, done, R) in enumerate(_cases(t)):
        w0 = TR.dense_matrix(ci, co, 9000 + 10 * ci + co + s).astype(np.int64)
        w1 = TR.dense_matrix(ci, co, 9200 + 10 * ci + co + s).astype(np.int64)
        x = TR.noise(9100 + s, F, ci)
        mod = TR.RampModel(w1)
        mod.w0, mod.done, mod.R = w0, done, R
        want = mod.run(x).astype(np.int64).reshape(-1)
        got, paths = _emulate_any(x, w0, w1, done, R, t)
        seen |= paths
        assert np.array_equal(got[:want.size], want), (ci, co, F, done, R)
        assert (got[want.size:] == UNWRITTEN).all(), (ci, co, F)
    assert seen == {True, False}


def test_ramp_lds_fits_at_the_plans_tile(cm):
    """the ramp kernel keeps W0 and W1 beside the target at the plain kernel's tile: still within 64 KiB, every pair"""
    for ci in range(1, 17):
        for co in range(1, 17):
            p = cm.plan_mix(1, ci, co, 1)
            if not p.fast:
                extra = 8 * ((co * ((ci + 1) // 2) + 3) // 4 * 4)
                assert p.lds_bytes + extra <= 65536, (ci, co)


def test_kernel_assembly_house_rules():
    """make asm produces build/k_mixramp.s: it holds kernels and the dot instruction, no scalar load has a register AND
    an immediate offset (tests/test_abi.py tells why), and the four mono / stereo kernels keep every register out of
    scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_mixramp.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_dot2\w*_i32_i16", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_mixramp.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_mixr_fast" in k}
    assert len(fast) == 4 and any("k_mixr_any" in k for k in scratch), sorted(scratch)
    assert all(v == 0 for v in fast.values()), fast
    assert not [k for k in scratch if "k_mix_fast" in k or "k_mix_any" in k]     # (tests/test_mix_host.py counts those)
    src = "".join(open(os.path.join(PKG, "csrc", f)).read() for f in ("k_mixramp.hip", "k_mix.h"))
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_(?!K_MIX_H\b)\w+", m.group(1)), m.group(0)   # (but the header's include guard)
