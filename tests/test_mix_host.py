"""CPU: the host side of channel mixing (cmhip_mix_*): the header, the presets to the integer, the matrix check, NULL
and descriptor refusals, the launcher's plan for every pair of channel counts, an emulation of k_mix_any's
decomposition (16-byte vectors staged into pair planes, one thread per frame, the staged output tile, the ragged
ends) and of k_mix_fast's (a lane's units and vectors, the weight in the half of its frame) against the model of
tests/test_gpu_mix.py at the plan's own tile_frames, and the generated assembly of k_mix.hip.  Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_mix", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RH = _load("test_mix_ramp_host")   # the emulations of both kernels' decomposition: no ramp running, they are k_mix.hip's
TG = RH.TR.TG                      # tests/test_gpu_mix.py: the model and the dense matrices of the GPU tests
UNWRITTEN = RH.UNWRITTEN

PRESETS = {
    "MIX_MONO_TO_STEREO": (0, 1, 2, [[16384], [16384]]),
    "MIX_STEREO_TO_MONO": (1, 2, 1, [[8192, 8192]]),
    "MIX_STEREO_TO_MS": (2, 2, 2, [[8192, 8192], [8192, -8192]]),
    "MIX_51_TO_STEREO": (3, 6, 2, [[16384, 0, 11585, 0, 11585, 0], [0, 16384, 11585, 0, 0, 11585]]),
    "MIX_51_TO_STEREO_NORM": (4, 6, 2, [[6786, 0, 4799, 0, 4799, 0], [0, 6786, 4799, 0, 0, 4799]]),
}


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_mix_desc_t d; unsigned int ci, co; int16_t w[12]; (void)sizeof(d);\n"
           "if (cmhip_mix_preset(CMHIP_MIX_51_TO_STEREO_NORM, &ci, &co, w, 12)) return 1;\n"
           "if (CMHIP_MIX_MONO_TO_STEREO + CMHIP_MIX_STEREO_TO_MONO + CMHIP_MIX_STEREO_TO_MS + CMHIP_MIX_51_TO_STEREO"
           " != 6u) return 2;\n"
           "return cmhip_mix_check(ci, co, w) + (cmhip_mix_new(0) != 0) + cmhip_mix_sync(0)"
           " + (cmhip_mix_hip_stream(0) != 0) + cmhip_mix_run(0, 0, 0, 0, 0, 0, 0) + cmhip_mix_set_matrix(0, -1, w)"
           " + cmhip_mix_get_matrix(0, 0, w) + (cmhip_mix_free(0), 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_presets(cm):
    lib = cm.lib
    header = open(os.path.join(ROOT, "include", "coolmic_hip.h")).read()
    for name, (number, ci, co, rows) in PRESETS.items():
        assert getattr(cm, name) == number
        assert re.search(r"#define\s+CMHIP_%s\s+%du\b" % (name, number), header), name
        a, b = C.c_uint(77), C.c_uint(77)
        assert lib.cmhip_mix_preset(number, C.byref(a), C.byref(b), None, 0) == 0          # the geometry only
        assert (a.value, b.value) == (ci, co)
        w = np.full(ci * co + 1, 77, dtype=np.int16)
        assert lib.cmhip_mix_preset(number, None, None, w.ctypes.data, ci * co - 1) == cm.ERROR_INVAL
        assert (w == 77).all()                                                            # a short cap: nothing written
        assert lib.cmhip_mix_preset(number, None, None, w.ctypes.data, ci * co) == 0
        assert w[:-1].reshape(co, ci).tolist() == rows and w[-1] == 77
        got = cm.mix_preset(number)
        assert got[:2] == (ci, co) and got[2].tolist() == rows
        assert cm.mix_check(ci, co, rows) == 0
        # the integers are printed in the header
        for row in rows:
            assert "{" + ", ".join(str(v) for v in row) + "}" in header, (name, row)
    assert (np.asarray(PRESETS["MIX_51_TO_STEREO_NORM"][3]).sum(axis=1) == 16384).all()
    a = C.c_uint(77)
    assert lib.cmhip_mix_preset(5, C.byref(a), C.byref(a), None, 0) == cm.ERROR_INVAL and a.value == 77
    with pytest.raises(cm.CoolmicError):
        cm.mix_preset(99)


def test_check(cm):
    assert cm.mix_check(2, 1, [[-32768, 32767]]) == 0                        # sum |w| = 65535
    assert cm.mix_check(2, 1, [[-32768, -32768]]) == cm.ERROR_INVAL          # 65536
    assert cm.mix_check(3, 2, [[1, 2, 3], [32767, 32767, 2]]) == cm.ERROR_INVAL
    assert cm.mix_check(3, 2, [[1, 2, 3], [32767, 32767, 1]]) == 0
    w16 = np.full((16, 16), 4095, dtype=np.int16)
    assert cm.mix_check(16, 16, w16) == 0
    w16[15, 15] = -4111                                                       # 15 * 4095 + 4111 = 65536
    assert cm.mix_check(16, 16, w16) == cm.ERROR_INVAL
    one = np.ones((17, 17), dtype=np.int16)
    for ci, co in ((0, 1), (1, 0), (17, 1), (1, 17)):
        assert cm.mix_check(ci, co, one) == cm.ERROR_INVAL, (ci, co)
    assert cm.mix_check(2, 2, None) == cm.ERROR_FAULT
    assert b"mix" in cm.lib.cmhip_last_error()


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    w = np.zeros(4, dtype=np.int16)
    assert lib.cmhip_mix_new(None) is None
    assert lib.cmhip_mix_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_mix_set_matrix(None, -1, w.ctypes.data) == cm.ERROR_FAULT
    assert lib.cmhip_mix_get_matrix(None, 0, w.ctypes.data) == cm.ERROR_FAULT
    assert lib.cmhip_mix_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_mix_hip_stream(None) is None
    lib.cmhip_mix_free(None)
    # descriptors are refused before any device is touched
    for streams, ci, co, frames in ((0, 2, 1, 1024), (1, 0, 1, 1024), (1, 2, 0, 1024), (1, 17, 1, 1024), (1, 2, 17, 1024),
                                    (1, 2, 1, 0), (1, 2, 1, (1 << 30) + 1), (1, 1, 16, (1 << 27) + 1)):
        d = cm.MixDesc(0, streams, ci, co, frames, None)
        assert lib.cmhip_mix_new(C.byref(d)) is None, (streams, ci, co, frames)
        assert b"mix_new" in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Mixer(streams, ci, co, frames)


def _lds_bytes(ci, co, tile):
    cp = (ci + 1) // 2
    return 4 * ((co * cp + 3) // 4 * 4) + 4 * cp * tile + 2 * co * tile


def test_plan(cm):
    for ci in range(1, 17):
        for co in range(1, 17):
            fast = ci <= 2 and co <= 2
            p = cm.plan_mix(5, ci, co, 1)                         # a one-frame run: one workgroup per stream
            assert (p.err, p.grid, p.chunks) == (0, 5, 1), (ci, co)
            assert p.fast == (1 if fast else 0) and p.block == (64 if fast else 256)
            t = p.tile_frames
            assert t % 8 == 0 and t >= 8
            assert p.lds_bytes <= 65536                          # what a workgroup may use without a raised limit
            if fast:
                assert p.lds_bytes == 0 and t == (2048 if (ci, co) == (1, 1) else 1024)
            else:
                assert p.lds_bytes == _lds_bytes(ci, co, t)
                assert t == 1024 or _lds_bytes(ci, co, 2 * t) > 65536        # the largest power of two that fits
            for frames in (t - 1, t, t + 1, 100000):
                q = cm.plan_mix(3, ci, co, frames)
                assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
    assert cm.plan_mix(5, 16, 16, 1).tile_frames == 512 and cm.plan_mix(5, 3, 2, 1).tile_frames == 1024
    # no grid of 2^31 workgroups
    p = cm.plan_mix(1 << 20, 2, 1, 1 << 21)                      # 2^20 streams x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_mix(1 << 20, 2, 1, (1 << 21) - 1024)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    p = cm.plan_mix(1 << 21, 16, 16, 1 << 19)                    # 2^21 streams x 2^10 tiles of 512
    assert p.err != 0 and p.grid == 0
    assert cm.plan_mix(0, 2, 1, 100).grid == 0 and cm.plan_mix(4, 2, 1, 0).grid == 0
    assert cm.plan_mix(0, 2, 1, 100).err == 0
    for ci, co in ((0, 1), (17, 1), (1, 0), (1, 17)):
        assert cm.plan_mix(4, ci, co, 100).grid == 0


# ---------------------------------------------------------------------------
# The decomposition of k_mix_any (csrc/k_mix.hip), step by step in Python: the tile's 16-byte vectors (the ragged last
# one of the stream zero padded, none past it), the scatter into CP planes of dwords (even C_in: by dwords, odd: by
# halves, the unused half never written), one thread per frame with the kernel-form matrix, the interleaved output tile
# and its whole vectors / ragged end.  It holds the index arithmetic (every plane element read was written, nothing past
# a stream's count is read or written) where no GPU is.  The steps are tests/test_mix_ramp_host.py's emulation of
# k_mixr_any with no ramp running: the kernels share them.

def _emulate_any(x, W, tile):
    """x int16 [F][C_in], W [C_out][C_in] -> the output slot as the kernel leaves it (UNWRITTEN where it stored nothing)"""
    W = np.asarray(W, dtype=np.int64)
    outs, paths = RH._emulate_any(x, W, W, 0, 0, tile)
    assert paths <= {False}                                      # the plain path alone
    return outs


@pytest.mark.parametrize("ci,co", [(3, 2), (6, 2), (5, 3), (16, 16), (1, 16)])
def test_emulated_decomposition_equals_the_model(cm, ci, co):
    p = cm.plan_mix(1, ci, co, 1)
    assert p.fast == 0
    t = p.tile_frames
    for s, F in enumerate((2 * t + 13, t, t - 1, t + 1, 1, 0, 7, 8, 9)):
        W = TG.dense_matrix(ci, co, 9000 + 10 * ci + co + s)
        x = TG.noise(9100 + s, F, ci)
        want = TG.model_mix(x, W).astype(np.int64).reshape(-1)
        got = _emulate_any(x, W, t)
        assert np.array_equal(got[:want.size], want), (ci, co, F)
        assert (got[want.size:] == UNWRITTEN).all(), (ci, co, F)  # nothing past the stream's count
    # the kernel form: dword k of row o is W[o][2k] | W[o][2k+1] << 16, an odd C_in padded with zero
    W = TG.dense_matrix(ci, co, 1)
    lo, hi = RH._kernel_form(W.astype(np.int64))
    assert np.array_equal(lo, W[:, 0::2]) and np.array_equal(hi[:, :ci // 2], W[:, 1::2])


def _emulate_fast(x, W):
    """k_mix_fast<CI, CO> (csrc/k_mix.h, mixr_fast_tile without the ramp): a lane's units, their vectors on both sides,
    one dot per output sample on the input dword that holds the frame -- with mono input the weight in the half the
    frame sits in -> the slot"""
    W = np.asarray(W, dtype=np.int64)
    outs, tile, paths = RH._emulate_fast(x, W, W, 0, 0)
    assert paths <= {False}
    return outs, tile


@pytest.mark.parametrize("ci,co", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_emulated_fast_forms_equal_the_model(cm, ci, co):
    t = cm.plan_mix(1, ci, co, 1).tile_frames
    for s, F in enumerate((2 * t + 13, t, t - 1, t + 1, 1, 0, 3, 4, 5, 7, 8, 9)):
        W = TG.dense_matrix(ci, co, 9500 + 10 * ci + co + s)
        x = TG.noise(9600 + s, F, ci)
        want = TG.model_mix(x, W).astype(np.int64).reshape(-1)
        got, tile = _emulate_fast(x, W)
        assert tile == t
        assert np.array_equal(got[:want.size], want), (ci, co, F)
        assert (got[want.size:] == UNWRITTEN).all(), (ci, co, F)


def test_kernel_assembly_house_rules():
    """make asm produces build/k_mix.s: it holds kernels and the dot instruction, no scalar load has a register AND an
    immediate offset (tests/test_abi.py tells why; every workgroup indexes the matrix table with its stream), and the
    four mono / stereo kernels keep every register out of scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_mix.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_dot2\w*_i32_i16", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_mix.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_mix_fast" in k}
    assert len(fast) == 4 and any("k_mix_any" in k for k in scratch), sorted(scratch)
    assert all(v == 0 for v in fast.values()), fast
    src = "".join(open(os.path.join(PKG, "csrc", f)).read() for f in ("k_mix.hip", "k_mix.h"))
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_(?!K_MIX_H\b)\w+", m.group(1)), m.group(0)   # (but the header's include guard)
