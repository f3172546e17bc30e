"""CPU: the host side of loudness metering (ITU-R BS.1770 / EBU R128): the K-weighting coefficients, the LUFS finish,
the gating, the result structure, NULL handling, the headers, the launcher's plan and the generated assembly of
k_loud.hip.  Nothing here needs a GPU.

The model is the plain-Python restatement of the specification in include/coolmic_hip.h below: Python floats are IEEE
doubles, Python arithmetic is unfused, and log10, tan and pow come from libm."""
import ctypes as C
import cmath
import math
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")

_libm = C.CDLL("libm.so.6")
for _n, _k in (("log10", 1), ("tan", 1), ("pow", 2)):
    getattr(_libm, _n).restype = C.c_double
    getattr(_libm, _n).argtypes = [C.c_double] * _k

TABLE_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def _bits(x):
    return struct.pack("<d", x)


# ---------------------------------------------------------------------------
# the model


def coefficients(rate):
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = _libm.tan(math.pi * f0 / rate)
    Vh = _libm.pow(10.0, G / 20.0)
    Vb = _libm.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
         2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = _libm.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def lufs(v):
    return -math.inf if v == 0 else -0.691 + 10.0 * _libm.log10(v)


def integrate(z):
    """-> (integrated, relative threshold, gated blocks)"""
    B = [(((z[i - 3] + z[i - 2]) + z[i - 1]) + z[i]) * 0.25 for i in range(3, len(z))]
    kept = [b for b in B if lufs(b) > -70.0]
    if not kept:
        return -math.inf, -math.inf, 0
    total = 0.0
    for b in kept:
        total += b
    thr = lufs(total / float(len(kept))) - 10.0
    kept = [b for b in kept if lufs(b) > thr]
    if not kept:
        return -math.inf, thr, 0
    total = 0.0
    for b in kept:
        total += b
    return lufs(total / float(len(kept))), thr, len(kept)


def _lib_integrate(cm, z):
    arr = (C.c_double * len(z))(*z)
    i, t, g = C.c_double(1.0), C.c_double(1.0), C.c_size_t(99)
    assert cm.lib.cmhip_loud_integrate(arr, len(z), C.byref(i), C.byref(t), C.byref(g)) == 0
    return i.value, t.value, g.value


def _same(got, want, what):
    assert (_bits(got[0]), _bits(got[1]), got[2]) == (_bits(want[0]), _bits(want[1]), want[2]), (what, got, want)


# ---------------------------------------------------------------------------
# coefficients


def test_coefficients_at_48k_are_the_bs1770_table(cm):
    """within 5e-15: half a unit of the table's last printed digit, the table's own precision"""
    c = cm.loud_coefficients(48000)
    assert len(c) == 10
    for got, want in zip(c, TABLE_48K):
        assert abs(got - want) <= 5e-15, (got, want)
    assert c[5:8] == [1.0, -2.0, 1.0]


def test_coefficients_are_the_model_bit_for_bit(cm):
    for rate in (8000, 32000, 44100, 48000, 96000, 192000):
        got, want = cm.loud_coefficients(rate), coefficients(rate)
        assert [_bits(v) for v in got] == [_bits(v) for v in want], rate
    cm.lib.cmhip_loud_coefficients(48000, None)              # NULL: nothing to do, no crash


# ---------------------------------------------------------------------------
# LUFS and gating


def test_lufs_is_the_host_formula_bit_for_bit(cm):
    assert cm.lib.cmhip_loud_lufs(0.0) == -math.inf
    assert _bits(cm.lib.cmhip_loud_lufs(1.0)) == _bits(-0.691)
    rng = np.random.default_rng(1770)
    for v in [5e-324, 1e-300, 1e-9, 0.25, 4.0] + (10.0 ** rng.uniform(-9.5, 0.5, size=10000)).tolist():
        assert _bits(cm.lib.cmhip_loud_lufs(v)) == _bits(lufs(v)), v


def _z_for(l):                                   # the mean square whose loudness is l LUFS
    return 10.0 ** ((l + 0.691) / 10.0)


def test_integrate_is_the_model_bit_for_bit_on_random_lists(cm):
    rng = np.random.default_rng(3341)
    for k in range(10000):
        n = int(rng.integers(1, 41))
        kind = k % 4
        if kind == 0:                            # anywhere in -90 .. 0 LUFS
            l = rng.uniform(-90.0, 0.0, size=n)
        elif kind == 1:                          # a programme with quiet passages: the relative gate works
            l = np.where(rng.random(n) < 0.4, rng.uniform(-60.0, -35.0, size=n), rng.uniform(-25.0, -15.0, size=n))
        elif kind == 2:                          # around the absolute gate
            l = rng.uniform(-72.0, -68.0, size=n)
        else:
            l = rng.uniform(-90.0, 0.0, size=n)
            l[rng.random(n) < 0.2] = -math.inf   # digital silence
        z = [0.0 if v == -math.inf else _z_for(float(v)) for v in l]
        _same(_lib_integrate(cm, z), integrate(z), (k, z))


def test_integrate_edges(cm):
    for n in range(4):                           # fewer than 4 sub-blocks: no block at all
        _same(_lib_integrate(cm, [0.1] * n), (-math.inf, -math.inf, 0), n)
    assert cm.lib.cmhip_loud_integrate(None, 0, None, None, None) == 0
    assert cm.lib.cmhip_loud_integrate(None, 4, None, None, None) == cm.ERROR_FAULT
    # all below the absolute gate
    z = [_z_for(-75.0)] * 50
    _same(_lib_integrate(cm, z), (-math.inf, -math.inf, 0), "below the gate")
    assert integrate(z) == (-math.inf, -math.inf, 0)
    # exactly four sub-blocks: one block
    z = [0.01, 0.02, 0.03, 0.04]
    want = integrate(z)
    assert want[2] == 1 and _bits(want[0]) == _bits(lufs((((0.01 + 0.02) + 0.03) + 0.04) * 0.25))
    _same(_lib_integrate(cm, z), want, "one block")
    # the relative gate removes blocks: 100 loud sub-blocks, then 100 at 30 LU less (above -70)
    z = [_z_for(-20.0)] * 100 + [_z_for(-50.0)] * 100
    want = integrate(z)
    assert want[2] < len(z) - 3 and -20.1 < want[0] < -19.9 and -33.1 < want[1] < -32.9
    _same(_lib_integrate(cm, z), want, "relative gate")
    assert cm.loud_integrate(z) == want


TECH_3341 = [({-23: 20}, -23.0), ({-33: 20}, -33.0), ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
             ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0),
             ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)]


def test_tech_3341_tone_sequences_as_synthetic_sub_blocks(cm):
    """EBU Tech 3341 cases 1-5: stereo 1 kHz sines at the given dBFS (peak) for the given seconds; a sub-block of such
    a tone has z = 2 channels * (A^2 / 2) * |H(1 kHz)|^2 with H the K-weighting at 48 kHz.  Integrated loudness within
    +-0.1 LU of the target, the tolerance Tech 3341 itself allows."""
    c = coefficients(48000)
    w = cmath.exp(-2j * math.pi * 1000.0 / 48000.0)
    gain = 1.0
    for k in (0, 5):
        gain *= abs((c[k] + c[k + 1] * w + c[k + 2] * w * w) / (1.0 + c[k + 3] * w + c[k + 4] * w * w)) ** 2
    assert 0.69 < 10.0 * math.log10(gain) < 0.70             # what the -0.691 of the formula cancels
    for seq, target in TECH_3341:
        seq = list(seq.items()) if isinstance(seq, dict) else seq
        z = []
        for dbfs, seconds in seq:
            z += [2.0 * (10.0 ** (dbfs / 10.0) / 2.0) * gain] * int(round(seconds * 10))
        got = _lib_integrate(cm, z)
        print("Tech 3341", seq, "integrated", got[0], "threshold", got[1], "gated", got[2])
        assert abs(got[0] - target) <= 0.1, (seq, got)
        _same(got, integrate(z), seq)


# ---------------------------------------------------------------------------
# the interface


def test_result_struct_layout(cm, tmp_path):
    T = cm.LoudnessResult
    names = ["rate", "channels", "frames", "blocks", "gated_blocks", "momentary", "short_term", "integrated",
             "relative_threshold"]
    assert C.sizeof(T) == 64
    assert [n for n, _ in T._fields_] == names
    assert [getattr(T, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    src = tmp_path / "layout.c"                  # and the C compiler agrees with the mirror
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <coolmic-dsp/vumeter.h>\n'
                   'int main(void){printf("%zu", sizeof(coolmic_loudness_result_t));\n'
                   + "".join('printf(" %%zu", offsetof(coolmic_loudness_result_t, %s));\n' % n for n in names)
                   + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [64, 0, 4, 8, 16, 24, 32, 40, 48, 56]


def test_null_arguments_are_faults(cm):
    r = cm.LoudnessResult()
    w = (C.c_double * 16)(*([1.0] * 16))
    lib = cm.lib
    assert lib.cmhip_batch_set_loudness(None, 1) == cm.ERROR_FAULT
    assert lib.cmhip_batch_get_loudness(None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_loud_set_weights(None, -1, w) == cm.ERROR_FAULT
    assert lib.cmhip_batch_loud_result(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert lib.cmhip_batch_loud_results(None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_loud_raw(None, 0, None, 0, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_loud_reset(None, -1) == cm.ERROR_FAULT
    assert lib.coolmic_group_set_loudness(None, 1) == cm.ERROR_FAULT
    assert lib.coolmic_group_loudness(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert lib.coolmic_group_loudnesses(None, None, None) == cm.ERROR_FAULT
    assert lib.coolmic_group_loudness_set_weights(None, -1, w) == cm.ERROR_FAULT
    assert lib.coolmic_group_loudness_reset(None, -1) == cm.ERROR_FAULT
    assert len({cm.ERROR_FAULT, cm.ERROR_INVAL, cm.ERROR_BUSY, cm.ERROR_NOMEM, cm.ERROR_NONE}) == 5
    for e in (cm.ERROR_FAULT, cm.ERROR_INVAL, cm.ERROR_BUSY, cm.ERROR_NOMEM):
        assert e < 0 and lib.coolmic_error2string(e)
    assert lib.cmhip_debug_loud_count() >= 0


def test_headers_still_compile_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n#include <coolmic-dsp/group.h>\n#include <coolmic-dsp/vumeter.h>\n"
           "int main(void){coolmic_loudness_result_t r; double c[10], i, t; size_t g; (void)sizeof(r);\n"
           "cmhip_loud_coefficients(48000, c); (void)cmhip_loud_integrate(c, 10, &i, &t, &g);\n"
           "(void)coolmic_group_loudness_reset(0, -1);\n"
           "return cmhip_loud_lufs(c[0]) > 0.;}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_plan_is_a_lane_per_row_and_a_wave_per_workgroup(cm):
    p = cm.plan_loud(4096, 2, 65536)                         # the config-2 shape: 8192 rows
    assert (p.err, p.vec, p.block, p.grid) == (0, 1, 64, 128)
    p = cm.plan_loud(70, 1, 800)
    assert (p.err, p.vec, p.grid) == (0, 1, 2)
    p = cm.plan_loud(5, 6, 100)
    assert (p.err, p.vec, p.block, p.grid) == (0, 0, 64, 1)
    p = cm.plan_loud(65, 16, 1)
    assert (p.err, p.vec, p.grid) == (0, 0, 17)
    p = cm.plan_loud((1 << 32) - 1, 16, 1)                   # more rows than a 32-bit row number holds: refused
    assert p.err != 0 and p.grid == 0
    p = cm.plan_loud((1 << 32) - 1, 1, 1)
    assert p.err == 0 and p.grid == 1 << 26
    assert cm.plan_loud(0, 2, 100).grid == 0 and cm.plan_loud(4, 2, 0).grid == 0 and cm.plan_loud(4, 17, 9).grid == 0


def test_kernel_assembly_house_rules():
    """make asm produces build/k_loud.s: the recurrence is unfused (no v_fma_f64: every product and sum is rounded
    once), double denormals are kept, no kernel uses scratch memory, and no scalar load has a register AND an immediate
    offset (tests/test_abi.py tells why)"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_loud.s")).read()
    assert text.count(".amdhsa_kernel") == 3
    assert "v_mul_f64" in text and "v_add_f64" in text
    assert "v_fma_f64" not in text and "v_mad_f64" not in text
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)
    assert modes == ["3"] * 3, modes                         # 3: denormals in and out
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_loud.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch
    src = open(os.path.join(PKG, "csrc", "k_loud.hip")).read() + open(os.path.join(PKG, "csrc", "cmhip_loud.hip")).read()
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_\w+", m.group(1)), m.group(0)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*=.*\bk_loud\.hip\b.*\bcmhip_loud\.hip\b", mk, flags=re.M)
    assert re.search(r"^asm:.*build/k_loud\.s", mk, flags=re.M)


def test_the_package_does_not_name_the_checker():
    """what this feature added to or touched in the package directory does not speak of the test infrastructure"""
    for f in ("__init__.py", "csrc/k_loud.hip", "csrc/cmhip_loud.hip", "csrc/cmhip_internal.h", "csrc/cmhip_engine.h",
              "csrc/cmhip_batch.hip", "csrc/group.hip", "Makefile"):
        assert "oracle" not in open(os.path.join(PKG, f), errors="replace").read().lower(), f
