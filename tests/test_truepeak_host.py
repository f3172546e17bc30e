"""CPU: the host side of true-peak metering (ITU-R BS.1770 Annex 2): the filter table, the dBTP finish, the result
structure, NULL handling, the headers, the launcher's plan and the generated assembly of k_tpeak.hip.  Nothing here
needs a GPU."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")

P0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
P1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
FULL_SCALE = 268435456


def _bits(x):
    return struct.pack("<d", x)


def test_coefficients_are_the_specified_table(cm):
    h = np.zeros(48, dtype=np.int16)
    cm.lib.cmhip_tp_coefficients(h.ctypes.data)
    h = h.reshape(4, 12)
    assert h[0].tolist() == P0
    assert h[1].tolist() == P1
    assert h[2].tolist() == P1[::-1]
    assert h[3].tolist() == P0[::-1]
    assert h.astype(np.int64).sum(axis=1).tolist() == [8205, 7971, 7971, 8205]
    assert int(np.abs(h.astype(np.int64)).sum(axis=1).max()) <= 16571
    assert cm.tp_coefficients().tolist() == h.tolist()
    cm.lib.cmhip_tp_coefficients(None)                       # NULL: nothing to do, no crash


def test_dbtp_is_the_host_formula_bit_for_bit(cm):
    libm = C.CDLL("libm.so.6")
    libm.log10.restype = C.c_double
    libm.log10.argtypes = [C.c_double]
    assert cm.lib.cmhip_tp_dbtp(0) == -math.inf
    assert _bits(cm.lib.cmhip_tp_dbtp(FULL_SCALE)) == _bits(0.0)
    assert cm.lib.cmhip_tp_dbtp(1) == -168.57679757182947
    assert cm.lib.cmhip_tp_dbtp(270996320) == float.fromhex("0x1.51cc5f944547ap-4")
    rng = np.random.default_rng(1770)
    peaks = [1, 270996320, 542986257] + rng.integers(1, 542986258, size=10000).tolist()
    for p in peaks:
        want = 20. * libm.log10(p / 268435456.)
        assert _bits(cm.lib.cmhip_tp_dbtp(p)) == _bits(want), p
    assert cm.lib.cmhip_tp_dbtp(542986257) > 6.11            # not capped at 0


def test_result_struct_layout(cm, tmp_path):
    T = cm.TruePeakResult
    assert C.sizeof(T) == 224
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 16, 20, 88, 96]
    assert [n for n, _ in T._fields_] == ["rate", "channels", "frames", "global_peak", "channel_peak",
                                          "global_dbtp", "channel_dbtp"]
    # and the C compiler agrees with the mirror
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <coolmic-dsp/vumeter.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(coolmic_truepeak_result_t),\n'
                   'offsetof(coolmic_truepeak_result_t, rate), offsetof(coolmic_truepeak_result_t, channels),\n'
                   'offsetof(coolmic_truepeak_result_t, frames), offsetof(coolmic_truepeak_result_t, global_peak),\n'
                   'offsetof(coolmic_truepeak_result_t, channel_peak), offsetof(coolmic_truepeak_result_t, global_dbtp),\n'
                   'offsetof(coolmic_truepeak_result_t, channel_dbtp));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [224, 0, 4, 8, 16, 20, 88, 96]


def test_null_arguments_are_faults(cm):
    r = cm.TruePeakResult()
    assert cm.lib.cmhip_batch_set_true_peak(None, 1) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_get_true_peak(None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_tp_result(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_tp_results(None, None, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_tp_reset(None, -1) == cm.ERROR_FAULT
    assert cm.lib.coolmic_group_set_true_peak(None, 1) == cm.ERROR_FAULT
    assert cm.lib.coolmic_group_true_peak(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert cm.lib.coolmic_group_true_peaks(None, None, None) == cm.ERROR_FAULT
    assert cm.lib.coolmic_error2string(cm.ERROR_FAULT) and cm.lib.coolmic_error2string(cm.ERROR_INVAL)


def test_headers_still_compile_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n#include <coolmic-dsp/group.h>\n#include <coolmic-dsp/vumeter.h>\n"
           "int main(void){coolmic_truepeak_result_t r; int16_t h[48]; (void)sizeof(r); cmhip_tp_coefficients(h);\n"
           "return cmhip_tp_dbtp(h[0] > 0 ? 1u : 2u) > 0.;}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_plan_refuses_a_grid_of_2_to_the_31_workgroups(cm):
    p = cm.plan_tpeak(4096, 2, 65536)                        # the config-2 shape: 32 tiles of 8 KiB per stream
    assert (p.err, p.fast, p.block, p.chunks, p.grid) == (0, 1, 64, 32, 4096 * 32)
    p = cm.plan_tpeak(8192, 1, 65536)
    assert (p.err, p.fast, p.chunks, p.grid) == (0, 1, 16, 8192 * 16)
    p = cm.plan_tpeak(64, 6, 16384)                          # other channel counts: a workgroup per 1024 frames
    assert (p.err, p.fast, p.block, p.chunks, p.grid) == (0, 0, 256, 16, 64 * 16)
    p = cm.plan_tpeak(3, 2, 1)
    assert (p.err, p.chunks, p.grid) == (0, 1, 3)
    p = cm.plan_tpeak(1 << 20, 1, 1 << 23)                   # 2^20 streams x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_tpeak(1 << 20, 1, (1 << 23) - 4096)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    p = cm.plan_tpeak(1 << 21, 3, 1 << 20)                   # 2^21 streams x 2^10 tiles
    assert p.err != 0 and p.grid == 0
    assert cm.plan_tpeak(0, 2, 100).grid == 0 and cm.plan_tpeak(4, 2, 0).grid == 0


def test_kernel_assembly_house_rules():
    """make asm produces build/k_tpeak.s: no scalar load with a register AND an immediate offset (tests/test_abi.py
    tells why), the dot instruction is the one the design counts, and the mono / stereo kernels keep every register
    out of scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_tpeak.s")).read()
    assert ".amdhsa_kernel" in text and "v_dot2c_i32_i16" in text
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_tpeak.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_tpeak_fast" in k}
    assert len(fast) == 2, sorted(scratch)
    assert all(v == 0 for v in fast.values()), fast
    src = open(os.path.join(PKG, "csrc", "k_tpeak.hip")).read()
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_\w+", m.group(1)), m.group(0)
