"""CPU: tests/cpp/denoise_plan_test.cpp, the stand-alone program over csrc/denoise_plan.h (the target rule on its
edges, the smoothing, sat32, the block reference against a block walked the way the kernel walks it, rows under cuts
with the mirror's bookkeeping), built by g++ alone and run plainly and under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "denoise_plan_test.cpp")


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "denoise_plan_test", [])            # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "40"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "denoise plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "denoise_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        # only a toolchain without the sanitizers' runtimes is a reason to skip; any other failure is the program's
        # (a diagnostic at a place in the source, "file.cpp:12:3: error: ...", is a compile error, not a missing library)
        assert not re.search(r"\.(cpp|h):\d+:\d+: (fatal )?error", r.stderr), r.stderr
        assert re.search(r"asan|ubsan|sanitize", r.stderr, flags=re.I), r.stderr
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "8"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "denoise plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]
