"""CPU: tests/cpp/spec_plan_test.cpp, the stand-alone program over csrc/spec_plan.h's bookkeeping (which blocks a run
completes, where their samples lie, what state it leaves), built by g++ alone and run plainly and under
AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "spec_plan_test.cpp")


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "spec_plan_test", [])                  # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "200"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "spec plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "spec_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "30"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "spec plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]
