"""CPU: csrc/stage_io.h, the checks every stage object makes before it touches anything -- the range of streams a call
names and a run's pointers, strides, counts and overlap -- as a stand-alone C++ program (tests/cpp/stage_io_test.cpp),
plainly and under AddressSanitizer + UBSan.  It restates the refusals of the GPU tests' test_refusals for the limiter's
and the bus's shapes, the edges of both overlap rules, the counts, the sizes that would wrap, and the stream range.
Nothing here needs a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "stage_io_test.cpp")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_stage_io(tmp_path):
    exe, r = _build(tmp_path, "stage_io_test", [])                           # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "stage io ok:" in out.stdout, out.stdout + out.stderr


def test_stage_io_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "stage_io_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                               "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "stage io ok:" in out.stdout, out.stdout + out.stderr[-2000:]


def test_no_second_copy_of_the_checks():
    """the run check, the stream range and the stream's creation exist once: in csrc/stage_io.h and csrc/cmhip_stage.h
    (the batch creates its own streams)"""
    csrc = os.path.join(PKG, "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    assert [f for f, t in text.items() if "hipStreamCreateWithFlags" in t] == ["cmhip_batch.hip", "cmhip_stage.h"]
    assert [f for f, t in text.items() if "stream < -1" in t or "stream >= (long)" in t] == []
    assert sum(t.count('in and out must be 16-byte aligned') for t in text.values()) == 1
    assert "#include <hip" not in text["stage_io.h"] and "CountsRing" not in text["cmhip_internal.h"]
