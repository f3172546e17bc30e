"""CPU: tests/cpp/watch_plan_test.cpp, the stand-alone program over csrc/watch_plan.h's run-length arithmetic (tile
summaries built word by word, their combine, the fold from an incoming state, the launch plan) against the header's
online reference, built by g++ alone and run plainly and under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "watch_plan_test.cpp")


def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "watch_plan_test", [])                 # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "watch plan ok: 20000 cases" in out.stdout, out.stdout + out.stderr


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    # the toolchain has the sanitizers' runtimes (a program of one line says so); then the real build must succeed
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + SAN, capture_output=True, text=True)
    assert r.returncode == 0, "no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-500:]
    exe, r = _build_plan_test(tmp_path, "watch_plan_san", SAN)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "watch plan ok: 20000 cases" in out.stdout, out.stdout + out.stderr[-2000:]
