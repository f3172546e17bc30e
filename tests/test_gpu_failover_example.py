"""GPU: examples/batch_failover.c builds against the public headers and the library and shows what the failover switch
is for: two seconds of dead air in the programme reach the listener as half a second, the output goes to the backup and
comes back, and the signal watch behind the switch says so."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def test_batch_failover_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_failover"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_failover.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0] == ("programme of 288000 frames, silent from 96000 to 192000; switch: windows of 1024 frames, leave "
                      "after 23, return after 23, fade 1024 frames"), out
    # the silence begins in window 93, which is still live; windows 94..116 are the 23 dead ones, so the fade begins at
    # frame 117 * 1024 = 119808, and its frame 5 is the first above the watch's quiet of 32: (5 * 32 * 8000 + 16384) >> 15
    # = 39.  The programme is back in window 187; windows 187..209 are the 23 live ones: back at 210 * 1024 = 215040.
    assert 119808 + 5 - 96000 == 23813 and 119808 // 4800 == 24 and 215040 // 4800 == 44
    assert out[1:] == ["input: longest dead air 96000 frames (2000.0 ms)",
                       "output: longest dead air 23813 frames (496.1 ms)",
                       "output went to the backup in block 24 and came back in block 44; switches 2"], out
