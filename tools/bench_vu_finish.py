#!/usr/bin/env python3
"""What the opt-in device-side dB finish (CMHIP_VU_FINISH_DEVICE) buys a step that closes a VU window per block.

The config-2 shape (4096 stereo streams, channel swap + gains {750,1250}/1000, PCM materialised) at T = 512 / 2880 /
4096 frames per block, a window per block and per 20 blocks, in the loop of bench.py's `small_blocks` leg (launch,
snapshot, the collect in two halves, up to three snapshots pending).  Host and device finish alternate, REPS
repetitions each, medians.  Beside the wall time of a step: the process's CPU seconds per step (getrusage, all
threads -- the helper pool included).  The table is taken twice, each in a fresh child process: with the helper pool
as the library sizes it, and with CMHIP_POOL_THREADS=1 (the share of one rank of eight under a 16-CPU quota).

A library without cmhip_batch_vu_set_finish (COOLMIC_HIP_LIB=<an older build>) is measured in host mode alone: that
is how the parent commit's step is taken in the same session.

    python tools/bench_vu_finish.py [--reps N] [--steps N]      the two tables, one JSON line each
    python tools/bench_vu_finish.py --child [...]               one table in this process (e.g. under rocprofv3
                                                                --kernel-trace --stats, the program after `--`)
"""
import argparse
import ctypes as C
import json
import os
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, CH, CAP = 4096, 2, 4096


def loop(b, frames, every, nsteps, results, rcs):
    """benchlib.legs.small_blocks' loop: the finish of window k-1 runs beside launch and snapshot of block k+1"""
    collecting, waiting = False, 0
    for i in range(nsteps):
        b.run(frames)
        if i % every != every - 1:
            continue
        b.vu_snapshot()
        waiting += 1
        if collecting:
            b.vu_collect_end()
            collecting = False
            waiting -= 1
        if waiting >= 2:
            b.vu_collect_begin(results, rcs)
            collecting = True
    if collecting:
        b.vu_collect_end()
        waiting -= 1
    while waiting:
        b.vu_collect(results, rcs)
        waiting -= 1
    b.sync()


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def table(reps, steps):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    has_setter = hasattr(cm.lib, "cmhip_batch_vu_set_finish")
    b = cm.Batch(S, CH, CAP, flags=cm.OUT_PCM | cm.VU)
    b.set_gain(-1, 2, 1000, [750, 1250])
    b.set_chmap(-1, [1, 0])
    b.generate(cm.GEN_NOISE, 12345, CAP)
    results, rcs = (cm.VuResult * S)(), (C.c_int * S)()
    modes = ["host", "device"] if has_setter else ["host"]
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                  # clocks up before anything is timed
        for _ in range(16):
            b.run(CAP)
        b.sync()
    out = {"library": cm.LIB_PATH, "has_setter": has_setter, "pool_threads_env": os.environ.get("CMHIP_POOL_THREADS"),
           "reps": reps, "steps": steps, "shape": [S, CH], "rows": {}}
    for frames in (512, 2880, 4096):
        for every in (1, 20):
            wall = {m: [] for m in modes}
            cpu = {m: [] for m in modes}
            for rep in range(reps + 1):                    # (the first repetition warms every mode up, untimed)
                for m in modes:
                    if has_setter:
                        assert b.vu_set_finish(1 if m == "device" else 0) == 0
                    b.vu_reset(-1)
                    b.sync()
                    loop(b, frames, every, 200, results, rcs)
                    c0, t1 = cpu_seconds(), time.perf_counter()
                    loop(b, frames, every, steps, results, rcs)
                    t2, c1 = time.perf_counter(), cpu_seconds()
                    if rep:
                        wall[m].append((t2 - t1) / steps * 1e6)
                        cpu[m].append((c1 - c0) / steps * 1e6)
            out["rows"]["T%d_every%d" % (frames, every)] = {
                m: {"step_us_median": round(statistics.median(wall[m]), 2), "step_us_min": round(min(wall[m]), 2),
                    "step_us_max": round(max(wall[m]), 2), "cpu_us_per_step_median": round(statistics.median(cpu[m]), 2)}
                for m in modes}
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(table(a.reps, a.steps)), flush=True)
        return 0
    # this process never touches the GPU: each table gets a fresh child, which reads the pool size when it starts
    for pool in (None, "1"):
        env = dict(os.environ)
        if pool is None:
            env.pop("CMHIP_POOL_THREADS", None)
        else:
            env["CMHIP_POOL_THREADS"] = pool
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--steps",
                            str(a.steps)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows = json.loads(line)["rows"]
        sys.stderr.write("helper pool: %s\n" % ("library default" if pool is None else pool + " thread"))
        for k, v in rows.items():
            sys.stderr.write("  %-16s " % k + "   ".join(
                "%s %6.1f us/step (%.1f-%.1f), cpu %6.1f us/step" % (m, d["step_us_median"], d["step_us_min"],
                                                                       d["step_us_max"], d["cpu_us_per_step_median"])
                for m, d in v.items()) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
