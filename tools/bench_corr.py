#!/usr/bin/env python3
"""What the phase-correlation meter (cmhip_batch_set_correlation) costs a step, and how far k_corr_fast is from its
bounds.

Shape: config 2 (4096 x 2 x 65536), a CMHIP_VU-only batch created the default way, GEN_NOISE input, the gains and map
of bench.py's config.  After 150 ms of the batch's own launches the step (launch + wait) is timed with correlation off
and on, alternating in one process on the same arrays: medians of REPS x STEPS steps; the pass's own time is their
difference.  Beside them: the batch's measured read ceiling (cmhip_batch_ceiling mode 0), the VALU instructions per
stereo frame of the whole-tile form counted in build/k_corr.s (`make asm`), and the issue floor that count implies
(4 cycles per wave instruction, 2.4 GHz, 256 CUs x 4 SIMDs x 64 lanes).

The kernel's own duration comes from a run under the profiler, the program directly after `--`, no counters:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_corr.py --profile

    python tools/bench_corr.py [--reps N] [--steps N]      one JSON line
    python tools/bench_corr.py --count-asm                 the instruction counts alone (no GPU needed)
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, C, T, GAIN, CMAP = 4096, 2, 65536, (2, 1000, [750, 1250]), [1, 0]
LANES_PER_CYCLE = 256 * 4 * 64 / 4.0               # lane-instructions the chip issues per cycle
CLOCK_HZ = 2.4e9
LANE_FRAMES = 32                                   # k_corr.hip: CORR_LANE_FRAMES


def count_asm():
    """k_corr_fast's whole-tile form: the stretch of build/k_corr.s with the first 96 dot instructions and no
    compare-and-select of a ragged tile.  VALU instructions (the wave's reduction and the loads' address arithmetic
    included) and wait states per stereo frame, registers and occupancy from the usage report."""
    base = os.path.join(ROOT, "libcoolmic-dsp_amd", "build")
    if not os.path.exists(os.path.join(base, "k_corr.s")):
        return None
    text = open(os.path.join(base, "k_corr.s")).read()
    m = re.search(r"^_ZN5cmhip11k_corr_fastENS_8CorrArgsE:(.*?)s_endpgm", text, flags=re.S | re.M)
    if not m:
        return None
    out = None
    for seg in m.group(1).split("; sched_barrier"):
        ins = [ln.split()[0] for ln in seg.splitlines()
               if ln.strip() and not ln.strip().startswith((";", ".")) and not ln.strip().endswith(":")]
        dots = sum(i.startswith("v_dot2") for i in ins)
        if dots < 3 * LANE_FRAMES or any(i.startswith("v_cndmask") for i in ins):
            continue
        # cut behind the last dot's accumulation: what follows is the wave's reduction and the other form
        last = max(k for k, i in enumerate(ins) if i.startswith("v_dot2"))
        head = ins[:last + 1]
        if sum(i.startswith("v_dot2") for i in head) != 3 * LANE_FRAMES:
            continue
        valu = [i for i in head if i.startswith("v_")]
        out = {"valu_per_frame": round(len(valu) / LANE_FRAMES, 2),
               "dots_per_frame": 3.0,
               "s_nop_per_frame": round(sum(i == "s_nop" for i in head) / LANE_FRAMES, 2)}
        break
    usage = os.path.join(base, "k_corr.usage.txt")
    if out and os.path.exists(usage):
        u = re.search(r"Function Name: \S*k_corr_fast.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                      r"Occupancy \[waves/SIMD\]: (\d+)", open(usage).read(), flags=re.S)
        if u:
            out.update(vgprs=int(u.group(1)), scratch_bytes=int(u.group(2)), occupancy_waves_per_simd=int(u.group(3)))
    return out


def timed(b, frames, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        b.run(frames)
    b.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--profile", action="store_true", help="a short run for the profiler: 20 steps with correlation on")
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    counts = count_asm()
    if a.count_asm:
        print(json.dumps({"k_corr_fast": counts}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    if cm.device_count() < 1:
        raise SystemExit("bench_corr: no HIP device visible; nothing is measured without one")
    b = cm.Batch(S, C, T, flags=cm.VU)
    b.set_gain(-1, *GAIN)
    b.set_chmap(-1, CMAP)
    b.generate(cm.GEN_NOISE, 12345, T)
    b.sync()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:                 # the batch's own launches bring the clocks up
        for _ in range(8):
            b.run(T)
        b.sync()
    if a.profile:
        assert b.set_correlation(1) == 0
        for _ in range(20):
            b.run(T)
        b.sync()
        b.close()
        return
    off, on = [], []
    for _ in range(a.reps):
        assert b.set_correlation(0) == 0
        off.append(timed(b, T, a.steps))
        assert b.set_correlation(1) == 0
        on.append(timed(b, T, a.steps))
    out, rc = b.corr_results()
    assert rc[0] == 0 and out[0].frames == a.steps * T
    frames = S * T
    read_gbs = b.ceiling(0, 10)
    line = {"shape": "c2", "streams": S, "channels": C, "frames": T, "reps": a.reps, "steps": a.steps,
            "step_ms_off": round(statistics.median(off), 4), "step_ms_on": round(statistics.median(on), 4),
            "step_ms_off_all": [round(v, 4) for v in off], "step_ms_on_all": [round(v, 4) for v in on],
            "corr_ms_by_difference": round(statistics.median(on) - statistics.median(off), 4),
            "read_ceiling_GBs": round(read_gbs, 1),
            "read_ceiling_ms": round(frames * C * 2 / (read_gbs * 1e9) * 1e3, 4) if read_gbs > 0 else None,
            "correlation_stream0": out[0].correlation[0], "balance_db_stream0": out[0].balance_db[0]}
    if counts:
        line.update(counts)
        line["issue_floor_ms"] = round(frames * counts["valu_per_frame"] / LANES_PER_CYCLE / CLOCK_HZ * 1e3, 4)
    print(json.dumps(line), flush=True)
    b.close()


if __name__ == "__main__":
    main()
