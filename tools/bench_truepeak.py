#!/usr/bin/env python3
"""What true-peak metering (cmhip_batch_set_true_peak) costs a step, and how far k_tpeak is from its bounds.

Shapes: config 2 (4096 x 2 x 65536), config 4 (8192 mono x 65536) and x6 (2730 x 6 x 16384), each a CMHIP_VU-only
batch created the default way, GEN_NOISE input, the gains and maps of bench.py's configs.  After 150 ms of the
batch's own launches the step (launch + wait) is timed with true peak off and on, alternating in one process:
medians of REPS x STEPS steps.  Beside them: the batch's measured read ceiling (cmhip_batch_ceiling mode 0), the
VALU instructions per sample of the mono / stereo loops counted in build/k_tpeak.s (`make asm`), and the issue floor
that count implies (4 cycles per wave instruction, 2.4 GHz, 256 CUs x 4 SIMDs x 64 lanes).

The kernel's own duration comes from a run under the profiler, the program directly after `--`, no counters:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_truepeak.py --profile

    python tools/bench_truepeak.py [--reps N] [--steps N]      one JSON line per shape
    python tools/bench_truepeak.py --count-asm                 the instruction counts alone (no GPU needed)
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "c2": (4096, 2, 65536, (2, 1000, [750, 1250]), [1, 0]),
    "c4": (8192, 1, 65536, (1, 1000, [900]), None),
    "x6": (2730, 6, 16384, (1, 1000, [900]), None),
}
LANES_PER_CYCLE = 256 * 4 * 64 / 4.0               # lane-instructions the chip issues per cycle
CLOCK_HZ = 2.4e9
TP_U = 8                                           # k_tpeak.hip: vectors per lane, and the halo vectors it loads besides
HALO = {1: 2, 2: 3}


def count_asm():
    """VALU instructions per sample of k_tpeak_fast<C>, from the stretches between the scheduling barriers of its
    whole-tile form: one sample of the FIR (24 dot instructions), one vector of the transform."""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_tpeak.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for C in (1, 2):
        m = re.search(r"^_ZN5cmhip12k_tpeak_fastILi%dEEEvNS_6TpArgsE:(.*?)s_endpgm" % C, text, flags=re.S | re.M)
        if not m:
            return None
        fir, gain = [], []
        for seg in m.group(1).split("; sched_barrier"):
            ins = [ln.split()[0] for ln in seg.splitlines()
                   if ln.strip() and not ln.strip().startswith((";", ".")) and not ln.strip().endswith(":")]
            valu = [i for i in ins if i.startswith("v_")]
            dots = sum(i.startswith("v_dot2c") for i in ins)
            masked = any(i.startswith(("v_cmp", "v_cndmask")) for i in ins)
            if dots == 24 and not masked:
                fir.append(len(valu))
            elif dots == 0 and sum(i == "v_mul_hi_u32" for i in ins) == 8 and len(ins) < 120:
                gain.append(len(valu) / 8.0)
        if not fir or not gain:
            return None
        f, g = statistics.median(fir), statistics.median(gain) * (TP_U + HALO[C]) / TP_U
        out[C] = {"fir_valu_per_sample": round(f, 2), "transform_valu_per_sample_with_halo": round(g, 2),
                  "valu_per_sample": round(f + g, 2)}
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
    ap.add_argument("--shapes", default="c2,c4,x6")
    ap.add_argument("--profile", action="store_true", help="a short run for the profiler: 20 steps with true peak on")
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    counts = count_asm()
    if a.count_asm:
        print(json.dumps({"k_tpeak_valu": counts}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    for name in a.shapes.split(","):
        S, C, T, gain, cmap = SHAPES[name]
        b = cm.Batch(S, C, T, flags=cm.VU)
        b.set_gain(-1, *gain)
        if cmap:
            b.set_chmap(-1, cmap)
        b.generate(cm.GEN_NOISE, 12345, T)
        b.sync()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:             # the batch's own launches bring the clocks up
            for _ in range(8):
                b.run(T)
            b.sync()
        if a.profile:
            assert b.set_true_peak(1) == 0
            for _ in range(20):
                b.run(T)
            b.sync()
            b.close()
            continue
        off, on = [], []
        for _ in range(a.reps):
            assert b.set_true_peak(0) == 0
            off.append(timed(b, T, a.steps))
            assert b.set_true_peak(1) == 0
            on.append(timed(b, T, a.steps))
        out, rc = b.tp_results()
        assert rc[0] == 0 and out[0].frames == a.steps * T
        samples = S * C * T
        read_gbs = b.ceiling(0, 10)
        line = {"shape": name, "streams": S, "channels": C, "frames": T, "reps": a.reps, "steps": a.steps,
                "step_ms_off": round(statistics.median(off), 4), "step_ms_on": round(statistics.median(on), 4),
                "step_ms_off_all": [round(v, 4) for v in off], "step_ms_on_all": [round(v, 4) for v in on],
                "true_peak_ms_by_difference": round(statistics.median(on) - statistics.median(off), 4),
                "read_ceiling_GBs": round(read_gbs, 1),
                "read_ceiling_ms": round(samples * 2 / (read_gbs * 1e9) * 1e3, 4) if read_gbs > 0 else None,
                "dbtp_stream0": out[0].global_dbtp}
        if counts and C in counts:
            line.update(counts[C])
            line["issue_floor_ms"] = round(samples * counts[C]["valu_per_sample"] / LANES_PER_CYCLE / CLOCK_HZ * 1e3, 4)
        print(json.dumps(line), flush=True)
        b.close()


if __name__ == "__main__":
    main()
