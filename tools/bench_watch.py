#!/usr/bin/env python3
"""What the signal watch (cmhip_batch_set_watch) costs a step, and how far its tile pass is from its bounds.

Shapes: config 2 (4096 x 2 x 65536) and config 4's per-GPU share (8192 x 1 x 65536), a CMHIP_VU-only batch created the
default way, GEN_NOISE input, the gains and map of bench.py's config.  After 150 ms of the batch's own launches the
step (launch + wait) is timed with every meter off, with the watch on and -- in the same process on the same arrays,
the yardstick beside it -- with phase correlation on instead (stereo only), alternating: medians of REPS x STEPS steps;
a pass's own time is the difference to the step without it.  Then the watch's two kernels alone between HIP events
(cmhip_test_watch_time: the tile pass, the fold), the median of 15 launches after 5.  Beside them: the batch's measured
read ceiling (cmhip_batch_ceiling mode 0), the VALU instructions per frame of the whole-tile form counted in
build/k_watch.s (`make asm`), the kernel's registers from its usage report, and the issue floor the VALU count implies
(4 cycles per wave instruction, 2.4 GHz, 256 CUs x 4 SIMDs x 64 lanes).

The input is noise: a word of 64 frames is almost always all zeros for every predicate, one step of the run reader.
--dead measures the same with every slot silent instead (every quiet word all ones, one step as well).

    python tools/bench_watch.py [--reps N] [--steps N] [--dead]     one JSON line per shape
    python tools/bench_watch.py --count-asm                          the instruction counts alone (no GPU needed)
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c2": (4096, 2, 65536, (2, 1000, [750, 1250]), [1, 0]), "c4": (8192, 1, 65536, (1, 1000, [750]), None)}
LANES_PER_CYCLE = 256 * 4 * 64 / 4.0               # lane-instructions the chip issues per cycle
CLOCK_HZ = 2.4e9
KERNEL = {1: "_ZN5cmhip12k_watch_fastILi1EEEvNS_9WatchArgsE", 2: "_ZN5cmhip12k_watch_fastILi2EEEvNS_9WatchArgsE"}


# VALU instructions per frame and lane of the whole-tile form, counted by hand in build/k_watch.s (`make asm`), the loop
# over the tile's words up to its masks.  Stereo: address 1, perm 1, gain 12, the signed result 2, sums 2, compares 4.
# Mono, per dword of two frames: address and packing
# 3, gain 12, the signed result 2, sum 1, compares 4.
VALU_PER_FRAME = {1: 11.0, 2: 22.0}


def count_asm(channels):
    """registers, LDS, scratch and occupancy of k_watch_fast<C> from the usage report of `make asm`, beside the hand
    count above"""
    usage = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_watch.usage.txt")
    if not os.path.exists(usage):
        return None
    u = re.search(r"Function Name: %s.*?SGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                  r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)" % KERNEL[channels],
                  open(usage).read(), flags=re.S)
    if not u:
        return None
    return {"valu_per_frame": VALU_PER_FRAME[channels], "sgprs": int(u.group(1)), "vgprs": int(u.group(2)),
            "scratch_bytes": int(u.group(3)), "occupancy_waves_per_simd": int(u.group(4)), "lds_bytes": int(u.group(5))}


def timed(b, frames, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        b.run(frames)
    b.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(cm, name, a):
    S, Cn, T, gain, cmap = SHAPES[name]
    b = cm.Batch(S, Cn, T, flags=cm.VU)
    b.set_gain(-1, *gain)
    b.set_chmap(-1, cmap)
    if a.dead:
        import numpy as np
        z = np.zeros(T * Cn, dtype=np.int16)
        for s in range(S):
            b.upload(s, z)
    else:
        b.generate(cm.GEN_NOISE, 12345, T)
    b.sync()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:                 # the batch's own launches bring the clocks up
        for _ in range(8):
            b.run(T)
        b.sync()
    off, on, corr = [], [], []
    for _ in range(a.reps):
        assert b.set_watch(0) == 0
        off.append(timed(b, T, a.steps))
        assert b.set_watch(1) == 0
        on.append(timed(b, T, a.steps))
        assert b.set_watch(0) == 0
        if Cn == 2:
            assert b.set_correlation(1) == 0
            corr.append(timed(b, T, a.steps))
            assert b.set_correlation(0) == 0
    assert b.set_watch(1) == 0
    b.run(T)
    out, rc = b.watch_results()
    assert rc[0] == 0 and out[0].frames == T
    tile, fold = [], []
    for k in range(20):
        t_ms, f_ms = cm.watch_time(b, T)
        if k >= 5:
            tile.append(t_ms)
            fold.append(f_ms)
    b.watch_reset(-1)
    frames = S * T
    read_gbs = b.ceiling(0, 10)
    med = statistics.median
    line = {"shape": name, "input": "silence" if a.dead else "noise", "streams": S, "channels": Cn, "frames": T,
            "reps": a.reps, "steps": a.steps,
            "step_ms_off": round(med(off), 4), "step_ms_watch": round(med(on), 4),
            "step_ms_off_all": [round(v, 4) for v in off], "step_ms_watch_all": [round(v, 4) for v in on],
            "watch_ms_by_difference": round(med(on) - med(off), 4),
            "tile_pass_ms_events": round(med(tile), 4), "tile_pass_ms_min": round(min(tile), 4),
            "fold_ms_events": round(med(fold), 4),
            "read_ceiling_GBs": round(read_gbs, 1),
            "read_ceiling_ms": round(frames * Cn * 2 / (read_gbs * 1e9) * 1e3, 4) if read_gbs > 0 else None,
            "dead_frames_stream0": out[0].dead_frames, "dc_stream0": out[0].dc[0]}
    if corr:
        line["step_ms_corr"] = round(med(corr), 4)
        line["corr_ms_by_difference"] = round(med(corr) - med(off), 4)
    counts = count_asm(Cn)
    if counts:
        line.update(counts)
        line["issue_floor_ms"] = round(frames * counts["valu_per_frame"] / LANES_PER_CYCLE / CLOCK_HZ * 1e3, 4)
    print(json.dumps(line), flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--shapes", default="c2,c4")
    ap.add_argument("--dead", action="store_true", help="every slot silent instead of noise")
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    if a.count_asm:
        print(json.dumps({"k_watch_fast<1>": count_asm(1), "k_watch_fast<2>": count_asm(2)}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    if cm.device_count() < 1:
        raise SystemExit("bench_watch: no HIP device visible; nothing is measured without one")
    for name in a.shapes.split(","):
        measure(cm, name, a)


if __name__ == "__main__":
    main()
