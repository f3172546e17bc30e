#!/usr/bin/env python3
"""What loudness metering (cmhip_batch_set_loudness) costs a step, and how k_loud's time moves with the row count.

The kernel is serial along a stream (the recurrence's bits are fixed); rows -- one channel of one stream -- are its
only parallelism, one lane each.  Shapes: stereo streams of 65536 frames, 64 / 512 / 4096 / 32768 of them (128, 1024,
8192 and 65536 rows; 4096 streams is the config-2 shape), each a CMHIP_VU-only batch created the default way, GEN_NOISE
input, config 2's gains and map.  After 150 ms of the batch's own launches the step (launch + wait) is timed with
loudness off and on, alternating in one process: medians of REPS x STEPS steps; the difference is the pass.  Beside
them the instruction count per sample and row over the stereo loop of build/k_loud.s (`make asm`).

The kernel's own duration comes from a run under the profiler, the program directly after `--`, no counters:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_loudness.py --profile [--shapes r8192]

HBM traffic comes from a counter pass of its own (no tracing beside it):

    rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/bench_loudness.py --profile --shapes r8192

    python tools/bench_loudness.py [--reps N] [--steps N] [--shapes r128,r1024,r8192,r65536]   one JSON line per shape
    python tools/bench_loudness.py --group               the group's step, 1024 streams x 512 frames, off and on
    python tools/bench_loudness.py --count-asm           the instruction count alone (no GPU needed)
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 65536
SHAPES = {"r128": 64, "r1024": 512, "r8192": 4096, "r65536": 32768}       # stereo streams


def count_asm():
    """Instructions of k_loud_vec<2>'s vector loop in build/k_loud.s: the span of the backward branch that holds the
    most v_mul_f64 (four frames of the recurrence, the sub-block edges' code included), per frame."""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_loud.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    m = re.search(r"^_ZN5cmhip10k_loud_vecILi2EEEvNS_8LoudArgsE:(.*?)s_endpgm", text, flags=re.S | re.M)
    if not m:
        return None
    lines = [ln.split(";")[0].strip() for ln in m.group(1).splitlines()]
    lines = [ln for ln in lines if ln and (not ln.startswith(".") or re.fullmatch(r"\.LBB\w+:", ln))]
    label_at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    best = None
    for i, ln in enumerate(lines):
        mm = re.match(r"s_cbranch_\w+\s+(\.LBB\w+)", ln) or re.match(r"s_branch\s+(\.LBB\w+)", ln)
        if mm and mm.group(1) in label_at and label_at[mm.group(1)] < i:
            span = [x.split()[0] for x in lines[label_at[mm.group(1)]:i + 1] if not x.endswith(":")]
            muls = sum(x == "v_mul_f64" for x in span)
            if best is None or muls > best[0]:
                best = (muls, span)
    if not best or best[0] < 4:
        return None
    span = best[1]
    valu = [x for x in span if x.startswith("v_")]
    return {"loop_frames": 4, "valu_per_sample": round(len(valu) / 4.0, 2),
            "f64_per_sample": round(sum(x.endswith("_f64") or "f64" in x for x in valu) / 4.0, 2),
            "all_instructions_per_sample": round(len(span) / 4.0, 2)}


def timed(b, frames, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        b.run(frames)
    b.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def group_step(cm, reps):
    """coolmic_group_t, 1024 stereo null sources x 512-frame blocks: the pump with loudness off and on, alternating"""
    N, block, C, rounds = 1024, 512, 2, 8
    res = {"off": [], "on": []}
    for rep in range(reps):
        for mode in ("off", "on"):
            grp = cm.Group(C, N, block, queue_blocks=rounds + 2)
            grp.set_pull_threads(4)
            if mode == "on":
                assert grp.set_loudness(1) == 0
            hs = []
            for i in range(N):
                dev = cm.Snddev("null", 48000, C)
                h = dev.get_iohandle()
                slot = grp.add_stream(h)
                h.unref()
                dev.unref()
                grp.set_master_gain(slot, C, 1000, [900, 1100])
                hs.append(grp.get_iohandle(slot))
            nbytes = block * 2 * C
            for _ in range(2):
                grp.pump()
                for h in hs:
                    h.read(nbytes)
            t0 = time.perf_counter()
            for _ in range(rounds):
                grp.pump()
            n, _d = hs[0].read(nbytes)
            t1 = time.perf_counter()
            assert n == nbytes
            res[mode].append((t1 - t0) / rounds * 1e3)
            for i, h in enumerate(hs):
                for r in range(rounds if i else rounds - 1):
                    h.read(nbytes)
            for h in hs:
                h.unref()
            grp.unref()
    print(json.dumps({"group": True, "streams": N, "channels": C, "block": block, "pull_threads": 4, "reps": reps,
                      "pump_ms_off": round(statistics.median(res["off"]), 4),
                      "pump_ms_on": round(statistics.median(res["on"]), 4),
                      "pump_ms_off_all": [round(v, 4) for v in res["off"]],
                      "pump_ms_on_all": [round(v, 4) for v in res["on"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default="r128,r1024,r8192,r65536")
    ap.add_argument("--profile", action="store_true", help="a short run for the profiler: 5 steps with loudness on")
    ap.add_argument("--group", action="store_true")
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    counts = count_asm()
    if a.count_asm:
        print(json.dumps({"k_loud_vec2": counts}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    if a.group:
        group_step(cm, a.reps)
        return
    for name in a.shapes.split(","):
        S, C, T = SHAPES[name], 2, FRAMES
        b = cm.Batch(S, C, T, flags=cm.VU)
        b.set_gain(-1, 2, 1000, [750, 1250])
        b.set_chmap(-1, [1, 0])
        b.generate(cm.GEN_NOISE, 12345, T)
        b.sync()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:             # the batch's own launches bring the clocks up
            for _ in range(8):
                b.run(T)
            b.sync()
        if a.profile:
            assert b.set_loudness(1) == 0
            for _ in range(5):
                b.run(T)
            b.sync()
            b.close()
            continue
        off, on = [], []
        for _ in range(a.reps):
            assert b.set_loudness(0) == 0
            off.append(timed(b, T, a.steps))
            assert b.set_loudness(1) == 0
            on.append(timed(b, T, a.steps))
        rc, r = b.loud_result(0)
        assert rc == 0 and r.frames == a.steps * T
        line = {"shape": name, "rows": S * C, "streams": S, "channels": C, "frames": T, "reps": a.reps, "steps": a.steps,
                "step_ms_off": round(statistics.median(off), 4), "step_ms_on": round(statistics.median(on), 4),
                "step_ms_off_all": [round(v, 4) for v in off], "step_ms_on_all": [round(v, 4) for v in on],
                "loudness_ms_by_difference": round(statistics.median(on) - statistics.median(off), 4),
                "ns_per_sample_of_a_row": round((statistics.median(on) - statistics.median(off)) * 1e6 / T, 2),
                "integrated_stream0": r.integrated}
        if counts:
            line.update(counts)
        print(json.dumps(line), flush=True)
        b.close()


if __name__ == "__main__":
    main()
