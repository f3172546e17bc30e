#!/usr/bin/env python3
"""What the spectrum meter (cmhip_batch_set_spectrum) costs a step at n = 8, 10 and 12.

Shape: config 2 (4096 x 2 x 65536), a CMHIP_VU-only batch created the default way, GEN_NOISE input, the gains and map
of bench.py's config, both channels metered over the default bin octaves.  After 150 ms of the batch's own launches
the step (launch + wait) is timed with the meter off and on, alternating in one process on the same arrays: medians
of REPS x STEPS steps; the pass's own time is their difference.  Beside them: the batch's measured read ceiling
(cmhip_batch_ceiling mode 0) and what a plain read of the same slots takes at it, and from build/k_spec.s and
build/k_spec.usage.txt (`make asm`) the VALU instructions of one butterfly, registers, LDS, occupancy and scratch per
size.  Every input sample is in two blocks (the hop is N / 2), and a block of N samples runs n N / 2 butterflies: n
butterflies per input sample.

    python tools/bench_spec.py [--reps N] [--steps N]      one JSON line per size, into profiles/spec_bench.txt too
    python tools/bench_spec.py --count-asm                 the static figures alone (no GPU needed)
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
SIZES = (8, 10, 12)


def count_asm():
    """per size: the VALU instructions of the butterfly loop's body (the basic block of k_spec<n> with the most 64-bit
    multiply-adds), of the whole kernel text, and the usage report's figures"""
    base = os.path.join(ROOT, "libcoolmic-dsp_amd", "build")
    if not os.path.exists(os.path.join(base, "k_spec.s")):
        return None
    text = open(os.path.join(base, "k_spec.s")).read()
    usage = open(os.path.join(base, "k_spec.usage.txt")).read() if os.path.exists(os.path.join(base, "k_spec.usage.txt")) else ""
    out = {}
    for n in SIZES:
        name = "_ZN5cmhip6k_specILj%dEEEvNS_8SpecArgsE" % n
        m = re.search(r"^%s:(.*?)s_endpgm" % re.escape(name), text, flags=re.S | re.M)
        if not m:
            continue
        blocks, cur = [], []
        for ln in m.group(1).splitlines():
            ln = ln.strip()
            if not ln or ln.startswith((";", ".")) and not ln.endswith(":"):
                continue
            if ln.endswith(":"):
                blocks.append(cur)
                cur = []
            else:
                cur.append(ln.split()[0])
        blocks.append(cur)
        body = max(blocks, key=lambda b: sum(i.startswith("v_mad_i64_i32") or i.startswith("v_mad_u64_u32") for i in b))
        valu = sum(i.startswith("v_") for i in body)
        d = {"valu_per_butterfly": valu,
             "mad64_per_butterfly": sum(i.startswith(("v_mad_i64_i32", "v_mad_u64_u32")) for i in body),
             "lds_ops_per_butterfly": sum(i.startswith("ds_") for i in body),
             "valu_per_input_sample_in_the_stages": n * valu,
             "valu_in_kernel_text": sum(i.startswith("v_") for b in blocks for i in b)}
        u = re.search(r"Function Name: %s.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                      r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)" % re.escape(name), usage, flags=re.S)
        if u:
            d.update(vgprs=int(u.group(1)), scratch_bytes=int(u.group(2)), occupancy_waves_per_simd=int(u.group(3)),
                     lds_bytes=int(u.group(4)))
        out[n] = d
    return out


def timed(b, frames, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        b.run(frames)
    b.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    counts = count_asm() or {}
    if a.count_asm:
        print(json.dumps({"k_spec": counts}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    if cm.device_count() < 1:
        raise SystemExit("bench_spec: no HIP device visible; nothing is measured without one")
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
    read_gbs = b.ceiling(0, 10)
    lines = []
    for n in SIZES:
        off, on = [], []
        for _ in range(a.reps):
            assert b.set_spectrum(0) == 0
            assert b.spec_configure(n) == 0
            off.append(timed(b, T, a.steps))
            assert b.set_spectrum(1) == 0
            on.append(timed(b, T, a.steps))
        rc, r = b.spec_result(0)
        blocks = (a.steps * T - (1 << n)) // (1 << (n - 1)) + 1
        assert rc == 0 and r.frames == a.steps * T and r.blocks == blocks
        line = {"shape": "c2", "streams": S, "channels": C, "frames": T, "fft_log2": n, "metered_channels": 2,
                "reps": a.reps, "steps": a.steps,
                "step_ms_off": round(statistics.median(off), 4), "step_ms_on": round(statistics.median(on), 4),
                "step_ms_off_all": [round(v, 4) for v in off], "step_ms_on_all": [round(v, 4) for v in on],
                "spec_ms_by_difference": round(statistics.median(on) - statistics.median(off), 4),
                "read_ceiling_GBs": round(read_gbs, 1),
                "plain_read_ms": round(S * T * C * 2 / (read_gbs * 1e9) * 1e3, 4) if read_gbs > 0 else None,
                "db_stream0_channel0": [round(r.db[0][k], 3) for k in range(r.bands)]}
        line.update(counts.get(n, {}))
        print(json.dumps(line), flush=True)
        lines.append(line)
    assert b.set_spectrum(0) == 0
    b.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "spec_bench.txt"), "w") as f:
        f.write("# python tools/bench_spec.py --reps %d --steps %d  (one JSON line per block size)\n" % (a.reps, a.steps))
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
