#!/usr/bin/env python3
"""How long a run of the dynamics stage (cmhip_dyn_run, csrc/k_dyn.hip) takes, and what it moves.

Shapes: mono and stereo at the short geometry (a = 6, b = 6, H = 0: 18 passes), mono and stereo at the longest one
(a = 10, b = 9, H = 1536: 30 passes), and six channels at the short one; 65536 frames per stream and as many streams as
make about 1 GiB of input.  The input is GEN_NOISE in the slots of a batch used as device memory, the curve a
compressor and gate (-18 dBFS 4:1 knee 6 dB, -45 dBFS 1:2 range 40 dB), the output plain device memory.  After 150 ms of
the stage's own launches every run is bracketed by HIP events on the stage's stream; reported is the median of --steps
runs and the bandwidth of the algorithmic bytes, 4 * C per frame.  Beside it, on the same input slots:
cmhip_batch_ceiling's plain copy (read + write), the yardstick, and the peak limiter (tools/bench_lim.py's loop) at its
nearest pass counts (a = 8, H = 1024: 19 passes; a = 9, H = 1536: 20 passes).

    python tools/bench_dyn.py [--steps N] [--shapes a,b]      one JSON line per shape
    python tools/bench_dyn.py --count-asm                     per kernel the instructions of build/k_dyn.s
                                                              (`make asm`; no GPU needed), and the passes per geometry
    python tools/bench_dyn.py --key [--steps N] [--shapes a,b]
        side-chain keys (cmhip_dyn_set_key; k_dynk<CT, DET>): per shape, on one object, the same slots and in one
        process, the plain run (no key set: k_dyn<CT, DET>), the plain run again (its repeat shows the spread of
        the unkeyed kernels inside one session), a run with every odd stream keyed on its even neighbour, a run with
        every stream keyed (on its neighbour, 2i <-> 2i + 1), and the plain run a third time after the keys were
        cleared; one JSON line per shape with the medians and their min-max
    python tools/bench_dyn.py --rms [--steps N] [--shapes a,b]
        the RMS detector (cmhip_dyn_new_detector; DET = DYN_DETECT_RMS) beside the mean detector: per shape two objects of
        one geometry on the same arrays in one process, in the order mean, RMS, mean again, then both with every stream
        keyed (2i <-> 2i + 1); one JSON line per shape with the medians, their min-max, the pass counts of both plans
        and RMS over mean beside (P + a) / P; then the instruction counts of the RMS kernels
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {          # streams, channels, frames, detector_log2, smooth_log2, hold
    "m1_a6_b6": (8192, 1, 65536, 6, 6, 0),
    "s2_a6_b6": (4096, 2, 65536, 6, 6, 0),
    "m1_a10_b9_h1536": (8192, 1, 65536, 10, 9, 1536),
    "s2_a10_b9_h1536": (4096, 2, 65536, 10, 9, 1536),
    "x6_a6_b6": (1365, 6, 65536, 6, 6, 0),
}
LIMITER = {         # the limiter beside a shape: lookahead_log2, hold
    "m1_a6_b6": (8, 1024), "s2_a6_b6": (8, 1024), "m1_a10_b9_h1536": (9, 1536), "s2_a10_b9_h1536": (9, 1536),
}
CURVE = dict(comp_threshold_db=-18.0, comp_ratio=4.0, comp_knee_db=6.0, gate_threshold_db=-45.0, gate_ratio=2.0,
             gate_range_db=40.0)
ELEMENTS = 30       # per thread and pass (k_dyn.hip: DYN_R)


def passes(a, b, hold):
    """doubling passes of a tile: detector sum, maximum (and the combining one when W is no power of two), ramp sum"""
    W = (1 << b) + hold
    p = W.bit_length() - 1
    return {"detector_sum": a, "max": p + (1 if W > (1 << p) else 0), "ramp_sum": b,
            "all": a + p + (1 if W > (1 << p) else 0) + b}


def count_asm(stem="k_dyn"):
    """per kernel of build/k_dyn.s that `stem` names -- "k_dyn": k_dyn<CT, MEAN>, "k_dynk": k_dynk<CT, MEAN>, "k_dynrms":
    k_dyn<CT, RMS>, "k_dynrmsk": k_dynk<CT, RMS>; printed as <stem>_fast<CT> and, for CT = 0, <stem>_any, the names the
    earlier records carry -- all its instructions by class, and, cut at the barriers, the two phases of a doubling
    pass over a thread's 30 elements and the curve lookup between the passes"""
    template, det = {"k_dyn": ("k_dyn", 0), "k_dynk": ("k_dynk", 0), "k_dynrms": ("k_dyn", 1),
                     "k_dynrmsk": ("k_dynk", 1)}[stem]
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_dyn.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^_ZN5cmhip\d+%sILi(\d)ELj%dEE\w*:.*?^\s*s_endpgm" % (template, det), text, flags=re.S | re.M):
        ct, body = m.group(1), m.group(0)
        name = "%s_fast<%s>" % (stem, ct) if ct != "0" else stem + "_any"
        # the kernel cut at its barriers.  Inside a loop of doubling passes the stretch from one pass's middle barrier
        # to the next one's holds the first one's 30 writes and the next one's 30 partner reads: one pass's worth of
        # work, the leanest stretch with both.  The curve lookup (30 table reads, 30 writes) is the heaviest such stretch.
        segs, cur = [], []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                continue
            op = ln.split()[0]
            if op == "s_barrier":
                segs.append(cur)
                cur = []
            else:
                cur.append(op)
        segs.append(cur)
        ops = [op for b in segs for op in b]

        def classes(b):
            n = lambda pre: sum(op.startswith(pre) for op in b)
            return {"valu": n("v_"), "salu": n("s_"), "lds_reads": n("ds_read") + n("ds_load"),
                    "lds_writes": n("ds_write") + n("ds_store"), "loads_16B": n("global_load_dwordx4"),
                    "stores_16B": n("global_store_dwordx4")}
        cl = [classes(b) for b in segs]
        both = [c for c in cl if c["lds_writes"] >= ELEMENTS and c["lds_reads"] >= ELEMENTS]
        rec = {"whole_kernel": dict(classes(ops), barriers=len(segs) - 1), "stretches_with_30_reads_and_30_writes": both}
        if both:
            lean, heavy = min(both, key=lambda c: c["valu"]), max(both, key=lambda c: c["valu"])
            rec["per_element_and_pass"] = {k: round(lean[k] / ELEMENTS, 2) for k in ("valu", "salu", "lds_reads", "lds_writes")}
            rec["per_element_of_the_lookup"] = {k: round(heavy[k] / ELEMENTS, 2) for k in ("valu", "lds_reads", "lds_writes")}
        # the loops of doubling passes as the assembler laid them out: from a backward branch's target to the branch, two
        # barriers inside.  (In the RMS kernels the stretch with 30 reads and 30 writes above is not a pass but the first
        # split -- own elements read, squared, the low halves written -- so there the loops are the per-pass figures.)
        ins, labels = [], {}
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            lab = re.match(r"(\.LBB\w+):", ln)
            if lab:
                labels[lab.group(1)] = len(ins)
            elif ln and not ln.startswith(".") and not ln.endswith(":"):
                ins.append(ln)
        found = []
        for k, ln in enumerate(ins):
            br = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ln)
            if br and labels.get(br.group(1), k + 1) <= k:
                b = [x.split()[0] for x in ins[labels[br.group(1)]:k + 1]]
                n = lambda pre: sum(op.startswith(pre) for op in b)
                if n("s_barrier") == 2 and n("ds_read") >= ELEMENTS - 1 and n("ds_write") >= ELEMENTS - 1:
                    found.append({"valu": n("v_"), "salu": n("s_") - n("s_barrier") - n("s_waitcnt") - n("s_nop"),
                                  "lds_reads": n("ds_read"), "lds_writes": n("ds_write"), "instructions": len(b)})
        rec["pass_loops"] = found
        if stem.startswith("k_dynrms"):
            rec.pop("per_element_and_pass", None)
        out[name] = rec
    return {"kernels": out, "passes": {k: passes(v[3], v[4], v[5]) for k, v in SHAPES.items()}}


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def timed(hip, stage, steps, run):
    """median, min, max in ms of `steps` runs bracketed by events on the stage's stream, after 150 ms of its own launches"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    st = C.c_void_p(stage.hip_stream())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:                 # the stage's own launches bring the clocks up
        run()
        stage.sync()
    ms = []
    for _ in range(steps):
        assert hip.hipEventRecord(e0, st) == 0
        run()
        assert hip.hipEventRecord(e1, st) == 0
        assert hip.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        ms.append(t.value)
    return statistics.median(ms), min(ms), max(ms)


def keyed(a):
    """--key: the plain run, its repeat, odd streams keyed, every stream keyed, the plain run again: one object per shape"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, ch, F, la, lb, hold = SHAPES[name]
        S -= S % 2                                              # pairs
        src = cm.Batch(S, ch, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        m = cm.Dynamics(S, ch, la, lb, hold, F, curve=cm.dyn_design(**CURVE))
        out_stride = (F * ch + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
        run = lambda: m.run(src.dev_in, src.stride, F, dst, out_stride)
        rec = lambda t: {"kernel_ms_median": round(t[0], 4), "kernel_ms_min": round(t[1], 4), "kernel_ms_max": round(t[2], 4)}
        line = {"shape": name, "key": True, "streams": S, "channels": ch, "frames": F, "detector_log2": la,
                "smooth_log2": lb, "hold": hold, "steps": a.steps, "passes": passes(la, lb, hold)["all"]}
        line["plain"] = rec(timed(hip, m, a.steps, run))
        line["plain_repeated"] = rec(timed(hip, m, a.steps, run))
        for s in range(1, S, 2):
            m.set_key(s, s - 1)
        line["odd_streams_keyed"] = rec(timed(hip, m, a.steps, run))
        for s in range(0, S, 2):
            m.set_key(s, s + 1)
        line["every_stream_keyed"] = rec(timed(hip, m, a.steps, run))
        m.set_key(-1, -1)
        line["plain_after_clearing"] = rec(timed(hip, m, a.steps, run))
        base = line["plain"]["kernel_ms_median"]
        for k in ("plain_repeated", "odd_streams_keyed", "every_stream_keyed", "plain_after_clearing"):
            line[k]["over_plain"] = round(line[k]["kernel_ms_median"] / base, 4)
        line["MB_read_by_the_detector_from_another_slot"] = {"odd_streams_keyed": round(S // 2 * F * ch * 2 / 1e6, 1),
                                                             "every_stream_keyed": round(S * F * ch * 2 / 1e6, 1)}
        print(json.dumps(line), flush=True)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_dynk": count_asm("k_dynk")}))


def rms(a):
    """--rms: per shape the mean detector, the RMS detector, the mean detector again, then both with every stream keyed"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, ch, F, la, lb, hold = SHAPES[name]
        S -= S % 2                                              # pairs
        src = cm.Batch(S, ch, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        curve = cm.dyn_design(**CURVE)
        mean = cm.Dynamics(S, ch, la, lb, hold, F, curve=curve)
        root = cm.Dynamics(S, ch, la, lb, hold, F, curve=curve, detector=cm.DYN_DETECT_RMS)
        assert (mean.detector(), root.detector()) == (cm.DYN_DETECT_MEAN, cm.DYN_DETECT_RMS)
        out_stride = (F * ch + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
        rec = lambda t: {"kernel_ms_median": round(t[0], 4), "kernel_ms_min": round(t[1], 4), "kernel_ms_max": round(t[2], 4)}
        go = lambda m: rec(timed(hip, m, a.steps, lambda: m.run(src.dev_in, src.stride, F, dst, out_stride)))
        pm, pr = cm.plan_dyn(S, ch, la, lb, hold, F), cm.plan_dynrms(S, ch, la, lb, hold, F)
        line = {"shape": name, "rms": True, "streams": S, "channels": ch, "frames": F, "detector_log2": la,
                "smooth_log2": lb, "hold": hold, "steps": a.steps, "passes_mean": pm.passes, "passes_rms": pr.passes,
                "lds_bytes": [pm.lds_bytes, pr.lds_bytes], "expected_rms_over_mean": round(pr.passes / pm.passes, 4)}
        line["mean"] = go(mean)
        line["rms_detector"] = go(root)
        line["mean_repeated"] = go(mean)
        for m in (mean, root):
            for s in range(S):
                m.set_key(s, s ^ 1)
        line["mean_every_stream_keyed"] = go(mean)
        line["rms_every_stream_keyed"] = go(root)
        line["min_gain_stream0"] = {"mean": int(mean.min_gain()[0]), "rms": int(root.min_gain()[0])}
        line["rms_over_mean"] = round(line["rms_detector"]["kernel_ms_median"] / line["mean"]["kernel_ms_median"], 4)
        line["rms_over_mean_keyed"] = round(line["rms_every_stream_keyed"]["kernel_ms_median"] /
                                            line["mean_every_stream_keyed"]["kernel_ms_median"], 4)
        line["mean_repeated_over_mean"] = round(line["mean_repeated"]["kernel_ms_median"] / line["mean"]["kernel_ms_median"], 4)
        print(json.dumps(line), flush=True)
        mean.close()
        root.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_dynrms": count_asm("k_dynrms"), "k_dynrmsk": count_asm("k_dynrmsk")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--count-asm", action="store_true")
    ap.add_argument("--key", action="store_true")
    ap.add_argument("--rms", action="store_true")
    a = ap.parse_args()
    if a.count_asm:
        print(json.dumps({"k_dyn": count_asm(), "k_dynk": count_asm("k_dynk"), "k_dynrms": count_asm("k_dynrms"),
                          "k_dynrmsk": count_asm("k_dynrmsk")}))
        return
    if a.rms:
        rms(a)
        return
    if a.key:
        keyed(a)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, ch, F, la, lb, hold = SHAPES[name]
        src = cm.Batch(S, ch, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        m = cm.Dynamics(S, ch, la, lb, hold, F, curve=cm.dyn_design(**CURVE))
        out_stride = (F * ch + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
        med, lo, hi = timed(hip, m, a.steps, lambda: m.run(src.dev_in, src.stride, F, dst, out_stride))
        p = cm.plan_dyn(S, ch, la, lb, hold, F)
        rd = wr = S * F * ch * 2
        copy = src.ceiling(1)
        line = {"shape": name, "streams": S, "channels": ch, "frames": F, "detector_log2": la, "smooth_log2": lb,
                "hold": hold, "curve": CURVE, "steps": a.steps, "kernel_ms_median": round(med, 4),
                "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "halo_reread": round((p.tile_frames + p.halo) / p.tile_frames, 3),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "ceiling_copy_GBs_on_the_input_slots": round(copy, 1),
                "of_ceiling": round((rd + wr) / med / 1e6 / copy, 3) if copy > 0 else None,
                "min_gain_stream0": int(m.min_gain()[0]), "passes": passes(la, lb, hold),
                "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "halo": p.halo, "chunks": p.chunks,
                         "grid": p.grid, "block": p.block, "lds_bytes": p.lds_bytes, "passes": p.passes}}
        m.close()
        if name in LIMITER:
            a_l, h_l = LIMITER[name]
            lim = cm.Limiter(S, ch, a_l, h_l, F, threshold=29204, drive=8192)
            lmed, llo, lhi = timed(hip, lim, a.steps, lambda: lim.run(src.dev_in, src.stride, F, dst, out_stride))
            W = (1 << a_l) + h_l
            lp = W.bit_length() - 1 + (1 if W & (W - 1) else 0) + a_l
            line["limiter_on_the_same_slots"] = {"lookahead_log2": a_l, "hold": h_l, "passes": lp,
                                                 "kernel_ms_median": round(lmed, 4), "kernel_ms_min": round(llo, 4),
                                                 "kernel_ms_max": round(lhi, 4),
                                                 "dyn_ms_over_lim_ms": round(med / lmed, 3),
                                                 "dyn_ms_per_pass_over_lim_ms_per_pass": round(med / p.passes / (lmed / lp), 3)}
            lim.close()
        print(json.dumps(line), flush=True)
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_dyn": count_asm()}))


if __name__ == "__main__":
    main()
