#!/usr/bin/env python3
"""How long a limiter run with the true-peak detector (cmhip_lim_new_detector, csrc/k_limtp.hip) takes, beside the
sample detector of the same geometry on the same arrays.

Shapes: mono and stereo at lookahead 64 with the shortest hold (a = 6, H = 1), mono and stereo at lookahead 256 with a
hold of 1024 frames (a = 8, H = 1024), and six channels at a = 6, H = 1; 65536 frames per stream and as many streams as
make about 1 GiB of input.  The input is GEN_NOISE in the slots of a batch used as device memory (full-scale noise
driven by 2 against a threshold of 29204: every frame is reduced), the output plain device memory.  Per shape and
detector: after 150 ms of the limiter's own launches every run is bracketed by HIP events on the limiter's stream;
reported is the median of --steps runs and the bandwidth of the algorithmic bytes, 4 * C per frame.  Beside them:
cmhip_batch_ceiling's plain copy on the input batch's own slots (read + write), the yardstick.

    python tools/bench_limtp.py [--steps N] [--shapes a,b]    one JSON line per shape
    python tools/bench_limtp.py --count-asm                   per kernel the instructions of build/k_limtp.s (`make asm`;
                                                              no GPU needed): the whole kernel, and the FIR's share per
                                                              sample of the fast forms
    python tools/bench_limtp.py --release [--steps N] [--shapes a,b]
        tools/bench_lim.py --release with the true-peak detector: release_log2 0 (k_limtp.hip's kernel), 6 and 11
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
SHAPES = {          # streams, channels, frames, lookahead_log2, hold
    "m1_a6": (8192, 1, 65536, 6, 1),
    "s2_a6": (4096, 2, 65536, 6, 1),
    "m1_a8_h1024": (8192, 1, 65536, 8, 1024),
    "s2_a8_h1024": (4096, 2, 65536, 8, 1024),
    "x6_a6": (1365, 6, 65536, 6, 1),
}
THRESHOLD, DRIVE = 29204, 8192
FAST_SAMPLES = {"1": 4 * 8, "2": 7 * 8}      # samples of a thread's own vectors in the unrolled step 1 (4 / 7 vectors)


def count_asm():
    """per kernel of build/k_limtp.s: all its instructions by class; for the fast forms step 1 is fully unrolled over the
    thread's own vectors, so dots / samples is the FIR's cost and (VALU of the kernel - VALU of k_lim's kernel) / samples
    bounds what the detector adds per sample"""
    out = {}
    for stem in ("k_limtp", "k_lim"):
        path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", stem + ".s")
        if not os.path.exists(path):
            return None
        text = open(path).read()
        for m in re.finditer(r"^(_ZN5cmhip\w*%s_(?:fast|any)\w*):.*?^\s*s_endpgm" % stem, text, flags=re.S | re.M):
            sym, body = m.group(1), m.group(0)
            f = re.search(r"_fastILi(\d)E", sym)
            name = "%s_fast<%s>" % (stem, f.group(1)) if f else stem + "_any"
            ops = []
            for ln in body.splitlines():
                ln = ln.split(";")[0].strip()
                if ln and not ln.startswith(".") and not ln.endswith(":"):
                    ops.append(ln.split()[0])
            n = lambda pre: sum(op.startswith(pre) for op in ops)
            out[name] = {"valu": n("v_"), "salu": n("s_"), "dot2": n("v_dot2"), "mad_u64": n("v_mad_u64_u32"),
                         "mad_i64": n("v_mad_i64_i32"), "rcp": n("v_rcp"), "perm_alignbit": n("v_perm") + n("v_alignbit"),
                         "lds_reads": n("ds_read") + n("ds_load"), "lds_writes": n("ds_write") + n("ds_store"),
                         "barriers": n("s_barrier"), "loads_16B": n("global_load_dwordx4"),
                         "stores_16B": n("global_store_dwordx4")}
    per_sample = {}
    for c, samples in FAST_SAMPLES.items():
        tp, sm = out.get("k_limtp_fast<%s>" % c), out.get("k_lim_fast<%s>" % c)
        if tp and sm:
            per_sample["fast<%s>" % c] = {"samples_in_step_1": samples, "dot2": round(tp["dot2"] / samples, 2),
                                          "valu_added": round((tp["valu"] - sm["valu"]) / samples, 2)}
    return {"kernels": out, "step_1_per_sample": per_sample}


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--count-asm", action="store_true")
    ap.add_argument("--release", action="store_true")
    a = ap.parse_args()
    if a.count_asm:
        print(json.dumps({"k_limtp": count_asm()}))
        return
    if a.release:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import __graft_entry__ as ge
        import bench_lim
        bench_lim.release_main(ge.load_package(), SHAPES, a.shapes.split(","), a.steps, 1)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, ch, F, la, hold = SHAPES[name]
        src = cm.Batch(S, ch, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        out_stride = (F * ch + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        rd = wr = S * F * ch * 2
        copy = src.ceiling(1)
        line = {"shape": name, "streams": S, "channels": ch, "frames": F, "lookahead_log2": la, "hold": hold,
                "threshold": THRESHOLD, "drive": DRIVE, "steps": a.steps, "read_MB": round(rd / 1e6, 1),
                "written_MB": round(wr / 1e6, 1), "ceiling_copy_GBs_on_the_input_slots": round(copy, 1)}
        for det, key in ((cm.LIM_DETECT_TRUE_PEAK, "true_peak"), (cm.LIM_DETECT_SAMPLE, "sample")):
            m = cm.Limiter(S, ch, la, hold, F, threshold=THRESHOLD, drive=DRIVE, detector=det)
            st = C.c_void_p(m.hip_stream())
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:         # the limiter's own launches bring the clocks up
                m.run(src.dev_in, src.stride, F, dst, out_stride)
                m.sync()
            ms = []
            for _ in range(a.steps):
                assert hip.hipEventRecord(e0, st) == 0
                m.run(src.dev_in, src.stride, F, dst, out_stride)
                assert hip.hipEventRecord(e1, st) == 0
                assert hip.hipEventSynchronize(e1) == 0
                t = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
                ms.append(t.value)
            p = (cm.plan_limtp if det else cm.plan_lim)(S, ch, la, hold, F)
            med = statistics.median(ms)
            line[key] = {"delay": m.delay(), "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4),
                         "kernel_ms_max": round(max(ms), 4), "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                         "of_ceiling": round((rd + wr) / med / 1e6 / copy, 3) if copy > 0 else None,
                         "min_gain_stream0": int(m.min_gain()[0]),
                         "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "halo": p.halo, "chunks": p.chunks,
                                  "grid": p.grid, "block": p.block, "lds_bytes": p.lds_bytes}}
            m.close()
        line["true_peak_over_sample"] = round(line["true_peak"]["kernel_ms_median"] / line["sample"]["kernel_ms_median"], 3)
        print(json.dumps(line), flush=True)
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_limtp": count_asm()}))


if __name__ == "__main__":
    main()
