#!/usr/bin/env python3
"""How long a limiter run (cmhip_lim_run, csrc/k_lim.hip) takes, and what it moves.

Shapes: mono and stereo at lookahead 64 without hold (a = 6, H = 0), mono and stereo at lookahead 256 with a hold of
1024 frames (a = 8, H = 1024), and six channels at a = 6, H = 0; 65536 frames per stream and as many streams as make
about 1 GiB of input.  The input is GEN_NOISE in the slots of a batch used as device memory (full-scale noise driven by
2 against a threshold of 29204: every frame is reduced), the output plain device memory.  After 150 ms of the limiter's
own launches every run is bracketed by HIP events on the limiter's stream; reported is the median of --steps runs and
the bandwidth of the algorithmic bytes, 4 * C per frame.  Beside it: cmhip_batch_ceiling's plain copy on the input
batch's own slots (read + write), the yardstick.

    python tools/bench_lim.py [--steps N] [--shapes a,b]      one JSON line per shape
    python tools/bench_lim.py --count-asm                     per kernel the instructions of build/k_lim.s (`make asm`;
                                                              no GPU needed), and the passes per geometry
    python tools/bench_lim.py --release [--steps N] [--shapes a,b]
        the release stage (cmhip_lim_new_release, csrc/k_limrel.hip): per shape three limiters in one process on the same
        arrays, release_log2 0 (k_lim.hip's kernel as it always ran), 6 and 11, timed the same way; beside each time its
        ratio to the release_log2 0 time and what the structure predicts, (P + rho) / P * (t + halo_rho) / (t + halo_0),
        P the passes without the stage
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
    "m1_a6": (8192, 1, 65536, 6, 0),
    "s2_a6": (4096, 2, 65536, 6, 0),
    "m1_a8_h1024": (8192, 1, 65536, 8, 1024),
    "s2_a8_h1024": (4096, 2, 65536, 8, 1024),
    "x6_a6": (1365, 6, 65536, 6, 0),
}
THRESHOLD, DRIVE = 29204, 8192
ELEMENTS = 26       # per thread and pass (csrc/k_lim.h: LIM_R, the slots of the kernels without a release)


def passes(a, hold):
    """doubling passes of a tile: minimum (and the combining one when W is no power of two), sum"""
    W = (1 << a) + hold
    p = W.bit_length() - 1
    return {"min": p + (1 if W > (1 << p) else 0), "sum": a}


def count_asm():
    """per kernel of build/k_lim.s: all its instructions by class, and the straight-line block with the most LDS
    operations -- the body of one doubling pass over a thread's 26 elements"""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_lim.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN5cmhip\w*k_lim_(?:fast|any)\w*):.*?^\s*s_endpgm", text, flags=re.S | re.M):
        sym, body = m.group(1), m.group(0)
        f = re.search(r"k_lim_fastILi(\d)E", sym)
        name = "k_lim_fast<%s>" % f.group(1) if f else "k_lim_any"
        blocks, cur = [], []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                if ln.startswith(".LBB") and cur:
                    blocks.append(cur)
                    cur = []
                continue
            cur.append(ln.split()[0])
            if ln.startswith(("s_cbranch", "s_branch")):
                blocks.append(cur)
                cur = []
        blocks.append(cur)
        ops = [op for b in blocks for op in b]

        def classes(b):
            n = lambda pre: sum(op.startswith(pre) for op in b)
            return {"valu": n("v_"), "lds_reads": n("ds_read") + n("ds_load"), "lds_writes": n("ds_write") + n("ds_store"),
                    "barriers": n("s_barrier"), "loads_16B": n("global_load_dwordx4"),
                    "stores_16B": n("global_store_dwordx4"), "mad_i64": n("v_mad_i64_i32"), "rcp": n("v_rcp")}
        best = max(blocks, key=lambda b: sum(op.startswith("ds_") for op in b))
        rec = {"whole_kernel": classes(ops), "largest_lds_block": classes(best)}
        lb = rec["largest_lds_block"]
        rec["per_element_of_that_block"] = {k: round(lb[k] / ELEMENTS, 2) for k in ("valu", "lds_reads", "lds_writes")}
        out[name] = rec
    return {"kernels": out, "passes": {k: passes(v[3], v[4]) for k, v in SHAPES.items()}}


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


RELEASES = (0, 6, 11)


def timed_runs(cm, hip, m, src, F, dst, out_stride, steps):
    """150 ms of the limiter's own launches, then `steps` runs bracketed by HIP events -> the times in ms"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    st = C.c_void_p(m.hip_stream())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        m.run(src.dev_in, src.stride, F, dst, out_stride)
        m.sync()
    ms = []
    for _ in range(steps):
        assert hip.hipEventRecord(e0, st) == 0
        m.run(src.dev_in, src.stride, F, dst, out_stride)
        assert hip.hipEventRecord(e1, st) == 0
        assert hip.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        ms.append(t.value)
    return ms


def release_main(cm, shapes, names, steps, detector):
    """--release: per shape one JSON line with the release_log2 0, 6 and 11 limiters of one detector"""
    hip = hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    for name in names:
        S, ch, F, la, hold = shapes[name]
        src = cm.Batch(S, ch, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        out_stride = (F * ch + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        rd = wr = S * F * ch * 2
        P = sum(passes(la, hold).values())
        line = {"shape": name, "detector": detector, "streams": S, "channels": ch, "frames": F, "lookahead_log2": la,
                "hold": hold, "threshold": THRESHOLD, "drive": DRIVE, "steps": steps, "passes_without_release": P}
        base = None
        for rho in RELEASES:
            m = cm.Limiter(S, ch, la, hold, F, threshold=THRESHOLD, drive=DRIVE, detector=detector, release_log2=rho)
            ms = timed_runs(cm, hip, m, src, F, dst, out_stride, steps)
            p = cm.plan_limrel(detector, S, ch, la, hold, rho, F)
            med = statistics.median(ms)
            if rho == 0:
                base = (med, p.tile_frames + p.halo)
            line["release_log2_%d" % rho] = {
                "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1), "over_release_0": round(med / base[0], 3),
                "predicted_over_release_0": round((P + rho) / P * (p.tile_frames + p.halo) / base[1], 3),
                "min_gain_stream0": int(m.min_gain()[0]), "halo": p.halo, "lds_bytes": p.lds_bytes}
            m.close()
        print(json.dumps(line), flush=True)
        cm.lib.cmhip_device_free(0, dst)
        src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--count-asm", action="store_true")
    ap.add_argument("--release", action="store_true")
    a = ap.parse_args()
    if a.count_asm:
        print(json.dumps({"k_lim": count_asm()}))
        return
    if a.release:
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        release_main(ge.load_package(), SHAPES, a.shapes.split(","), a.steps, 0)
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
        m = cm.Limiter(S, ch, la, hold, F, threshold=THRESHOLD, drive=DRIVE)
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
        st = C.c_void_p(m.hip_stream())
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:             # the limiter's own launches bring the clocks up
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
        p = cm.plan_lim(S, ch, la, hold, F)
        med = statistics.median(ms)
        rd = wr = S * F * ch * 2
        copy = src.ceiling(1)
        line = {"shape": name, "streams": S, "channels": ch, "frames": F, "lookahead_log2": la, "hold": hold,
                "threshold": THRESHOLD, "drive": DRIVE, "steps": a.steps, "kernel_ms_median": round(med, 4),
                "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "halo_reread": round((p.tile_frames + p.halo) / p.tile_frames, 3),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "ceiling_copy_GBs_on_the_input_slots": round(copy, 1),
                "of_ceiling": round((rd + wr) / med / 1e6 / copy, 3) if copy > 0 else None,
                "min_gain_stream0": int(m.min_gain()[0]), "passes": passes(la, hold),
                "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "halo": p.halo, "chunks": p.chunks,
                         "grid": p.grid, "block": p.block, "lds_bytes": p.lds_bytes}}
        print(json.dumps(line), flush=True)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_lim": count_asm()}))


if __name__ == "__main__":
    main()
