#!/usr/bin/env python3
"""How long a mixer run (cmhip_mix_run, csrc/k_mix.hip) takes, and what it moves.

Shapes: 4096 stereo streams x 65536 frames -> mono, 8192 mono -> stereo, 4096 x 2 -> 2 (mid/side), 1365 x 6 -> 2 with
both 5.1 presets, and 512 x 16 -> 16 with dense matrices.  The input is GEN_NOISE in the slots of a batch used as
device memory, the output plain device memory.  After 150 ms of the mixer's own launches every run is bracketed by HIP
events on the mixer's stream; reported is the median of --steps runs and the bandwidth of the algorithmic bytes,
2 * (C_in + C_out) per frame.  Beside it: cmhip_batch_ceiling's plain copy on the input batch's own slots (buffers of
the input's size, read + write), the yardstick.

    python tools/bench_mix.py [--steps N] [--shapes a,b]      one JSON line per shape
    python tools/bench_mix.py --ramp [--steps N] [--shapes a,b]
                                                              matrix ramps (csrc/k_mixramp.hip), per shape (default
                                                              s2_to_ms, s2_to_m1) in one process on the same buffers:
                                                              (a) a plain run, (b) a run with every stream mid-ramp,
                                                              (c) a run with one stream in 64 ramping
    python tools/bench_mix.py --count-asm                     instructions per output sample of each kernel, from
                                                              build/k_mix.s (`make asm`; no GPU needed)
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
SHAPES = {          # streams, C_in, C_out, frames, preset (None: dense)
    "s2_to_m1": (4096, 2, 1, 65536, "MIX_STEREO_TO_MONO"),
    "m1_to_s2": (8192, 1, 2, 65536, "MIX_MONO_TO_STEREO"),
    "s2_to_ms": (4096, 2, 2, 65536, "MIX_STEREO_TO_MS"),
    "x6_to_s2_itu": (1365, 6, 2, 65536, "MIX_51_TO_STEREO"),
    "x6_to_s2_norm": (1365, 6, 2, 65536, "MIX_51_TO_STEREO_NORM"),
    "x16_to_x16": (512, 16, 16, 65536, None),
}
# output samples a lane makes per pass of the mono / stereo kernels' whole-tile path (MixFast, csrc/k_mix.h)
FAST_OUTPUTS = {(1, 1): 32, (1, 2): 32, (2, 1): 16, (2, 2): 32}


def count_asm(stem="k_mix", fast="k_mix_fast", slow="k_mix_any"):
    """per kernel of build/<stem>.s (k_mixramp, k_mixr_fast, k_mixr_any: the ramp kernels, whose block with the most
    dots is the ramp path of a whole tile): the straight-line block with the most dot instructions (the whole-tile path of a mono / stereo
    kernel, the inner loop of k_mix_any) -> its VALU instructions, dots, shifts, packs, loads and stores"""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", stem + ".s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN5cmhip\w*(?:%s|%s)\w*):.*?^\s*s_endpgm" % (fast, slow), text, flags=re.S | re.M):
        sym, body = m.group(1), m.group(0)
        f = re.search(fast + r"ILi(\d)ELi(\d)E", sym)
        name = fast + "<%s, %s>" % f.groups() if f else slow
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
        if stem != "k_mix":                          # the ramp path: the blocks that compute positions
            blocks = [b for b in blocks if any(op.startswith(("v_mul_hi", "v_mad_u64")) for op in b)] or blocks
        best = max(blocks, key=lambda b: sum(op.startswith("v_dot2") for op in b))
        n = lambda pre: sum(op.startswith(pre) for op in best)
        rec = {"valu": n("v_"), "dot2": n("v_dot2"), "ashr": n("v_ashr"), "cvt_pk": n("v_cvt_pk"), "mov": n("v_mov"),
               "mul": n("v_mul") + n("v_mad"),
               "loads_16B": n("global_load_dwordx4"), "stores_16B": n("global_store_dwordx4"), "lds": n("ds_")}
        if f:
            outs = FAST_OUTPUTS[(int(f.group(1)), int(f.group(2)))]
            rec["outputs_per_lane"] = outs
            rec["valu_per_output_sample"] = round(rec["valu"] / outs, 2)
        else:
            rec["instructions_per_dot2_of_the_inner_loop"] = round(len(best) / max(rec["dot2"], 1), 2)
        out[name] = rec
    return out


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


RAMP_SHAPES = "s2_to_ms,s2_to_m1"
RAMP_FRAMES = 1 << 20              # longer than any run here: a stream that ramps is inside its ramp for the whole run


def ramp_leg(cm, np, hip, name, steps):
    """(a) plain, (b) every stream mid-ramp, (c) one stream in 64 mid-ramp: the same mixer and buffers, each run
    bracketed by events; the ramp calls that put the streams where the leg wants them are issued before the bracket,
    the position update that follows a ramp run is inside it (it is part of what such a run costs)"""
    S, ci, co, F, preset = SHAPES[name]
    src = cm.Batch(S, ci, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
    src.generate(cm.GEN_NOISE, 12345, F)
    src.sync()
    W = cm.mix_preset(getattr(cm, preset))[2]
    W2 = np.ascontiguousarray(-W)
    m = cm.Mixer(S, ci, co, F, matrix=W)
    out_stride = (F * co + 7) // 8 * 8
    dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
    assert dst
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    st = C.c_void_p(m.hip_stream())

    def plain():
        m.set_matrix(-1, W)

    def all_ramp():
        m.set_matrix(-1, W)
        m.ramp_matrix(-1, W2, RAMP_FRAMES)

    def some_ramp():
        m.set_matrix(-1, W)
        for s in range(0, S, 64):
            m.ramp_matrix(s, W2, RAMP_FRAMES)

    def timed(prepare, want_ramping):
        ms = []
        for _ in range(steps):
            prepare()
            assert sum(m.ramp_state(s)[1] != 0 for s in range(0, S, 64)) == want_ramping
            assert hip.hipEventRecord(e0, st) == 0
            m.run(src.dev_in, src.stride, F, dst, out_stride)
            assert hip.hipEventRecord(e1, st) == 0
            assert hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            ms.append(t.value)
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:                 # the mixer's own launches bring the clocks up
        m.run(src.dev_in, src.stride, F, dst, out_stride)
        m.sync()
    a = timed(plain, 0)
    b = timed(all_ramp, len(range(0, S, 64)))
    c = timed(some_ramp, len(range(0, S, 64)))
    a2 = timed(plain, 0)                                   # the plain run again: what the spread of a repeat is
    line = {"shape": name, "ramp": True, "streams": S, "channels_in": ci, "channels_out": co, "frames": F,
            "steps": steps, "plain": a, "every_stream_mid_ramp": b, "one_stream_in_64_mid_ramp": c, "plain_again": a2,
            "all_over_plain": round(b["ms_median"] / a["ms_median"], 3),
            "some_over_plain": round(c["ms_median"] / a["ms_median"], 3)}
    print(json.dumps(line), flush=True)
    m.close()
    cm.lib.cmhip_device_free(0, dst)
    src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--ramp", action="store_true")
    ap.add_argument("--count-asm", action="store_true")
    a = ap.parse_args()
    if a.shapes is None:
        a.shapes = RAMP_SHAPES if a.ramp else ",".join(SHAPES)
    if a.count_asm:
        print(json.dumps({"k_mix": count_asm(), "k_mixramp": count_asm("k_mixramp", "k_mixr_fast", "k_mixr_any")}))
        return
    if a.ramp:
        sys.path.insert(0, ROOT)
        import numpy as np
        import __graft_entry__ as ge
        cm = ge.load_package()
        hip = hip_runtime()
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        for name in a.shapes.split(","):
            ramp_leg(cm, np, hip, name, a.steps)
        return
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, ci, co, F, preset = SHAPES[name]
        src = cm.Batch(S, ci, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        if preset is None:
            rng = np.random.default_rng(1)
            B = 65535 // ci
            W = rng.integers(3 * B // 4, B + 1, size=(co, ci)) * rng.choice([-1, 1], size=(co, ci))
        else:
            W = cm.mix_preset(getattr(cm, preset))[2]
        m = cm.Mixer(S, ci, co, F, matrix=W)
        out_stride = (F * co + 7) // 8 * 8
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
        while time.perf_counter() - t0 < 0.15:             # the mixer's own launches bring the clocks up
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
        p = cm.plan_mix(S, ci, co, F)
        med = statistics.median(ms)
        rd, wr = S * F * ci * 2, S * F * co * 2
        copy = src.ceiling(1)
        line = {"shape": name, "streams": S, "channels_in": ci, "channels_out": co, "frames": F,
                "matrix": preset or "dense", "steps": a.steps, "kernel_ms_median": round(med, 4),
                "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "ceiling_copy_GBs_on_the_input_slots": round(copy, 1),
                "of_ceiling": round((rd + wr) / med / 1e6 / copy, 3) if copy > 0 else None,
                "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "chunks": p.chunks, "grid": p.grid,
                         "block": p.block, "lds_bytes": p.lds_bytes}}
        print(json.dumps(line), flush=True)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_mix": count_asm()}))


if __name__ == "__main__":
    main()
