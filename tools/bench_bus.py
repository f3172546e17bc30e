#!/usr/bin/env python3
"""How long a mix-bus run (cmhip_bus_run, csrc/k_bus.hip) takes, and what it moves.

Shapes, 65536 frames each: K = 2, 8, 32 mono sends onto 4096 mono buses and K = 8 stereo sends onto 4096 stereo buses,
every send from a stream of its own (K * 4096 streams: each input byte is read once); 5.1 -> stereo with K = 4 onto 1024
buses (k_bus_any); mix-minus of 64 mono participants (every stream read by 63 buses).  The input is GEN_NOISE in the
slots of a batch used as device memory, the output plain device memory.  After 150 ms of the bus's own launches every
run is bracketed by HIP events on the bus's stream; reported is the median of --steps runs and the bandwidth of the
algorithmic bytes, (K * C_in + C_out) * 2 per bus frame.  Beside it, measured in the same process on a 4096 x 65536
mono batch: cmhip_batch_ceiling's plain read and plain copy.  The fast forms run twice, with plain and with non-temporal
input loads (cmhip_test_bus_nt_loads); the library's default is the first.

    python tools/bench_bus.py [--steps N] [--shapes a,b]      one JSON line per shape
    python tools/bench_bus.py --ramp [--steps N] [--shapes a,b]   beside it, send ramps (cmhip_bus_ramp_sends, csrc/
                                                              k_busramp.hip) with plain loads: every send mid-ramp, one
                                                              send in 64 mid-ramp, and no send ramping once ramps have
                                                              been used (the plain kernels again)
    python tools/bench_bus.py --count-asm                     VALU instructions per output sample and send of each
                                                              kernel, from build/k_bus.s (`make asm`; no GPU needed)

--ramp: a ramp lasts 2^20 frames at most, 16 runs of these shapes, so the ramp modes warm up with 3 runs and time 10 at
the most: every timed run lies inside the ramps.  The timed span holds the ramp kernel and the small kernel that
advances the positions behind it, not the table's upload (queued before the first event).
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
FRAMES = 65536
SHAPES = {          # buses, C_in, C_out, sends per bus (None: mix-minus of `buses` participants)
    "mono_k2": (4096, 1, 1, 2),
    "mono_k8": (4096, 1, 1, 8),
    "mono_k32": (4096, 1, 1, 32),
    "stereo_k8": (4096, 2, 2, 8),
    "x6_to_s2_k4": (1024, 6, 2, 4),
    "mix_minus_64": (64, 1, 1, None),
}
# output samples a lane makes per send of the mono / stereo kernels (MixFast::NOUT, csrc/k_mix.h)
FAST_OUTPUTS = {(1, 1): 32, (1, 2): 32, (2, 1): 16, (2, 2): 32}


def count_asm():
    """per kernel: the straight-line block with the most dot instructions (one send of a whole tile in a mono / stereo
    kernel, the inner loop of k_bus_any) -> its VALU instructions, dots, loads"""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_bus.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN5cmhip\w*k_bus_(?:fast|any)\w*):.*?^\s*s_endpgm", text, flags=re.S | re.M):
        sym, body = m.group(1), m.group(0)
        f = re.search(r"k_bus_fastILi(\d)ELi(\d)ELb(\d)E", sym)
        name = "k_bus_fast<%s, %s, nt=%s>" % f.groups() if f else "k_bus_any"
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
        best = max(blocks, key=lambda b: sum(op.startswith("v_dot2") for op in b))
        n = lambda pre: sum(op.startswith(pre) for op in best)
        rec = {"valu": n("v_"), "dot2": n("v_dot2"), "mov": n("v_mov"), "add64": n("v_addc") + n("v_add_co"),
               "loads_16B": n("global_load_dwordx4"), "lds": n("ds_")}
        if f:
            outs = FAST_OUTPUTS[(int(f.group(1)), int(f.group(2)))]
            rec["outputs_per_lane"] = outs
            rec["valu_per_output_sample_and_send"] = round(rec["valu"] / max(rec["dot2"], 1), 2)
        else:
            rec["instructions_per_dot2_of_the_inner_loop"] = round(len(best) / max(rec["dot2"], 1), 2)
        out[name] = rec
    return out


# frames a lane makes per send of the mono / stereo kernels (TILE_FRAMES / 64)
FAST_FRAMES = {(1, 1): 32, (1, 2): 16, (2, 1): 16, (2, 2): 16}


def count_asm_ramp():
    """k_busr_fast, from build/k_busramp.s: the straight-line block of one send of a whole tile INSIDE its ramp (the one
    with the position's wide multiply and the dots) and the one outside it -> VALU instructions per frame and send"""
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_busramp.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN5cmhip\w*k_busr_fast\w*):.*?^\s*s_endpgm", text, flags=re.S | re.M):
        f = re.search(r"k_busr_fastILi(\d)ELi(\d)ELb(\d)E", m.group(1))
        blocks, cur = [], []
        for ln in m.group(0).splitlines():
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
        n = lambda b, pre: sum(op.startswith(pre) for op in b)
        wide = lambda b: n(b, "v_mul_hi_u32") + n(b, "v_mad_u64_u32")
        ramp = [b for b in blocks if wide(b) and n(b, "v_dot2")]
        plain = [b for b in blocks if not wide(b) and n(b, "v_dot2") >= 16]
        frames = FAST_FRAMES[(int(f.group(1)), int(f.group(2)))]
        out["k_busr_fast<%s, %s, nt=%s>" % f.groups()] = {
            "frames_per_lane": frames,
            "ramp_valu_per_frame_and_send": round(max(n(b, "v_") for b in ramp) / frames, 2) if ramp else None,
            "plain_valu_per_frame_and_send": round(max(n(b, "v_") for b in plain) / frames, 2) if plain else None}
    return out


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--count-asm", action="store_true")
    ap.add_argument("--ramp", action="store_true")
    a = ap.parse_args()
    if a.count_asm:
        print(json.dumps({"k_bus": count_asm(), "k_busramp": count_asm_ramp()}))
        return
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as ge
    cm = ge.load_package()
    yard = cm.Batch(4096, 1, FRAMES, flags=cm.OUT_PCM | cm.VU, rate=48000)
    yard.generate(cm.GEN_NOISE, 1, FRAMES)
    yard.sync()
    hip = hip_runtime()
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for name in a.shapes.split(","):
        B, ci, co, K = SHAPES[name]
        rng = np.random.default_rng(1)
        if K is None:
            S = B
            bus, stream, W = cm.bus_mix_minus(B, 16384 // (B - 1), ci)
            k_of_bus = B - 1
        else:
            S = B * K
            bus = np.repeat(np.arange(B, dtype=np.uint32), K)
            stream = np.arange(S, dtype=np.uint32)
            lim = min(65535 // ci, int(16384 / (K * ci) ** 0.5))
            W = rng.integers(3 * lim // 4, lim + 1, size=(S, co, ci)) * rng.choice([-1, 1], size=(S, co, ci))
            k_of_bus = K
        src = cm.Batch(S, ci, FRAMES, flags=cm.VU, rate=48000)   # (device memory for the streams)
        src.generate(cm.GEN_NOISE, 12345, FRAMES)
        src.sync()
        m = cm.Bus(S, B, ci, co, FRAMES, len(bus))
        m.set_routing(bus, stream, W)
        out_stride = (FRAMES * co + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, B * out_stride * 2)
        assert dst
        st = C.c_void_p(m.hip_stream())
        p = cm.plan_bus(B, ci, co, FRAMES)
        flags = cm.bus_compile(B, S, ci, co, bus, stream, W)[2]
        line = {"shape": name, "streams": S, "buses": B, "channels_in": ci, "channels_out": co, "frames": FRAMES,
                "sends_per_bus": k_of_bus, "groups_per_bus": round(float(flags.sum()) / B, 2), "steps": a.steps}
        rd, wr = B * k_of_bus * FRAMES * ci * 2, B * FRAMES * co * 2

        def timed(steps):
            ms = []
            for _ in range(steps):
                assert hip.hipEventRecord(e0, st) == 0
                m.run(src.dev_in, src.stride, FRAMES, dst, out_stride)
                assert hip.hipEventRecord(e1, st) == 0
                assert hip.hipEventSynchronize(e1) == 0
                t = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
                ms.append(t.value)
            return ms

        for policy in (("plain", "nt") if p.fast else ("plain",)):
            cm.lib.cmhip_test_bus_nt_loads(m.h, 1 if policy == "nt" else 0)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:             # the bus's own launches bring the clocks up
                m.run(src.dev_in, src.stride, FRAMES, dst, out_stride)
                m.sync()
            ms = timed(a.steps)
            med = statistics.median(ms)
            line[policy + "_loads"] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4),
                                       "kernel_ms_max": round(max(ms), 4),
                                       "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1)}
        if a.ramp:
            cm.lib.cmhip_test_bus_nt_loads(m.h, 0)
            Wt = np.ascontiguousarray(W[::-1], dtype=np.int16)   # targets: the same matrices, handed round
            W0 = np.ascontiguousarray(W, dtype=np.int16)
            steps = min(a.steps, 10)
            assert (3 + steps) * FRAMES < 1 << 20
            modes = {}
            for mode in ("every_send_mid_ramp", "one_send_in_64_mid_ramp", "no_send_ramping"):
                m.ramp_sends(0, W0, 0)                           # everything steps back; ramp state exists from now on
                if mode == "every_send_mid_ramp":
                    m.ramp_sends(0, Wt, 1 << 20)
                elif mode == "one_send_in_64_mid_ramp":
                    for j in range(0, len(bus), 64):
                        m.ramp_sends(j, Wt[j:j + 1], 1 << 20)
                ramping = sum(1 for j in range(0, len(bus), 64) if m.ramp_state(j)[1]) if mode != "no_send_ramping" else 0
                for _ in range(3):
                    m.run(src.dev_in, src.stride, FRAMES, dst, out_stride)
                m.sync()
                ms = timed(steps)
                med = statistics.median(ms)
                modes[mode] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4),
                               "kernel_ms_max": round(max(ms), 4), "steps": steps, "sampled_sends_ramping": ramping,
                               "of_plain_loads": round(med / line["plain_loads"]["kernel_ms_median"], 3)}
            pr = cm.plan_busramp(B, ci, co, FRAMES)
            modes["plan"] = {"tile_frames": pr.tile_frames, "grid": pr.grid, "lds_bytes": pr.lds_bytes}
            line["ramp"] = modes
        read, copy = yard.ceiling(0), yard.ceiling(1)
        best = line["plain_loads"]["GBs_read_plus_written"]
        line.update({"read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                     "ceiling_read_GBs": round(read, 1), "ceiling_copy_GBs": round(copy, 1),
                     "plain_of_read_ceiling": round(best / read, 3) if read > 0 else None,
                     "plain_of_copy_ceiling": round(best / copy, 3) if copy > 0 else None,
                     "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "chunks": p.chunks, "grid": p.grid,
                              "block": p.block, "lds_bytes": p.lds_bytes}})
        print(json.dumps(line), flush=True)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    yard.close()
    print(json.dumps({"k_bus": count_asm()}))


if __name__ == "__main__":
    main()
