#!/usr/bin/env python3
"""How long a filter run (cmhip_iir_run, csrc/k_iir.hip) takes, beside a plain copy of the same slots.

Shapes: 4096 stereo and 8192 mono streams x 65536 frames, and 1365 streams of 6 channels, each at 1, 2, 4 and 8
sections.  The input is GEN_NOISE in the slots of a batch used as device memory, the output plain device memory; every
section of every stream is the 40 Hz high-pass of cmhip_iir_design at 48 kHz.  After 150 ms of the object's own launches
every run is bracketed by two HIP events on its stream, and reported are the median of --steps runs and, bracketed the
same way on the same stream in the same process, the median of a device-to-device copy (hipMemcpyAsync) of the input
slots into the output slots.  That copy is a yardstick, not a ceiling: the run is a recurrence along every stream and
is expected to be bound by the latency of its dependent chain, frames x (B + NP - 1) / B steps of it, not by memory.
Each line reports the time per step of the recurrence in nanoseconds beside the ratio to the copy.  Also: registers,
LDS, scratch and waves per SIMD of the nine kernels from build/k_iir.usage.txt (`make asm`) and the launcher's plan.

--ramp: coefficient ramps (cmhip_iir_ramp, csrc/k_iirramp.hip).  In the same process, on the same arrays and bracketed
the same way, every case is timed three times: the plain run, a run in which every section of every stream is in the
middle of a ramp, and a run in which one stream in 64 is (so every workgroup of the ramp kernels holds mostly sections
at rest).  The ramps are started anew in front of every run, outside the bracket, between the 40 Hz and a 160 Hz
high-pass and over 2^20 frames, so that no run sees one end.  The lines are APPENDED to FILE, with the ramp kernels'
resources from build/k_iirramp.usage.txt behind them.

    python tools/bench_iir.py [--steps N] [--shapes a,b] [--sections 1,2] [--out FILE]   one JSON line per case, also in FILE
    python tools/bench_iir.py --ramp [...]                               the three timings per case, appended to FILE
    python tools/bench_iir.py --usage                                    the kernels' resources alone (no GPU needed)
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
BUILD = os.path.join(ROOT, "libcoolmic-dsp_amd", "build")
SHAPES = {"s2": (4096, 2, 65536), "m1": (8192, 1, 65536), "c6": (1365, 6, 65536)}


def usage(stem="k_iir"):
    path = os.path.join(BUILD, stem + ".usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(path).read(), flags=re.S):
        stem = re.search(r"k_iirr?_[a-z]+", m.group(1)).group(0)
        width = re.search(r"ILi(\d)ELi(\d)E", m.group(1))
        name = "%s<%s, %s>" % (stem, width.group(1), width.group(2)) if width else stem
        f = dict(re.findall(r"remark:\s+([\w \[\]/]+): (\d+)", m.group(2)))
        out[name] = {"vgprs": int(f["VGPRs"]), "sgprs": int(f["TotalSGPRs"]), "scratch": int(f["ScratchSize [bytes/lane]"]),
                     "lds_bytes": int(m.group(3)), "waves_per_simd_by_registers": int(f["Occupancy [waves/SIMD]"])}
    return out


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events and the copy"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sections", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    ap.add_argument("--ramp", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_iir": usage(), "k_iirramp": usage("k_iirramp")}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    lines = []
    cut = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0)
    cut160 = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 160.0)
    for name in a.shapes.split(","):
        S, Cn, F = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        out_stride = (F * Cn + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
            hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        ev = []
        for i in range(2):
            e = C.c_void_p()
            assert hip.hipEventCreate(C.byref(e)) == 0
            ev.append(e)
        in_bytes = S * src.stride * 2
        for N in (int(v) for v in a.sections.split(",")):
            m = cm.Filter(S, Cn, N, F)
            for k in range(N):
                m.set(-1, k, cut)
            st = C.c_void_p(m.hip_stream())

            def timed(fn, before=None):
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.15:         # the step's own launches bring the clocks up
                    if before:
                        before()
                    fn()
                    m.sync()
                ts = []
                for _ in range(a.steps):
                    if before:
                        before()                               # (host only, outside the bracket)
                    assert hip.hipEventRecord(ev[0], st) == 0
                    fn()
                    assert hip.hipEventRecord(ev[1], st) == 0
                    assert hip.hipEventSynchronize(ev[1]) == 0
                    t = C.c_float()
                    assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
                    ts.append(t.value)
                return ts

            def copy():
                assert hip.hipMemcpyAsync(dst, src.dev_in, min(in_bytes, S * out_stride * 2), 3, st) == 0   # device to device

            def run():
                m.run(src.dev_in, src.stride, F, dst, out_stride)

            turn = [0]

            def ramp_every(stride):
                def before():                                  # every section of every stride-th stream, mid-ramp
                    turn[0] += 1
                    to = cut160 if turn[0] % 2 else cut
                    for s in ([-1] if stride == 1 else range(0, S, stride)):
                        for k in range(N):
                            m.ramp(s, k, to, cm.IIR_RAMP_MAX)
                return before

            copies, runs = timed(copy), timed(run)
            med, medc = statistics.median(runs), statistics.median(copies)
            ramped = {}
            if a.ramp:
                for key, stride in (("all", 1), ("one_in_64", 64)):
                    ts = timed(run, ramp_every(stride))
                    assert m.ramp_state(0, 0)[1] == cm.IIR_RAMP_MAX
                    ramped[key] = {"run_ms_median": round(statistics.median(ts), 4), "run_ms_min": round(min(ts), 4),
                                   "run_ms_max": round(max(ts), 4), "ratio_to_plain": round(statistics.median(ts) / med, 3)}
                    for k in range(N):
                        m.set(-1, k, cut)
            clips, overs = m.state()
            p = cm.plan_iir(S, Cn, N, F)
            steps = p.tiles * (p.tile + p.np - 1)
            line = {"shape": name, "streams": S, "channels": Cn, "frames": F, "sections": N, "steps": a.steps,
                    "run_ms_median": round(med, 4), "run_ms_min": round(min(runs), 4), "run_ms_max": round(max(runs), 4),
                    "copy_ms_median": round(medc, 4), "ratio_to_copy": round(med / medc, 2),
                    "recurrence_steps": steps, "ns_per_step": round(med * 1e6 / steps, 1),
                    "waves": p.grid, "clips": int(clips.sum()), "overs": int(overs.sum()),
                    "plan": {"fast": p.fast, "np": p.np, "streams_per_workgroup": p.spw, "grid": p.grid, "block": p.block,
                             "tile_frames": p.tile, "tiles": p.tiles, "lds_bytes": p.lds_bytes}}
            if a.ramp:
                line["ramp"] = ramped
            print(json.dumps(line), flush=True)
            lines.append(line)
            m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_iirramp": usage("k_iirramp")} if a.ramp else {"k_iir": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a" if a.ramp else "w") as f:
            f.write("# python tools/bench_iir.py%s --steps %d --shapes %s --sections %s\n"
                    % (" --ramp" if a.ramp else "", a.steps, a.shapes, a.sections))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
