#!/usr/bin/env python3
"""How long a delay run (cmhip_delay_run, csrc/k_delay.hip) takes, beside a plain copy of the same slots.

Shapes: 4096 stereo and 8192 mono streams x 65536 frames, max_delay = 48000.  Cases: d = 0, d = 63, d = 64 (the control:
a source on a 16-byte edge, so no second vector is loaded; d = 63 against it shows what the misaligned source costs),
d = 48000, and every stream mid-ramp (0 -> 63 over 2^20 frames, so a whole run stays inside the ramp).  The input is
GEN_NOISE in the slots of a batch used as device memory, the output plain device memory.  After 150 ms of the object's own
launches every run is bracketed by HIP events on its stream; reported is the median of --steps runs and, bracketed the
same way on the same stream in the same process, the median of a device-to-device copy (hipMemcpyAsync) of the input
slots into the output slots.  That copy is a yardstick, not a ceiling: it runs at about 5 TB/s here, below what the
part's memory can move, so a ratio to the floor below 1 means the kernel moves its bytes faster than the copy moves its.

Floors by bytes moved, in units of the copy (which reads and writes every sample once): a run reads its input, writes its
output and writes the ring -- 1.5 x the copy -- and reads min(d, F) frames of the ring per stream beside: 1.5 + d / (2 F),
2 x from d = F on.  Each case reports its ratio to the copy and to that floor.  Also: registers, scratch and waves per
SIMD of the three kernels from build/k_delay.usage.txt (`make asm`) and the launcher's plan of the shape.

    python tools/bench_delay.py [--steps N] [--shapes a,b] [--out FILE]   one JSON line per shape and case, also written to FILE
    python tools/bench_delay.py --usage                                    the kernels' resources alone (no GPU needed)
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
MAX_DELAY = 48000
SHAPES = {"s2": (4096, 2, 65536), "m1": (8192, 1, 65536)}
CASES = ["d0", "d63", "d64", "d48000", "ramp"]


def usage():
    path = os.path.join(BUILD, "k_delay.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", open(path).read(), flags=re.S):
        name = ("k_delay_any" if "k_delay_any" in m.group(1)
                else "k_delay_fast<%s>" % re.search(r"ILi(\d)E", m.group(1)).group(1))
        f = dict(re.findall(r"remark:\s+([\w \[\]/]+): (\d+)", m.group(2)))
        out[name] = {"vgprs": int(f["VGPRs"]), "sgprs": int(f["TotalSGPRs"]), "scratch": int(f["ScratchSize [bytes/lane]"]),
                     "waves_per_simd_by_registers": int(f["Occupancy [waves/SIMD]"])}
    return out


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events and the copy"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_delay": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    lines = []
    for name in a.shapes.split(","):
        S, Cn, F = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        m = cm.Delay(S, Cn, MAX_DELAY, F)
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
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        st = C.c_void_p(m.hip_stream())
        in_bytes = S * src.stride * 2

        def timed(fn, before=None):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:             # the step's own launches bring the clocks up
                if before:
                    before()
                fn()
                m.sync()
            ms = []
            for _ in range(a.steps):
                if before:
                    before()
                assert hip.hipEventRecord(e0, st) == 0
                fn()
                assert hip.hipEventRecord(e1, st) == 0
                assert hip.hipEventSynchronize(e1) == 0
                t = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
                ms.append(t.value)
            return ms

        def copy():
            assert hip.hipMemcpyAsync(dst, src.dev_in, min(in_bytes, S * out_stride * 2), 3, st) == 0   # device to device

        def run():
            m.run(src.dev_in, src.stride, F, dst, out_stride)

        def mid_ramp():                                        # every stream at the start of a ramp longer than a run
            m.set(-1, 0)
            m.ramp(-1, 63, 1 << 20)

        p = cm.plan_delay(S, Cn, MAX_DELAY, F, F)
        medc = statistics.median(timed(copy))
        for case in CASES:
            d = {"d0": 0, "d63": 63, "d64": 64, "d48000": 48000, "ramp": 63}[case]
            if case != "ramp":
                m.set(-1, d)
            ms = timed(run, mid_ramp if case == "ramp" else None)
            med = statistics.median(ms)
            unit = S * F * Cn * 2                              # bytes of every sample once
            floor = 1.5 + min(d, F) / (2.0 * F) * (2 if case == "ramp" else 1) if d else 1.5
            line = {"shape": name, "case": case, "streams": S, "channels": Cn, "frames": F, "max_delay": MAX_DELAY,
                    "delay": d, "steps": a.steps, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4),
                    "kernel_ms_max": round(max(ms), 4), "copy_ms_median": round(medc, 4),
                    "copy_GBs_read_plus_written": round(2 * unit / medc / 1e6, 1),
                    "floor_in_copies": round(floor, 4), "GBs_at_floor_bytes": round(2 * unit * floor / med / 1e6, 1),
                    "ratio_to_copy": round(med / medc, 3), "ratio_to_floor": round(med / medc / floor, 3),
                    "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "chunks": p.chunks, "grid": p.grid,
                             "ring_frames": p.ring_frames}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_delay": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_delay.py --steps %d --shapes %s\n" % (a.steps, a.shapes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
