#!/usr/bin/env python3
"""How long a leveller run (cmhip_agc_run, csrc/k_agc.hip) takes, kernel by kernel, beside a plain copy of the same slots.

Shapes: 4096 stereo and 8192 mono streams x 65536 frames, and 1365 streams of 6 channels, at window_log2 = 12.  The input
is GEN_NOISE in the slots of a batch used as device memory, the output plain device memory; the parameters are those of
cmhip_agc_design for -20 dB, +-24 dB, 3 and 10 dB/s at 48 kHz.  After 150 ms of the object's own launches every run is
bracketed by HIP events on its stream -- four of them, in front of, between and behind the three launches (the test hook
cmhip_test_agc_run_events) -- and reported are the medians of --steps runs per kernel and for the whole run and,
bracketed the same way on the same stream in the same process, the median of a device-to-device copy (hipMemcpyAsync)
of the input slots into the output slots.  That copy is a yardstick, not a ceiling.

Floor by bytes moved, in units of the copy (which reads and writes every sample once): the run reads its input twice
and writes it once -- 1.5 x the copy; the energy pass alone 0.5 x, the apply pass 1 x.  Each line reports the ratio of
the whole run to the copy and to that floor.  Also: registers, LDS, scratch and waves per SIMD of the seven kernels from
build/k_agc.usage.txt (`make asm`) and the launcher's plan of the shape.

    python tools/bench_agc.py [--steps N] [--shapes a,b] [--out FILE]   one JSON line per shape, also written to FILE
    python tools/bench_agc.py --usage                                    the kernels' resources alone (no GPU needed)
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
WINDOW_LOG2 = 12
SHAPES = {"s2": (4096, 2, 65536), "m1": (8192, 1, 65536), "c6": (1365, 6, 65536)}


def usage():
    path = os.path.join(BUILD, "k_agc.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(path).read(), flags=re.S):
        stem = re.search(r"k_agc_[a-z_]+", m.group(1)).group(0)
        width = re.search(r"ILi(\d)E", m.group(1))
        name = "%s<%s>" % (stem, width.group(1)) if width else stem
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agc_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_agc": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    lines = []
    par = cm.agc_design(48000.0, WINDOW_LOG2, -20.0, -60.0, 24.0, -24.0, 0.0, 3.0, 10.0)
    for name in a.shapes.split(","):
        S, Cn, F = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        m = cm.Leveller(S, Cn, WINDOW_LOG2, F, params=par)
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
        ev = (C.c_void_p * 4)()
        for i in range(4):
            e = C.c_void_p()
            assert hip.hipEventCreate(C.byref(e)) == 0
            ev[i] = e
        st = C.c_void_p(m.hip_stream())
        in_bytes = S * src.stride * 2

        def elapsed(e0, e1):
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            return t.value

        def warm(fn):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:             # the step's own launches bring the clocks up
                fn()
                m.sync()

        def copy():
            assert hip.hipMemcpyAsync(dst, src.dev_in, min(in_bytes, S * out_stride * 2), 3, st) == 0   # device to device

        def run():
            assert cm.lib.cmhip_test_agc_run_events(m.h, src.dev_in, src.stride, F, None, dst, out_stride, ev) == 0

        warm(copy)
        copies = []
        for _ in range(a.steps):
            assert hip.hipEventRecord(ev[0], st) == 0
            copy()
            assert hip.hipEventRecord(ev[1], st) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            copies.append(elapsed(ev[0], ev[1]))
        warm(run)
        parts = [[], [], [], []]                               # energy, step, apply, the whole run
        for _ in range(a.steps):
            run()
            assert hip.hipEventSynchronize(ev[3]) == 0
            for i in range(3):
                parts[i].append(elapsed(ev[i], ev[i + 1]))
            parts[3].append(elapsed(ev[0], ev[3]))
        med = [statistics.median(p) for p in parts]
        medc = statistics.median(copies)
        gain, level, clips = m.state()
        p = cm.plan_agc(S, Cn, WINDOW_LOG2, F, F)
        unit = S * F * Cn * 2                                  # bytes of every sample once
        line = {"shape": name, "streams": S, "channels": Cn, "frames": F, "window_log2": WINDOW_LOG2, "steps": a.steps,
                "energy_ms_median": round(med[0], 4), "step_ms_median": round(med[1], 4), "apply_ms_median": round(med[2], 4),
                "run_ms_median": round(med[3], 4), "run_ms_min": round(min(parts[3]), 4), "run_ms_max": round(max(parts[3]), 4),
                "copy_ms_median": round(medc, 4), "copy_GBs_read_plus_written": round(2 * unit / medc / 1e6, 1),
                "floor_in_copies": 1.5, "GBs_at_floor_bytes": round(3 * unit / med[3] / 1e6, 1),
                "energy_ratio_to_copy": round(med[0] / medc, 3), "apply_ratio_to_copy": round(med[2] / medc, 3),
                "ratio_to_copy": round(med[3] / medc, 3), "ratio_to_floor": round(med[3] / medc / 1.5, 3),
                "gain_of_stream_0": int(gain[0]), "level_of_stream_0": int(level[0]), "clips": int(clips.sum()),
                "plan": {"fast": p.fast, "tile_frames": 1 << p.tile_log2, "chunks": p.chunks, "grid": p.grid, "block": p.block,
                         "nw": p.nw, "step_grid": p.step_grid}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_agc": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_agc.py --steps %d --shapes %s\n" % (a.steps, a.shapes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
