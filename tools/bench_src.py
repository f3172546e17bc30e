#!/usr/bin/env python3
"""How long a resampler run (cmhip_src_run, csrc/k_src.hip) takes, and what it moves.

Shapes: 4096 stereo streams x 65536 input frames at 44100 -> 48000 and 48000 -> 44100, 8192 mono streams x 65536 at
16000 -> 48000 and 48000 -> 8000, and 2730 x 6 channels x 16384 at 44100 -> 48000.  The input is GEN_NOISE in the
slots of a batch used as device memory, the output plain device memory.  After 150 ms of the resampler's own launches
every run is bracketed by HIP events on the resampler's stream; reported is the median of --steps runs, the bytes
read and written per run (input slots + output slots; the table and the halos are re-read from the caches) and the
bandwidth those give.  Beside them: registers, LDS and waves per SIMD of the three kernels from build/k_src.usage.txt
(`make asm`), and the launcher's plan of the shape.

    python tools/bench_src.py [--steps N] [--shapes a,b]      one JSON line per shape
    python tools/bench_src.py --usage                         the kernels' resources alone (no GPU needed)
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
SHAPES = {
    "s2_441_48": (4096, 2, 65536, 44100, 48000),
    "s2_48_441": (4096, 2, 65536, 48000, 44100),
    "m1_16_48": (8192, 1, 65536, 16000, 48000),
    "m1_48_8": (8192, 1, 65536, 48000, 8000),
    "x6_441_48": (2730, 6, 16384, 44100, 48000),
}


def usage():
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_src.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", open(path).read(), flags=re.S):
        name = "k_src_any" if "k_src_any" in m.group(1) else "k_src_fast<%s>" % re.search(r"ILi(\d)E", m.group(1)).group(1)
        f = dict(re.findall(r"remark:\s+([\w \[\]/]+): (\d+)", m.group(2)))
        out[name] = {"vgprs": int(f["VGPRs"]), "sgprs": int(f["TotalSGPRs"]), "scratch": int(f["ScratchSize [bytes/lane]"]),
                     "waves_per_simd_by_registers": int(f["Occupancy [waves/SIMD]"])}
    return out


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
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_src": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, Cn, F, ri, ro = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=ri)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        r = cm.Resampler(S, Cn, ri, ro, F)
        L, M, T = r.geometry()
        out_stride = (r.max_out_frames() * Cn + 7) // 8 * 8
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
        st = C.c_void_p(r.hip_stream())
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:             # the resampler's own launches bring the clocks up
            counts = r.run(src.dev_in, src.stride, F, dst, out_stride)
            r.sync()
        ms, outs = [], 0
        for _ in range(a.steps):
            assert hip.hipEventRecord(e0, st) == 0
            counts = r.run(src.dev_in, src.stride, F, dst, out_stride)
            assert hip.hipEventRecord(e1, st) == 0
            assert hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            ms.append(t.value)
            outs = int(counts.sum())
        p = cm.plan_src(S, Cn, L, M, T, int(counts.max()))
        med = statistics.median(ms)
        rd, wr = S * F * Cn * 2, outs * Cn * 2
        line = {"shape": name, "streams": S, "channels": Cn, "frames_in": F, "rate_in": ri, "rate_out": ro,
                "L": L, "M": M, "T": T, "steps": a.steps, "kernel_ms_median": round(med, 4),
                "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "output_Msamples_per_ms": round(outs * Cn / med / 1e6, 2),
                "dot2_per_output_sample": (T + 7) // 8 * 4,
                "plan": {"fast": p.fast, "tile_out": p.tile_out, "tile_in": p.tile_in, "chunks": p.chunks, "grid": p.grid,
                         "table_lds": p.table_lds, "lds_bytes": p.lds_bytes,
                         "workgroups_per_cu_by_lds": 160 * 1024 // p.lds_bytes}}
        print(json.dumps(line), flush=True)
        r.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_src": usage()}))


if __name__ == "__main__":
    main()
