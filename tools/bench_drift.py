#!/usr/bin/env python3
"""How long a drift run (cmhip_drift_run, csrc/k_drift.hip) takes, and what it moves.

Shapes: 4096 stereo and 8192 mono streams x 65536 input frames at delta 0 and at +200 ppm, and 2730 x 6 channels x
16384 at +200 ppm, with the designed default table (128 phases, 32 taps).  The input is GEN_NOISE in the slots of a
batch used as device memory, the output plain device memory.  After 150 ms of the stage's own launches every run is
bracketed by HIP events on the stage's stream (the reset to position 0 that precedes it lies in front of the first event); reported is the median of --steps runs, the bytes read and written per
run (input slots + output slots; the table and the halos are re-read from the caches) and the bandwidth those give.
Beside them, in the same process and on the same arrays: a resampler (cmhip_src_run) at 44100 -> 48000, which does half
the dot work per output sample, and a hipMemcpyAsync of the input slots to the output, device to device.  Then:
registers, LDS and waves per SIMD of the three kernels from build/k_drift.usage.txt (`make asm`), and the launcher's
plan of the shape.

    python tools/bench_drift.py [--steps N] [--shapes a,b]    one JSON line per shape
    python tools/bench_drift.py --usage                       the kernels' resources alone (no GPU needed)
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
    "s2_0": (4096, 2, 65536, 0.0),
    "s2_200": (4096, 2, 65536, 200.0),
    "m1_0": (8192, 1, 65536, 0.0),
    "m1_200": (8192, 1, 65536, 200.0),
    "x6_200": (2730, 6, 16384, 200.0),
}


def usage():
    path = os.path.join(ROOT, "libcoolmic-dsp_amd", "build", "k_drift.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", open(path).read(), flags=re.S):
        name = "k_drift_any" if "k_drift_any" in m.group(1) else "k_drift_fast<%s>" % re.search(r"ILi(\d)E", m.group(1)).group(1)
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


def timed(hip, st, steps, run, sync, before=None):
    """run() bracketed by events on stream st -> (median, min, max) ms over `steps` runs, after 150 ms of warm-up;
    before() is queued in front of the first event of every run and is not timed"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        if before:
            before()
        run()
        sync()
    ms = []
    for _ in range(steps):
        if before:
            before()
        assert hip.hipEventRecord(e0, st) == 0
        run()
        assert hip.hipEventRecord(e1, st) == 0
        assert hip.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        ms.append(t.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_drift": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    for name in a.shapes.split(","):
        S, Cn, F, ppm = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=48000)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        d = cm.Drift(S, Cn, F)
        r = cm.Resampler(S, Cn, 44100, 48000, F)
        phi, T = d.geometry()
        L, M, Ts = r.geometry()
        delta = cm.drift_ppm(ppm)
        d.set(-1, delta)
        out_stride = (max(d.max_out_frames(), r.max_out_frames()) * Cn + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, S * out_stride * 2)
        assert dst
        if hip is None:
            hip = hip_runtime()
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
            hip.hipEventDestroy.argtypes = [C.c_void_p]
            hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        got = {}

        def run_drift():
            got["drift"] = d.run(src.dev_in, src.stride, F, dst, out_stride)

        def run_src():
            got["src"] = r.run(src.dev_in, src.stride, F, dst, out_stride)

        st_d, st_r = C.c_void_p(d.hip_stream()), C.c_void_p(r.hip_stream())
        nbytes = S * src.stride * 2

        def run_copy():
            assert hip.hipMemcpyAsync(dst, src.dev_in, nbytes, 3, st_d) == 0          # hipMemcpyDeviceToDevice

        # (every timed run from position 0, the same work: the reset, a small memset, is queued in front of the events)
        med, lo, hi = timed(hip, st_d, a.steps, run_drift, d.sync, before=lambda: d.reset(-1))
        smed, slo, shi = timed(hip, st_r, a.steps, run_src, r.sync)
        cmed, clo, chi = timed(hip, st_d, a.steps, run_copy, d.sync)
        outs, souts = int(got["drift"].sum()), int(got["src"].sum())
        p = cm.plan_drift(S, Cn, phi, T, int(got["drift"].max()))
        rd, wr = S * F * Cn * 2, outs * Cn * 2
        line = {"shape": name, "streams": S, "channels": Cn, "frames_in": F, "ppm": ppm, "delta": delta,
                "phase_log2": phi, "T": T, "steps": a.steps, "kernel_ms_median": round(med, 4),
                "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "output_Msamples_per_ms": round(outs * Cn / med / 1e6, 2), "dot2_per_output_sample": T,
                "src_441_48": {"L": L, "M": M, "T": Ts, "kernel_ms_median": round(smed, 4), "kernel_ms_min": round(slo, 4),
                               "kernel_ms_max": round(shi, 4),
                               "output_Msamples_per_ms": round(souts * Cn / smed / 1e6, 2),
                               "dot2_per_output_sample": (Ts + 7) // 8 * 4},
                "memcpy_d2d": {"MB": round(nbytes / 1e6, 1), "ms_median": round(cmed, 4), "ms_min": round(clo, 4),
                               "ms_max": round(chi, 4), "GBs_read_plus_written": round(2 * nbytes / cmed / 1e6, 1)},
                "drift_over_src_per_output_sample": round((med / (outs * Cn)) / (smed / (souts * Cn)), 3),
                "plan": {"fast": p.fast, "tile_out": p.tile_out, "tile_in": p.tile_in, "chunks": p.chunks, "grid": p.grid,
                         "table_lds": p.table_lds, "lds_bytes": p.lds_bytes,
                         "workgroups_per_cu_by_lds": 160 * 1024 // p.lds_bytes}}
        print(json.dumps(line), flush=True)
        d.close()
        r.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    print(json.dumps({"k_drift": usage()}))


if __name__ == "__main__":
    main()
