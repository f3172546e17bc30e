#!/usr/bin/env python3
"""How long a band-split run (cmhip_split_run, csrc/k_split.hip) takes, beside a plain copy of the same slots.

Shapes: 4096 stereo streams x 65536 frames at B = 3, T = 255, and 8192 mono streams x 65536 frames at B = 2, T = 1023
(crossovers 300 / 3000 Hz and 1000 Hz at 48 kHz, the library's own design).  The input is GEN_NOISE in the slots of a
batch used as device memory, the output plain device memory, band-major.  After 150 ms of the object's own launches
every run is bracketed by HIP events on its stream; reported is the median of --steps runs, the bytes read and written
per run and the bandwidth those give, and beside them the same for a device-to-device copy of the input slots into the
first band's slots, bracketed the same way on the same stream.  Also: the VALU issue floor from the count of dot
instructions a sample needs, (B-1) * Tp / 2 with Tp = T + 1 rounded up to 8, registers, scratch and waves per SIMD of the
three kernels from build/k_split.usage.txt (`make asm`), the dot instructions counted in build/k_split.s, and the
launcher's plan of the shape.

    python tools/bench_split.py [--steps N] [--shapes a,b] [--out FILE]   one JSON line per shape, also appended to FILE
    python tools/bench_split.py --usage                                    the kernels' resources alone (no GPU needed)
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
RATE = 48000
SHAPES = {
    "s2_b3_t255": (4096, 2, 65536, 3, 255, [300.0, 3000.0]),
    "m1_b2_t1023": (8192, 1, 65536, 2, 1023, [1000.0]),
}


def usage():
    path = os.path.join(BUILD, "k_split.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", open(path).read(), flags=re.S):
        name = ("k_split_any" if "k_split_any" in m.group(1)
                else "k_split_fast<%s>" % re.search(r"ILi(\d)E", m.group(1)).group(1))
        f = dict(re.findall(r"remark:\s+([\w \[\]/]+): (\d+)", m.group(2)))
        out[name] = {"vgprs": int(f["VGPRs"]), "sgprs": int(f["TotalSGPRs"]), "scratch": int(f["ScratchSize [bytes/lane]"]),
                     "waves_per_simd_by_registers": int(f["Occupancy [waves/SIMD]"])}
    asm = os.path.join(BUILD, "k_split.s")
    if os.path.exists(asm):
        out["v_dot2_in_file"] = len(re.findall(r"^\s*v_dot2\w*_i32_i16", open(asm).read(), flags=re.M))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_split": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    lines = []
    for name in a.shapes.split(","):
        S, Cn, F, B, T, xs = SHAPES[name]
        src = cm.Batch(S, Cn, F, flags=cm.VU, rate=RATE)
        src.generate(cm.GEN_NOISE, 12345, F)
        src.sync()
        m = cm.BandSplit(S, Cn, B, T, F, rate=RATE, crossover_hz=xs)
        _, q = m.get_table()
        out_stride = (F * Cn + 7) // 8 * 8
        dst = cm.lib.cmhip_device_alloc(0, B * S * out_stride * 2)
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

        def timed(fn):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:             # the step's own launches bring the clocks up
                fn()
                m.sync()
            ms = []
            for _ in range(a.steps):
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

        ms_copy = timed(copy)
        ms = timed(lambda: m.run(src.dev_in, src.stride, F, dst, out_stride))
        m.clips(clear=True)
        m.run(src.dev_in, src.stride, F, dst, out_stride)
        clips = int(m.clips().sum())                           # of one run from the history the runs before left
        p = cm.plan_split(S, Cn, B, T, F)
        med, medc = statistics.median(ms), statistics.median(ms_copy)
        rd, wr = S * F * Cn * 2, B * S * F * Cn * 2
        dots = (B - 1) * p.tp // 2
        line = {"shape": name, "streams": S, "channels": Cn, "frames": F, "bands": B, "taps": T, "q": q.tolist(),
                "steps": a.steps, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4),
                "kernel_ms_max": round(max(ms), 4), "read_MB": round(rd / 1e6, 1), "written_MB": round(wr / 1e6, 1),
                "GBs_read_plus_written": round((rd + wr) / med / 1e6, 1),
                "input_Msamples_per_ms": round(S * F * Cn / med / 1e6, 2),
                "copy_ms_median": round(medc, 4), "copy_GBs_read_plus_written": round(2 * rd / medc / 1e6, 1),
                "dot2_per_input_sample": dots, "dot2_G_per_s": round(S * F * Cn * dots / med / 1e6, 1),
                "saturated_samples_per_run": clips,
                "plan": {"fast": p.fast, "tile_frames": p.tile_frames, "chunks": p.chunks, "grid": p.grid, "row": p.row,
                         "table_words": p.table_words, "lds_bytes": p.lds_bytes,
                         "workgroups_per_cu_by_lds": 160 * 1024 // p.lds_bytes}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_split": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_split.py --steps %d --shapes %s\n" % (a.steps, a.shapes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
