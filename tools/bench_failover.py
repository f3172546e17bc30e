#!/usr/bin/env python3
"""How long a failover switch run (cmhip_failover_run, csrc/k_failover.hip) takes, kernel by kernel, beside a leveller
run and a plain copy of the same slots in the same process.

Shapes: 4096 stereo and 8192 mono outputs x 65536 frames, and 1365 outputs of 6 channels; window_log2 = 12; as many
input slots as outputs, output o with the K = 1, 2 or 4 candidates o, o + 1, ... (mod S); steady (every candidate is
noise and live, the output stays on its main source) and, for K > 1, every output in mid-fade.  The input is GEN_NOISE
in the slots of a batch used as device memory, the output plain device memory.

Mid-fade: fade_log2 = 16, so a changeover lasts 65536 frames, sixteen windows.  In front of every timed run the outputs
are reset, run over one window (not timed) and forced to candidate 1: the timed run's first frame is the window edge at
which the fade begins, and all sixteen of its windows are fade windows.  The state says so after every timed run
(`fade_window_after` 15).

After 150 ms of the object's own launches every run is bracketed by HIP events on its stream -- four of them, in front
of, between and behind the three launches (the test hook cmhip_test_failover_run_events) -- and reported are the medians
of --steps runs per kernel and for the whole run.  Beside it, bracketed the same way: a leveller run over the same
arrays (cmhip_test_agc_run_events, the parameters of tools/bench_agc.py) and a device-to-device copy (hipMemcpyAsync) of
the input slots into the output slots.  That copy is a yardstick, not a ceiling: it moves 2 bytes per output byte, the
switch K + 2 of them when steady (K reads of the energy pass, a read and a write of the apply pass) and K + 3 in a fade,
so `floor_ms` is the copy's time times (K + 2) / 2 or (K + 3) / 2.  Last: registers, LDS, scratch and waves per SIMD of
the seven kernels from build/k_failover.usage.txt (`make asm`).

    python tools/bench_failover.py [--steps N] [--shapes a,b] [--out FILE]   one JSON line per case, also written to FILE
    python tools/bench_failover.py --usage                                    the kernels' resources alone (no GPU needed)
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
W_LOG2 = 12
SOURCES = (1, 2, 4)


def usage():
    path = os.path.join(BUILD, "k_failover.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(path).read(), flags=re.S):
        stem = re.search(r"k_failover_[a-z]+(?:_fast|_any)?", m.group(1)).group(0)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "failover_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_failover": usage()}))
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cm = ge.load_package()
    hip = None
    lines = []
    w, W = W_LOG2, 1 << W_LOG2
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
        ev = (C.c_void_p * 4)()
        for i in range(4):
            e = C.c_void_p()
            assert hip.hipEventCreate(C.byref(e)) == 0
            ev[i] = e
        in_bytes = S * src.stride * 2

        def elapsed(e0, e1):
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            return t.value

        def warm(fn, obj):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:             # the step's own launches bring the clocks up
                fn()
                obj.sync()

        agc = cm.Leveller(S, Cn, w, F, params=cm.agc_design(48000.0, w, -20.0, -60.0, 24.0, -24.0, 0.0, 3.0, 10.0))
        st = C.c_void_p(agc.hip_stream())

        def copy():
            assert hip.hipMemcpyAsync(dst, src.dev_in, min(in_bytes, S * out_stride * 2), 3, st) == 0   # device to device

        def run_agc():
            assert cm.lib.cmhip_test_agc_run_events(agc.h, src.dev_in, src.stride, F, None, dst, out_stride, ev) == 0

        warm(copy, agc)
        copies = []
        for _ in range(a.steps):
            assert hip.hipEventRecord(ev[0], st) == 0
            copy()
            assert hip.hipEventRecord(ev[1], st) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            copies.append(elapsed(ev[0], ev[1]))
        warm(run_agc, agc)
        lev = []
        for _ in range(a.steps):
            run_agc()
            assert hip.hipEventSynchronize(ev[3]) == 0
            lev.append(elapsed(ev[0], ev[3]))
        agc.close()
        medc, medl = statistics.median(copies), statistics.median(lev)
        for K in SOURCES:
            for fade in ((False, True) if K > 1 else (False,)):
                m = cm.Failover(S, S, Cn, w, F)
                for o in range(S):
                    m.set_sources(o, [(o + i) % S for i in range(K)])
                auto = cm.failover_params(w, fade_log2=16)
                forced = cm.failover_params(w, fade_log2=16, force=1) if fade else auto

                def timed():
                    if fade:                                   # one window on the main source, then the forced changeover
                        m.reset()
                        m.set(-1, auto)
                        m.run(src.dev_in, src.stride, W, dst, out_stride)
                        m.set(-1, forced)
                    assert cm.lib.cmhip_test_failover_run_events(m.h, src.dev_in, src.stride, F, None, dst, out_stride, ev) == 0

                warm(timed, m)
                parts = [[], [], [], []]                       # energy, step, apply, the whole run
                for _ in range(a.steps):
                    timed()
                    assert hip.hipEventSynchronize(ev[3]) == 0
                    for i in range(3):
                        parts[i].append(elapsed(ev[i], ev[i + 1]))
                    parts[3].append(elapsed(ev[0], ev[3]))
                med = [statistics.median(p) for p in parts]
                state = m.state()
                floor = medc * ((K + 3) if fade else (K + 2)) / 2.0
                p = cm.plan_agc(S * 4, Cn, w, F, F)
                line = {"shape": name, "outputs": S, "inputs": S, "channels": Cn, "frames": F, "window_log2": w,
                        "sources": K, "mode": "fade" if fade else "steady", "steps": a.steps,
                        "energy_ms_median": round(med[0], 4), "step_ms_median": round(med[1], 4),
                        "apply_ms_median": round(med[2], 4), "run_ms_median": round(med[3], 4),
                        "run_ms_min": round(min(parts[3]), 4), "run_ms_max": round(max(parts[3]), 4),
                        "copy_ms_median": round(medc, 4), "agc_run_ms_median": round(medl, 4),
                        "floor_ms": round(floor, 4), "ratio_to_copy": round(med[3] / medc, 3),
                        "ratio_to_floor": round(med[3] / floor, 3), "ratio_to_leveller": round(med[3] / medl, 3),
                        "from_to_after": [int(state["from"][0]), int(state["to"][0])],
                        "fade_window_after": int(state["fade_window"][0]), "switches_of_output_0": int(state["switches"][0]),
                        "plan": {"fast": p.fast, "tile_frames": 1 << p.tile_log2, "chunks": p.chunks, "energy_grid": p.grid,
                                 "apply_grid": p.grid // 4, "block": p.block, "nw": p.nw}}
                print(json.dumps(line), flush=True)
                lines.append(line)
                m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_failover": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_failover.py --steps %d --shapes %s\n" % (a.steps, a.shapes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
