#!/usr/bin/env python3
"""How long an automixer run (cmhip_automix_run, csrc/k_automix.hip) takes, kernel by kernel, beside a leveller run and a
plain copy of the same slots in the same process.

Shapes: 4096 stereo and 8192 mono streams x 65536 frames, and 1365 streams of 6 channels; window_log2 = 8 and 12; every
stream in a group, groups of 4 and of 64 consecutive streams (the last group takes what is left).  The input is
GEN_NOISE in the slots of a batch used as device memory, the output plain device memory; the automixer's parameters are
attack 1, release 3, the rest at their defaults.  After 150 ms of the object's own launches every run is bracketed by
HIP events on its stream -- five of them, in front of, between and behind the four launches (the test hook
cmhip_test_automix_run_events; the clearing of the groups' sums lies in the first interval, with the energy pass) -- and
reported are the medians of --steps runs per kernel and for the whole run.  Beside it, bracketed the same way: a
leveller run over the same arrays (cmhip_test_agc_run_events, the parameters of tools/bench_agc.py) with the spread of
its own --steps runs, and a device-to-device copy (hipMemcpyAsync) of the input slots into the output slots.  That copy
is a yardstick, not a ceiling.

The energy and the apply pass are the leveller's tile bodies: the expectation is that they take what the leveller's take,
and that the run exceeds the leveller's by the two lane-per-stream kernels.  Each line says by how much it does
(`over_leveller_ms`), what the two small kernels take (`level_plus_share_ms`, against the leveller's `agc_step_ms`) and
the leveller's own spread (`agc_run_ms_max - agc_run_ms_min`).  Last: registers, LDS, scratch and waves per SIMD of the
eight kernels from build/k_automix.usage.txt (`make asm`).

    python tools/bench_automix.py [--steps N] [--shapes a,b] [--out FILE]   one JSON line per case, also written to FILE
    python tools/bench_automix.py --usage                                    the kernels' resources alone (no GPU needed)
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
WINDOWS = (8, 12)
GROUPS = (4, 64)


def usage():
    path = os.path.join(BUILD, "k_automix.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(path).read(), flags=re.S):
        stem = re.search(r"k_automix_[a-z]+(?:_fast|_any)?", m.group(1)).group(0)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "automix_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_automix": usage()}))
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
        ev = (C.c_void_p * 5)()
        for i in range(5):
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

        for w in WINDOWS:
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
            lev = [[], [], [], []]                             # energy, step, apply, the whole run
            for _ in range(a.steps):
                run_agc()
                assert hip.hipEventSynchronize(ev[3]) == 0
                for i in range(3):
                    lev[i].append(elapsed(ev[i], ev[i + 1]))
                lev[3].append(elapsed(ev[0], ev[3]))
            agc.close()
            medl = [statistics.median(p) for p in lev]
            medc = statistics.median(copies)
            for members in GROUPS:
                m = cm.Automixer(S, Cn, w, F, params=cm.automix_params(attack=1, release=3))
                for s in range(S):
                    m.set_group(s, s // members)

                def run():
                    assert cm.lib.cmhip_test_automix_run_events(m.h, src.dev_in, src.stride, F, None, dst, out_stride, ev) == 0

                warm(run, m)
                parts = [[], [], [], [], []]                   # energy (with the clearing), level, share, apply, the whole run
                for _ in range(a.steps):
                    run()
                    assert hip.hipEventSynchronize(ev[4]) == 0
                    for i in range(4):
                        parts[i].append(elapsed(ev[i], ev[i + 1]))
                    parts[4].append(elapsed(ev[0], ev[4]))
                med = [statistics.median(p) for p in parts]
                gain, power, share = m.state()
                p = cm.plan_agc(S, Cn, w, F, F)
                line = {"shape": name, "streams": S, "channels": Cn, "frames": F, "window_log2": w, "group_members": members,
                        "steps": a.steps,
                        "energy_ms_median": round(med[0], 4), "level_ms_median": round(med[1], 4),
                        "share_ms_median": round(med[2], 4), "apply_ms_median": round(med[3], 4),
                        "run_ms_median": round(med[4], 4), "run_ms_min": round(min(parts[4]), 4),
                        "run_ms_max": round(max(parts[4]), 4),
                        "agc_energy_ms_median": round(medl[0], 4), "agc_step_ms_median": round(medl[1], 4),
                        "agc_apply_ms_median": round(medl[2], 4), "agc_run_ms_median": round(medl[3], 4),
                        "agc_run_ms_min": round(min(lev[3]), 4), "agc_run_ms_max": round(max(lev[3]), 4),
                        "copy_ms_median": round(medc, 4),
                        "energy_ratio_to_leveller": round(med[0] / medl[0], 3),
                        "apply_ratio_to_leveller": round(med[3] / medl[2], 3),
                        "run_ratio_to_leveller": round(med[4] / medl[3], 3), "ratio_to_copy": round(med[4] / medc, 3),
                        "over_leveller_ms": round(med[4] - medl[3], 4),
                        "level_plus_share_ms": round(med[1] + med[2], 4),
                        "gain_of_stream_0": int(gain[0]), "sum_of_squares_of_group_0": int((gain[:members].astype("int64") ** 2).sum()),
                        "plan": {"fast": p.fast, "tile_frames": 1 << p.tile_log2, "chunks": p.chunks, "grid": p.grid,
                                 "block": p.block, "nw": p.nw, "step_grid": p.step_grid}}
                print(json.dumps(line), flush=True)
                lines.append(line)
                m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_automix": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_automix.py --steps %d --shapes %s\n" % (a.steps, a.shapes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
