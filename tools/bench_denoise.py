#!/usr/bin/env python3
"""How long a noise suppressor run (cmhip_denoise_run, csrc/k_denoise.hip) takes, beside a plain copy of the same slots
and beside the spectrum meter's pass at the same block size.

Shapes: 4096 stereo and 8192 mono streams x 65536 frames, at fft_log2 = 8, 10 and 12.  The input is GEN_NOISE in the slots
of a batch used as device memory, the output plain device memory.  Two settings: the creation defaults (every gain at
unity: a pure delay, but both transforms of every block are computed all the same -- the kernel has no shortcut), and
mid-suppression (the profile learned from the first run, then floor 4125, over 64, shifts 1 and 2 over the same noise:
about every bin moves).  After a warm-up run every run is bracketed by two HIP events on the object's stream; reported are
the medians of --steps runs and, bracketed the same way in the same process,
  - the median of a device-to-device copy (hipMemcpyAsync) of the input slots into the output slots: a yardstick, not a
    ceiling -- the copy reads and writes every sample once, as the suppressor does;
  - the spectrum meter's pass over the same slots at the same N with every channel selected: the median of the batch's
    run with the meter on less the median with it off.  Per block the suppressor computes two transforms of the
    spectrum's cost, one forward and one inverse, so twice that pass is the arithmetic it cannot do without.
Also: registers, LDS, scratch and waves per SIMD of the five kernels from build/k_denoise.usage.txt (`make asm`).

    python tools/bench_denoise.py [--steps N] [--shapes a,b] [--sizes 8,10,12] [--out FILE]
    python tools/bench_denoise.py --usage                                  the kernels' resources alone (no GPU needed)
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "libcoolmic-dsp_amd", "build")
SHAPES = {"s2": (4096, 2, 65536), "m1": (8192, 1, 65536)}


def usage():
    path = os.path.join(BUILD, "k_denoise.usage.txt")
    if not os.path.exists(path):
        return None
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", open(path).read(), flags=re.S):
        n = re.search(r"ILj(\d+)E", m.group(1)).group(1)
        f = dict(re.findall(r"remark:\s+([\w \[\]/]+): (\d+)", m.group(2)))
        lds = int(m.group(3))
        out["k_denoise<%s>" % n] = {"vgprs": int(f["VGPRs"]), "sgprs": int(f["TotalSGPRs"]),
                                    "scratch": int(f["ScratchSize [bytes/lane]"]), "lds_bytes": lds,
                                    "waves_per_simd_by_registers": int(f["Occupancy [waves/SIMD]"]),
                                    "workgroups_per_cu_by_lds": min(8, 163840 // lds)}
    return out


def hip_runtime():
    """the HIP runtime the engine is bound to, for the events and the copy"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sizes", default="8,10,12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.txt"))
    ap.add_argument("--usage", action="store_true")
    a = ap.parse_args()
    if a.usage:
        print(json.dumps({"k_denoise": usage()}))
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
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        in_bytes = S * src.stride * 2

        def timed(fn, st, steps):
            """the median, the least and the most of `steps` calls, each bracketed by two events on stream st, in ms"""
            ts = []
            for _ in range(steps):
                assert hip.hipEventRecord(e0, st) == 0
                fn()
                assert hip.hipEventRecord(e1, st) == 0
                assert hip.hipEventSynchronize(e1) == 0
                t = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
                ts.append(t.value)
            return statistics.median(ts), min(ts), max(ts)

        bst = C.c_void_p(src.hip_stream())
        for n in [int(v) for v in a.sizes.split(",")]:
            # the spectrum meter's pass at this N over every channel: the batch's run with it less the run without
            assert src.set_spectrum(False) == 0
            src.run(F)
            off = timed(lambda: src.run(F), bst, a.steps)[0]
            assert src.spec_configure(n, None, list(range(Cn))) == 0 and src.set_spectrum(True) == 0
            src.run(F)
            on = timed(lambda: src.run(F), bst, a.steps)[0]
            assert src.set_spectrum(False) == 0
            spec_ms = on - off
            m = cm.Denoiser(S, Cn, n, F)
            st = C.c_void_p(m.hip_stream())
            src.sync()

            def copy():
                assert hip.hipMemcpyAsync(dst, src.dev_in, min(in_bytes, S * out_stride * 2), 3, st) == 0   # device to device

            def run():
                m.run(src.dev_in, src.stride, F, dst, out_stride)

            copy()
            m.sync()
            medc = timed(copy, st, max(a.steps, 10))[0]
            for setting in ("defaults", "mid"):
                if setting == "mid":
                    m.learn(-1, True)
                run()                                                    # the warm-up; for "mid" the profile too
                if setting == "mid":
                    m.learn(-1, False)
                    m.set(-1, cm.denoise_params(floor=4125, over=64, rise_shift=1, fall_shift=2))
                    run()                                                # the gains settle
                m.sync()
                med, lo, hi = timed(run, st, a.steps)
                clips, sat, learned = m.state()
                _, g = m.get_profile(0, 0)
                blocks = F // (1 << (n - 1))                             # per row and run, once the row is under way
                line = {"shape": name, "streams": S, "channels": Cn, "frames": F, "fft_log2": n, "setting": setting,
                        "steps": a.steps, "run_ms_median": round(med, 3), "run_ms_min": round(lo, 3), "run_ms_max": round(hi, 3),
                        "copy_ms_median": round(medc, 4), "spectrum_pass_ms": round(spec_ms, 3),
                        "ratio_to_copy": round(med / medc, 1), "ratio_to_spectrum_pass": round(med / spec_ms, 2),
                        "us_per_block_and_row": round(1000.0 * med / blocks / (S * Cn), 5),
                        "blocks_per_row": blocks, "rows": S * Cn, "mean_gain_of_row_0": round(float(g.mean()), 1),
                        "clips": int(clips.sum()), "sat": int(sat.sum()), "learned_blocks_of_stream_0": int(learned[0])}
                print(json.dumps(line), flush=True)
                lines.append(line)
            m.close()
        cm.lib.cmhip_device_free(0, dst)
        src.close()
    lines.append({"k_denoise": usage()})
    print(json.dumps(lines[-1]))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python tools/bench_denoise.py --steps %d --shapes %s --sizes %s\n" % (a.steps, a.shapes, a.sizes))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
