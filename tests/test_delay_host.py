"""CPU: the delay stage's host side (cmhip_delay_crossfade, cmhip_delay_ms, the refusals, csrc/delay_plan.h) and an
emulation of k_delay.hip's decomposition -- tiles, their classes, aligned vectors and the funnel shift, the ring's head,
granules and ragged end -- against the model of tests/test_gpu_delay.py.  No GPU is used: where a test needs an object
it takes the test hook's object without a device (cmhip_test_delay_new_dry): the mirror and every check are the real ones."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "delay_plan_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_delay", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_delay")           # the model and the cases of the GPU tests


# ---------------------------------------------------------------------------
# the specification as code

def test_crossfade_equals_the_formula(cm):
    p = np.arange(32769, dtype=np.int64)
    for a, b in ((-32768, -32768), (-32768, 32767), (32767, -32768), (32767, 32767)):
        want = TG.crossfade(a, b, p)
        got = np.array([cm.delay_crossfade(a, b, int(v)) for v in p], dtype=np.int64)
        assert np.array_equal(got, want), (a, b)
        assert want.min() >= -32768 and want.max() <= 32767
        # the implementer's form is the same integer
        assert np.array_equal(a + ((p * (b - a) + 16384) >> 15), want)
    rng = np.random.default_rng(5)
    a = rng.integers(-32768, 32768, size=20000)
    b = rng.integers(-32768, 32768, size=20000)
    pp = rng.integers(0, 32769, size=20000)
    want = TG.crossfade(a, b, pp)
    got = np.array([cm.delay_crossfade(int(x), int(y), int(v)) for x, y, v in zip(a, b, pp)], dtype=np.int64)
    assert np.array_equal(got, want) and want.min() >= -32768 and want.max() <= 32767
    assert np.array_equal(a + ((pp * (b - a) + 16384) >> 15), want)
    for v in (-32768, -1, 0, 1, 12345, 32767):                                  # a == b returns a at every p
        assert {cm.delay_crossfade(v, v, int(q)) for q in range(0, 32769, 7)} == {v}
    assert cm.delay_crossfade(5, 900, 32768) == 900 and cm.delay_crossfade(5, 900, 0) == 5
    assert cm.delay_crossfade(5, 900, 1 << 31) == 900                           # p above 32768 counts as 32768
    # the positions the crossfade is fed with: the model's restatement is the library's, p(R) = 32768, p(1) = 0 at 32769
    pos = cm.lib.cmhip_mix_ramp_position
    for R in (2, 3, 1000, 32769, 1 << 20):
        assert pos(R, R) == 32768 and cm.delay_crossfade(5, 900, pos(R, R)) == 900
        k = np.unique(np.concatenate([np.arange(1, min(R, 3000) + 1), np.linspace(1, R, 500).astype(np.int64)]))
        assert np.array_equal(TG.ramp_position(k, R), np.array([pos(int(v), R) for v in k]))
    assert pos(1, 32769) == 0 and cm.delay_crossfade(5, 900, pos(1, 32769)) == 5


def test_delay_ms(cm):
    for rate, ms in ((48000, 0.0), (48000, 1.0), (44100, 2.5), (48000, 5000.0), (44100, 0.0113378684), (8000, 0.0624),
                     (96000, 33.3666)):
        assert cm.delay_ms(rate, ms) == int(np.rint(rate * ms / 1000.0)), (rate, ms)
    assert cm.delay_ms(48000, -1.0) == 0 and cm.delay_ms(48000, float("nan")) == 0


# ---------------------------------------------------------------------------
# refusals

def test_null_arguments_and_creation_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_delay_new(None) is None
    assert lib.cmhip_delay_set(None, -1, 0) == cm.ERROR_FAULT
    assert lib.cmhip_delay_ramp(None, -1, 0, 8) == cm.ERROR_FAULT
    assert lib.cmhip_delay_get(None, 0, None, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_delay_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_delay_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_delay_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_delay_hip_stream(None) is None and lib.cmhip_delay_max_delay(None) == 0
    lib.cmhip_delay_free(None)
    # descriptors that are refused before any device is touched
    for kw in (dict(streams=0), dict(channels=0), dict(channels=17), dict(max_frames=0),
               dict(max_delay=2 ** 31 - 64), dict(max_delay=2 ** 30, channels=2, max_frames=8), dict(max_frames=2 ** 31),
               dict(max_delay=2 ** 63, max_frames=2 ** 63), dict(max_delay=2 ** 27 - 64, channels=16)):
        f = dict(device=0, streams=2, channels=1, max_delay=9, max_frames=64, hip_stream=None)
        f.update(kw)
        assert lib.cmhip_delay_new(C.byref(cm.DelayDesc(**f))) is None, kw
        assert lib.cmhip_last_error()


@pytest.fixture
def delay(cm):
    """an object for the refusals that need one: the test hook's, with the host mirror and every check and no device
    behind it (tests/test_gpu_delay.py runs the same checks on a real one)"""
    d = cm.test_delay_without_device(3, 2, 9, 64)
    yield d
    d.close()


def check_object_refusals(cm, d):
    """every refusal of an object, and that each leaves the state as it was (d: cm.Delay(3, 2, 9, 64))"""
    lib = cm.lib
    assert d.max_delay() == 9 and d.get(0) == (0, 0, 0, 0)
    assert d.set_rc(0, 10) == cm.ERROR_INVAL and d.set_rc(3, 1) == cm.ERROR_INVAL and d.set_rc(-2, 1) == cm.ERROR_INVAL
    assert d.ramp_rc(0, 10, 8) == cm.ERROR_INVAL and d.ramp_rc(3, 1, 8) == cm.ERROR_INVAL
    assert d.ramp_rc(0, 1, (1 << 20) + 1) == cm.ERROR_INVAL
    assert [d.get(s) for s in range(3)] == [(0, 0, 0, 0)] * 3
    assert d.ramp_rc(1, 9, 1 << 20) == 0 and d.get(1) == (9, 0, 0, 1 << 20)
    for stream in (1, -1):                                                      # BUSY while ramping, the state unchanged
        assert d.ramp_rc(stream, 4, 8) == cm.ERROR_BUSY
        assert b"stream 1" in lib.cmhip_last_error()
        assert [d.get(s) for s in range(3)] == [(0, 0, 0, 0), (9, 0, 0, 1 << 20), (0, 0, 0, 0)]
    assert d.ramp_rc(0, 4, 8) == 0 and d.set_rc(-1, 7) == 0                     # a set ends every ramp
    assert [d.get(s) for s in range(3)] == [(7, 7, 0, 0)] * 3
    assert d.ramp_rc(2, 3, 0) == 0 and d.ramp_rc(1, 2, 1) == 0                  # R of 0 or 1 is a set
    assert [d.get(s) for s in range(3)] == [(7, 7, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0)]
    v = C.c_uint32(77)
    assert lib.cmhip_delay_get(d.h, 3, C.byref(v), None, None, None) == cm.ERROR_INVAL and v.value == 77
    assert lib.cmhip_delay_get(d.h, 0, None, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_delay_get(d.h, 0, C.byref(v), None, None, None) == 0 and v.value == 7
    assert lib.cmhip_delay_reset(d.h, 3) == cm.ERROR_INVAL
    # every stage_run_check case (the addresses are never read: every one of these calls is refused)
    assert d.ramp_rc(0, 1, 100) == 0
    before = [d.get(s) for s in range(3)]
    A, B, st = 0x10000, 0x20000, 128
    bad_count = np.array([64, 65, 1], dtype=np.uint32)
    for args, rc in (((None, st, 64, B, st), cm.ERROR_FAULT), ((A, st, 64, None, st), cm.ERROR_FAULT),
                     ((A + 2, st, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B + 8, st), cm.ERROR_INVAL),
                     ((A, st + 4, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, st + 2), cm.ERROR_INVAL),
                     ((A, st, 65, B, st), cm.ERROR_INVAL),                                    # frames > max_frames
                     ((A, 120, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, 120), cm.ERROR_INVAL),      # strides below frames * C
                     ((2 ** 64 - 512, st, 64, B, st), cm.ERROR_INVAL),                        # past the address space
                     ((A, st, 64, A, st), cm.ERROR_INVAL), ((A, st, 64, A + 3 * st * 2 - 16, st), cm.ERROR_INVAL),
                     ((A + 16, st, 64, A, st), cm.ERROR_INVAL)):                              # the arrays share a byte
        assert d.run_rc(*args) == rc, args
    assert d.run_rc(A, st, 64, B, st, frames_per_stream=bad_count) == cm.ERROR_INVAL
    assert b"frames_per_stream[1]" in lib.cmhip_last_error()
    assert [d.get(s) for s in range(3)] == before                               # no refused run moved the ramp
    assert d.run_rc(A, st, 0, B, st) == 0 and [d.get(s) for s in range(3)] == before      # no frames: nothing happens


def test_refusals_of_an_object(cm, delay):
    check_object_refusals(cm, delay)


# ---------------------------------------------------------------------------
# the plan

def test_plan(cm):
    for ch in range(1, 17):
        p = cm.plan_delay(5, ch, 9, 100, 1)
        fast = 1 if ch <= 2 else 0
        assert (p.err, p.grid, p.chunks, p.fast, p.block) == (0, 5, 1, fast, 64 if fast else 256)
        assert p.tile_frames == (2048 // ch if fast else 256) and p.tile_vecs * 8 == p.tile_frames * ch
        assert p.ring_frames == 112 and (p.ring_frames * ch) % 8 == 0
        p = cm.plan_delay(7, ch, 0, 3 * p.tile_frames, 2 * p.tile_frames + 1)
        assert (p.chunks, p.grid) == (3, 21) and p.ring_frames == 3 * p.tile_frames
    assert cm.plan_delay(3, 2, 48000, 512, 512).ring_frames == 48512
    assert cm.plan_delay(3, 2, 1, 6, 6).ring_frames == 8
    assert cm.plan_delay(1 << 20, 2, 0, 1 << 21, 1 << 21).err == 1              # the grid would reach 2^31 workgroups
    assert cm.plan_delay(1 << 20, 2, 0, 1 << 21, 1 << 20).err == 0
    for bad in ((0, 2, 9, 64), (3, 0, 9, 64), (3, 17, 9, 64), (3, 2, 9, 0), (3, 2, 2 ** 30, 8)):
        p = cm.plan_delay(*bad, 8)
        assert (p.err, p.grid, p.ring_frames) == (0, 0, 0), bad


def test_tile_classes(cm):
    B, Fr, M = cm.DELAY_BEHIND, cm.DELAY_FRONT, cm.DELAY_MIXED
    CAP = 4096
    assert cm.delay_tap(0, 2048, 0, 100, CAP) == (B, 0)                         # d = 0: the input itself
    assert cm.delay_tap(2048, 2048, 2048, 100, CAP) == (B, 0)
    assert cm.delay_tap(2048, 100, 63, 100, CAP) == (B, 1985)
    assert cm.delay_tap(0, 2048, 2048, 2048, CAP) == (Fr, 0)                    # wholly in front, no wrap
    assert cm.delay_tap(0, 2048, 2048, 100, CAP) == (M, 0)                      # ... across the ring's wrap
    assert cm.delay_tap(0, 100, 2048, 100, CAP) == (Fr, 2148)                   # (P - D) mod CAP
    assert cm.delay_tap(0, 2048, 2047, 2047, CAP) == (M, 0)                     # on the seam
    assert cm.delay_tap(0, 8, 9, 4090, CAP) == (Fr, 4081)
    assert cm.delay_tap(0, 8, 9, 4, CAP) == (M, 0)
    assert cm.delay_tap(0, 8, 4096, 0, CAP) == (Fr, 0)                          # D = CAP


# ---------------------------------------------------------------------------
# the kernel's decomposition, emulated

GARBAGE = 23130                        # what the input slot holds behind a stream's count


def emulate_run(cm, C, cap, ring, pos, rec, x, bug=None):
    """one stream's run as k_delay.hip cuts it.  ring: int64 [cap * C], changed in place; rec: (d1, d0, R, done)
    -> int16 [F][C].   bug: a mistake made on purpose -- 'seam', 'ring_tail', 'head', 'wrap', 'fade_frame' (the ramp
    starts a frame late), 'fade_sample' (a sample's number taken for its frame's: the division by C forgotten)"""
    d1, d0, R, done = rec
    x = np.asarray(x, dtype=np.int64).reshape(-1, C)
    F = x.shape[0]
    N, P, CAP = F * C, pos * C, cap * C
    plan = cm.plan_delay(1, C, 0, max(F, 1), max(F, 1))
    tile = plan.tile_vecs * 8
    stride = (N + 7) // 8 * 8 + 8
    ins = np.full(stride, GARBAGE, dtype=np.int64)
    ins[:N] = x.reshape(-1)
    old = ring.copy()                  # what the run may read: nothing it writes (checked below)
    out = np.full(N, 1 << 40, dtype=np.int64)
    written = np.zeros(CAP, dtype=bool)

    def fetch(base, nvec, a, sh):
        w = np.zeros(16, dtype=np.int64)
        if a < nvec:
            w[:8] = base[8 * a:8 * a + 8]
        if sh and a + 1 < nvec:
            w[8:] = base[8 * a + 8:8 * a + 16]
        return w[sh:sh + 8]

    def source(D, e0, length, e):
        cls, q = cm.delay_tap(e0, length, D, P, CAP)
        if bug == "wrap" and cls == cm.DELAY_MIXED and e0 + length <= D:
            cls, q = cm.DELAY_FRONT, (P + CAP + e0 - D) % CAP                   # the wrap goes unnoticed
        t = (e - e0) // 8
        if cls == cm.DELAY_BEHIND:
            return fetch(ins, stride // 8, q // 8 + t, q % 8)
        if cls == cm.DELAY_FRONT:
            return fetch(old, CAP // 8, q // 8 + t, q % 8)
        vcls, vq = cm.delay_tap(e, 8, D, P, CAP)                                 # a mixed tile: vector by vector
        if vcls == cm.DELAY_BEHIND:
            return fetch(ins, stride // 8, vq // 8, vq % 8)
        if vcls == cm.DELAY_FRONT:
            return fetch(old, CAP // 8, vq // 8, vq % 8)
        v = np.zeros(8, dtype=np.int64)
        for i in range(8):
            ee = e + i
            if ee < N:
                behind = ee > D if bug == "seam" else ee >= D
                v[i] = ins[ee - D] if behind and ee >= D else old[(P + CAP + ee - D) % CAP]
        return v

    h = (8 - P % 8) % 8
    for k in range(-(-N // tile)):
        e0 = k * tile
        length = min(tile, N - e0)
        if k == 0 and bug != "head":
            for i in range(min(h, N)):
                ring[(P + i) % CAP] = ins[i]
                written[(P + i) % CAP] = True
        for t in range(plan.tile_vecs):
            e = e0 + 8 * t
            if e >= N:                                                           # past the count: nothing is loaded
                continue
            y = source(d1 * C, e0, length, e)
            if done < R:
                y0 = source(d0 * C, e0, length, e)
                f = (e + np.arange(8)) // (1 if bug == "fade_sample" else C) + (1 if bug == "fade_frame" else 0)
                y = TG.crossfade(y0, y, TG.ramp_position(done + f + 1, R))
            n = min(8, max(0, N - e))
            out[e:e + n] = y[:n]
            es = e + h                                                           # the ring's granule
            g = fetch(ins, stride // 8, e // 8, h)
            if es < N:
                r = (P + es) % CAP
                assert r % 8 == 0 and r + 8 <= CAP
                n = 8 if es + 8 <= N else (0 if bug == "ring_tail" else N - es)
                assert not written[r:r + n].any()
                ring[r:r + n] = g[:n]
                written[r:r + n] = True
    if bug is None:
        lo = np.arange(P, P + N) % CAP
        assert written[lo].all() and written.sum() == N                          # exactly the run's samples
        assert np.array_equal(ring[lo], x.reshape(-1))
    assert (out < (1 << 40)).all()
    return out.reshape(-1, C).astype(np.int16)


def emulate_case(cm, C, max_delay, t, runs, seed, bug=None):
    """-> True when the emulation equals the model over the runs.  runs: per run a list of (count, action) per stream,
    action None, ('set', d) or ('ramp', d, R)"""
    S = len(runs[0])
    cap = cm.plan_delay(S, C, max_delay, 2 * t + 5, 1).ring_frames
    models = [TG.Model(C, max_delay) for _ in range(S)]
    rings = [np.zeros(cap * C, dtype=np.int64) for _ in range(S)]
    pos = [0] * S
    same = True
    for k, run in enumerate(runs):
        for s, (n, act) in enumerate(run):
            if act and act[0] == "set":
                models[s].set(act[1])
            elif act:
                models[s].ramp(act[1], act[2])
            m = models[s]
            x = TG.noise(seed + 100 * k + s, n, C)
            rec = (m.d1, m.d0, m.R, m.done)
            got = emulate_run(cm, C, cap, rings[s], pos[s], rec, x, bug)
            pos[s] = (pos[s] + n) % cap
            same = same and np.array_equal(got, m.run(x))
    return same


def case_runs(t, max_delay, nruns, ramps):
    counts, delays = TG.counts_of(t), TG.delays_of(t, max_delay)
    runs = []
    for k in range(nruns):
        run = []
        for s in range(3):
            d = delays[(5 * k + 7 * s) % len(delays)]
            act = ("ramp", d, [2, 3, 8, t + 1][(k + s) % 4]) if ramps and (k + s) % 2 else ("set", d)
            run.append((counts[(k + 3 * s) % len(counts)], act))
        runs.append(run)
    return runs


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("which", range(4))
def test_emulation_equals_the_model_on_steps(cm, which, channels):
    """tile classes, the ring's wrap, its ragged ends and the seam: steps through every delay, twice round the ring"""
    t = TG.tile_of(cm, channels)
    max_delay = TG.max_delays_of(t)[which]
    assert emulate_case(cm, channels, max_delay, t, case_runs(t, max_delay, 24, False), 1000 * which + channels)


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_emulation_equals_the_model_on_ramps(cm, channels):
    t = TG.tile_of(cm, channels)
    assert emulate_case(cm, channels, 3 * t, t, case_runs(t, 3 * t, 16, True), 77 + channels)


@pytest.mark.parametrize("bug,channels", [("seam", 1), ("ring_tail", 1), ("head", 1), ("wrap", 1), ("fade_frame", 1),
                                          ("seam", 2), ("wrap", 3), ("ring_tail", 5), ("fade_frame", 2), ("fade_frame", 3),
                                          ("fade_sample", 2), ("fade_sample", 3)])
def test_the_cases_notice_mistakes(cm, bug, channels):
    """a mistake made on purpose in the emulation is caught by the same cases, interleaved channels included: a ramp
    that starts a frame late, or that takes a sample's number for its frame's, shows only where C > 1 matters"""
    t = TG.tile_of(cm, channels)
    ramps = bug.startswith("fade")
    assert emulate_case(cm, channels, 3 * t, t, case_runs(t, 3 * t, 16, ramps), 5)
    assert not emulate_case(cm, channels, 3 * t, t, case_runs(t, 3 * t, 16, ramps), 5, bug=bug)


# ---------------------------------------------------------------------------
# the stand-alone plan program

def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program_over_random_geometries(tmp_path):
    exe, r = _build_plan_test(tmp_path, "delay_plan_test", [])                 # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "4000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "delay plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "delay_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "600"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "delay plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_delay_desc_t d; uint32_t a, b, c, e; d.device = 0; d.streams = d.channels = 1;\n"
           "d.max_delay = 9; d.max_frames = 1; d.hip_stream = 0;\n"
           "return (cmhip_delay_new(0) != 0) + cmhip_delay_set(0, -1, 0) + cmhip_delay_ramp(0, -1, 0, 8)"
           " + cmhip_delay_get(0, 0, &a, &b, &c, &e) + cmhip_delay_run(0, 0, 0, 0, 0, 0, 0) + cmhip_delay_reset(0, -1)"
           " + cmhip_delay_sync(0) + (cmhip_delay_hip_stream(0) != 0) + (int)cmhip_delay_max_delay(0)"
           " + (int)cmhip_delay_ms(48000, 1.0) + cmhip_delay_crossfade(1, 2, 3) + (cmhip_delay_free(0), 0) + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "free", "set", "ramp", "get", "run", "reset", "sync", "hip_stream", "max_delay", "ms", "crossfade"):
        assert hasattr(cm.lib, "cmhip_delay_" + name), name
    assert hasattr(cm.lib, "cmhip_test_plan_delay")


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_delay.s: it holds the three kernels by name, and the resource usage beside it shows
    that the mono / stereo kernels keep every register out of scratch memory"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_delay.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 3 and sum("k_delay_fast" in n for n in names) == 2 and sum("k_delay_any" in n for n in names) == 1
    usage = open(os.path.join(PKG, "build", "k_delay.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    fast = [n for n in scratch if "k_delay_fast" in n]
    assert len(fast) == 2 and not [n for n in fast if scratch[n]], scratch
