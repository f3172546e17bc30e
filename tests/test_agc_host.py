"""CPU: the leveller's host side (cmhip_agc_check, cmhip_agc_design, the refusals, the mirror, csrc/agc_plan.h) and an
emulation of k_agc.hip's decomposition -- window-aligned tiles cut at 16-byte vectors, partial sums added in any order,
the lane's walk over a run's windows, the nodes table -- against the model of tests/test_gpu_agc.py.  No GPU is used:
where a test needs an object it takes the test hook's object without a device (cmhip_test_agc_new_dry): the mirror and
every check are the real ones."""
import collections
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "agc_plan_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_agc", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_agc")             # the model and the cases of the GPU tests


# ---------------------------------------------------------------------------
# the specification as code

def test_step_equals_the_formula(cm):
    rng = np.random.default_rng(12)
    sets = [TG.palette(k) for k in range(8)] + [TG.params(**TG.FAST_FALL)]
    for _ in range(40):
        lo, hi = sorted(int(v) for v in rng.integers(1, 65536, size=2))
        sets.append(TG.params(target=int(rng.integers(1, 32768)), gate=int(rng.integers(0, 2000)), gain_min=lo, gain_max=hi,
                              rise=int(rng.choice([0, 1, 65535, int(rng.integers(0, 65536))])),
                              fall=int(rng.choice([0, 1, 65535, int(rng.integers(0, 65536))])), initial=lo))
    trace = collections.Counter()
    for p in sets:
        cp = cm.AgcParams(**p)
        assert cm.agc_check(6, cp) == 0
        levels = [0, 1, 2, 299, 300, 301, 32767, 32768] + [int(v) for v in rng.integers(0, 32769, size=12)]
        for L in levels:
            D = min(max((p["target"] << 12) // L, p["gain_min"]), p["gain_max"]) if L else p["gain_min"]
            gains = {p["gain_min"], p["gain_max"], D, max(p["gain_min"], D - 1), min(p["gain_max"], D + 1)}
            gains |= {int(v) for v in rng.integers(p["gain_min"], p["gain_max"] + 1, size=6)}
            for A in gains:
                got = cm.agc_step(A, L, cp)
                assert got == TG.step(A, L, p, trace), (A, L, p)
                assert p["gain_min"] <= got <= p["gain_max"]
    assert all(trace[b] > 0 for b in TG.BRANCHES), trace
    # the header's figures
    q = cm.AgcParams(**TG.params(gate=0, gain_min=1, gain_max=65535, rise=1, fall=1))
    assert [cm.agc_step(a, 300, q) for a in (44740, 44741, 44742)] == [44741] * 3
    f = cm.AgcParams(**TG.params(**TG.FAST_FALL))
    assert cm.agc_step(65535, 32768, f) == 4095 and cm.agc_step(4095, 32768, f) == 4095


def test_the_palette_takes_every_branch():
    """eight streams of the model alone take every branch of the step, so do the GPU cases of eight streams and more"""
    signals, plist, _ = TG.model_case(8, 2, 6, 7)
    trace = collections.Counter()
    clips = []
    for s in range(8):
        m = TG.Model(2, 6, plist[s])
        m.run(signals[s])
        trace += m.trace
        clips.append(m.clips)
    assert all(trace[b] > 0 for b in TG.BRANCHES), trace
    assert sum(clips) > 0 and 0 in clips


def test_the_model_gives_the_issues_figures():
    n = np.arange(40 * 64)
    m = TG.Model(1, 6, TG.params(target=3277, gate=0, gain_min=1, gain_max=65535, rise=20000, fall=20000))
    y = m.run(np.where((n // 5) % 2 == 0, 300, -300).astype(np.int16))
    assert m.a_hi == 44741 == (3277 << 12) // 300 and m.level == 300 and m.clips == 0
    assert set(np.unique(y[-640:]).tolist()) == {-3277, 3277}
    m = TG.Model(1, 6, TG.params(**TG.FAST_FALL))
    m.run(np.full(128, -32768, dtype=np.int16))
    assert m.nodes == [65535, 65535, 4095] and m.level == 32768 and m.clips == 128
    # unity parameters: the input, bit for bit; no frames: nothing changes
    x = np.random.default_rng(3).integers(-32768, 32768, size=(1000, 3)).astype(np.int16)
    m = TG.Model(3, 7)
    assert np.array_equal(m.run(x), x) and m.clips == 0
    before = (m.n, m.a_lo, m.a_hi, m.level, m.sums.tolist())
    m.run(x[:0])
    assert before == (m.n, m.a_lo, m.a_hi, m.level, m.sums.tolist())


# ---------------------------------------------------------------------------
# design

def design_model(rate, w, target_db, gate_db, max_db, min_db, init_db, rise, fall):
    """the header's formulas -> (the parameters, the distance of every value from a half before it is rounded)"""
    W = float(1 << w)
    raw = dict(target=32768.0 * 10.0 ** (target_db / 20.0), gate=32768.0 * 10.0 ** (gate_db / 20.0),
               gain_max=4096.0 * 10.0 ** (max_db / 20.0), gain_min=4096.0 * 10.0 ** (min_db / 20.0),
               initial=4096.0 * 10.0 ** (init_db / 20.0),
               rise=(10.0 ** (rise * W / rate / 20.0) - 1.0) * 65536.0,
               fall=(1.0 - 10.0 ** (-fall * W / rate / 20.0)) * 65536.0)
    margin = min(abs(v - math.floor(v) - 0.5) for v in raw.values())
    lim = dict(target=(1, 32767), gate=(0, 32767), gain_max=(1, 65535), gain_min=(1, 65535), rise=(0, 65535), fall=(0, 65535))
    p = {k: int(min(max(np.rint(raw[k]), lim[k][0]), lim[k][1])) for k in lim}
    p["initial"] = int(min(max(np.rint(raw["initial"]), p["gain_min"]), p["gain_max"]))
    return p, margin


DESIGNS = [(48000.0, 12, -20.0, -60.0, 24.0, -12.0, 0.0, 3.0, 10.0), (44100.0, 10, -18.0, -50.0, 20.0, -6.0, 6.0, 1.5, 6.0),
           (8000.0, 6, -23.0, -70.0, 12.0, 0.0, 3.0, 20.0, 40.0), (96000.0, 14, -14.0, -45.0, 6.0, -20.0, -3.0, 0.5, 2.0),
           (48000.0, 12, -20.0, -60.0, 30.0, -80.0, 40.0, 0.0, 0.0),            # gains clamped at both ends, frozen
           (48000.0, 14, 3.0, -200.0, 24.0, 24.0, -5.0, 500.0, 5000.0)]          # target, gate, rise and fall clamped


def test_design_equals_the_formulas(cm):
    for d in DESIGNS:
        want, margin = design_model(*d)
        assert margin > 1e-6, (d, margin)          # no value so near a half that the last bit of pow() decides
        got = cm.agc_design(*d).as_dict()
        assert got == want, d
        assert cm.agc_check(d[1], cm.AgcParams(**got)) == 0
    p = cm.agc_design(*DESIGNS[0])
    assert (p.rise, p.fall) == (1960, 6132) and (p.target, p.gate) == (3277, 33)
    assert (p.gain_max, p.gain_min, p.initial) == (64917, 1029, 4096)
    p = cm.agc_design(*DESIGNS[4])
    assert (p.gain_max, p.gain_min, p.initial, p.rise, p.fall) == (65535, 1, 65535, 0, 0)
    p = cm.agc_design(*DESIGNS[5])
    assert (p.target, p.gate, p.rise, p.fall) == (32767, 0, 65535, 65535) and p.initial == p.gain_min == p.gain_max


def test_design_refusals(cm):
    lib = cm.lib
    good = list(DESIGNS[0])
    out = cm.AgcParams(*([7] * 7))
    assert lib.cmhip_agc_design(None, C.byref(out)) == cm.ERROR_FAULT
    assert lib.cmhip_agc_design(C.byref(cm.AgcLawDesc(*good)), None) == cm.ERROR_FAULT
    for i in range(9):
        for bad in (float("nan"), float("inf"), float("-inf")):
            d = list(good)
            d[i] = bad
            assert lib.cmhip_agc_design(C.byref(cm.AgcLawDesc(*d)), C.byref(out)) == cm.ERROR_INVAL, (i, bad)
    for i, bad in ((0, 0.0), (0, -48000.0), (1, 5.0), (1, 15.0), (1, 12.5), (7, -1.0), (8, -0.5), (5, 25.0)):
        d = list(good)
        d[i] = bad
        assert lib.cmhip_agc_design(C.byref(cm.AgcLawDesc(*d)), C.byref(out)) == cm.ERROR_INVAL, (i, bad)
        assert lib.cmhip_last_error()
    assert out.as_dict() == dict.fromkeys(cm.AGC_PARAM_NAMES, 7)           # no refused call wrote anything


def test_check(cm):
    for w in range(0, 20):
        assert cm.agc_check(w) == (0 if 6 <= w <= 14 else cm.ERROR_INVAL), w
    assert cm.agc_check(6, cm.agc_params()) == 0
    for kw in (dict(target=0), dict(target=32768), dict(gate=32768), dict(gain_min=0, initial=1), dict(gain_min=4097),
               dict(gain_max=4095), dict(initial=4095), dict(gain_max=8192, initial=8193), dict(gain_min=0, gain_max=0, initial=0)):
        assert cm.agc_check(6, cm.agc_params(**kw)) == cm.ERROR_INVAL, kw
    for kw in (dict(target=1), dict(target=32767, gate=32767), dict(gain_min=1, gain_max=65535, initial=65535),
               dict(rise=65535, fall=65535), dict(gain_min=1, initial=1)):
        assert cm.agc_check(14, cm.agc_params(**kw)) == 0, kw


# ---------------------------------------------------------------------------
# refusals

def test_null_arguments_and_creation_refusals(cm):
    lib = cm.lib
    p = cm.agc_params()
    assert lib.cmhip_agc_new(None) is None and lib.cmhip_test_agc_new_dry(None) is None
    assert lib.cmhip_agc_set(None, -1, C.byref(p)) == cm.ERROR_FAULT
    assert lib.cmhip_agc_get(None, 0, C.byref(p)) == cm.ERROR_FAULT
    assert lib.cmhip_agc_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_agc_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_agc_state(None, None, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_agc_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_agc_hip_stream(None) is None
    assert lib.cmhip_test_agc_step(1, 1, None) == 0
    lib.cmhip_agc_free(None)
    # descriptors that are refused before any device is touched
    for kw in (dict(streams=0), dict(channels=0), dict(channels=17), dict(max_frames=0), dict(window_log2=5),
               dict(window_log2=15), dict(max_frames=2 ** 31), dict(max_frames=2 ** 30, channels=2),
               dict(max_frames=2 ** 27, channels=16), dict(max_frames=2 ** 63)):
        f = dict(device=0, streams=2, channels=1, window_log2=6, max_frames=64, hip_stream=None)
        f.update(kw)
        assert lib.cmhip_agc_new(C.byref(cm.AgcDesc(**f))) is None, kw
        assert lib.cmhip_last_error()
        assert lib.cmhip_test_agc_new_dry(C.byref(cm.AgcDesc(**f))) is None, kw


@pytest.fixture
def leveller(cm):
    """an object for the refusals that need one: the test hook's, with the host mirror and every check and no device
    behind it (tests/test_gpu_agc.py runs the same checks on a real one)"""
    d = cm.test_agc_without_device(3, 2, 6, 64)
    yield d
    d.close()


def check_object_refusals(cm, d):
    """every refusal of an object, and that each leaves the state as it was (d: cm.Leveller(3, 2, 6, 64))"""
    lib = cm.lib
    default = cm.agc_params().as_dict()
    assert default == TG.params() and [d.get(s).as_dict() for s in range(3)] == [default] * 3
    gain, level, clips = d.state()
    assert gain.tolist() == [4096] * 3 and level.tolist() == [0] * 3 and clips.tolist() == [0] * 3
    assert lib.cmhip_agc_state(d.h, None, None, None, 1) == 0            # any of the three may be NULL
    # set and get: per stream and for -1, and the refusals
    a, b = TG.palette(0), TG.palette(4)
    assert d.set_rc(1, cm.AgcParams(**a)) == 0
    assert [d.get(s).as_dict() for s in range(3)] == [default, a, default]
    assert d.set_rc(-1, cm.AgcParams(**b)) == 0
    assert [d.get(s).as_dict() for s in range(3)] == [b] * 3
    assert d.state()[0].tolist() == [b["initial"]] * 3                   # before frame 0: the initial in force
    assert d.set_rc(2, cm.AgcParams(**a)) == 0
    before = [d.get(s).as_dict() for s in range(3)]
    assert before == [b, b, a]
    good = cm.AgcParams(**default)
    assert d.set_rc(3, good) == cm.ERROR_INVAL and d.set_rc(-2, good) == cm.ERROR_INVAL
    assert lib.cmhip_agc_set(d.h, 0, None) == cm.ERROR_FAULT
    for kw in (dict(target=0), dict(target=32768), dict(gate=32768), dict(gain_min=0), dict(gain_min=5000),
               dict(initial=4097), dict(gain_max=4000)):
        for stream in (0, -1):
            assert d.set_rc(stream, cm.agc_params(**kw)) == cm.ERROR_INVAL, kw
    v = cm.AgcParams(*([9] * 7))
    assert lib.cmhip_agc_get(d.h, 3, C.byref(v)) == cm.ERROR_INVAL and v.target == 9
    assert lib.cmhip_agc_get(d.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_agc_reset(d.h, 3) == cm.ERROR_INVAL and lib.cmhip_agc_reset(d.h, -2) == cm.ERROR_INVAL
    assert [d.get(s).as_dict() for s in range(3)] == before
    # every stage_run_check case (the addresses are never read: every one of these calls is refused)
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
    assert d.run_rc(A, st, 0, B, st) == 0                                # no frames: nothing happens
    assert [d.get(s).as_dict() for s in range(3)] == before
    gain, level, clips = d.state()                                       # no refused run moved a stream off frame 0
    assert gain.tolist() == [b["initial"], b["initial"], a["initial"]] and level.tolist() == [0] * 3
    assert clips.tolist() == [0] * 3
    assert d.set_rc(-1, good) == 0 and lib.cmhip_agc_reset(d.h, -1) == 0 and lib.cmhip_agc_reset(d.h, 1) == 0


def test_refusals_of_an_object(cm, leveller):
    check_object_refusals(cm, leveller)
    assert leveller.run_rc(0x10000, 128, 64, 0x20000, 128) == cm.ERROR_INVAL      # a dry object launches nothing
    assert b"no device" in cm.lib.cmhip_last_error()
    leveller.sync()
    assert leveller.hip_stream() == 0


# ---------------------------------------------------------------------------
# the plan

def test_plan(cm):
    for ch in range(1, 17):
        fast = 1 if ch <= 2 else 0
        for w in range(6, 15):
            p = cm.plan_agc(5, ch, w, 1000, 1000)
            most = (11 if ch == 1 else 10) if fast else 8
            assert (p.err, p.fast, p.block, p.tile_log2) == (0, fast, 64 if fast else 256, min(w, most))
            tile = 1 << p.tile_log2
            assert p.chunks == -(-1000 // tile) + 1 and p.grid == 5 * p.chunks and p.step_grid == 1
            assert p.nw == 1000 // (1 << w) + 2
            assert tile * ch <= (2048 if fast else 4096)                  # four vectors a lane, two a thread
    assert cm.plan_agc(65, 2, 6, 64, 1).step_grid == 2 and cm.plan_agc(64, 2, 6, 64, 1).step_grid == 1
    p = cm.plan_agc(3, 2, 6, 64, 0)
    assert (p.err, p.grid, p.nw) == (0, 0, 3)
    assert cm.plan_agc(1 << 20, 1, 6, 1 << 21, 1 << 21).err == 1          # the grid would reach 2^31 workgroups
    assert cm.plan_agc(1 << 20, 1, 14, 1 << 21, 1 << 21).err == 0
    for bad in ((0, 2, 6, 64), (3, 0, 6, 64), (3, 17, 6, 64), (3, 2, 5, 64), (3, 2, 15, 64), (3, 2, 6, 0), (3, 2, 6, 2 ** 30)):
        p = cm.plan_agc(*bad, 8)
        assert (p.err, p.grid, p.nw) == (0, 0, 0), bad


def test_run_windows(cm):
    r = cm.agc_run(0, 0, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (0, 0, 0, 0, 0)
    r = cm.agc_run(0, 64, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (0, 1, 1, 0, 0)
    r = cm.agc_run(63, 1, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (0, 1, 1, 1, 0)
    r = cm.agc_run(63, 66, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (0, 3, 2, 1, 1)
    r = cm.agc_run((1 << 40) + 5, 323, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (1 << 34, 6, 5, 59, 8)
    r = cm.agc_run(10, 3, 6)
    assert (r.first, r.nwin, r.complete, r.head, r.tail) == (0, 1, 0, 3, 0)


# ---------------------------------------------------------------------------
# the kernels' decomposition, emulated

class Emulation:
    """one stream as the three kernels treat it.  bug: a mistake made on purpose -- 'tail' (the energy pass drops a
    tile's ragged end), 'carry' (the carried partial window is forgotten), 'window' (a tile's window is taken from its
    place in the run, not in the stream), 'node' (the apply pass reads the nodes a window late)"""

    def __init__(self, cm, channels, w, max_frames, p, seed, bug=None):
        self.cm, self.C, self.w, self.W, self.max_frames = cm, channels, w, 1 << w, max_frames
        self.nw = cm.plan_agc(1, channels, w, max_frames, 0).nw
        self.table = np.zeros((self.nw, channels), dtype=np.int64)       # zero between runs
        self.p = dict(p)
        self.pos = 0
        self.psum = np.zeros(channels, dtype=np.int64)
        self.a_lo = self.a_hi = self.level = 0
        self.clips = 0
        self.rng = np.random.default_rng(seed)
        self.bug = bug

    def state(self):
        return (self.p["initial"] if self.pos == 0 else self.a_hi), self.level, self.clips

    def tiles(self, plan, count):
        out = []
        for t in self.rng.permutation(plan.chunks):                     # workgroups run in any order
            tl, sp = self.cm.agc_tile(self.pos & 0xffffffff, count, self.w, plan.tile_log2, int(t), self.C)
            if tl.fa < tl.fb:
                assert tl.fb - tl.fa <= 1 << plan.tile_log2 and tl.win < self.nw
                assert (sp.sa, sp.sb) == (tl.fa * self.C, tl.fb * self.C) and sp.hend - sp.sa <= 7 and sp.sb - sp.tb <= 7
                assert sp.sa <= sp.hend <= sp.tb <= sp.sb and (sp.ve - sp.vb) * 8 == sp.tb - sp.hend     # whole vectors between
                assert sp.ve == sp.vb or sp.vb * 8 == sp.hend
                assert sp.ve - sp.vb <= (256 if plan.fast else 512)
                out.append((tl, sp))
        return out

    def run(self, x, frames):
        """x: int16 [count][C] of a run whose largest count is `frames` -> int16 [count][C]"""
        Cn, w = self.C, self.w
        x = np.asarray(x, dtype=np.int64).reshape(-1, Cn)
        count = x.shape[0]
        if frames == 0:
            return x.astype(np.int16)
        plan = self.cm.plan_agc(1, Cn, w, self.max_frames, frames)
        flat = np.concatenate([x.reshape(-1), np.full(16, TG.POISON, dtype=np.int64)])     # the slot past the count
        chan = np.arange(flat.size) % Cn
        tiles = self.tiles(plan, count)
        assert sum(tl.fb - tl.fa for tl, _ in tiles) == count
        # 1. energy: per tile and piece a partial sum per channel; the adds arrive in any order
        partial = []
        for tl, sp in tiles:
            pieces = [(sp.sa, sp.hend), (sp.vb * 8, sp.ve * 8)] + ([] if self.bug == "tail" else [(sp.tb, sp.sb)])
            win = (tl.fa >> w) if self.bug == "window" else tl.win
            for lo, hi in pieces:
                if lo < hi:
                    sq = flat[lo:hi] ** 2
                    partial.append((win, np.array([int(sq[chan[lo:hi] == c].sum()) for c in range(Cn)], dtype=np.int64)))
        for i in self.rng.permutation(len(partial)):
            self.table[partial[i][0]] += partial[i][1]
        # 2. step: the lane's walk
        if count:
            r = self.cm.agc_run(self.pos, count, w)
            assert r.nwin <= self.nw
            cp = self.cm.AgcParams(**self.p)
            nodes = np.zeros(self.nw + 1, dtype=np.int64)
            carried = (self.pos & (self.W - 1)) != 0
            if self.pos == 0:
                self.a_lo = self.a_hi = self.p["initial"]
                self.level = 0
            for i in range(r.nwin):
                if (i > 0 or not carried) and r.first + i >= 1:
                    self.a_lo, self.a_hi = self.a_hi, self.cm.agc_step(self.a_hi, self.level, cp)
                nodes[i], nodes[i + 1] = self.a_lo, self.a_hi
                sums = self.table[i] + (self.psum if i == 0 and carried and self.bug != "carry" else 0)
                self.table[i] = 0
                if i < r.complete:
                    self.level = math.isqrt(int(sums.max()) >> w)
                else:
                    self.psum = sums.copy()
            assert not self.table.any()
        # 3. apply
        y = np.full(count * Cn, 1 << 40, dtype=np.int64)
        for tl, sp in tiles:
            k = tl.win + (1 if self.bug == "node" and tl.win + 1 < self.nw else 0)
            a0, a1 = int(nodes[k]), int(nodes[k + 1])
            for lo, hi in ((sp.sa, sp.hend), (sp.vb * 8, sp.ve * 8), (sp.tb, sp.sb)):
                if lo < hi:
                    e = np.arange(lo, hi)
                    j = tl.j + (e // Cn - tl.fa)
                    assert j.min() >= 0 and j.max() < self.W
                    g = a0 + (((a1 - a0) * j) >> w)
                    v = (flat[lo:hi] * g + 2048) >> 12
                    out = np.clip(v, -32768, 32767)
                    self.clips += int((out != v).sum())
                    assert (y[lo:hi] == 1 << 40).all()                   # no sample twice
                    y[lo:hi] = out
        assert (y < (1 << 40)).all()                                     # ... and none left out
        self.pos += count
        return y.reshape(-1, Cn).astype(np.int16)


def emulate_case(cm, streams, channels, w, seed, bug=None):
    """-> True when the emulation equals the model over a GPU test's case: outputs, clips and state after every run"""
    signals, plist, cuts = TG.model_case(streams, channels, w, seed)
    max_frames = 5 * (1 << w) + 3
    same = True
    for s in range(streams):
        m, e = TG.Model(channels, w, plist[s]), Emulation(cm, channels, w, max_frames, plist[s], seed + s, bug)
        at = 0
        for counts in cuts:
            x = signals[s][at:at + counts[s]]
            at += counts[s]
            got, want = e.run(x, max(counts)), m.run(x)
            same = same and np.array_equal(got, want) and e.state() == m.state()
        assert at == len(signals[s])
    return same


@pytest.mark.parametrize("channels", [1, 2, 3, 6, 16])
@pytest.mark.parametrize("w", [6, 8])
def test_emulation_equals_the_model(cm, w, channels):
    assert emulate_case(cm, 8 if w == 6 else 3, channels, w, 1000 * w + 10 * channels)


@pytest.mark.parametrize("bug,channels", [("tail", 1), ("tail", 3), ("carry", 1), ("carry", 6), ("window", 2),
                                          ("window", 16), ("node", 1), ("node", 5)])
def test_the_cases_notice_mistakes(cm, bug, channels):
    """a mistake made on purpose in the emulation is caught by the same cases"""
    assert emulate_case(cm, 8, channels, 6, 5)
    assert not emulate_case(cm, 8, channels, 6, 5, bug=bug)


# ---------------------------------------------------------------------------
# the stand-alone plan program

def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "agc_plan_test", [])                   # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "agc plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "agc_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "agc plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_agc_desc_t d; cmhip_agc_params_t p; cmhip_agc_law_desc_t l; uint32_t g, v; uint64_t c;\n"
           "d.device = 0; d.streams = d.channels = 1; d.window_log2 = 6; d.max_frames = 1; d.hip_stream = 0;\n"
           "p.target = p.gate = p.gain_min = p.gain_max = p.rise = p.fall = p.initial = 1;\n"
           "l.rate = l.window_log2 = l.target_db = l.gate_db = l.max_gain_db = l.min_gain_db = l.initial_gain_db = 0;\n"
           "l.rise_db_per_s = l.fall_db_per_s = 0;\n"
           "return (cmhip_agc_new(0) != 0) + cmhip_agc_set(0, -1, &p) + cmhip_agc_get(0, 0, &p)"
           " + cmhip_agc_run(0, 0, 0, 0, 0, 0, 0) + cmhip_agc_reset(0, -1) + cmhip_agc_state(0, &g, &v, &c, 0)"
           " + cmhip_agc_sync(0) + (cmhip_agc_hip_stream(0) != 0) + cmhip_agc_check(6, &p) + cmhip_agc_design(&l, &p)"
           " + (cmhip_agc_free(0), 0) + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "free", "set", "get", "run", "reset", "state", "sync", "hip_stream", "check", "design"):
        assert hasattr(cm.lib, "cmhip_agc_" + name) and "cmhip_agc_" + name in cm.SIGNATURES, name
    for name in ("plan_agc", "agc_run", "agc_tile", "agc_new_dry", "agc_step"):
        assert hasattr(cm.lib, "cmhip_test_" + name), name
    assert C.sizeof(cm.AgcParams) == 14 and C.sizeof(cm.AgcLawDesc) == 72


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_agc.s: it holds the seven kernels by name, and the resource usage beside it shows that
    none of them keeps a register in scratch memory"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_agc.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 7, names
    for stem, n in (("k_agc_energy_fast", 2), ("k_agc_energy_any", 1), ("k_agc_step", 1), ("k_agc_apply_fast", 2),
                    ("k_agc_apply_any", 1)):
        assert sum(stem in name for name in names) == n, (stem, names)
    usage = open(os.path.join(PKG, "build", "k_agc.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 7 and not [n for n in scratch if scratch[n]], scratch
    # the body's loads and stores are 16 bytes wide, and the adds into the table are 64-bit integer adds
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text and "global_atomic_add_x2" in text
