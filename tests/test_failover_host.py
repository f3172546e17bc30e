"""CPU: the failover switch's host side (cmhip_failover_check, _design, _step, the refusals, the mirror through an object
without a device, csrc/failover_plan.h) and an emulation of k_failover.hip's walk -- the energy table per run, the lane
per output with its carried sums, counters and plan word, the plan words per window of the run, the apply pass -- held
against tests/failover_model.py over the GPU test's case, and shown to notice three planted mistakes."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import failover_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "failover_plan_test.cpp")


def cparams(cm, w, p):
    return cm.failover_params(w, **p)


def pack(fr, to, phi, q):
    return fr | to << 2 | phi << 4 | q << 16


def unpack(v):
    return v & 3, (v >> 2) & 3, (v >> 4) & 31, v >> 16


# ---------------------------------------------------------------------------
# check, design, step

def test_check(cm):
    assert cm.failover_check(6, 1) == 0 and cm.failover_check(14, 4) == 0
    for w in (5, 15):
        assert cm.failover_check(w, 1) == cm.ERROR_INVAL
    for k in (0, 5):
        assert cm.failover_check(6, k) == cm.ERROR_INVAL
    for w, K in ((6, 1), (9, 3), (14, 4)):
        good = FM.params(w)
        assert cm.failover_check(w, K, cparams(cm, w, good)) == 0
        for kw in (dict(quiet=(0, 0, 0, 32768)), dict(quiet=(40000, 0, 0, 0)), dict(fail_windows=0), dict(return_windows=0),
                   dict(fade_log2=w - 1), dict(fade_log2=17), dict(force=K), dict(force=-2)):
            p = dict(good, **kw)
            assert not FM.params_ok(p, w, K)
            assert cm.failover_check(w, K, cparams(cm, w, p)) == cm.ERROR_INVAL, kw
        for kw in (dict(quiet=(0, 32767, 1, 2)), dict(fail_windows=65535, return_windows=65535), dict(fade_log2=16),
                   dict(force=K - 1), dict(fade_log2=w)):
            assert cm.failover_check(w, K, cparams(cm, w, dict(good, **kw))) == 0, kw


def design_model(rate, w, quiet_db, fail_s, return_s, fade_ms):
    W = 1 << w

    def clamp(v, lo, hi):
        return int(min(max(v, lo), hi))

    def rint(v):
        return float(np.rint(v))

    return dict(quiet=tuple(clamp(rint(32768 * 10 ** (q / 20)), 0, 32767) for q in quiet_db),
                fail_windows=clamp(max(1, rint(fail_s * rate / W)), 1, 65535),
                return_windows=clamp(max(1, rint(return_s * rate / W)), 1, 65535),
                fade_log2=clamp(rint(math.log2(fade_ms * rate / 1000)), w, 16) if fade_ms > 0 else w, force=-1)


def test_design_equals_the_formulas(cm):
    rng = np.random.default_rng(7)
    for _ in range(300):
        rate = float(rng.choice([8000, 44100, 48000, 96000]))
        w = int(rng.integers(6, 15))
        q = tuple(float(v) for v in rng.uniform(-100, 3, size=4))
        fs, rs, ms = float(rng.uniform(0, 30)), float(rng.uniform(0, 4000)), float(rng.uniform(-1, 3000))
        assert cm.failover_design(rate, w, q, fs, rs, ms).as_dict() == design_model(rate, w, q, fs, rs, ms)
    p = cm.failover_design(48000, 12, -60.0, 2.0, 5.0, 100.0)
    assert p.as_dict() == dict(quiet=(33, 33, 33, 33), fail_windows=23, return_windows=59, fade_log2=12, force=-1)
    assert cm.failover_design(48000, 10, -60.0, 0.0, 0.0, 100.0).fade_log2 == 12     # 4800 frames: 2^12 is nearest
    assert cm.failover_check(12, 1, p) == 0


def test_design_refusals(cm):
    lib = cm.lib
    good = dict(rate=48000.0, window_log2=12.0, fail_s=1.0, return_s=1.0, fade_ms=10.0)

    def rc(**kw):
        f = dict(good, **kw)
        law = cm.FailoverLawDesc(f["rate"], f["window_log2"], (C.c_double * 4)(*f.get("quiet_db", (-60.0,) * 4)),
                                 f["fail_s"], f["return_s"], f["fade_ms"])
        return lib.cmhip_failover_design(C.byref(law), C.byref(cm.FailoverParams()))

    assert rc() == 0
    for kw in (dict(rate=0.0), dict(rate=-1.0), dict(rate=float("nan")), dict(window_log2=5.0), dict(window_log2=15.0),
               dict(window_log2=7.5), dict(fail_s=-1.0), dict(return_s=-0.1), dict(fade_ms=float("inf")),
               dict(quiet_db=(0.0, float("nan"), 0.0, 0.0)), dict(fail_s=float("inf"))):
        assert rc(**kw) == cm.ERROR_INVAL, kw
    assert lib.cmhip_failover_design(None, C.byref(cm.FailoverParams())) == cm.ERROR_FAULT
    law = cm.FailoverLawDesc(48000.0, 12.0, (C.c_double * 4)(-60.0, -60.0, -60.0, -60.0), 1.0, 1.0, 1.0)
    assert lib.cmhip_failover_design(C.byref(law), None) == cm.ERROR_FAULT


def test_step_equals_the_model_on_an_exhaustive_grid(cm):
    """K <= 4, every cur and force, counters in {0, 1, R - 1, R, 65535}"""
    n = 0
    for K in range(1, 5):
        for R, Fw in ((1, 1), (2, 3), (3, 2), (65535, 65535)):
            lv = sorted({0, 1, R - 1, R, 65535})
            dv = sorted({1, Fw - 1, Fw, 65535} - {0})
            for force in range(-1, K):
                cp = cparams(cm, 6, FM.params(6, fail_windows=Fw, return_windows=R, force=force))
                p = FM.params(6, fail_windows=Fw, return_windows=R, force=force)
                for live in itertools.product(lv, repeat=K):
                    for cur in range(K):
                        for dcur in (dv if live[cur] == 0 else [0]):
                            lr = list(live) + [0] * (4 - K)
                            dr = [0 if v else 1 for v in lr]
                            dr[cur] = dcur
                            assert cm.failover_step(K, cp, cur, lr, dr) == FM.step(K, p, cur, lr, dr), (K, p, cur, lr, dr)
                            n += 1
    assert n > 20000
    cp = cparams(cm, 6, FM.params(6))
    z = np.zeros(4, dtype=np.uint32)
    # what the function cannot judge gives cur back
    assert cm.failover_step(0, cp, 0, z, z) == 0 and cm.failover_step(5, cp, 3, z, z) == 3 and cm.failover_step(2, cp, 2, z, z) == 2
    assert cm.lib.cmhip_failover_step(2, None, 1, z.ctypes.data, z.ctypes.data) == 1


def test_edge_equals_the_model_counters_at_their_saturation(cm):
    """one window edge -- counters, fade or decision, the switch count -- against the model's Output.edge on random
    states; 65534 is planted in the state, not reached by 65535 windows"""
    rng = np.random.default_rng(11)
    trace = FM.new_trace()
    for it in range(4000):
        w = int(rng.integers(6, 10))
        K = int(rng.integers(1, 5))
        p = FM.params(w, quiet=tuple(int(v) for v in rng.integers(0, 4, size=4)), fail_windows=int(rng.choice([1, 2, 65535])),
                      return_windows=int(rng.choice([1, 2, 65535])), fade_log2=w + int(rng.integers(0, 3)),
                      force=int(rng.integers(-1, K)))
        t = FM.Output(1, w, 0, trace)
        t.src, t.p, t.n = list(range(K)), p, 5 << w
        live = [int(rng.choice([0, 1, 2, 65534, 65535])) for _ in range(4)]
        t.live = [v if i < K else 0 for i, v in enumerate(live)]
        t.dead = [0 if v else int(rng.choice([1, 2, 65534, 65535])) if i < K else 0 for i, v in enumerate(t.live)]
        t.level = [int(rng.integers(0, 12)) if i < K else 0 for i in range(4)]
        fr, to = int(rng.integers(0, K)), int(rng.integers(0, K))
        phi = w + int(rng.integers(0, 3))
        t.plan = (fr, to, phi, int(rng.integers(0, 1 << (phi - w)))) if fr != to else (to, to, 0, 0)
        before = t.switches
        pl, lr, dr, sw = cm.failover_edge(pack(*t.plan), K, cparams(cm, w, p), w, t.level, t.live, t.dead)
        t.edge()
        assert unpack(pl) == t.plan and lr == t.live and dr == t.dead and sw == t.switches - before, (it, p, t.plan)
    assert all(trace[b] > 0 for b in FM.BRANCHES + FM.SATURATION), trace


def test_fade_is_the_delay_stages_crossfade(cm):
    rng = np.random.default_rng(3)
    for _ in range(3000):
        a, b = (int(v) for v in rng.integers(-32768, 32768, size=2))
        phi = int(rng.integers(6, 17))
        d = int(rng.integers(0, 1 << phi))
        p = (d << 15) >> phi
        assert p < 32768
        assert cm.failover_fade(a, b, d, phi) == cm.delay_crossfade(a, b, p) == FM.crossfade(a, b, p)
    assert cm.failover_fade(-32768, 32767, 0, 16) == -32768                      # the fade's first frame is x_from
    assert cm.failover_first(cparams(cm, 6, FM.params(6, force=-1))) == pack(0, 0, 0, 0)


def test_the_cases_take_every_branch():
    """on the CPU, before any device run: the palette reaches every branch of the decision, a fade over four windows
    that runs cut, and a fade that ends where the next begins"""
    for channels, w in FM.CASE_SHAPES:
        model = FM.Switch(FM.CASE_STREAMS, FM.CASE_OUTPUTS, channels, w)
        FM.play_model(model, FM.case_script(channels, w))
        assert all(model.trace[b] > 0 for b in FM.BRANCHES), (channels, w, model.trace)
        assert any(s[0] in (1, 2, 3) for s in FM.CASE_SOURCES[1:] if len(s) > 1)
    used = {s for lst in FM.CASE_SOURCES for s in lst}
    assert 4 not in used and sum(5 in lst for lst in FM.CASE_SOURCES) == 3        # read by nobody; the shared backup
    assert sorted({len(lst) for lst in FM.CASE_SOURCES}) == [1, 2, 4]


def test_the_model_is_a_copy_where_the_header_says_so():
    rng = np.random.default_rng(2)
    m = FM.Switch(3, 3, 2, 6)
    m.set_sources(2, [1, 0])
    xs = [rng.integers(-32768, 32768, size=(500, 2)).astype(np.int16) for _ in range(3)]
    ys = m.run(xs, [500, 0, 333])
    assert np.array_equal(ys[0], xs[0]) and ys[1].shape == (0, 2) and np.array_equal(ys[2], xs[1][:333])
    assert m.out[1].n == 0 and m.state()["switches"] == [0, 0, 0]


# ---------------------------------------------------------------------------
# the object without a device: refusals and the mirror

def test_null_arguments_and_creation_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_failover_new(None) is None and lib.cmhip_test_failover_new_dry(None) is None
    for f in (lib.cmhip_failover_sync, lib.cmhip_failover_hip_stream):
        assert not f(None) or f(None) == cm.ERROR_FAULT
    lib.cmhip_failover_free(None)
    assert lib.cmhip_failover_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_failover_state(None, None, None, None, None, 0, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_failover_run(None, 16, 8, 0, None, 32, 8) == cm.ERROR_FAULT
    good = dict(device=0, streams=2, outputs=2, channels=2, window_log2=6, max_frames=64, hip_stream=None)
    for kw in (dict(streams=0), dict(outputs=0), dict(outputs=1 << 29), dict(channels=0), dict(channels=17),
               dict(window_log2=5), dict(window_log2=15), dict(max_frames=0), dict(max_frames=1 << 30)):
        f = dict(good, **kw)
        assert lib.cmhip_test_failover_new_dry(C.byref(cm.FailoverDesc(**f))) is None, kw
        assert lib.cmhip_last_error()


@pytest.fixture
def switch(cm):
    d = cm.test_failover_without_device(3, 4, 2, 6, 64)
    yield d
    d.close()


def check_object_refusals(cm, d):
    """every refusal of an object, and that each leaves the mirror as it was (d: cm.Failover(3, 4, 2, 6, 64), new)"""
    lib = cm.lib
    w = 6
    default = FM.params(w)
    assert cm.failover_params(w).as_dict() == default and [d.get(o).as_dict() for o in range(4)] == [default] * 4
    assert [d.get_sources(o) for o in range(4)] == [[0], [1], [2], [2]]          # min(o, S - 1)
    st = d.state()
    assert st["from"].tolist() == [0] * 4 and st["to"].tolist() == [0] * 4 and st["switches"].tolist() == [0] * 4
    assert not st["live_run"].any() and not st["level"].any()
    assert lib.cmhip_failover_state(d.h, None, None, None, None, 0, None, None, None) == 0     # any pointer may be NULL
    # lists
    assert d.set_sources_rc(0, [2, 0]) == 0 and d.set_sources_rc(3, [1, 2, 0]) == 0
    for o, lst in ((4, [0]), (0, []), (0, [0, 1, 2, 0]), (0, [0, 3]), (0, [1, 1]), (0, [0, 1, 2, 1, 0])):
        assert d.set_sources_rc(o, lst) == cm.ERROR_INVAL, (o, lst)
    assert lib.cmhip_failover_set_sources(d.h, 0, 1, None) == cm.ERROR_FAULT
    assert [d.get_sources(o) for o in range(4)] == [[2, 0], [1], [2], [1, 2, 0]]
    n, s = C.c_uint(77), np.full(4, 9, dtype=np.uint32)
    assert lib.cmhip_failover_get_sources(d.h, 4, C.byref(n), s.ctypes.data) == cm.ERROR_INVAL and n.value == 77
    assert lib.cmhip_failover_get_sources(d.h, 0, None, s.ctypes.data) == cm.ERROR_FAULT
    # set and get: per output and for -1; a force the list is too short for
    a = FM.params(w, quiet=(1, 2, 3, 4), fail_windows=7, return_windows=9, fade_log2=9, force=1)
    b = FM.params(w, quiet=(5, 6, 7, 8), fail_windows=2, return_windows=3, fade_log2=16)
    assert d.set_rc(3, cparams(cm, w, a)) == 0 and d.get(3).as_dict() == a
    assert d.set_rc(-1, cparams(cm, w, b)) == 0 and [d.get(o).as_dict() for o in range(4)] == [b] * 4
    assert d.set_rc(0, cparams(cm, w, a)) == 0
    assert d.state()["to"].tolist() == [1, 0, 0, 0]                               # before frame 0: c0 = force
    assert d.set_rc(1, cparams(cm, w, a)) == cm.ERROR_INVAL                       # K = 1: force 1 is out of range
    assert d.set_rc(-1, cparams(cm, w, a)) == cm.ERROR_INVAL                      # ... and refuses the whole call
    assert b"output 1" in lib.cmhip_last_error()
    for kw in (dict(quiet=(0, 0, 32768, 0)), dict(fail_windows=0), dict(return_windows=0), dict(fade_log2=5),
               dict(fade_log2=17), dict(force=-2), dict(force=4)):
        for o in (0, 3, -1):
            assert d.set_rc(o, cparams(cm, w, dict(b, **kw))) == cm.ERROR_INVAL, kw
    assert d.set_rc(4, cparams(cm, w, b)) == cm.ERROR_INVAL and d.set_rc(-2, cparams(cm, w, b)) == cm.ERROR_INVAL
    assert lib.cmhip_failover_set(d.h, 0, None) == cm.ERROR_FAULT
    v = cm.failover_params(w, fail_windows=99)
    assert lib.cmhip_failover_get(d.h, 4, C.byref(v)) == cm.ERROR_INVAL and v.fail_windows == 99
    assert lib.cmhip_failover_get(d.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_failover_reset(d.h, 4) == cm.ERROR_INVAL and lib.cmhip_failover_reset(d.h, -2) == cm.ERROR_INVAL
    before = [d.get(o).as_dict() for o in range(4)], [d.get_sources(o) for o in range(4)]
    assert before == ([a, b, b, b], [[2, 0], [1], [2], [1, 2, 0]])
    # a new list makes the output automatic again
    assert d.set_sources_rc(0, [0, 1]) == 0 and d.get(0).as_dict() == dict(a, force=-1) and d.state()["to"][0] == 0
    assert d.set_rc(0, cparams(cm, w, a)) == 0 and d.set_sources_rc(0, [2, 0]) == 0 and d.set_rc(0, cparams(cm, w, a)) == 0
    # every stage_run_check case (the addresses are never read: every one of these calls is refused); S = 3, O = 4
    A, B, st = 0x10000, 0x20000, 128
    for args, rc in (((None, st, 64, B, st), cm.ERROR_FAULT), ((A, st, 64, None, st), cm.ERROR_FAULT),
                     ((A + 2, st, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B + 8, st), cm.ERROR_INVAL),
                     ((A, st + 4, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, st + 2), cm.ERROR_INVAL),
                     ((A, st, 65, B, st), cm.ERROR_INVAL),                                    # frames > max_frames
                     ((A, 120, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, 120), cm.ERROR_INVAL),      # strides below frames * C
                     ((2 ** 64 - 512, st, 64, B, st), cm.ERROR_INVAL),                        # past the address space
                     ((A, st, 64, A, st), cm.ERROR_INVAL), ((A, st, 64, A + 3 * st * 2 - 16, st), cm.ERROR_INVAL),
                     ((A + 4 * st * 2 - 16, st, 64, A, st), cm.ERROR_INVAL)):                 # the arrays share a byte
        assert d.run_rc(*args) == rc, args
    assert d.run_rc(A, st, 64, B, st, frames_per_stream=np.array([64, 64, 64, 65], dtype=np.uint32)) == cm.ERROR_INVAL
    assert b"frames_per_output[3]" in lib.cmhip_last_error()                     # the counts are per OUTPUT: four of them
    assert d.run_rc(A, st, 65, B, st, frames_per_stream=np.array([99, 0, 0, 0], dtype=np.uint32)) == cm.ERROR_INVAL
    assert b"above the object's" in lib.cmhip_last_error()                       # frames > max_frames is said first
    assert d.run_rc(A, st, 0, B, st) == 0                                        # no frames: nothing happens
    assert d.run_rc(A, st, 0, B, st, frames_per_stream=np.zeros(4, dtype=np.uint32)) == 0
    assert ([d.get(o).as_dict() for o in range(4)], [d.get_sources(o) for o in range(4)]) == before
    assert d.state()["to"].tolist() == [1, 0, 0, 0]                               # no refused run moved an output off frame 0
    assert lib.cmhip_failover_reset(d.h, -1) == 0 and lib.cmhip_failover_reset(d.h, 2) == 0


def test_refusals_of_an_object(cm, switch):
    check_object_refusals(cm, switch)
    assert switch.run_rc(0x10000, 128, 64, 0x20000, 128) == cm.ERROR_INVAL       # a dry object launches nothing
    assert b"no device" in cm.lib.cmhip_last_error()
    switch.sync()
    assert switch.hip_stream() == 0


# ---------------------------------------------------------------------------
# k_failover.hip's walk, emulated

class Emulation:
    """O outputs as the host mirror and k_failover.hip hold them: the mirror's positions, parameters and lists; per run
    the rows' table of sums per window of the run and the plan words; per output the carried sums, the last levels, the
    counters and the plan word.  bug: a mistake made on purpose --
        "decide_first"  the decision is taken before the counters take the last window
        "ge"            LIVE is m >= quiet^2
        "restart"       a fade's length is read from the phi in force, not from the phi it began with"""

    def __init__(self, cm, streams, outputs, channels, w, max_frames, bug=None):
        self.cm, self.S, self.O, self.C, self.w, self.W, self.bug = cm, streams, outputs, channels, w, 1 << w, bug
        self.nw = max_frames // self.W + 2
        self.pos = [0] * outputs
        self.par = [FM.params(w) for _ in range(outputs)]
        self.src = [[min(o, streams - 1)] for o in range(outputs)]
        self.table = np.zeros((outputs, 4, self.nw, channels), dtype=np.int64)
        self.switches = [0] * outputs
        self.st = [dict(psum=np.zeros((4, channels), dtype=np.int64), level=[0] * 4, live=[0] * 4, dead=[0] * 4, plan=0)
                   for _ in range(outputs)]

    def _outs(self, output):
        return range(self.O) if output < 0 else [output]

    def set(self, output, p):
        for o in self._outs(output):
            self.par[o] = dict(p)

    def set_sources(self, o, streams):
        self.src[o] = list(streams)
        self.par[o] = dict(self.par[o], force=-1)
        self.pos[o] = 0

    def reset(self, output=-1):
        for o in self._outs(output):
            self.pos[o] = 0

    def state(self):
        out = dict(fr=[], to=[], fade_window=[], switches=list(self.switches), live_run=[], dead_run=[], level=[])
        for o in range(self.O):
            fresh = self.pos[o] == 0
            c0 = max(self.par[o]["force"], 0)
            fr, to, _, q = (c0, c0, 0, 0) if fresh else unpack(self.st[o]["plan"])
            K = len(self.src[o])
            out["fr"].append(fr)
            out["to"].append(to)
            out["fade_window"].append(q)
            for k, name in (("live", "live_run"), ("dead", "dead_run"), ("level", "level")):
                out[name].append([0 if fresh or i >= K else self.st[o][k][i] for i in range(4)])
        return out

    def _count(self, m, quiet, live, dead):
        is_live = m >= quiet * quiet if self.bug == "ge" else m > quiet * quiet
        return (min(live + 1, 65535), 0) if is_live else (0, min(dead + 1, 65535))

    def _edge(self, o, st):
        p, K, w = self.par[o], len(self.src[o]), self.w

        def counters():
            for c in range(K):
                st["live"][c], st["dead"][c] = self._count(st["level"][c], p["quiet"][c], st["live"][c], st["dead"][c])

        if self.bug != "decide_first":
            counters()
        fr, to, phi, q = unpack(st["plan"])
        length = p["fade_log2"] if self.bug == "restart" else phi
        if fr != to and q + 1 < (1 << max(length - w, 0)):
            st["plan"] = pack(fr, to, phi, q + 1)
        else:
            want = self.cm.failover_step(K, cparams(self.cm, w, p), to, st["live"], st["dead"])
            if want != to:
                self.switches[o] += 1
                st["plan"] = pack(to, want, p["fade_log2"], 0)
            else:
                st["plan"] = pack(to, to, 0, 0)
        if self.bug == "decide_first":
            counters()

    def run(self, slots, counts):
        Cn, w, W = self.C, self.w, self.W
        slots = [np.asarray(x, dtype=np.int64).reshape(-1, Cn) for x in slots]
        if max(counts) == 0:
            return [np.empty((0, Cn), dtype=np.int16) for _ in counts]
        runs = [self.cm.agc_run(self.pos[o], counts[o], w) for o in range(self.O)]
        assert all(r.nwin <= self.nw for r in runs)
        plan = [[None] * (self.nw + 1) for _ in range(self.O)]
        # energy: row (o, i) has output o's count and position and reads candidate i's slot; count 0 past the list
        for o in range(self.O):
            for i, s in enumerate(self.src[o]):
                for k in range(runs[o].nwin):
                    lo = max(0, (runs[o].first + k) * W - self.pos[o])
                    hi = min(counts[o], (runs[o].first + k + 1) * W - self.pos[o])
                    self.table[o, i, k] += (slots[s][lo:hi] ** 2).sum(axis=0)
        # step
        for o in range(self.O):
            r, st, K = runs[o], self.st[o], len(self.src[o])
            if counts[o] == 0:
                continue
            if self.pos[o] == 0:
                st["live"], st["dead"], st["level"] = [0] * 4, [0] * 4, [0] * 4
                st["plan"] = pack(max(self.par[o]["force"], 0), max(self.par[o]["force"], 0), 0, 0)
            carried = (self.pos[o] & (W - 1)) != 0
            for k in range(r.nwin):
                if (k > 0 or not carried) and r.first + k >= 1:
                    self._edge(o, st)
                plan[o][k] = st["plan"]
                for i in range(K):
                    sums = self.table[o, i, k] + (st["psum"][i] if k == 0 and carried else 0)
                    self.table[o, i, k] = 0
                    if k < r.complete:
                        st["level"][i] = int(sums.max()) >> w
                    else:
                        st["psum"][i] = sums
        assert not self.table.any()
        # apply: frame f of the run lies in window (j0 + f) >> w of the run
        ys = []
        for o in range(self.O):
            n = counts[o]
            f = np.arange(n, dtype=np.int64)
            at = (self.pos[o] & (W - 1)) + f
            win, j = at >> w, at & (W - 1)
            y = np.empty((n, Cn), dtype=np.int64)
            for k in set(win.tolist()):
                fr, to, phi, q = unpack(plan[o][k])
                sel = win == k
                a, b = slots[self.src[o][fr]][:n][sel], slots[self.src[o][to]][:n][sel]
                if fr == to:
                    y[sel] = b
                else:
                    p = (((q * W + j[sel]) << 15) >> phi)[:, None]
                    y[sel] = a + ((p * (b - a) + 16384) >> 15)
            ys.append(y.astype(np.int16))
            self.pos[o] += n
        return ys


def emulate_case(cm, channels, w, bug=None):
    """-> True when the emulation equals the model over the GPU test's case: outputs and state after every operation;
    the case's runs begin and end inside windows and inside fades"""
    model = FM.Switch(FM.CASE_STREAMS, FM.CASE_OUTPUTS, channels, w)
    e = Emulation(cm, FM.CASE_STREAMS, FM.CASE_OUTPUTS, channels, w, 5 * (1 << w) + 3, bug)
    same, inside_fade, inside_window = True, 0, 0
    for op in FM.case_script(channels, w):
        if op[0] == "run":
            got, want = e.run(op[1], op[2]), model.run(op[1], op[2])
            same = same and all(np.array_equal(a, b) for a, b in zip(got, want))
            for t in model.out:
                if t.n and t.n & ((1 << w) - 1):
                    inside_window += 1
                    inside_fade += t.plan[0] != t.plan[1]
        elif op[0] == "set":
            e.set(op[1], op[2])
            model.set(op[1], op[2])
        elif op[0] == "sources":
            e.set_sources(op[1], op[2])
            model.set_sources(op[1], op[2])
        else:
            e.reset(op[1])
            model.reset(op[1])
        same = same and e.state() == model.state()
    assert inside_window > 20 and inside_fade > 3
    return same


@pytest.mark.parametrize("channels,w", FM.CASE_SHAPES)
def test_emulation_equals_the_model(cm, channels, w):
    assert emulate_case(cm, channels, w)


@pytest.mark.parametrize("bug", ["decide_first", "ge", "restart"])
@pytest.mark.parametrize("channels,w", [(1, 6), (3, 6), (2, 7)])
def test_the_cases_notice_mistakes(cm, bug, channels, w):
    """a mistake made on purpose in the emulation is caught by the same cases"""
    assert not emulate_case(cm, channels, w, bug=bug)


# ---------------------------------------------------------------------------
# the stand-alone plan program

def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "failover_plan_test", [])             # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "failover plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "failover_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "failover plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_failover_desc_t d; cmhip_failover_params_t p; cmhip_failover_law_desc_t l; uint32_t g[4], v;\n"
           "uint64_t c; unsigned n;\n"
           "d.device = 0; d.streams = d.outputs = d.channels = 1; d.window_log2 = 6; d.max_frames = 1; d.hip_stream = 0;\n"
           "p.quiet[3] = p.fail_windows = p.return_windows = p.fade_log2 = 1; p.force = -1;\n"
           "l.rate = l.window_log2 = l.quiet_db[3] = l.fail_s = l.return_s = l.fade_ms = 0;\n"
           "return (cmhip_failover_new(0) != 0) + cmhip_failover_set(0, -1, &p) + cmhip_failover_get(0, 0, &p)"
           " + cmhip_failover_set_sources(0, 0, 1, g) + cmhip_failover_get_sources(0, 0, &n, g)"
           " + cmhip_failover_run(0, 0, 0, 0, 0, 0, 0) + cmhip_failover_reset(0, -1)"
           " + cmhip_failover_state(0, &v, &v, &v, &c, 0, g, g, g)"
           " + cmhip_failover_sync(0) + (cmhip_failover_hip_stream(0) != 0) + cmhip_failover_check(6, 1, &p)"
           " + cmhip_failover_design(&l, &p) + (int)cmhip_failover_step(1, &p, 0, g, g) + (cmhip_failover_free(0), 0)"
           " + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "free", "set", "get", "set_sources", "get_sources", "run", "reset", "state", "sync", "hip_stream",
                 "check", "design", "step"):
        assert hasattr(cm.lib, "cmhip_failover_" + name) and "cmhip_failover_" + name in cm.SIGNATURES, name
    for name in ("failover_new_dry", "failover_edge", "failover_first", "failover_fade", "failover_run_events"):
        assert hasattr(cm.lib, "cmhip_test_" + name), name
    assert C.sizeof(cm.FailoverParams) == 16 and C.sizeof(cm.FailoverLawDesc) == 72


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_failover.s: it holds the seven kernels by name, and the resource usage beside it shows
    that none of them keeps a register in scratch memory and that only the any-channel energy form has LDS"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_failover.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 7, names
    for stem, n in (("k_failover_energy_fast", 2), ("k_failover_energy_any", 1), ("k_failover_step", 1),
                    ("k_failover_apply_fast", 2), ("k_failover_apply_any", 1)):
        assert sum(stem in name for name in names) == n, (stem, names)
    usage = open(os.path.join(PKG, "build", "k_failover.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 7 and not [n for n in scratch if scratch[n]], scratch
    lds = {m.group(1): int(m.group(2))
           for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", usage, flags=re.S)}
    assert [n for n in lds if lds[n]] == [n for n in lds if "energy_any" in n]
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*=.*\bk_failover\.hip\b.*\bcmhip_failover\.hip\b", mk, flags=re.M) and "build/k_failover.s" in mk
