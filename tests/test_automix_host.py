"""CPU: the automixer's host side (cmhip_automix_check, cmhip_automix_design, the refusals, the mirror,
csrc/automix_plan.h) and an emulation of the walk of k_automix.hip's two lane-per-stream kernels -- a run's windows, the
carried partial window, the groups' sums cleared per run, the nodes table -- against the model of tests/automix_model.py
over the GPU test's cases.  No GPU is used: where a test needs an object it takes the test hook's object without a
device (cmhip_test_automix_new_dry): the mirror and every check are the real ones."""
import collections
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import automix_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "automix_plan_test.cpp")


# ---------------------------------------------------------------------------
# the specification as code

def test_power_and_share_equal_the_formulas(cm):
    rng = np.random.default_rng(5)
    trace = collections.Counter()
    for u in (0, 1, 4095, 4096, 2048):
        for at, re_ in ((0, 0), (8, 8), (0, 8), (3, 1)):
            p = AM.params(weight=u, attack=at, release=re_)
            cp = cm.AutomixParams(**p)
            assert cm.automix_check(6, cp) == 0
            for m in [0, 1, 2 ** 30, 2 ** 30 - 1, 4096, 4097] + [int(v) for v in rng.integers(0, 2 ** 30 + 1, size=6)]:
                V = ((m * u) >> 12) << 8
                for P in {0, 1, V, max(V - 1, 0), min(V + 1, 2 ** 38), V // 2, 2 ** 38, int(rng.integers(0, 2 ** 38 + 1))}:
                    got = cm.automix_power(P, m, cp)
                    assert got == AM.power(P, m, p, trace), (P, m, p)
                    assert 0 <= got <= 2 ** 38
    for _ in range(3000):
        n = int(rng.integers(1, 7))
        Ps = [int(rng.choice([0, 1, 2 ** 38, int(rng.integers(0, 2 ** 38 + 1)), int(rng.integers(0, 500))])) for _ in range(n)]
        total, floor = sum(Ps), int(rng.choice([0, 0, int(rng.integers(0, 4097))]))
        squares = 0
        for P in Ps:
            before = int(rng.integers(0, 4097))
            got = cm.automix_share(P, total, floor, before)
            assert got == AM.share(P, total, floor, before, trace) and got <= 4096
            squares += cm.automix_share(P, total, 0, 0) ** 2
        assert squares <= 2 ** 24
    assert all(trace[b] > 0 for b in AM.BRANCHES), trace
    # the header's figures
    for n, want in ((1, 4096), (2, 2896), (3, 2364), (4, 2048)):
        assert cm.automix_share(12345, n * 12345, 0, 0) == want == math.isqrt(2 ** 24 // n)
    assert cm.automix_share(0, 777, 0, 9) == 0 and cm.automix_share(0, 777, 50, 9) == 50 and cm.automix_share(777, 777, 50, 9) == 4096
    assert cm.automix_share(0, 0, 50, 9) == 9


def square(frames, channels, amp=8000, half=5):
    n = np.arange(frames)
    return np.where((n // half) % 2 == 0, amp, -amp).astype(np.int16)[:, None].repeat(channels, axis=1)


def test_the_model_gives_the_issues_figures():
    W = 64
    for n, want in ((1, 4096), (2, 2896), (3, 2364), (4, 2048)):
        d = AM.Desk(4, 1, 6)
        for s in range(n):
            d.set_group(s, 0)
        xs = [square(4 * W, 1) for _ in range(4)]
        ys = d.run(xs)
        gain, power, share = d.state()
        assert gain[:n] == [want] * n and gain[n:] == [4096] * (4 - n) and share[:n] == [want] * n
        assert len(set(power[:n])) == 1 and power[0] == (8000 * 8000) << 8
        for s in range(n, 4):
            assert np.array_equal(ys[s], xs[s])                          # in no group: a copy
        if n == 1:
            assert np.array_equal(ys[0], xs[0])                          # a group of one with a level: a copy
        else:
            assert set(np.unique(ys[0][3 * W:]).tolist()) == {(8000 * want + 2048) >> 12, (-8000 * want + 2048) >> 12}
    # a talker against silence, with floors
    d = AM.Desk(4, 2, 6)
    for s in range(4):
        d.set(s, AM.params(floor=100 * s))
        d.set_group(s, 3)
    d.run([square(3 * W, 2)] + [np.zeros((3 * W, 2), dtype=np.int16)] * 3)
    assert d.state()[0] == [4096, 100, 200, 300]
    # a group of one that starts low is a copy from its third window on
    d = AM.Desk(1, 1, 6)
    d.set(0, AM.params(initial=0))
    d.set_group(0, 0)
    x = square(5 * W, 1)
    y = d.run([x])[0]
    assert not y[:W].any() and np.array_equal(y[2 * W:], x[2 * W:]) and not np.array_equal(y[W:2 * W], x[W:2 * W])
    assert all(sq <= 2 ** 24 for sq, bare in d.squares if bare)


def test_the_cases_take_every_branch():
    trace = collections.Counter()
    for channels, w in AM.CASE_SHAPES:
        d = AM.case_desk(channels, w)
        signals, cuts = AM.case(channels, w)
        out = AM.walk(d, signals, cuts)
        trace += d.trace
        assert all(sq <= 2 ** 24 for sq, bare in d.squares if bare) and any(bare for _, bare in d.squares)
        assert np.array_equal(out[5], signals[5])                        # the stream in no group
        assert all(np.abs(o.astype(np.int64)).max() <= np.abs(x.astype(np.int64)).max() for o, x in zip(out, signals))
        assert any(0 in c for c in cuts) and {c[0] for c in cuts} == {c[2] for c in cuts}
        assert all(c[0] == c[1] == c[2] and c[3] == c[4] for c in cuts) and any(c[0] != c[3] for c in cuts)
    assert all(trace[b] > 0 for b in AM.BRANCHES), trace


# ---------------------------------------------------------------------------
# design, check

def design_model(rate, w, weight_db, floor_db, initial_db, attack_ms, release_ms):
    """the header's formulas -> (the parameters, the distance of every value from a half before it is rounded)"""
    W = float(1 << w)
    raw = dict(weight=4096.0 * 10.0 ** (weight_db / 10.0), floor=4096.0 * 10.0 ** (floor_db / 20.0),
               initial=4096.0 * 10.0 ** (initial_db / 20.0))
    lim = dict(weight=4096, floor=4096, initial=4096, attack=8, release=8)
    for k, ms in (("attack", attack_ms), ("release", release_ms)):
        raw[k] = math.log2(ms * rate / 1000.0 / W) if ms > 0 else 0.0
    margin = min(abs(v - math.floor(v) - 0.5) for v in raw.values())
    return {k: int(min(max(np.rint(raw[k]), 0), lim[k])) for k in lim}, margin


DESIGNS = [(48000.0, 8, 0.0, -100.0, 0.0, 0.0, 0.0), (48000.0, 8, -3.0, -15.0, -6.0, 10.0, 200.0),
           (44100.0, 6, -10.0, -40.0, -20.0, 5.0, 50.0), (8000.0, 14, -1.0, 0.0, 3.0, 1.0, 1e6),     # shifts clamped
           (96000.0, 10, -60.0, 6.0, -200.0, 30.0, 3000.0), (48000.0, 12, -0.5, -30.0, -1.0, 400.0, 90.0)]


def test_design_equals_the_formulas(cm):
    for d in DESIGNS:
        want, margin = design_model(*d)
        assert margin > 1e-6, d
        p = cm.automix_design(*d)
        assert p.as_dict() == want, d
        assert cm.automix_check(int(d[1]), p) == 0
    assert cm.automix_design(*DESIGNS[0]).as_dict() == AM.params(floor=0)
    assert cm.automix_design(*DESIGNS[1]).as_dict() == dict(weight=2053, floor=728, initial=2053, attack=1, release=5)


def test_design_refusals(cm):
    lib = cm.lib
    out = cm.AutomixParams(*([7] * 5))
    good = list(DESIGNS[1])
    assert lib.cmhip_automix_design(None, C.byref(out)) == cm.ERROR_FAULT
    assert lib.cmhip_automix_design(C.byref(cm.AutomixLawDesc(*good)), None) == cm.ERROR_FAULT
    bads = [(i, v) for i in range(7) for v in (float("nan"), float("inf"), -float("inf"))]
    bads += [(0, 0.0), (0, -48000.0), (1, 5.0), (1, 15.0), (1, 8.5), (2, 0.25)]
    for i, bad in bads:
        d = list(good)
        d[i] = bad
        assert lib.cmhip_automix_design(C.byref(cm.AutomixLawDesc(*d)), C.byref(out)) == cm.ERROR_INVAL, (i, bad)
        assert lib.cmhip_last_error()
    assert out.as_dict() == dict.fromkeys(cm.AUTOMIX_PARAM_NAMES, 7)       # no refused call wrote anything


def test_check(cm):
    for w in range(0, 20):
        assert cm.automix_check(w) == (0 if 6 <= w <= 14 else cm.ERROR_INVAL), w
    assert cm.automix_check(6, cm.automix_params()) == 0
    for kw in (dict(weight=4097), dict(floor=4097), dict(attack=9), dict(release=9), dict(initial=4097), dict(weight=65535)):
        assert cm.automix_check(6, cm.automix_params(**kw)) == cm.ERROR_INVAL, kw
    for kw in (dict(weight=0, floor=0, initial=0), dict(weight=4096, floor=4096, attack=8, release=8, initial=4096)):
        assert cm.automix_check(14, cm.automix_params(**kw)) == 0, kw


# ---------------------------------------------------------------------------
# refusals

def test_null_arguments_and_creation_refusals(cm):
    lib = cm.lib
    p = cm.automix_params()
    g = C.c_long(5)
    assert lib.cmhip_automix_new(None) is None and lib.cmhip_test_automix_new_dry(None) is None
    assert lib.cmhip_automix_set(None, -1, C.byref(p)) == cm.ERROR_FAULT
    assert lib.cmhip_automix_get(None, 0, C.byref(p)) == cm.ERROR_FAULT
    assert lib.cmhip_automix_set_group(None, 0, 0) == cm.ERROR_FAULT
    assert lib.cmhip_automix_get_group(None, 0, C.byref(g)) == cm.ERROR_FAULT and g.value == 5
    assert lib.cmhip_automix_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_automix_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_automix_state(None, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_automix_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_automix_hip_stream(None) is None
    assert lib.cmhip_test_automix_power(1, 1, None) == 0
    lib.cmhip_automix_free(None)
    # descriptors that are refused before any device is touched
    for kw in (dict(streams=0), dict(channels=0), dict(channels=17), dict(max_frames=0), dict(window_log2=5),
               dict(window_log2=15), dict(max_frames=2 ** 31), dict(max_frames=2 ** 30, channels=2),
               dict(max_frames=2 ** 27, channels=16), dict(max_frames=2 ** 63)):
        f = dict(device=0, streams=2, channels=1, window_log2=6, max_frames=64, hip_stream=None)
        f.update(kw)
        assert lib.cmhip_automix_new(C.byref(cm.AutomixDesc(**f))) is None, kw
        assert lib.cmhip_last_error()
        assert lib.cmhip_test_automix_new_dry(C.byref(cm.AutomixDesc(**f))) is None, kw


@pytest.fixture
def automixer(cm):
    """an object for the refusals that need one: the test hook's, with the host mirror and every check and no device
    behind it (tests/test_gpu_automix.py runs the same checks on a real one)"""
    d = cm.test_automix_without_device(3, 2, 6, 64)
    yield d
    d.close()


def check_object_refusals(cm, d):
    """every refusal of an object, and that each leaves the state as it was (d: cm.Automixer(3, 2, 6, 64), new)"""
    lib = cm.lib
    default = cm.automix_params().as_dict()
    assert default == AM.params() and [d.get(s).as_dict() for s in range(3)] == [default] * 3
    assert [d.get_group(s) for s in range(3)] == [-1] * 3
    gain, power, share = d.state()
    assert gain.tolist() == [4096] * 3 and power.tolist() == [0] * 3 and share.tolist() == [4096] * 3
    assert lib.cmhip_automix_state(d.h, None, None, None) == 0           # any of the three may be NULL
    # set and get: per stream and for -1, and the refusals
    a, b = AM.palette(1), AM.palette(4)
    assert d.set_rc(1, cm.AutomixParams(**a)) == 0
    assert [d.get(s).as_dict() for s in range(3)] == [default, a, default]
    assert d.set_rc(-1, cm.AutomixParams(**b)) == 0
    assert [d.get(s).as_dict() for s in range(3)] == [b] * 3
    assert d.state()[0].tolist() == [4096] * 3                           # in no group: unity, whatever `initial` says
    assert d.set_rc(2, cm.AutomixParams(**a)) == 0
    # groups: 0 and 2 in group 2, 1 in none
    assert d.set_group_rc(0, 2) == 0 and d.set_group_rc(2, 2) == 0 and d.set_group_rc(1, 0) == 0 and d.set_group_rc(1, -1) == 0
    before = [d.get(s).as_dict() for s in range(3)], [d.get_group(s) for s in range(3)]
    assert before == ([b, b, a], [2, -1, 2])
    assert d.state()[0].tolist() == [b["initial"], 4096, a["initial"]]   # before frame 0: the initial in force
    assert d.state()[2].tolist() == [b["initial"], 4096, a["initial"]]
    good = cm.AutomixParams(**default)
    assert d.set_rc(3, good) == cm.ERROR_INVAL and d.set_rc(-2, good) == cm.ERROR_INVAL
    assert lib.cmhip_automix_set(d.h, 0, None) == cm.ERROR_FAULT
    for kw in (dict(weight=4097), dict(floor=4097), dict(attack=9), dict(release=9), dict(initial=4097)):
        for stream in (0, -1):
            assert d.set_rc(stream, cm.automix_params(**kw)) == cm.ERROR_INVAL, kw
    for stream, group in ((3, 0), (-1, 0), (-2, 0), (0, 3), (0, -2), (2 ** 40, 0), (0, 2 ** 40)):
        assert d.set_group_rc(stream, group) == cm.ERROR_INVAL, (stream, group)
    v = cm.AutomixParams(*([9] * 5))
    g = C.c_long(77)
    assert lib.cmhip_automix_get(d.h, 3, C.byref(v)) == cm.ERROR_INVAL and v.weight == 9
    assert lib.cmhip_automix_get(d.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_automix_get_group(d.h, 3, C.byref(g)) == cm.ERROR_INVAL and g.value == 77
    assert lib.cmhip_automix_get_group(d.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_automix_reset(d.h, 3) == cm.ERROR_INVAL and lib.cmhip_automix_reset(d.h, -2) == cm.ERROR_INVAL
    assert ([d.get(s).as_dict() for s in range(3)], [d.get_group(s) for s in range(3)]) == before
    # every stage_run_check case (the addresses are never read: every one of these calls is refused)
    A, B, st = 0x10000, 0x20000, 128
    for args, rc in (((None, st, 64, B, st), cm.ERROR_FAULT), ((A, st, 64, None, st), cm.ERROR_FAULT),
                     ((A + 2, st, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B + 8, st), cm.ERROR_INVAL),
                     ((A, st + 4, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, st + 2), cm.ERROR_INVAL),
                     ((A, st, 65, B, st), cm.ERROR_INVAL),                                    # frames > max_frames
                     ((A, 120, 64, B, st), cm.ERROR_INVAL), ((A, st, 64, B, 120), cm.ERROR_INVAL),      # strides below frames * C
                     ((2 ** 64 - 512, st, 64, B, st), cm.ERROR_INVAL),                        # past the address space
                     ((A, st, 64, A, st), cm.ERROR_INVAL), ((A, st, 64, A + 3 * st * 2 - 16, st), cm.ERROR_INVAL),
                     ((A + 16, st, 64, A, st), cm.ERROR_INVAL)):                              # the arrays share a byte
        assert d.run_rc(*args) == rc, args
    assert d.run_rc(A, st, 64, B, st, frames_per_stream=np.array([64, 65, 64], dtype=np.uint32)) == cm.ERROR_INVAL
    assert b"frames_per_stream[1]" in lib.cmhip_last_error()
    # two members of one group with different counts: both streams and both counts are named
    assert d.run_rc(A, st, 64, B, st, frames_per_stream=np.array([10, 5, 11], dtype=np.uint32)) == cm.ERROR_INVAL
    msg = lib.cmhip_last_error()
    assert b"stream 0 has 10 frames" in msg and b"stream 2" in msg and b"has 11" in msg, msg
    assert d.run_rc(A, st, 0, B, st) == 0                                # no frames: nothing happens
    assert d.run_rc(A, st, 0, B, st, frames_per_stream=np.zeros(3, dtype=np.uint32)) == 0    # equal counts of 0 are fine
    assert ([d.get(s).as_dict() for s in range(3)], [d.get_group(s) for s in range(3)]) == before
    gain, power, share = d.state()                                       # no refused run moved a stream off frame 0
    assert gain.tolist() == [b["initial"], 4096, a["initial"]] and power.tolist() == [0] * 3
    assert d.set_rc(-1, good) == 0 and lib.cmhip_automix_reset(d.h, -1) == 0 and lib.cmhip_automix_reset(d.h, 1) == 0
    for s in range(3):
        assert d.set_group_rc(s, -1) == 0


def test_refusals_of_an_object(cm, automixer):
    check_object_refusals(cm, automixer)
    assert automixer.run_rc(0x10000, 128, 64, 0x20000, 128) == cm.ERROR_INVAL      # a dry object launches nothing
    assert b"no device" in cm.lib.cmhip_last_error()
    automixer.sync()
    assert automixer.hip_stream() == 0


# ---------------------------------------------------------------------------
# the two lane-per-stream kernels' walk, emulated

class Emulation:
    """S streams as the host mirror and k_automix.hip hold them: the mirror's positions, parameters and groups; per run
    the records, the table of sums per window of the run, the windows' P, the groups' sums and the nodes; per stream the
    carried sums, P, the two nodes and the pending one.  bug: a mistake made on purpose --
        "gsum"   the groups' sums are not cleared between runs
        "early"  pending is applied a window early: the nodes move on behind the share and not in front of it
        "carry"  the carried partial window is forgotten"""

    def __init__(self, cm, streams, channels, w, max_frames, bug=None):
        self.cm, self.S, self.C, self.w, self.W, self.bug = cm, streams, channels, w, 1 << w, bug
        self.nw = max_frames // self.W + 2
        self.pos = [0] * streams
        self.par = [AM.params() for _ in range(streams)]
        self.group = [-1] * streams
        self.table = np.zeros((streams, self.nw, channels), dtype=np.int64)
        self.gsum = [[0] * self.nw for _ in range(streams)]
        self.st = [dict(psum=np.zeros(channels, dtype=np.int64), power=0, a_lo=0, a_hi=0, pending=0) for _ in range(streams)]

    # the mirror (csrc/automix_plan.h)
    def set(self, stream, p):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.par[s] = dict(p)

    def _reset_group(self, g):
        for s in range(self.S):
            if self.group[s] == g:
                self.pos[s] = 0

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            if self.group[s] < 0:
                self.pos[s] = 0
            else:
                self._reset_group(self.group[s])

    def set_group(self, s, g):
        if self.group[s] >= 0:
            self._reset_group(self.group[s])
        self.group[s] = g
        self.reset(s)

    def state(self):
        out = []
        for s in range(self.S):
            if self.group[s] < 0:
                out.append((4096, 0, 4096))
            elif self.pos[s] == 0:
                out.append((self.par[s]["initial"], 0, self.par[s]["initial"]))
            else:
                out.append((self.st[s]["a_hi"], self.st[s]["power"], self.st[s]["pending"]))
        return tuple(list(v) for v in zip(*out))

    def run(self, xs):
        Cn, w, W = self.C, self.w, self.W
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, Cn) for x in xs]
        counts = [x.shape[0] for x in xs]
        if max(counts) == 0:
            return [x.astype(np.int16) for x in xs]
        for g in set(self.group) - {-1}:                                 # what cmhip_automix_run refuses
            assert len({counts[s] for s in range(self.S) if self.group[s] == g}) == 1
        runs = [self.cm.agc_run(self.pos[s], counts[s], w) for s in range(self.S)]
        assert all(r.nwin <= self.nw for r in runs)
        if self.bug != "gsum":
            self.gsum = [[0] * self.nw for _ in range(self.S)]
        power = [[None] * self.nw for _ in range(self.S)]
        nodes = [[None] * (self.nw + 1) for _ in range(self.S)]
        # energy: a stream in no group has count 0 in the energy pass's records
        for s in range(self.S):
            if self.group[s] >= 0:
                for i in range(runs[s].nwin):
                    lo = max(0, (runs[s].first + i) * W - self.pos[s])
                    hi = min(counts[s], (runs[s].first + i + 1) * W - self.pos[s])
                    self.table[s, i] += (xs[s][lo:hi] ** 2).sum(axis=0)
        # level
        for s in range(self.S):
            r, st = runs[s], self.st[s]
            if counts[s] == 0 or self.group[s] < 0:
                continue
            cp = self.cm.AutomixParams(**self.par[s])
            P = 0 if self.pos[s] == 0 else st["power"]
            carried = (self.pos[s] & (W - 1)) != 0
            for i in range(r.nwin):
                sums = self.table[s, i] + (st["psum"] if i == 0 and carried and self.bug != "carry" else 0)
                self.table[s, i] = 0
                if i < r.complete:
                    P = self.cm.automix_power(P, int(sums.max()) >> w, cp)
                    power[s][i] = P
                    self.gsum[self.group[s]][i] += P
                else:
                    st["psum"] = sums.copy()
            st["power"] = P
        assert not self.table.any()
        # share
        for s in range(self.S):
            r, st, p = runs[s], self.st[s], self.par[s]
            if counts[s] == 0:
                continue
            if self.group[s] < 0:
                for i in range(r.nwin + 1):
                    nodes[s][i] = 4096
                continue
            if self.pos[s] == 0:
                st["a_lo"] = st["a_hi"] = st["pending"] = p["initial"]
            carried = (self.pos[s] & (W - 1)) != 0
            for i in range(r.nwin):
                early = self.bug == "early" and i < r.complete
                if early:
                    st["pending"] = self.cm.automix_share(power[s][i], self.gsum[self.group[s]][i], p["floor"], st["pending"])
                if (i > 0 or not carried) and r.first + i >= 1:
                    st["a_lo"], st["a_hi"] = st["a_hi"], st["pending"]
                nodes[s][i], nodes[s][i + 1] = st["a_lo"], st["a_hi"]
                if i < r.complete and not early:
                    st["pending"] = self.cm.automix_share(power[s][i], self.gsum[self.group[s]][i], p["floor"], st["pending"])
        # apply: frame f of the run lies in window (j0 + f) >> w of the run
        ys = []
        for s in range(self.S):
            f = np.arange(counts[s], dtype=np.int64)
            at = (self.pos[s] & (W - 1)) + f
            win, j = at >> w, at & (W - 1)
            a0 = np.array([nodes[s][i] for i in win], dtype=np.int64)
            a1 = np.array([nodes[s][i + 1] for i in win], dtype=np.int64)
            g = a0 + (((a1 - a0) * j) >> w)
            ys.append(((xs[s] * g[:, None] + 2048) >> 12).astype(np.int16))
            self.pos[s] += counts[s]
        return ys


def emulate_case(cm, channels, w, bug=None):
    """-> True when the emulation equals the model over the GPU test's case: outputs and state after every run"""
    signals, cuts = AM.case(channels, w)
    d = AM.case_desk(channels, w)
    e = Emulation(cm, AM.CASE_STREAMS, channels, w, 5 * (1 << w) + 3, bug)
    for s in range(AM.CASE_STREAMS):
        e.set(s, AM.palette(s))
        if AM.CASE_GROUPS[s] >= 0:
            e.set_group(s, AM.CASE_GROUPS[s])
    at = [0] * AM.CASE_STREAMS
    same = True
    for k, counts in enumerate(cuts):
        xs = [signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)]
        at = [a + n for a, n in zip(at, counts)]
        got, want = e.run(xs), d.run(xs)
        same = same and all(np.array_equal(a, b) for a, b in zip(got, want)) and e.state() == d.state()
        if k == 3:                                                       # a reset and a change of group on the way
            for o in (e, d):
                o.reset(3)
                o.set_group(2, 6)
                o.set_group(2, 0)
            same = same and e.state() == d.state()
    return same


@pytest.mark.parametrize("channels,w", AM.CASE_SHAPES)
def test_emulation_equals_the_model(cm, channels, w):
    assert emulate_case(cm, channels, w)


@pytest.mark.parametrize("bug", ["gsum", "early", "carry"])
@pytest.mark.parametrize("channels,w", [(1, 6), (3, 6), (2, 8)])
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
    exe, r = _build_plan_test(tmp_path, "automix_plan_test", [])              # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "automix plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "automix_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "automix plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_automix_desc_t d; cmhip_automix_params_t p; cmhip_automix_law_desc_t l; uint32_t g, v;\n"
           "uint64_t c; long grp;\n"
           "d.device = 0; d.streams = d.channels = 1; d.window_log2 = 6; d.max_frames = 1; d.hip_stream = 0;\n"
           "p.weight = p.floor = p.attack = p.release = p.initial = 1;\n"
           "l.rate = l.window_log2 = l.weight_db = l.floor_db = l.initial_db = l.attack_ms = l.release_ms = 0;\n"
           "return (cmhip_automix_new(0) != 0) + cmhip_automix_set(0, -1, &p) + cmhip_automix_get(0, 0, &p)"
           " + cmhip_automix_set_group(0, 0, -1) + cmhip_automix_get_group(0, 0, &grp)"
           " + cmhip_automix_run(0, 0, 0, 0, 0, 0, 0) + cmhip_automix_reset(0, -1) + cmhip_automix_state(0, &g, &c, &v)"
           " + cmhip_automix_sync(0) + (cmhip_automix_hip_stream(0) != 0) + cmhip_automix_check(6, &p)"
           " + cmhip_automix_design(&l, &p) + (cmhip_automix_free(0), 0) + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "free", "set", "get", "set_group", "get_group", "run", "reset", "state", "sync", "hip_stream",
                 "check", "design"):
        assert hasattr(cm.lib, "cmhip_automix_" + name) and "cmhip_automix_" + name in cm.SIGNATURES, name
    for name in ("automix_new_dry", "automix_power", "automix_share", "automix_run_events"):
        assert hasattr(cm.lib, "cmhip_test_" + name), name
    assert C.sizeof(cm.AutomixParams) == 10 and C.sizeof(cm.AutomixLawDesc) == 56
    assert C.sizeof(cm.AutomixDesc) == C.sizeof(cm.AgcDesc)


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_automix.s: it holds the eight kernels by name, and the resource usage beside it shows
    that none of them keeps a register in scratch memory"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_automix.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 8, names
    for stem, n in (("k_automix_energy_fast", 2), ("k_automix_energy_any", 1), ("k_automix_level", 1),
                    ("k_automix_share", 1), ("k_automix_apply_fast", 2), ("k_automix_apply_any", 1)):
        assert sum(stem in name for name in names) == n, (stem, names)
    usage = open(os.path.join(PKG, "build", "k_automix.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 8 and not [n for n in scratch if scratch[n]], scratch
    # the groups' sums take 64-bit integer adds
    assert "global_atomic_add_x2" in text
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*=.*\bk_automix\.hip\b.*\bcmhip_automix\.hip\b", mk, flags=re.M) and "build/k_automix.s" in mk
