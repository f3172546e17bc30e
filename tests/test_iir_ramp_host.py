"""CPU: the filter's coefficient ramps on the host side -- csrc/iir_ramp.h through its stand-alone program (plain and
under AddressSanitizer + UBSan), cmhip_iir_ramp / _ramp_state / _ramp_section and the mirror on an object without a
device (cmhip_test_iir_new_dry), an emulation of k_iirramp.hip's two decompositions -- lane = (row, section), skewed
frames, every lane's position from its own done, R and frame -- against the frame-by-frame model of
tests/test_gpu_iir_ramp.py, and on that model alone what a ramp is for: a move that clicks less than a step."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
RAMP_SRC = os.path.join(ROOT, "tests", "cpp", "iir_ramp_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_iir_ramp_host", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TR = _load("test_gpu_iir_ramp")        # the model, the numpy rule, the schedule of the GPU tests
TH = _load("test_iir_host")            # the emulation of the plain kernels
TG = TR.TG
ONE, BIG, P_ONE, RAMP_MAX = TR.ONE, TR.BIG, TR.P_ONE, TR.RAMP_MAX


# ---------------------------------------------------------------------------
# the stand-alone program

def _build(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        RAMP_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_ramp_program(tmp_path):
    exe, r = _build(tmp_path, "iir_ramp_test", [])                         # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "iir ramp ok:" in out.stdout, out.stdout + out.stderr


def test_ramp_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "iir_ramp_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "40"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "iir ramp ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the rule through the ABI

def pairs(cm):
    ends = [TR.ends(cm, k) for k in range(14)]
    return [(ends[i], ends[(i + j) % 14]) for i in range(14) for j in (1, 3, 5, 12)]


def test_ramp_section_equals_the_numpy_rule(cm):
    sweep = np.unique(np.concatenate([np.arange(0, 40), np.arange(0, P_ONE + 1, 97), np.arange(P_ONE - 40, P_ONE + 1),
                                      [16383, 16384, 16385]]))
    for c0, c1 in pairs(cm):
        want = TR.ramp_section(np.array(c0)[None], np.array(c1)[None], sweep)
        for p, w in zip(sweep.tolist(), want.tolist()):
            got = cm.iir_ramp_section(cm.IirSection(*c0), cm.IirSection(*c1), p)
            assert got.as_tuple() == tuple(w), (c0, c1, p)
            assert cm.iir_check(got) == 0
        assert cm.iir_ramp_section(cm.IirSection(*c0), cm.IirSection(*c1), 0).as_tuple() == tuple(c0)
        for p in (P_ONE, P_ONE + 1, 2 ** 32 - 1):
            assert cm.iir_ramp_section(cm.IirSection(*c0), cm.IirSection(*c1), p).as_tuple() == tuple(c1)
    # a whole low-cut sweep keeps its zero on z = 1
    lo, hi = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0), cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 160.0)
    first = cm.iir_design(cm.IIR_HIGHPASS1, 48000.0, 20.0)
    for a, b in ((lo, hi), (hi, first), (first, lo)):
        for p in range(0, P_ONE + 1, 61):
            c = cm.iir_ramp_section(a, b, p)
            assert c.b0 + c.b1 + c.b2 == 0 and cm.iir_response_db([c], 48000.0, 0.0) == -np.inf
    # NULL: nothing is written, nothing crashes; an end outside the range counts as the bound
    out = cm.IirSection(7, 7, 7, 7, 7)
    cm.lib.cmhip_iir_ramp_section(None, C.byref(lo), 5, C.byref(out))
    cm.lib.cmhip_iir_ramp_section(C.byref(lo), None, 5, C.byref(out))
    cm.lib.cmhip_iir_ramp_section(C.byref(lo), C.byref(hi), 5, None)
    assert out.as_tuple() == (7, 7, 7, 7, 7)
    wild = cm.IirSection(2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, 0)
    assert cm.iir_ramp_section(wild, wild, 12345).as_tuple() == (BIG, -BIG, BIG, 0, 0)


def test_position_is_the_mixers(cm):
    for R in (0, 1, 2, 3, 63, 64, 65, 480, 44100, RAMP_MAX - 1, RAMP_MAX):
        ns = sorted({0, 1, 2, R // 2, max(R, 2) - 2, max(R, 1) - 1, R, R + 1, R + 2})
        want = [cm.lib.cmhip_mix_ramp_position(n, R) for n in ns]
        assert TR.position(ns, R).tolist() == want, R
        if R >= 2:                              # the kernels' own clock: frame f of a run entered at `done`
            for done in (0, 1, R // 2, R - 1):
                for f in (0, 1, 63, 64, R - done - 1, R - done, R - done + 5):
                    _, p = cm.iir_ramp_at(TG.UNITY, TG.UNITY, done, R, f)
                    assert p == cm.lib.cmhip_mix_ramp_position(min(done + f + 1, R), R), (R, done, f)
    for done, R in ((0, 0), (5, 5), (9, 5), (0, 1)):      # at rest: the end, whatever the frame
        assert cm.iir_ramp_at(TG.palette(cm, 0), TG.palette(cm, 1), done, R, 17) == (TG.palette(cm, 1), P_ONE)


# ---------------------------------------------------------------------------
# the mirror on an object without a device

@pytest.fixture
def filt(cm):
    d = cm.test_iir_without_device(3, 2, 2, 64)
    yield d
    d.close()


def mirror_of(d):
    return [(d.get(s, k).as_tuple(), d.ramp_state(s, k)) for s in range(3) for k in range(2)]


def check_ramp_refusals(cm, d):
    """every refusal of cmhip_iir_ramp and cmhip_iir_ramp_state, and that each leaves the mirror as it was (d: a filter
    of 3 streams, 2 channels, 2 sections)"""
    lib = cm.lib
    a, b = TG.palette(cm, 0), TG.palette(cm, 6)
    d.set(-1, 0, cm.IirSection(*a))
    d.ramp(1, 1, cm.IirSection(*b), 100)                 # one section under way
    before = mirror_of(d)
    assert before[3] == (TG.UNITY, (0, 100)) and before[0] == (a, (0, 0))
    good = cm.IirSection(*TG.palette(cm, 3))
    assert lib.cmhip_iir_ramp(None, 0, 0, C.byref(good), 10) == cm.ERROR_FAULT
    assert lib.cmhip_iir_ramp(d.h, 0, 0, None, 10) == cm.ERROR_FAULT
    for stream, section, frames in ((3, 0, 10), (-2, 0, 10), (0, 2, 10), (-1, 2, 10), (0, 0, RAMP_MAX + 1), (-1, 1, 2 ** 32 - 1),
                                    (1, 1, RAMP_MAX + 1)):
        assert d.ramp_rc(stream, section, good, frames) == cm.ERROR_INVAL, (stream, section, frames)
        assert lib.cmhip_last_error()
    for sec in ((ONE, 0, 0, 0, ONE), (ONE, 0, 0, ONE, 0), (BIG + 1, 0, 0, 0, 0), (0, 0, 0, 1, -(ONE - 1))):
        for stream in (1, -1):
            for frames in (0, 1, 2, 100):
                assert d.ramp_rc(stream, 1, cm.IirSection(*sec), frames) == cm.ERROR_INVAL, (sec, frames)
    done, frames = C.c_uint32(77), C.c_uint32(77)
    assert lib.cmhip_iir_ramp_state(None, 0, 0, C.byref(done), C.byref(frames)) == cm.ERROR_FAULT
    assert lib.cmhip_iir_ramp_state(d.h, 3, 0, C.byref(done), C.byref(frames)) == cm.ERROR_INVAL
    assert lib.cmhip_iir_ramp_state(d.h, 0, 2, C.byref(done), C.byref(frames)) == cm.ERROR_INVAL
    assert (done.value, frames.value) == (77, 77)
    assert lib.cmhip_iir_ramp_state(d.h, 1, 1, None, None) == 0                    # either may be NULL
    assert lib.cmhip_iir_ramp_state(d.h, 1, 1, None, C.byref(frames)) == 0 and frames.value == 100
    assert lib.cmhip_iir_ramp_state(d.h, 1, 1, C.byref(done), None) == 0 and done.value == 0
    assert mirror_of(d) == before
    assert lib.cmhip_iir_reset(d.h, -1) == 0 and mirror_of(d) == before            # a reset leaves ramps alone
    assert d.ramp_rc(-1, 0, good, RAMP_MAX) == 0                                   # the longest ramp is allowed
    assert [d.ramp_state(s, 0) for s in range(3)] == [(0, RAMP_MAX)] * 3
    for k in range(2):
        d.set(-1, k, cm.iir_section())
    assert mirror_of(d) == [(TG.UNITY, (0, 0))] * 6


def test_refusals_change_nothing(cm, filt):
    check_ramp_refusals(cm, filt)


def test_get_and_ramp_state_through_a_ramp_and_a_retarget(cm, filt):
    """a dry object runs nothing, so its ramps stay at their first frame: get is c(p(0)) = the section in force when
    the ramp began, a retarget starts from there, a set ends the ramp"""
    d = filt
    a, b, c = (TG.palette(cm, k) for k in (0, 3, 8))
    assert mirror_of(d) == [(TG.UNITY, (0, 0))] * 6
    d.set(0, 0, cm.IirSection(*a))
    d.ramp(0, 0, cm.IirSection(*b), 480)
    assert d.get(0, 0).as_tuple() == a and d.ramp_state(0, 0) == (0, 480)
    d.ramp(0, 0, cm.IirSection(*c), 64)                  # a retarget: from the section in force
    assert d.get(0, 0).as_tuple() == a and d.ramp_state(0, 0) == (0, 64)
    d.ramp(-1, 1, cm.IirSection(*b), 2)                  # every stream
    assert [d.ramp_state(s, 1) for s in range(3)] == [(0, 2)] * 3 and d.get(2, 1).as_tuple() == TG.UNITY
    d.set(0, 0, cm.IirSection(*b))                       # a set ends the ramp with a step
    assert d.get(0, 0).as_tuple() == b and d.ramp_state(0, 0) == (0, 0)
    assert d.run_rc(0x10000, 128, 0, 0x20000, 128) == 0 and d.ramp_state(1, 1) == (0, 2)     # no frames: no advance
    assert d.run_rc(0x10000, 128, 64, 0x20000, 128) == cm.ERROR_INVAL                        # a dry object launches nothing
    assert d.ramp_state(1, 1) == (0, 2)


@pytest.mark.parametrize("frames", [0, 1])
def test_a_ramp_of_no_or_one_frame_is_a_set(cm, filt, frames):
    d, e = filt, cm.test_iir_without_device(3, 2, 2, 64)
    try:
        for stream, section, k in ((0, 0, 1), (-1, 1, 6), (2, 0, 9), (1, 1, 3)):
            sec = cm.IirSection(*TG.palette(cm, k))
            d.ramp(stream, section, sec, frames)
            e.set(stream, section, sec)
            assert mirror_of(d) == mirror_of(e)
        d.ramp(1, 0, cm.IirSection(*TG.palette(cm, 2)), 300)             # ... also on a section that ramps
        d.ramp(1, 0, cm.IirSection(*TG.palette(cm, 7)), frames)
        e.set(1, 0, cm.IirSection(*TG.palette(cm, 7)))
        assert mirror_of(d) == mirror_of(e) and d.ramp_state(1, 0) == (0, 0)
    finally:
        e.close()


def test_the_mirror_follows_the_model(cm):
    """the library's mirror arithmetic (the kernels' hook at frame f = done - 1 is c(p(done))) against the model's now()
    along a ramp with a retarget, step by step"""
    m = TR.RampModel(1, 1, 1)
    a, b, c = TG.palette(cm, 6), TG.palette(cm, 1), TG.palette(cm, 9)
    m.set(0, 0, a)
    m.ramp(0, 0, b, 130)
    x = np.zeros((1, 1), dtype=np.int16)
    for step in range(200):
        if step == 57:
            m.ramp(0, 0, c, 65)                          # from c(p(57)) of the first ramp
        done, R = m.ramp_state(0, 0)
        if done:
            got, p = cm.iir_ramp_at(tuple(int(v) for v in m.c0[0, 0]), tuple(int(v) for v in m.c1[0, 0]), 0, R, done - 1)
            assert got == m.now(0, 0) and p == int(TR.position(done, R))
        assert cm.iir_check(cm.IirSection(*m.now(0, 0))) == 0
        m.run([x])
    assert m.now(0, 0) == c and m.ramp_state(0, 0) == (0, 0) and m.trace["retarget"] == 1


# ---------------------------------------------------------------------------
# the ramp kernels' decompositions, emulated

class RampEmulation(TH.Emulation):
    """tests/test_iir_host.py's emulation of a launch with what k_iirramp.hip adds: a lane is (row, section) and takes
    its section for ITS frame -- step i minus its skew -- from its own ends, done and R through the library's hook; the
    host advances the ramps behind the run.  bug 'position': a lane takes the step's position, not its frame's"""

    def __init__(self, cm, streams, channels, sections, seed, bug=None):
        super().__init__(cm, streams, channels, sections, seed, bug if bug != "position" else None)
        self.wrong_position = bug == "position"
        self.ends = [[[TG.UNITY, TG.UNITY, 0, 0] for _ in range(sections)] for _ in range(streams)]

    def ramping(self, s, k):
        return self.ends[s][k][2] < self.ends[s][k][3]

    def now(self, s, k):
        c0, c1, done, R = self.ends[s][k]
        return self.cm.iir_ramp_section(self.cm.IirSection(*c0), self.cm.IirSection(*c1),
                                        self.cm.lib.cmhip_mix_ramp_position(done, R)).as_tuple() if done < R else c1

    def set(self, stream, section, sec):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.ends[s][section] = [tuple(sec), tuple(sec), 0, 0]

    def ramp(self, stream, section, sec, frames):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.ends[s][section] = [self.now(s, section), tuple(sec), 0, frames]

    def at(self, s, k, frame):
        c0, c1, done, R = self.ends[s][k]
        return self.cm.iir_ramp_at(c0, c1, done, R, frame)[0]

    def run(self, xs):
        cm, Cn, N = self.cm, self.C, self.N
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, Cn) for x in xs]
        counts = [x.shape[0] for x in xs]
        plan = cm.plan_iir(self.S, Cn, N, max(counts))
        B, NP = plan.tile, plan.np
        pitch = plan.lds_bytes // 2 // plan.spw
        ins = [np.concatenate([x.reshape(-1), np.full(16, TG.POISON, dtype=np.int64)]) for x in xs]
        outs = [np.full(c * Cn + 16, TG.SENTINEL, dtype=np.int64) for c in counts]
        for wg in self.rng.permutation(plan.grid):
            s0 = int(wg) * plan.spw
            mine = range(s0, min(s0 + plan.spw, self.S))
            most = max(counts[s] for s in mine)
            vprev = {}
            for t in range(-(-most // B)):
                lds = np.full(plan.lds_bytes // 2, TG.POISON, dtype=np.int64)
                self.move(lds, ins, counts, s0, plan, t, False)
                for i in range(min(B, most - t * B) + NP - 1):
                    seen = dict(vprev)                                       # what the cross-lane move reads
                    for s in mine:
                        length = min(max(counts[s] - t * B, 0), B)
                        for c in range(Cn):
                            at = (s - s0) * pitch + c
                            if not plan.fast:                                # a lane is a row
                                if i < length:
                                    u = int(lds[at + i * Cn]) << 12
                                    for k in range(N):
                                        u, over = cm.iir_section_step(self.at(s, k, t * B + i), u, self.st[s][c][k])
                                        self.overs[s] += over
                                    y, clip = cm.iir_output(u)
                                    self.clips[s] += clip
                                    lds[at + i * Cn] = y
                                continue
                            for k in reversed(range(NP)):
                                f = i - k
                                if not 0 <= f < length:
                                    continue
                                u = int(lds[at + f * Cn]) << 12 if k == 0 else seen[(s, c, k - 1)]
                                if k < N:
                                    sec = self.at(s, k, t * B + (i if self.wrong_position else f))
                                    v, over = cm.iir_section_step(sec, u, self.st[s][c][k])
                                    self.overs[s] += over
                                else:
                                    v = u                                    # a padded lane: the identity at rest
                                vprev[(s, c, k)] = v
                                if k == NP - 1:
                                    y, clip = cm.iir_output(v)
                                    self.clips[s] += clip
                                    lds[at + f * Cn] = y
                self.move(lds, outs, counts, s0, plan, t, True)
        for s, n in enumerate(counts):                                       # the host, behind the run
            for k in range(N):
                e = self.ends[s][k]
                if e[2] < e[3]:
                    e[2] = min(e[2] + n, e[3])
                    if e[2] == e[3]:
                        self.ends[s][k] = [e[1], e[1], 0, 0]
        res = []
        for s, c in enumerate(counts):
            assert (outs[s][c * Cn:] == TG.SENTINEL).all()                   # nothing past the count
            res.append(outs[s][:c * Cn].reshape(-1, Cn))
        return res


class Both:
    """the schedule of the GPU tests drives a rig; here the rig is the model and the emulation side by side"""

    def __init__(self, model, emulation):
        self.model, self.e, self.S, self.N = model, emulation, model.S, model.N

    def set(self, stream, section, sec):
        self.model.set(stream, section, sec)
        self.e.set(stream, section, sec)

    def ramp(self, stream, section, sec, frames):
        self.model.ramp(stream, section, sec, frames)
        self.e.ramp(stream, section, sec, frames)


def emulate_case(cm, streams, channels, sections, seed, bug=None, runs=4):
    B = cm.plan_iir(1, channels, sections, 1).tile
    lengths = [B + 1, 0, 1, 2 * B + 1, 9, B - 1, 8, B, 7, 2]
    both = Both(TR.RampModel(streams, channels, sections), RampEmulation(cm, streams, channels, sections, seed, bug))
    for s in range(streams):
        for k in range(sections):
            both.set(s, k, TG.palette(cm, s + 5 * k + seed))
    same = True
    for r in range(runs):
        counts = TG.rotate(lengths, r, streams)
        TR.schedule(cm, both, r, B)
        if r == 2:
            both.model.reset(1 % streams)
            both.e.reset(1 % streams)
        xs = [TG.noise(seed + 10 * r + s, n, channels) for s, n in enumerate(counts)]
        got, want = both.e.run(xs), both.model.run(xs)
        m, e = both.model, both.e
        same = same and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
        same = same and e.clips == m.clips.tolist() and e.overs == m.overs.tolist() and np.array_equal(e.rows(), m.rows())
        same = same and all(e.now(s, k) == m.now(s, k) and tuple(e.ends[s][k][2:]) == m.ramp_state(s, k)
                            for s in range(streams) for k in range(sections))
    t = both.model.trace
    assert t["in_ramp"] > 0 and t["past_end"] > 0 and t["at_rest"] > 0, t
    return same


@pytest.mark.parametrize("channels,sections", [(1, 1), (1, 3), (2, 2), (2, 8), (3, 2), (5, 1), (16, 3)])
def test_emulation_equals_the_model(cm, channels, sections):
    assert emulate_case(cm, 3 if channels > 2 or sections > 4 else 4, channels, sections, 1)


@pytest.mark.parametrize("bug,channels,sections", [("ragged", 3, 2), ("ragged", 1, 2), ("position", 2, 3), ("position", 1, 8)])
def test_the_cases_notice_mistakes(cm, bug, channels, sections):
    """a mistake made on purpose in the emulation is caught by the same cases"""
    assert not emulate_case(cm, 3, channels, sections, 1, bug=bug)


# ---------------------------------------------------------------------------
# what a ramp is for, on the model alone

def test_a_ramped_peak_filter_clicks_less_than_a_stepped_one(cm):
    """a 1 kHz sine at -12 dBFS through a PEAK at 1 kHz that is moved from 0 to -12 dB: the largest second difference
    of the output around the move is smaller with a ramp of 480 frames than with the step"""
    n = np.arange(4800)
    x = np.rint(32767.0 * 10.0 ** (-12.0 / 20.0) * np.sin(2.0 * np.pi * 1000.0 * n / 48000.0)).astype(np.int16)[:, None]
    flat = cm.iir_design(cm.IIR_PEAK, 48000.0, 1000.0, 1.0, 0.0).as_tuple()
    cut = cm.iir_design(cm.IIR_PEAK, 48000.0, 1000.0, 1.0, -12.0).as_tuple()
    worst = {}
    for frames in (1, 480):
        m = TR.RampModel(1, 1, 1)
        m.set(0, 0, flat)
        before = m.run([x[:2400]])[0][:, 0].astype(np.int64)
        m.ramp(0, 0, cut, frames)
        after = m.run([x[2400:]])[0][:, 0].astype(np.int64)
        y = np.concatenate([before, after])
        assert m.clips[0] == 0 and m.overs[0] == 0
        worst[frames] = int(np.abs(np.diff(y[2400 - 8:2400 + 960], n=2)).max())
        assert abs(int(np.abs(after[-480:]).max()) - 32767 * 10.0 ** (-24.0 / 20.0)) < 40      # both arrive at -24 dBFS
    assert worst[480] < worst[1], worst


# ---------------------------------------------------------------------------
# the header, the exports, the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_iir_section_t a, b, c; uint32_t done, frames;\n"
           "a.b0 = b.b0 = CMHIP_IIR_ONE; a.b1 = a.b2 = a.a1 = a.a2 = b.b1 = b.b2 = b.a1 = b.a2 = 0;\n"
           "cmhip_iir_ramp_section(&a, &b, 16384, &c);\n"
           "return cmhip_iir_ramp(0, -1, 0, &c, CMHIP_IIR_RAMP_MAX) + cmhip_iir_ramp_state(0, 0, 0, &done, &frames);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("ramp", "ramp_state", "ramp_section"):
        assert hasattr(cm.lib, "cmhip_iir_" + name) and "cmhip_iir_" + name in cm.SIGNATURES, name
    assert hasattr(cm.lib, "cmhip_test_iir_ramp_at") and cm.IIR_RAMP_MAX == RAMP_MAX
    assert all(hasattr(cm.Filter, n) for n in ("ramp", "ramp_rc", "ramp_state")) and callable(cm.iir_ramp_section)


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_iirramp.s: the nine ramp kernels by name, none of which keeps a register in scratch
    memory; the interpolation is 64-bit multiply-adds of 32-bit factors, the hand-over a DPP row shift, the any form's
    ends come back from LDS in 16-byte vectors"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_iirramp.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 9, names
    assert sum("k_iirr_fast" in n for n in names) == 8 and sum("k_iirr_any" in n for n in names) == 1, names
    usage = open(os.path.join(PKG, "build", "k_iirramp.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 9 and not [n for n in scratch if scratch[n]], scratch
    assert "v_mad_i64_i32" in text and "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "row_shr:1" in text and "ds_read_b128" in text
