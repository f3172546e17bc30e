"""CPU: the filter stage's host side (cmhip_iir_check, cmhip_iir_design, cmhip_iir_response_db, the refusals, the
mirror, csrc/iir_plan.h), an emulation of k_iir.hip's two decompositions -- the tile staging with its ragged vectors,
the skewed pipeline of (row, section) lanes with its drain, the row loop -- against the model of tests/test_gpu_iir.py,
and two properties of the model itself: a low cut's state decays to exactly zero, and the output stays within a
measured distance of a float64 recurrence on the same coefficients.  No GPU is used: where a test needs an object it
takes the test hook's object without a device (cmhip_test_iir_new_dry): the mirror and every check are the real ones."""
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
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "iir_plan_test.cpp")
ONE = 1 << 26


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_iir", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_iir")             # the model and the cases of the GPU tests


# ---------------------------------------------------------------------------
# the specification as code

def test_section_and_output_equal_the_model(cm):
    """csrc/iir_plan.h's section and output step, frame by frame, against the model on one row"""
    for k in range(12):
        sec = TG.palette(cm, k)
        x = TG.noise(k, 300, 1)
        m = TG.Model(1, 1, 1)
        m.set(0, 0, sec)
        want = m.run([x])[0][:, 0]
        st, clips, overs = [0] * 5, 0, 0
        for f in range(300):
            v, over = cm.iir_section_step(sec, int(x[f, 0]) << 12, st)
            y, clip = cm.iir_output(v)
            assert y == want[f], (k, f)
            clips += clip
            overs += over
        assert (clips, overs) == (int(m.clips[0]), int(m.overs[0]))
        assert st == m.st[0, 0, 0].tolist()
    for v in (-2 ** 31 + 1, 2 ** 31 - 1, -2049, -2048, -2047, 2047, 2048, 32767 * 4096 + 2047, 32767 * 4096 + 2048,
              -32768 * 4096 - 2048, -32768 * 4096 - 2049):
        r = (v + 2048) >> 12
        assert cm.iir_output(v) == (min(max(r, -32768), 32767), int(not -32768 <= r <= 32767)), v


def test_the_model_takes_every_branch(cm):
    """the model alone, on the GPU tests' inputs, takes every branch: both sides of both clamps, negative and
    positive sums with and without a remainder"""
    signals, secs, cuts = TG.model_case(cm, 33, 2, 2, 202, runs=4)
    m = TG.Model(33, 2, 2)
    for s in range(33):
        for k in range(2):
            m.set(s, k, secs(s, k))
    at = [0] * 33
    for counts in cuts:
        m.run([signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)])
        at = [a + n for a, n in zip(at, counts)]
    assert all(m.trace[b] > 0 for b in TG.BRANCHES), m.trace
    assert (m.overs == 0).any() and (m.overs > 0).any() and (m.clips > 0).any()


def test_unity_is_the_identity_and_no_frames_change_nothing(cm):
    x = np.random.default_rng(3).integers(-32768, 32768, size=(500, 3)).astype(np.int16)
    m = TG.Model(1, 3, 4)
    assert np.array_equal(m.run([x])[0], x) and m.clips[0] == 0 and m.overs[0] == 0 and not m.st[..., 4].any()
    before = m.st.copy()
    m.run([x[:0]])
    assert np.array_equal(before, m.st)


# ---------------------------------------------------------------------------
# design, check, response

def design_model(kind, rate, f0, q, gain_db):
    """the header's formulas in Python's own libm -> (the five integers, the smallest distance of a product from a
    half before it is rounded)"""
    w0 = 2.0 * math.pi * f0 / rate
    cs, sn = math.cos(w0), math.sin(w0)
    alpha = sn / (2.0 * q)
    A = math.pow(10.0, gain_db / 40.0)
    sq = 2.0 * math.sqrt(A) * alpha
    K = math.tan(w0 / 2.0)
    b, a = {
        "BYPASS": ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
        "HIGHPASS": (((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)),
        "LOWPASS": (((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)),
        "LOWSHELF": ((A * ((A + 1.0) - (A - 1.0) * cs + sq), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs),
                      A * ((A + 1.0) - (A - 1.0) * cs - sq)),
                     ((A + 1.0) + (A - 1.0) * cs + sq, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - sq)),
        "HIGHSHELF": ((A * ((A + 1.0) + (A - 1.0) * cs + sq), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs),
                       A * ((A + 1.0) + (A - 1.0) * cs - sq)),
                      ((A + 1.0) - (A - 1.0) * cs + sq, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - sq)),
        "PEAK": ((1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)),
        "NOTCH": ((1.0, -2.0 * cs, 1.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)),
        "HIGHPASS1": ((1.0, -1.0, 0.0), (1.0 + K, K - 1.0, 0.0)),
        "LOWPASS1": ((K, K, 0.0), (1.0 + K, K - 1.0, 0.0)),
    }[kind]
    raw = [c / a[0] * float(ONE) for c in (b[0], b[1], b[2], a[1], a[2])]
    margin = min(abs(v - math.floor(v) - 0.5) for v in raw)
    n = [int(np.rint(v)) for v in raw]
    if kind == "HIGHPASS":
        n[1] = -(n[0] + n[2])
    if kind == "HIGHPASS1":
        n[1] = -n[0]
    return tuple(n), margin


DESIGNS = [(kind, rate, f0, q, g) for kind in ("BYPASS", "HIGHPASS", "LOWPASS", "LOWSHELF", "HIGHSHELF", "PEAK", "NOTCH",
                                               "HIGHPASS1", "LOWPASS1")
           for rate, f0, q, g in ((48000.0, 40.0, 0.7071, 6.0), (44100.0, 1000.0, 2.0, -12.0), (8000.0, 3400.0, 0.5, 4.0),
                                  (192000.0, 10.0, 0.7071, -3.0), (48000.0, 3183.1, 1.0, 3.0))]


def test_design_equals_the_formulas(cm):
    for kind, rate, f0, q, g in DESIGNS:
        want, margin = design_model(kind, rate, f0, q, g)
        assert margin > 1e-6 or kind in ("BYPASS", "HIGHPASS1"), (kind, rate, f0, margin)     # no product so near a half
        got = cm.iir_design(cm.IIR_KINDS.index(kind), rate, f0, q, g)
        assert got.as_tuple() == want, (kind, rate, f0, q, g)
        assert cm.iir_check(got) == 0
        if kind.startswith("HIGHPASS"):            # the zero on z = 1 exactly: the DC gain is 0, not a small number
            assert got.b0 + got.b1 + got.b2 == 0
            assert cm.iir_response_db([got], rate, 0.0) == -math.inf
    assert cm.iir_design(cm.IIR_BYPASS, 48000.0, 1.0).as_tuple() == TG.UNITY
    hp1 = cm.iir_design(cm.IIR_HIGHPASS1, 48000.0, 20.0)
    assert hp1.b2 == 0 and hp1.a2 == 0 and hp1.b1 == -hp1.b0 and hp1.a1 < 0


def test_design_refusals(cm):
    lib = cm.lib
    out = cm.IirSection(7, 7, 7, 7, 7)
    good = (cm.IIR_HIGHPASS, 48000.0, 40.0, 0.7, 0.0)
    assert lib.cmhip_iir_design(None, C.byref(out)) == cm.ERROR_FAULT
    assert lib.cmhip_iir_design(C.byref(cm.IirDesignDesc(*good)), None) == cm.ERROR_FAULT
    for i in range(1, 5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            d = list(good)
            d[i] = bad
            assert lib.cmhip_iir_design(C.byref(cm.IirDesignDesc(*d)), C.byref(out)) == cm.ERROR_INVAL, (i, bad)
    for i, bad in ((0, -1), (0, 9), (1, 0.0), (1, -48000.0), (2, 0.0), (2, -5.0), (2, 24000.0), (2, 30000.0), (3, 0.0),
                   (3, -1.0)):
        d = list(good)
        d[i] = bad
        assert lib.cmhip_iir_design(C.byref(cm.IirDesignDesc(*d)), C.byref(out)) == cm.ERROR_INVAL, (i, bad)
        assert lib.cmhip_last_error()
    # a result the check refuses: a shelf of +40 dB has b0 above 4
    assert lib.cmhip_iir_design(C.byref(cm.IirDesignDesc(cm.IIR_HIGHSHELF, 48000.0, 1000.0, 0.7, 40.0)),
                                C.byref(out)) == cm.ERROR_INVAL
    assert out.as_tuple() == (7, 7, 7, 7, 7)                          # no refused call wrote anything


def test_check_on_the_triangles_edges(cm):
    big = 1 << 28
    ok = [(ONE, 0, 0, 0, 0), (big, -big, big, 0, 0), (0, 0, 0, 0, 0), (1, 2, 3, 0, ONE - 1), (1, 2, 3, 0, -(ONE - 1)),
          (0, 0, 0, 2 * ONE - 2, ONE - 1), (0, 0, 0, -(2 * ONE - 2), ONE - 1), (0, 0, 0, ONE - 1, 0), (0, 0, 0, 0, -(ONE - 1)),
          (0, 0, 0, 1, -(ONE - 2)), (0, 0, 0, -1, -(ONE - 2))]
    bad = [(big + 1, 0, 0, 0, 0), (0, -big - 1, 0, 0, 0), (0, 0, big + 1, 0, 0), (0, 0, 0, 0, ONE), (0, 0, 0, 0, -ONE),
           (0, 0, 0, 2 * ONE - 1, ONE - 1), (0, 0, 0, -(2 * ONE - 1), ONE - 1), (0, 0, 0, ONE, 0), (0, 0, 0, -ONE, 0),
           (0, 0, 0, 1, -(ONE - 1)), (0, 0, 0, -1, -(ONE - 1)), (0, 0, 0, 2 ** 31 - 1, 0), (0, 0, 0, 0, -2 ** 31),
           (-2 ** 31, 0, 0, 0, 0)]
    for sec in ok:
        assert cm.iir_check(cm.IirSection(*sec)) == 0, sec
    for sec in bad:
        assert cm.iir_check(cm.IirSection(*sec)) == cm.ERROR_INVAL, sec
    assert cm.lib.cmhip_iir_check(None) == cm.ERROR_FAULT


def test_response_equals_numpy_on_the_integers(cm):
    secs = [cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0), cm.iir_design(cm.IIR_PEAK, 48000.0, 1000.0, 2.0, 6.0),
            cm.iir_design(cm.IIR_LOWPASS1, 48000.0, 3183.1)]
    for f in (1.0, 20.0, 40.0, 1000.0, 3183.1, 12000.0, 23999.0):
        z = np.exp(-2j * np.pi * f / 48000.0)
        h = 1.0
        for n in range(1, 4):
            s = secs[n - 1]
            h *= (s.b0 + s.b1 * z + s.b2 * z * z) / (ONE + s.a1 * z + s.a2 * z * z)
            assert abs(cm.iir_response_db(secs[:n], 48000.0, f) - 20.0 * np.log10(abs(h))) < 1e-9, (f, n)
    assert abs(cm.iir_response_db(secs[:1], 48000.0, 40.0) + 3.0103) < 0.01          # the corner of a Butterworth
    assert abs(cm.iir_response_db(secs[1:2], 48000.0, 1000.0) - 6.0) < 1e-4
    assert abs(cm.iir_response_db(secs[2:], 48000.0, 3183.1) + 3.0103) < 0.01
    assert cm.iir_response_db([cm.iir_section()], 48000.0, 123.0) == 0.0
    assert math.isnan(cm.lib.cmhip_iir_response_db(None, 1, 48000.0, 1.0))
    assert math.isnan(cm.iir_response_db(secs, 0.0, 1.0))


# ---------------------------------------------------------------------------
# refusals

def test_null_arguments_and_creation_refusals(cm):
    lib = cm.lib
    sec = cm.iir_section()
    assert lib.cmhip_iir_new(None) is None and lib.cmhip_test_iir_new_dry(None) is None
    assert lib.cmhip_iir_set(None, -1, 0, C.byref(sec)) == cm.ERROR_FAULT
    assert lib.cmhip_iir_get(None, 0, 0, C.byref(sec)) == cm.ERROR_FAULT
    assert lib.cmhip_iir_run(None, None, 0, 0, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_iir_reset(None, -1) == cm.ERROR_FAULT
    assert lib.cmhip_iir_state(None, None, None, 0) == cm.ERROR_FAULT
    assert lib.cmhip_iir_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_iir_hip_stream(None) is None
    lib.cmhip_iir_free(None)
    # descriptors that are refused before any device is touched
    for kw in (dict(streams=0), dict(channels=0), dict(channels=17), dict(max_frames=0), dict(sections=0),
               dict(sections=9), dict(max_frames=2 ** 31), dict(max_frames=2 ** 30, channels=2),
               dict(max_frames=2 ** 27, channels=16), dict(max_frames=2 ** 63)):
        f = dict(device=0, streams=2, channels=1, sections=2, max_frames=64, hip_stream=None)
        f.update(kw)
        assert lib.cmhip_iir_new(C.byref(cm.IirDesc(**f))) is None, kw
        assert lib.cmhip_last_error()
        assert lib.cmhip_test_iir_new_dry(C.byref(cm.IirDesc(**f))) is None, kw


@pytest.fixture
def filt(cm):
    """an object for the refusals that need one: the test hook's, with the host mirror and every check and no device
    behind it (tests/test_gpu_iir.py runs the same checks on a real one)"""
    d = cm.test_iir_without_device(3, 2, 2, 64)
    yield d
    d.close()


def check_object_refusals(cm, d):
    """every refusal of an object, and that each leaves the mirror as it was (d: cm.Filter(3, 2, 2, 64))"""
    lib = cm.lib
    assert [d.get(s, k).as_tuple() for s in range(3) for k in range(2)] == [TG.UNITY] * 6
    clips, overs = d.state()
    assert clips.tolist() == [0] * 3 and overs.tolist() == [0] * 3
    assert lib.cmhip_iir_state(d.h, None, None, 1) == 0                  # either may be NULL
    a, b = TG.palette(cm, 0), TG.palette(cm, 6)
    assert d.set_rc(1, 0, cm.IirSection(*a)) == 0
    assert [d.get(s, 0).as_tuple() for s in range(3)] == [TG.UNITY, a, TG.UNITY]
    assert d.set_rc(-1, 1, cm.IirSection(*b)) == 0
    assert [d.get(s, 1).as_tuple() for s in range(3)] == [b] * 3
    before = [d.get(s, k).as_tuple() for s in range(3) for k in range(2)]
    good = cm.iir_section()
    assert d.set_rc(3, 0, good) == cm.ERROR_INVAL and d.set_rc(-2, 0, good) == cm.ERROR_INVAL
    assert d.set_rc(0, 2, good) == cm.ERROR_INVAL and d.set_rc(-1, 2, good) == cm.ERROR_INVAL
    assert lib.cmhip_iir_set(d.h, 0, 0, None) == cm.ERROR_FAULT
    for sec in ((ONE, 0, 0, 0, ONE), (ONE, 0, 0, ONE, 0), ((1 << 28) + 1, 0, 0, 0, 0), (0, 0, 0, 1, -(ONE - 1))):
        assert cm.iir_check(cm.IirSection(*sec)) == cm.ERROR_INVAL
        for stream in (0, -1):
            assert d.set_rc(stream, 1, cm.IirSection(*sec)) == cm.ERROR_INVAL, sec
    v = cm.IirSection(9, 9, 9, 9, 9)
    assert lib.cmhip_iir_get(d.h, 3, 0, C.byref(v)) == cm.ERROR_INVAL and v.b0 == 9
    assert lib.cmhip_iir_get(d.h, 0, 2, C.byref(v)) == cm.ERROR_INVAL and v.a2 == 9
    assert lib.cmhip_iir_get(d.h, 0, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_iir_reset(d.h, 3) == cm.ERROR_INVAL and lib.cmhip_iir_reset(d.h, -2) == cm.ERROR_INVAL
    assert [d.get(s, k).as_tuple() for s in range(3) for k in range(2)] == before
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
    assert [d.get(s, k).as_tuple() for s in range(3) for k in range(2)] == before
    clips, overs = d.state()
    assert clips.tolist() == [0] * 3 and overs.tolist() == [0] * 3 and not d.rows().any()
    for k in range(2):
        assert d.set_rc(-1, k, good) == 0
    assert lib.cmhip_iir_reset(d.h, -1) == 0 and lib.cmhip_iir_reset(d.h, 1) == 0


def test_refusals_of_an_object(cm, filt):
    check_object_refusals(cm, filt)
    assert filt.run_rc(0x10000, 128, 64, 0x20000, 128) == cm.ERROR_INVAL           # a dry object launches nothing
    assert b"no device" in cm.lib.cmhip_last_error()
    filt.sync()
    assert filt.hip_stream() == 0


# ---------------------------------------------------------------------------
# the plan

def test_plan(cm):
    for ch in range(1, 17):
        for n in range(1, 9):
            p = cm.plan_iir(70, ch, n, 1000)
            fast = 1 if ch <= 2 else 0
            np_ = (1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8) if fast else 1
            assert (p.err, p.fast, p.np, p.block, p.tile) == (0, fast, np_, 64, 64)
            assert p.spw == 64 // (ch * np_) and p.spw >= 1 and p.spw * ch * np_ <= 64
            assert p.grid == -(-70 // p.spw) and p.tiles == -(-1000 // p.tile)
            pitch = p.tile * ch + 2 * ((ch + 1) // 2)        # the streams' tiles in LDS, a bank and more apart
            assert p.lds_bytes == p.spw * pitch * 2 <= 8192 + 256 and (p.tile * ch) % 8 == 0
    p = cm.plan_iir(3, 2, 2, 0)
    assert (p.err, p.grid, p.spw) == (0, 0, 16)
    for bad in ((0, 2, 2), (3, 0, 2), (3, 17, 2), (3, 2, 0), (3, 2, 9)):
        p = cm.plan_iir(*bad, 8)
        assert (p.err, p.grid, p.spw) == (0, 0, 0), bad


def test_tile_vectors(cm):
    """a tile's vectors cover the stream's samples once, whole while they lie below the count"""
    for ch in (1, 2, 3, 5, 16):
        nv = 64 * ch // 8
        for count in (0, 1, 2, 7, 8, 9, 63, 64, 65, 129):
            seen = []
            for t in range(4):
                for q in range(nv):
                    off, n = cm.iir_tile_vec(count, ch, t, q)
                    assert off == (t * nv + q) * 8 and n == min(max(count * ch - off, 0), 8)
                    seen += list(range(off, off + n))
            assert seen == list(range(count * ch)), (ch, count)


# ---------------------------------------------------------------------------
# the kernels' decompositions, emulated

class Emulation:
    """the streams as a launch treats them: workgroups of spw streams in any order, tiles through an LDS image moved
    in 16-byte vectors with ragged ends sample by sample, and between the moves either the skewed pipeline of (row,
    section) lanes (fast) or the row loop (any), on the library's own section and output functions.  bug: a mistake
    made on purpose -- 'drain' (a tile takes f steps, not f + NP - 1), 'ragged' (a cut vector is dropped), 'skew'
    (a lane reads its neighbour's result of the same step, not of the step before)"""

    def __init__(self, cm, streams, channels, sections, seed, bug=None):
        self.cm, self.S, self.C, self.N = cm, streams, channels, sections
        self.coef = [[TG.UNITY] * sections for _ in range(streams)]
        self.st = [[[[0] * 5 for _ in range(sections)] for _ in range(channels)] for _ in range(streams)]
        self.clips, self.overs = [0] * streams, [0] * streams
        self.rng = np.random.default_rng(seed)
        self.bug = bug

    def set(self, stream, section, sec):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.coef[s][section] = tuple(sec)

    def reset(self, stream):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.st[s] = [[[0] * 5 for _ in range(self.N)] for _ in range(self.C)]

    def rows(self):
        return np.array(self.st, dtype=np.int64).reshape(self.S * self.C, self.N, 5).astype(np.int32)

    def move(self, lds, slots, counts, s0, plan, t, out):
        Cn, nv, pitch = self.C, plan.tile * self.C // 8, plan.lds_bytes // 2 // plan.spw
        for i in self.rng.permutation(plan.spw * nv):
            j, q = divmod(int(i), nv)
            s = s0 + j
            if s >= self.S:
                continue
            off, n = self.cm.iir_tile_vec(counts[s], Cn, t, q)
            assert n == 0 or off + n <= counts[s] * Cn and n <= 8
            if n < 8 and self.bug == "ragged":
                continue
            if out:
                assert (slots[s][off:off + n] == TG.SENTINEL).all()          # no sample twice
                slots[s][off:off + n] = lds[j * pitch + q * 8:j * pitch + q * 8 + n]
            else:
                lds[j * pitch + q * 8:j * pitch + q * 8 + n] = slots[s][off:off + n]

    def run(self, xs):
        cm, Cn, N = self.cm, self.C, self.N
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, Cn) for x in xs]
        counts = [x.shape[0] for x in xs]
        plan = cm.plan_iir(self.S, Cn, N, max(counts))
        B, NP = plan.tile, plan.np
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
                steps = min(B, most - t * B) + (0 if self.bug == "drain" else NP - 1)
                for i in range(steps):
                    seen = dict(vprev)                                       # what the cross-lane move reads
                    for s in mine:
                        length = min(max(counts[s] - t * B, 0), B)
                        j = s - s0
                        for c in range(Cn):
                            at = j * (plan.lds_bytes // 2 // plan.spw) + c
                            if not plan.fast:                                # a lane is a row
                                if i < length:
                                    u = int(lds[at + i * Cn]) << 12
                                    for k in range(N):
                                        u, over = cm.iir_section_step(self.coef[s][k], u, self.st[s][c][k])
                                        self.overs[s] += over
                                    y, clip = cm.iir_output(u)
                                    self.clips[s] += clip
                                    lds[at + i * Cn] = y
                                continue
                            for k in (range(NP) if self.bug == "skew" else reversed(range(NP))):
                                f = i - k
                                if not 0 <= f < length:
                                    continue
                                src = vprev if self.bug == "skew" else seen
                                u = int(lds[at + f * Cn]) << 12 if k == 0 else src[(s, c, k - 1)]
                                if k < N:
                                    v, over = cm.iir_section_step(self.coef[s][k], u, self.st[s][c][k])
                                    self.overs[s] += over
                                else:
                                    v = u                                    # a padded lane: the identity
                                vprev[(s, c, k)] = v
                                if k == NP - 1:
                                    y, clip = cm.iir_output(v)
                                    self.clips[s] += clip
                                    lds[at + f * Cn] = y
                self.move(lds, outs, counts, s0, plan, t, True)
        res = []
        for s, c in enumerate(counts):
            assert (outs[s][c * Cn:] == TG.SENTINEL).all()                   # nothing past the count
            res.append(outs[s][:c * Cn].reshape(-1, Cn))
        return res


def emulate_case(cm, streams, channels, sections, seed, bug=None):
    """-> True when the emulation equals the model over a case of ragged runs with a set and a reset in the middle:
    outputs, counters and state after every run"""
    B = cm.plan_iir(1, channels, sections, 1).tile
    lengths = [B + 1, 0, 1, 2 * B + 1, 9, B - 1, 8, B, 7, 2]
    cuts = [TG.rotate(lengths, k, streams) for k in range(4)]
    m, e = TG.Model(streams, channels, sections), Emulation(cm, streams, channels, sections, seed, bug)
    for s in range(streams):
        for k in range(sections):
            for o in (m, e):
                o.set(s, k, TG.palette(cm, s + 5 * k + seed))
    same = True
    for r, counts in enumerate(cuts):
        if r == 2:
            for o in (m, e):
                o.set(-1, 0, TG.palette(cm, 3))
                o.reset(1 % streams)
        xs = [TG.noise(seed + 10 * r + s, n, channels) for s, n in enumerate(counts)]
        got, want = e.run(xs), m.run(xs)
        same = same and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
        same = same and e.clips == m.clips.tolist() and e.overs == m.overs.tolist() and np.array_equal(e.rows(), m.rows())
    return same


@pytest.mark.parametrize("channels,sections", [(1, 1), (1, 3), (2, 2), (2, 8), (1, 5), (3, 2), (5, 1), (16, 3)])
def test_emulation_equals_the_model(cm, channels, sections):
    assert emulate_case(cm, 3 if channels > 2 or sections > 4 else 5, channels, sections, 1)


@pytest.mark.parametrize("bug,channels,sections", [("drain", 1, 2), ("drain", 2, 8), ("ragged", 1, 1), ("ragged", 3, 2),
                                                   ("skew", 2, 3), ("skew", 1, 4)])
def test_the_cases_notice_mistakes(cm, bug, channels, sections):
    """a mistake made on purpose in the emulation is caught by the same cases"""
    assert not emulate_case(cm, 3, channels, sections, 1, bug=bug)


# ---------------------------------------------------------------------------
# two properties of the model

# the high-passes of the design palette, both orders
LOW_CUTS = [(kind, rate, f0) for rate, f0 in ((48000.0, 5.0), (48000.0, 20.0), (48000.0, 80.0), (192000.0, 10.0),
                                              (8000.0, 300.0)) for kind in ("HIGHPASS", "HIGHPASS1")]
# what test_distance_from_float64 measured (LSB of the output), the largest over LOW_CUTS; its bound is this plus the
# half LSB by which the reference's own last bit and the final rounding can each move a tie
MEASURED_DISTANCE = 0.672


def low_cut_model(cm):
    m = TG.Model(len(LOW_CUTS), 1, 1)
    for s, (kind, rate, f0) in enumerate(LOW_CUTS):
        m.set(s, 0, cm.iir_design(cm.IIR_KINDS.index(kind), rate, f0).as_tuple())
    return m


def row_step(sec, x, st):
    """one frame of one row through one section and the output step, in Python's own integers (st: u1, u2, v1, v2, e)"""
    b0, b1, b2, a1, a2 = sec
    u = x << 12
    acc = b0 * u + b1 * st[0] + b2 * st[1] - a1 * st[2] - a2 * st[3] + st[4]
    v = min(max(acc >> 26, -TG.V_MAX), TG.V_MAX)
    st[:] = [u, st[0], v, st[2], acc & (ONE - 1)]
    return min(max((v + 2048) >> 12, -32768), 32767)


def test_row_step_is_the_model(cm):
    for k in range(12):
        sec, x = TG.palette(cm, k), TG.noise(40 + k, 200, 1)
        m = TG.Model(1, 1, 1)
        m.set(0, 0, sec)
        st = [0] * 5
        assert [row_step(sec, int(v), st) for v in x[:, 0]] == m.run([x])[0][:, 0].tolist() and st == m.st[0, 0, 0].tolist()


def test_a_low_cut_decays_to_exactly_zero(cm, capsys):
    """a constant input, then silence: the output reaches exactly 0 and the histories their rest -- u1 = u2 = the
    input, v1 = v2 = 0 -- and stay there; the remainder e rests wherever below 2^26 it has come to, where it can move
    nothing: acc = e.  The frame counts are measured, not fixed."""
    lines = []
    for kind, rate, f0 in LOW_CUTS:
        sec = cm.iir_design(cm.IIR_KINDS.index(kind), rate, f0).as_tuple()
        st, reached = [0] * 5, []
        for level in (12345, 0):
            quiet = n = 0
            while quiet < 3:                             # three frames: u1, u2 have taken the level, v1, v2 are 0
                y = row_step(sec, level, st)
                n += 1
                quiet = quiet + 1 if y == 0 and st[2] == 0 else 0
                assert n < 2000000, (kind, rate, f0, level)
            assert st[:4] == [level << 12, level << 12, 0, 0] and 0 <= st[4] < ONE
            rest = list(st)
            for _ in range(2000):                        # ... and stays there
                assert row_step(sec, level, st) == 0 and st == rest
            reached.append(n - 3)
        lines.append("  %-9s %4.0f Hz at %6.0f: at rest %6d frames into a constant, %6d into silence"
                     % (kind, f0, rate, reached[0], reached[1]))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_distance_from_float64(cm, capsys):
    """the output against a float64 Direct Form I on the same integer coefficients, over the low cuts, on a sine plus
    DC plus noise: the largest distance stays within the measured one plus 0.5 LSB"""
    S, F = len(LOW_CUTS), 6000
    rng = np.random.default_rng(8)
    n = np.arange(F)
    x = (9000.0 * np.sin(2.0 * np.pi * n * 0.0123) + 5000.0 + rng.integers(-3000, 3001, size=F)).astype(np.int16)
    m = low_cut_model(cm)
    got = m.run([x[:, None]] * S)
    worst = []
    for s in range(S):
        b0, b1, b2, a1, a2 = (float(v) / ONE for v in m.coef[s, 0])
        u1 = u2 = y1 = y2 = 0.0
        ref = np.zeros(F)
        for f in range(F):
            u = float(x[f])
            y = b0 * u + b1 * u1 + b2 * u2 - a1 * y1 - a2 * y2
            u2, u1, y2, y1 = u1, u, y1, y
            ref[f] = y
        worst.append(float(np.abs(got[s][:, 0] - ref).max()))
    with capsys.disabled():
        print("\n  distance from float64, LSB:", " ".join("%.3f" % w for w in worst))
    assert max(worst) <= MEASURED_DISTANCE + 0.5, worst


# ---------------------------------------------------------------------------
# the stand-alone plan program

def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "iir_plan_test", [])                   # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "iir plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "iir_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "60"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "iir plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the header and the assembly

def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_iir_desc_t d; cmhip_iir_section_t c; cmhip_iir_design_desc_t g; uint64_t a, b;\n"
           "d.device = 0; d.streams = d.channels = d.sections = 1; d.max_frames = 1; d.hip_stream = 0;\n"
           "c.b0 = CMHIP_IIR_ONE; c.b1 = c.b2 = c.a1 = c.a2 = 0;\n"
           "g.kind = CMHIP_IIR_HIGHPASS1; g.rate = 48000; g.f0 = 20; g.q = 1; g.gain_db = 0;\n"
           "return (cmhip_iir_new(0) != 0) + cmhip_iir_set(0, -1, 0, &c) + cmhip_iir_get(0, 0, 0, &c)"
           " + cmhip_iir_run(0, 0, 0, 0, 0, 0, 0) + cmhip_iir_reset(0, -1) + cmhip_iir_state(0, &a, &b, 0)"
           " + cmhip_iir_sync(0) + (cmhip_iir_hip_stream(0) != 0) + cmhip_iir_check(&c) + cmhip_iir_design(&g, &c)"
           " + (cmhip_iir_response_db(&c, 1, 48000, 1) > 0) + (cmhip_iir_free(0), 0) + (int)sizeof(d)"
           " + CMHIP_IIR_BYPASS + CMHIP_IIR_LOWPASS + CMHIP_IIR_LOWSHELF + CMHIP_IIR_HIGHSHELF + CMHIP_IIR_PEAK"
           " + CMHIP_IIR_NOTCH + CMHIP_IIR_HIGHPASS + CMHIP_IIR_LOWPASS1;}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "free", "set", "get", "run", "reset", "state", "sync", "hip_stream", "check", "design",
                 "response_db"):
        assert hasattr(cm.lib, "cmhip_iir_" + name) and "cmhip_iir_" + name in cm.SIGNATURES, name
    for name in ("plan_iir", "iir_tile_vec", "iir_section", "iir_output", "iir_new_dry", "iir_rows"):
        assert hasattr(cm.lib, "cmhip_test_" + name), name
    assert C.sizeof(cm.IirSection) == 20 and C.sizeof(cm.IirDesignDesc) == 40 and cm.IIR_ONE == ONE


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_iir.s: it holds the nine kernels by name, and the resource usage beside it shows that
    none of them keeps a register in scratch memory"""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_iir.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 9, names
    assert sum("k_iir_fast" in n for n in names) == 8 and sum("k_iir_any" in n for n in names) == 1, names
    usage = open(os.path.join(PKG, "build", "k_iir.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 9 and not [n for n in scratch if scratch[n]], scratch
    # the products are 64-bit multiply-adds of 32-bit factors, the PCM moves in 16-byte vectors, and the sections'
    # hand-over is a DPP row shift, not a trip through LDS
    assert "v_mad_i64_i32" in text and "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "row_shr:1" in text
