"""GPU: what the opt-in meters of a batch have in common -- the switch, the window lifecycle, the reset's bounds -- held
side by side for true peak, correlation, the spectrum and the watch (and loudness where a clause applies to a meter
without windows), and the group's six results calls on a full group against one that is not full.

The per-meter files pin each meter's numbers; this file pins that the meters AGREE on the contract around them.  Where a
value is checked it comes from the numpy model of the meter's own file (test_gpu_truepeak.Model, test_gpu_corr.sums,
spec_model.Model, watch_model.Watch) or from equality between two groups fed the same sources, never from a second
call of the device code alone.

Shapes: 3 stereo streams, one ragged run of [F, 0, 1] frames with F one tile of the meter's stereo kernel (2048 frames)
plus 5; for the spectrum the smallest FFT (256, hop 128) and F = 389, two blocks and 5 frames.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_corr as corr_tests
import test_gpu_spec as spec_tests
import test_gpu_truepeak as tp_tests
import test_gpu_watch as watch_tests
from watch_model import Watch

pytestmark = pytest.mark.gpu

S, CH = 3, 2
SENTINEL = 0x5a


class Meter:
    def __init__(self, name, switch, result_type, frames):
        self.name, self.switch, self.result_type, self.F = name, switch, result_type, frames

    def Result(self, cm):
        return getattr(cm, self.result_type)

    def set(self, b, on):
        return getattr(b, "set_" + self.switch)(on)

    def get(self, b):
        return getattr(b, "get_" + self.switch)()

    def prepare(self, b):
        """what the meter wants settled while it is off"""
        if self.name == "spec":
            assert b.spec_configure(8) == 0

    def result(self, cm, b, s, out):
        return getattr(cm.lib, "cmhip_batch_%s_result" % self.name)(b.h, s, C.byref(out))

    def results(self, cm, b, out, rc):
        return getattr(cm.lib, "cmhip_batch_%s_results" % self.name)(b.h, out, rc)

    def reset(self, cm, b, s):
        return getattr(cm.lib, "cmhip_batch_%s_reset" % self.name)(b.h, s)

    def check(self, cm, r, y, what):
        """r against the meter's model of one window over the transformed samples y, from a fresh state"""
        frames = len(y) // CH
        if self.name == "tp":
            m = tp_tests.Model(CH)
            m.run(y)
            peaks, n = m.take()
            tp_tests._check_result(r, peaks, n, CH, what)
        elif self.name == "corr":
            corr_tests._check(r, corr_tests.sums(y, CH), frames, CH, what=what)
        elif self.name == "spec":
            m = spec_tests.model(cm, 8)
            spec_tests._check(r, m, y, CH, frames, 0, m.count(frames), what=what)
        elif self.name == "watch":
            w = Watch(CH)
            w.feed(y)
            watch_tests._check(r, w.result(), what)
        else:
            raise AssertionError(self.name)


WINDOWED = [Meter("tp", "true_peak", "TruePeakResult", 2053), Meter("corr", "correlation", "CorrResult", 2053),
            Meter("spec", "spectrum", "SpecResult", 389), Meter("watch", "watch", "WatchResult", 2053)]
ALL = WINDOWED + [Meter("loud", "loudness", "LoudnessResult", 2053)]
ids = lambda m: m.name                               # noqa: E731


def _sentinels(T, n):
    out = (T * n)()
    C.memset(out, SENTINEL, C.sizeof(out))
    rc = (C.c_int * n)(*([-12345] * n))
    return out, rc


def _noise(seed, frames, div=1):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32768, 32768, size=frames * CH, dtype=np.int64) // div).astype(np.int16)


def _biquad(cm):
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    return coef


def _ragged_run(b, m, seed, div=1):
    """one run of [F, 0, 1] frames with 32767 behind every count -> the streams' frames"""
    counts = [m.F, 0, 1]
    xs = []
    for s, n in enumerate(counts):
        x = np.full(m.F * CH, 32767, dtype=np.int16)
        x[:n * CH] = _noise(seed + s, n, div)
        b.upload(s, x)
        xs.append(x[:n * CH].copy())
    b.run(m.F, counts)
    return xs


# ---------------------------------------------------------------------------
# (a) off


@pytest.mark.parametrize("m", ALL, ids=ids)
def test_off_refuses_every_read(gpu, m):
    cm = gpu
    b = cm.Batch(S, CH, m.F, flags=cm.VU)
    T = m.Result(cm)
    out, rc = _sentinels(T, S)
    before = bytes(out)
    for state in ("never on", "turned off"):
        assert m.get(b) == 0, state
        assert m.result(cm, b, 0, out[0]) == cm.ERROR_INVAL, state
        assert m.results(cm, b, out, rc) == cm.ERROR_INVAL, state
        assert m.reset(cm, b, -1) == cm.ERROR_INVAL and m.reset(cm, b, 0) == cm.ERROR_INVAL, state
        assert bytes(out) == before and list(rc) == [-12345] * S, state
        if state == "never on":
            m.prepare(b)
            assert m.set(b, 1) == 0 and m.get(b) == 1
            assert m.set(b, 0) == 0
    b.close()


# ---------------------------------------------------------------------------
# (b) the switch


@pytest.mark.parametrize("m", ALL, ids=ids)
def test_on_twice_is_one_on_and_the_equaliser_excludes_the_meter(gpu, m):
    cm = gpu
    coef = _biquad(cm)
    b = cm.Batch(S, CH, m.F, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    m.prepare(b)
    assert b.set_eq(-1, coef) == 0
    assert m.set(b, 1) == cm.ERROR_INVAL and m.get(b) == 0           # sections: the meter stays off
    assert m.set(b, 0) == 0                                          # (off is always allowed)
    assert b.set_eq(-1, []) == 0
    assert m.set(b, 1) == 0 and m.get(b) == 1
    assert b.set_eq(-1, coef) == cm.ERROR_INVAL                      # the meter is on: no sections
    assert b.set_eq(-1, []) == 0                                     # (none stays allowed)
    # the second on leaves the open window alone
    x = _noise(7, m.F)
    for s in range(S):
        b.upload(s, x)
    b.run(m.F)
    assert m.set(b, 1) == 0 and m.get(b) == 1
    r = m.Result(cm)()
    assert m.result(cm, b, 1, r) == 0
    assert r.frames == m.F
    if m.name != "loud":
        m.check(cm, r, x, (m.name, "on twice"))
    b.close()


# ---------------------------------------------------------------------------
# (c), (d) a ragged run and what the reads leave behind


@pytest.mark.parametrize("m", WINDOWED, ids=ids)
def test_ragged_results(gpu, m):
    cm = gpu
    T = m.Result(cm)
    b = cm.Batch(S, CH, m.F, flags=cm.VU)
    m.prepare(b)
    assert m.set(b, 1) == 0
    # (d) before any run: a single result on an empty window leaves `out` alone
    one, _ = _sentinels(T, 1)
    before = bytes(one)
    for s in range(S):
        assert m.result(cm, b, s, one[0]) == cm.ERROR_INVAL and bytes(one) == before, s
    xs = _ragged_run(b, m, 100)
    assert m.result(cm, b, 1, one[0]) == cm.ERROR_INVAL and bytes(one) == before
    # (c)
    spectrum = m.name == "spec"
    out, rc = _sentinels(T, S)
    assert m.results(cm, b, out, rc) == 0
    assert list(rc) == [0, cm.ERROR_INVAL, cm.ERROR_INVAL if spectrum else 0]
    m.check(cm, out[0], xs[0], (m.name, "stream 0"))
    assert bytes(out[1]) == before
    if spectrum:
        assert bytes(out[2]) == before
    else:
        m.check(cm, out[2], xs[2], (m.name, "stream 2"))
    # right after: every window that closed is empty
    out2, rc2 = _sentinels(T, S)
    assert m.results(cm, b, out2, rc2) == 0
    assert list(rc2) == [cm.ERROR_INVAL] * S
    assert bytes(out2) == before * S
    assert m.result(cm, b, 0, one[0]) == cm.ERROR_INVAL and bytes(one) == before
    if spectrum:
        # stream 2 kept its frame: F - 1 more complete its two blocks, and the window accounts all F
        rest = _noise(200, m.F - 1)
        b.upload(2, rest)
        b.run(m.F - 1, [0, 0, m.F - 1])
        r = T()
        assert m.result(cm, b, 2, r) == 0
        m.check(cm, r, np.concatenate([xs[2], rest]), (m.name, "stream 2, its kept frame and the rest"))
        assert m.result(cm, b, 2, one[0]) == cm.ERROR_INVAL and bytes(one) == before
    b.close()


# ---------------------------------------------------------------------------
# (e) the reset's bounds


@pytest.mark.parametrize("m", ALL, ids=ids)
def test_reset_bounds(gpu, m):
    cm = gpu
    b = cm.Batch(S, CH, m.F, flags=cm.VU)
    m.prepare(b)
    assert m.set(b, 1) == 0
    assert m.reset(cm, b, -1) == 0
    assert m.reset(cm, b, S - 1) == 0
    assert m.reset(cm, b, S) == cm.ERROR_INVAL
    assert m.reset(cm, b, -2) == cm.ERROR_INVAL
    b.close()


# ---------------------------------------------------------------------------
# (f) off, then on


@pytest.mark.parametrize("m", WINDOWED, ids=ids)
def test_off_then_on_clears_a_window_that_held_frames(gpu, m):
    cm = gpu
    T = m.Result(cm)
    b = cm.Batch(S, CH, m.F, flags=cm.VU)
    m.prepare(b)
    assert m.set(b, 1) == 0
    _ragged_run(b, m, 300)                           # full scale
    assert m.set(b, 0) == 0 and m.set(b, 1) == 0
    out, rc = _sentinels(T, S)
    before = bytes(out)
    assert m.results(cm, b, out, rc) == 0
    assert list(rc) == [cm.ERROR_INVAL] * S and bytes(out) == before
    # a quarter of full scale into the fresh windows: a maximum or a sum left behind would show
    xs = _ragged_run(b, m, 400, div=4)
    r = T()
    assert m.result(cm, b, 0, r) == 0
    m.check(cm, r, xs[0], (m.name, "after off and on"))
    b.close()


# ---------------------------------------------------------------------------
# (g) the group's results calls: a full group and one that is not


GROUP_CALLS = [("vumeter_results", "VuResult", None), ("true_peaks", "TruePeakResult", "set_true_peak"),
               ("loudnesses", "LoudnessResult", "set_loudness"), ("correlations", "CorrResult", "set_correlation"),
               ("spectra", "SpecResult", "set_spectrum"), ("watches", "WatchResult", "set_watch")]


@pytest.mark.parametrize("call,result_type,switch", GROUP_CALLS, ids=[c[0] for c in GROUP_CALLS])
def test_group_results_full_and_not_full(gpu, call, result_type, switch):
    cm = gpu
    T = getattr(cm, result_type)
    N, block, room = 2, 256, 4
    sources = [_noise(500 + i, block).tobytes() for i in range(N)]
    got = {}
    for max_streams in (N, room):
        grp = cm.Group(CH, max_streams, block, queue_blocks=2)
        if switch == "set_spectrum":
            assert grp.spectrum_configure(8) == 0
        if switch:
            assert getattr(grp, switch)(1) == 0
        for i in range(N):
            h = cm.IoHandle.from_bytes(sources[i])
            assert grp.add_stream(h) == i
            h.unref()
        assert grp.pump() == N
        out, rc = _sentinels(T, room)
        assert getattr(cm.lib, "coolmic_group_" + call)(grp.ptr, out, rc) == 0
        got[max_streams] = (bytes(out), list(rc), [out[i].frames for i in range(N)])
        if switch:
            assert getattr(grp, switch)(0) == 0
        grp.unref()
    full, partial = got[N], got[room]
    size = C.sizeof(T)
    assert full[2] == [block] * N and partial[2] == [block] * N      # the one block each source held
    assert full[1][:N] == [0] * N and partial[1][:N] == [0] * N
    assert partial[0][:N * size] == full[0][:N * size]
    # neither call wrote past slot 1
    assert partial[0][N * size:] == bytes([SENTINEL]) * ((room - N) * size)
    assert partial[1][N:] == [-12345] * (room - N)
    assert full[0][N * size:] == partial[0][N * size:] and full[1][N:] == partial[1][N:]
