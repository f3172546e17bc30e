"""GPU: the phase-correlation / balance meter through the batch ABI, the group, the Python mirror and the C example.

Bar: bit-exact.  The window sums are integers and EQUAL the model's; every double is bit-equal to the host formula of
include/coolmic_hip.h evaluated here (math.sqrt, libm's log10 through ctypes).  The model is numpy int64 on the
transformed stream, orc.gain_apply(g, orc.chmap(map, raw, C), C) -- never another run of the device code.

Geometry the sizes below sit on: k_corr_fast gives one wave a tile of 2048 stereo frames (512 vectors of 4 frames) and
a lane the vectors lane, lane + 64, ... of it -- a lane's span is one vector, a row of 64 vectors is 256 frames; the
edges are therefore 4 frames (the vector), 256 (the row) and 2048 (the tile), not a 32-frame run per lane.
k_corr_any gives one workgroup 1024 frames.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
TILE, VEC, ROW, ANY_TILE = 2048, 4, 256, 1024

_libm = C.CDLL("libm.so.6")
_libm.log10.restype = C.c_double
_libm.log10.argtypes = [C.c_double]


def _bits(x):
    return struct.pack("<d", x)


def corr(ea, eb, x):
    if ea == 0 or eb == 0:
        return 0.0
    return min(1.0, max(-1.0, float(x) / math.sqrt(float(ea) * float(eb))))


def balance(ea, eb):
    if ea == 0 and eb == 0:
        return 0.0
    if eb == 0:
        return math.inf
    return 10.0 * _libm.log10(float(ea) / float(eb)) if ea else -math.inf


def sums(y, Cn, pairs=((0, 1),)):
    """the model: [(energy_a, energy_b, cross)] of transformed interleaved samples, in Python integers"""
    f = np.asarray(y, dtype=np.int64).reshape(-1, Cn)
    return [(int((f[:, a] * f[:, a]).sum()), int((f[:, b] * f[:, b]).sum()), int((f[:, a] * f[:, b]).sum()))
            for a, b in pairs]


def add(u, v):
    return [tuple(p + q for p, q in zip(s, t)) for s, t in zip(u, v)]


def _check(r, want, frames, Cn, pairs=((0, 1),), what="", rate=48000):
    assert (r.rate, r.channels, r.frames, r.pairs) == (rate, Cn, frames, len(pairs)), what
    got = [(r.energy_a[i], r.energy_b[i], r.cross[i]) for i in range(len(pairs))]
    print("corr", what, "got", got, "want", want)
    assert got == want, what
    for i, (a, b) in enumerate(pairs):
        assert (r.a[i], r.b[i]) == (a, b), what
        assert _bits(r.correlation[i]) == _bits(corr(*want[i])), (what, i)
        assert _bits(r.balance_db[i]) == _bits(balance(want[i][0], want[i][1])), (what, i)
    for i in range(len(pairs), 8):                   # entries at and beyond `pairs` are zero
        assert (r.a[i], r.b[i], r.energy_a[i], r.energy_b[i], r.cross[i]) == (0, 0, 0, 0, 0), what
        assert _bits(r.correlation[i]) == _bits(0.0) and _bits(r.balance_db[i]) == _bits(0.0), what


def _transform(orc, raw, Cn, g, cmap):
    x = np.asarray(raw, dtype=np.int16)
    if cmap is not None:
        x = orc.chmap(cmap, x, Cn)
    return orc.gain_apply(g, x, Cn)


def _set(orc, b, s, Cn, gains, cmap):
    """gain (None: disabled) and map (None: identity) of stream s (-1: all) -> the oracle's gain"""
    if gains is None:
        assert b.set_gain(s, 0, 0, None) == 0
        g = of.Gain()
    else:
        assert b.set_gain(s, Cn, 1000, gains) == 0
        rc, g = orc.gain(Cn, Cn, 1000, gains)
        assert rc == 0
    assert b.set_chmap(s, cmap) == 0
    return g


def _noise(rng, frames, Cn):
    return rng.integers(-32768, 32768, size=frames * Cn, dtype=np.int64).astype(np.int16)


def _stereo(cm, streams=1, max_frames=4103, flags=None):
    b = cm.Batch(streams, 2, max_frames, flags=cm.VU if flags is None else flags)
    assert b.get_correlation() == 0
    assert b.set_correlation(1) == 0
    assert b.get_correlation() == 1
    return b


def _one(b, stream=0):
    rc, r = b.corr_result(stream)
    assert rc == 0
    return r


# ---------------------------------------------------------------------------
# 1. the stereo kernel


@pytest.mark.parametrize("transform", ["identity", "general"])
def test_fast_kernel_edges(gpu, oracle, transform):
    """one stereo stream of 1 .. 4103 frames: a lone frame, the vector's edge (4 frames), 32 frames, the row's edge
    (256), the tile's (2048) and a ragged third tile"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(11)
    b = _stereo(cm)
    gains, cmap = (None, None) if transform == "identity" else ([750, 1250], [1, 0])
    g = _set(orc, b, 0, 2, gains, cmap)
    for frames in (1, 3, 4, 5, 31, 32, 33, ROW - 1, ROW, ROW + 1, 2047, 2048, 2049, 4103):
        b.upload(0, np.full(4103 * 2, 32767, dtype=np.int16))        # what lies behind the run's frames
        raw = _noise(rng, frames, 2)
        b.upload(0, raw)
        b.run(frames)
        _check(_one(b), sums(_transform(orc, raw, 2, g, cmap), 2), frames, 2, what=(transform, frames))
    b.close()


def test_extremes(gpu):
    cm = gpu
    n = 4103
    b = _stereo(cm)
    for (left, right), want in (((-32768, -32768), (n << 30, n << 30, n << 30)),
                                ((-32768, 32767), (n << 30, n * 32767 * 32767, -n * 32768 * 32767)),
                                ((32767, 0), (n * 32767 * 32767, 0, 0))):
        b.upload(0, np.tile(np.array([left, right], dtype=np.int16), n))
        b.run(n)
        r = _one(b)
        _check(r, [want], n, 2, what=(left, right))
    # (the last one: a silent leg)
    assert _bits(r.correlation[0]) == _bits(0.0) and r.balance_db[0] == math.inf
    b.upload(0, np.tile(np.array([-32768, -32768], dtype=np.int16), n))
    b.run(n)
    r = _one(b)
    assert _bits(r.correlation[0]) == _bits(1.0) and _bits(r.balance_db[0]) == _bits(0.0)
    b.upload(0, np.tile(np.array([-32768, 32767], dtype=np.int16), n))
    b.run(n)
    r = _one(b)
    assert r.cross[0] < 0 and -1.0 <= r.correlation[0] < -0.999
    b.close()


def test_planted_pattern(gpu):
    """all zeros but one frame (3, -5): on the first and last frame of a lane's span (a vector: lane 0's and lane 1's
    first, lane 63's first, lane 0's second and last), the last frame of tile 0, the first of tile 1, the first of the
    ragged tile and its last frame, one stream per position"""
    cm = gpu
    n = 4103
    places = [0, VEC - 1, VEC, 2 * VEC - 1, ROW - VEC, ROW - 1, ROW, ROW + VEC - 1, TILE - ROW, TILE - VEC, TILE - 1, TILE,
              TILE + VEC - 1, 2 * TILE - 1, 2 * TILE, n - VEC, n - 2, n - 1]
    b = _stereo(cm, streams=len(places))
    for s, at in enumerate(places):
        x = np.zeros(n * 2, dtype=np.int16)
        x[2 * at: 2 * at + 2] = (3, -5)
        b.upload(s, x)
    b.run(n)
    out, rc = b.corr_results()
    for s, at in enumerate(places):
        assert rc[s] == 0
        _check(out[s], [(9, 25, -15)], n, 2, what=("planted at", at))
        assert _bits(out[s].correlation[0]) == _bits(-1.0)
    b.close()


def test_ragged_runs(gpu, oracle):
    """seven streams with counts 0, 1, 4, 2047, 2048, 2049 and the maximum; 32767 behind every count"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(12)
    T = 4103
    counts = [0, 1, 4, TILE - 1, TILE, TILE + 1, T]
    b = _stereo(cm, streams=len(counts))
    g = _set(orc, b, -1, 2, [1900, 310], None)
    # a first run gives every stream a window, so that the stream with count 0 has one to keep
    first = [_noise(rng, 10, 2) for _ in counts]
    for s, x in enumerate(first):
        b.upload(s, x)
    b.run(10)
    raws = []
    for s, n in enumerate(counts):
        x = np.full(T * 2, 32767, dtype=np.int16)
        x[:n * 2] = _noise(rng, n, 2)
        b.upload(s, x)
        raws.append(x[:n * 2])
    b.run(T, counts)
    out, rc = b.corr_results()
    for s, n in enumerate(counts):
        want = add(sums(orc.gain_apply(g, first[s], 2), 2), sums(orc.gain_apply(g, raws[s], 2), 2))
        assert rc[s] == 0
        _check(out[s], want, 10 + n, 2, what=("ragged", n))
    b.close()


def test_cut_invariance(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(13)
    n = 4103
    x = _noise(rng, n, 2)
    b = _stereo(cm)
    g = _set(orc, b, 0, 2, [999, 1001], [1, 0])
    want = sums(_transform(orc, x, 2, g, [1, 0]), 2)
    b.upload(0, x)
    b.run(n)
    whole = _one(b)
    _check(whole, want, n, 2, what="one run")
    pos = 0
    for k in (1, TILE - 1, 2055):
        b.upload(0, x[2 * pos: 2 * (pos + k)])
        b.run(k)
        pos += k
    assert pos == n
    cut = _one(b)
    _check(cut, want, n, 2, what="three runs")
    assert bytes(whole) == bytes(cut)
    b.close()


# ---------------------------------------------------------------------------
# 2. windows


def test_windows(gpu):
    cm = gpu
    b = _stereo(cm, streams=3, max_frames=64)
    frame = {0: (3, -5), 1: (100, 7), 2: (-32768, 1)}
    want = {s: (l * l, r * r, l * r) for s, (l, r) in frame.items()}
    for s, lr in frame.items():
        b.upload(s, np.tile(np.array(lr, dtype=np.int16), 64))

    def scaled(s, k):
        return [tuple(k * v for v in want[s])]

    # an empty window: INVAL, `out` unchanged
    sentinel = cm.CorrResult()
    C.memset(C.byref(sentinel), 0x5a, C.sizeof(sentinel))
    before = bytes(sentinel)
    rc, _ = b.corr_result(1, out=sentinel)
    assert rc == cm.ERROR_INVAL and bytes(sentinel) == before
    assert cm.lib.cmhip_batch_corr_result(b.h, 3, C.byref(sentinel)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_corr_result(b.h, 0, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_corr_results(b.h, None, None) == cm.ERROR_FAULT
    # a result closes the window, the next one starts from zero
    b.run(10)
    b.run(7)
    _check(_one(b, 1), scaled(1, 17), 17, 2, what="window 1")
    rc, _ = b.corr_result(1, out=sentinel)
    assert rc == cm.ERROR_INVAL and bytes(sentinel) == before
    b.run(5)
    _check(_one(b, 1), scaled(1, 5), 5, 2, what="window 2")
    # _results: the per-stream rc, streams without a frame left alone; rc may be NULL
    b.run(4, [4, 0, 2])                              # streams 0 and 2 hold 10 + 7 + 5 + their share, stream 1 nothing
    out = (cm.CorrResult * 3)()
    C.memset(out, 0x5a, C.sizeof(out))
    out, rc = b.corr_results(out)
    assert rc == [0, cm.ERROR_INVAL, 0]
    _check(out[0], scaled(0, 26), 26, 2, what="results 0")
    assert bytes(out[1]) == before
    _check(out[2], scaled(2, 24), 24, 2, what="results 2")
    b.run(3)
    assert cm.lib.cmhip_batch_corr_results(b.h, out, None) == 0
    _check(out[1], scaled(1, 3), 3, 2, what="results without rc")
    # reset: one stream, all
    b.run(6)
    b.corr_reset(1)
    b.run(2)
    out, rc = b.corr_results()
    assert rc == [0, 0, 0]
    for s, k in ((0, 8), (1, 2), (2, 8)):
        _check(out[s], scaled(s, k), k, 2, what=("after reset(1)", s))
    b.run(6)
    b.corr_reset(-1)
    out, rc = b.corr_results()
    assert rc == [cm.ERROR_INVAL] * 3
    assert cm.lib.cmhip_batch_corr_reset(b.h, 3) == cm.ERROR_INVAL
    b.run(1)
    _check(_one(b, 2), scaled(2, 1), 1, 2, what="after reset(-1)")
    b.close()


# ---------------------------------------------------------------------------
# 3. the transform


def test_transform(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(14)
    n = 3001
    x = _noise(rng, n, 2)
    b = _stereo(cm, max_frames=n)

    def measure(gains, cmap):
        g = _set(orc, b, 0, 2, gains, cmap)
        b.upload(0, x)
        b.run(n)
        r = _one(b)
        y = _transform(orc, x, 2, g, cmap)
        _check(r, sums(y, 2), n, 2, what=(gains, cmap))
        return (r.energy_a[0], r.energy_b[0], r.cross[0]), y

    plain, _ = measure([1000, 1000], None)
    assert plain == sums(x, 2)[0]
    swapped, _ = measure([1000, 1000], [1, 0])       # a map that swaps the channels swaps the energies
    assert swapped == (plain[1], plain[0], plain[2])
    _, y = measure([3000, 65535], None)              # a gain that saturates: the sums follow the saturated samples
    assert (np.abs(y.astype(np.int64)) >= 32767).sum() > n // 2
    assert measure(None, None)[0] == plain           # gain disabled
    measure([1, 999], [0, 0])                        # both legs read channel 0, every gain below the scale
    b.close()


def test_in_place_pcm_batch(gpu, oracle):
    """the block kernel overwrites the slots the pass has read: queued ahead of it, the pass saw the input"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(15)
    S, n = 3, 4103
    b = _stereo(cm, streams=S, flags=cm.OUT_PCM | cm.VU | cm.INPLACE)
    g = _set(orc, b, -1, 2, [1700, 650], [1, 0])
    xs = [_noise(rng, n, 2) for _ in range(S)]
    for s in range(S):
        b.upload(s, xs[s])
    b.run(n)
    out, rc = b.corr_results()
    for s in range(S):
        y = _transform(orc, xs[s], 2, g, [1, 0])
        assert np.array_equal(b.download(s, n), y), s
        assert rc[s] == 0
        _check(out[s], sums(y, 2), n, 2, what=("in place", s))
    b.close()


# ---------------------------------------------------------------------------
# 4. every other case: k_corr_any

ANY_CASES = [(6, [(0, 1), (4, 5), (2, 3)]),
             (16, [(0, 1), (2, 3), (15, 14), (5, 9), (8, 0), (7, 13), (12, 11), (10, 6)]),
             (3, [(2, 0)]),
             (2, [(0, 1), (1, 0)])]


@pytest.mark.parametrize("Cn,pairs", ANY_CASES, ids=["6ch", "16ch", "3ch", "2ch-two-pairs"])
def test_any_kernel(gpu, oracle, Cn, pairs):
    """runs of 1, 1023, 1024, 1025 and 2051 frames (the workgroup's 1024 and its neighbours, a ragged third tile) with
    ragged counts, a map that is not the identity and gains of every kind, one window per run"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(100 + Cn)
    S, T = 5, 2051
    b = cm.Batch(S, Cn, T, flags=cm.VU)
    assert b.corr_set_pairs(pairs) == 0              # (allowed while correlation is off: no window exists)
    assert b.set_correlation(1) == 0
    params = []
    for s in range(S):
        gains = [None, [int(v) for v in rng.integers(500, 3000, Cn)], [int(v) for v in rng.integers(1, 1000, Cn)]][s % 3]
        cmap = [int(v) for v in rng.permutation(Cn)] if s != 2 else [int(v) for v in rng.integers(0, Cn, Cn)]
        params.append((_set(orc, b, s, Cn, gains, cmap), cmap))
    for frames in (1, ANY_TILE - 1, ANY_TILE, ANY_TILE + 1, T):
        counts = [frames, frames // 2, 0, 1, frames - 1]
        raws = []
        for s in range(S):
            x = np.full(T * Cn, 32767, dtype=np.int16)
            x[:counts[s] * Cn] = _noise(rng, counts[s], Cn)
            b.upload(s, x)
            raws.append(x[:counts[s] * Cn])
        b.run(frames, counts)
        out, rc = b.corr_results()
        for s in range(S):
            assert rc[s] == (0 if counts[s] else cm.ERROR_INVAL), (frames, s)
            if counts[s]:
                _check(out[s], sums(_transform(orc, raws[s], Cn, *params[s]), Cn, pairs), counts[s], Cn, pairs,
                       what=(Cn, frames, s))
    # uniform counts too, and two runs in one window
    xs = [_noise(rng, T, Cn) for _ in range(S)]
    for s in range(S):
        b.upload(s, xs[s])
    b.run(T)
    b.run(ANY_TILE + 1)
    out, rc = b.corr_results()
    for s in range(S):
        y = _transform(orc, xs[s], Cn, *params[s])
        _check(out[s], add(sums(y, Cn, pairs), sums(y[:(ANY_TILE + 1) * Cn], Cn, pairs)), T + ANY_TILE + 1, Cn, pairs,
               what=(Cn, "uniform", s))
    b.close()


def test_two_pairs_of_a_stereo_batch_mirror_each_other(gpu):
    cm = gpu
    b = cm.Batch(1, 2, 64, flags=cm.VU)
    assert b.corr_set_pairs([(1, 0)]) == 0           # the stereo kernel, the pair the other way round
    assert b.set_correlation(1) == 0
    b.upload(0, np.tile(np.array([3, -5], dtype=np.int16), 64))
    b.run(64)
    _check(_one(b), [(64 * 25, 64 * 9, -64 * 15)], 64, 2, [(1, 0)], what="(1, 0)")
    b.close()


# ---------------------------------------------------------------------------
# 5. refusals


def _pairs_arg(pairs):
    flat = [c for p in pairs for c in p]
    return (C.c_ubyte * max(len(flat), 2))(*flat)


def test_refusals(gpu):
    cm = gpu
    mono = cm.Batch(2, 1, 64, flags=cm.VU)
    assert mono.set_correlation(1) == cm.ERROR_INVAL and mono.get_correlation() == 0
    assert mono.set_correlation(0) == 0
    assert mono.corr_set_pairs([(0, 1)]) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_corr_results(mono.h, (cm.CorrResult * 2)(), None) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_corr_reset(mono.h, -1) == cm.ERROR_INVAL
    mono.close()
    assert cm.lib.cmhip_batch_set_correlation(None, 1) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_get_correlation(None) == cm.ERROR_FAULT

    b = cm.Batch(2, 6, 64, flags=cm.VU)
    assert b.corr_set_pairs([(0, 1), (4, 5), (2, 3)]) == 0
    for bad in ([], [(0, 1)] * 9, [(0, 1), (3, 3)], [(0, 6)], [(6, 0)], [(0, 1), (2, 255)]):
        assert cm.lib.cmhip_batch_corr_set_pairs(b.h, len(bad), _pairs_arg(bad)) == cm.ERROR_INVAL, bad
    assert cm.lib.cmhip_batch_corr_set_pairs(b.h, 1, None) == cm.ERROR_FAULT
    assert b.set_correlation(1) == 0
    x = np.tile(np.array([1, 2, 3, 4, 5, 6], dtype=np.int16), 64)
    b.upload(0, x)
    b.upload(1, x)
    assert b.corr_set_pairs([(0, 2)]) == 0           # on, every window empty: allowed
    assert b.corr_set_pairs([(0, 1), (4, 5), (2, 3)]) == 0
    b.run(8, [0, 8])
    assert b.corr_set_pairs([(0, 2)]) == cm.ERROR_BUSY               # stream 1 holds frames
    assert cm.lib.cmhip_batch_corr_set_pairs(b.h, 1, _pairs_arg([(3, 3)])) == cm.ERROR_INVAL
    three = [(0, 1), (4, 5), (2, 3)]
    _check(_one(b, 1), [(8, 32, 16), (200, 288, 240), (72, 128, 96)], 8, 6, three, what="the refused calls changed nothing")
    assert b.corr_set_pairs([(5, 0)]) == 0           # the result emptied the window
    b.run(8)
    # off and on again: empty windows, the pairs kept
    assert b.set_correlation(0) == 0 and b.get_correlation() == 0
    assert cm.lib.cmhip_batch_corr_result(b.h, 0, C.byref(cm.CorrResult())) == cm.ERROR_INVAL
    n0 = cm.lib.cmhip_debug_corr_count()
    b.run(8)                                         # (off: this run launches no pass)
    assert cm.lib.cmhip_debug_corr_count() == n0
    assert b.set_correlation(1) == 0
    out, rc = b.corr_results()
    assert rc == [cm.ERROR_INVAL] * 2
    b.run(4)
    assert cm.lib.cmhip_debug_corr_count() == n0 + 1
    _check(_one(b, 0), [(4 * 36, 4 * 1, 4 * 6)], 4, 6, [(5, 0)], what="pairs kept")
    b.close()


def test_correlation_and_equaliser_exclude_each_other(gpu):
    cm = gpu
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    e = cm.Batch(2, 2, 256, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    assert e.set_correlation(1) == 0
    assert e.set_eq(-1, coef) == cm.ERROR_INVAL      # sections while correlation is on
    assert e.set_eq(-1, []) == 0                     # (no sections stays allowed)
    assert e.set_correlation(0) == 0
    assert e.set_eq(-1, coef) == 0
    assert e.set_correlation(1) == cm.ERROR_INVAL and e.get_correlation() == 0
    assert e.set_eq(-1, []) == 0
    assert e.set_correlation(1) == 0
    e.upload(0, np.tile(np.array([3, -5], dtype=np.int16), 21))
    e.upload(1, np.zeros(42, dtype=np.int16))
    e.run(21)
    _check(_one(e, 0), [(21 * 9, 21 * 25, -21 * 15)], 21, 2, what="an EQ batch without sections")
    e.close()


# ---------------------------------------------------------------------------
# 6. beside the other meters


def test_beside_true_peak_and_loudness(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(16)
    S, T = 3, 5000                                   # (a 100 ms sub-block of loudness is 4800 frames)
    xs = [_noise(rng, T, 2) for _ in range(S)]
    counts = [T, 0, 2049]

    def run(tp, loud, co):
        b = cm.Batch(S, 2, T, flags=cm.OUT_PCM | cm.VU)
        g = _set(orc, b, -1, 2, [800, 1300], [1, 0])
        assert b.set_true_peak(tp) == 0 and b.set_loudness(loud) == 0 and b.set_correlation(co) == 0
        n0 = cm.lib.cmhip_debug_corr_count()
        for k, fps in enumerate((None, counts)):
            for s in range(S):
                b.upload(s, xs[s])
            b.run(T, fps)
            assert cm.lib.cmhip_debug_corr_count() == n0 + (k + 1 if co else 0)
        res = {}
        if tp:
            out, rc = b.tp_results()
            res["tp"] = [(rc[s], out[s].as_dict()) for s in range(S)]
        if loud:
            out, rc = b.loud_results()
            res["loud"] = [(rc[s], out[s].as_dict()) for s in range(S)]
        if co:
            out, rc = b.corr_results()
            res["corr"] = [(rc[s], bytes(out[s])) for s in range(S)]
            for s in range(S):
                y = _transform(orc, xs[s], 2, g, [1, 0])
                _check(out[s], add(sums(y, 2), sums(y[:counts[s] * 2], 2)), T + counts[s], 2, what=("beside", s))
        vu, rc = b.vu_results()
        res["vu"] = [(rc[s], vu[s].as_dict()) for s in range(S)]
        res["pcm"] = [b.download(s, T).tobytes() for s in range(S)]
        b.close()
        return res

    together = run(1, 1, 1)
    for alone in (run(1, 0, 0), run(0, 1, 0), run(0, 0, 1), run(0, 0, 0)):
        for key, val in alone.items():
            assert together[key] == val, key


# ---------------------------------------------------------------------------
# 7. a group


def _take(handle, nbytes):
    got = b""
    while len(got) < nbytes:
        n, data = handle.read(nbytes - len(got))
        assert n > 0
        got += data
    return np.frombuffer(got, dtype=np.int16)


def test_group(gpu, oracle):
    """two sine and two null sources, stereo.  A sine source is the 48-sample table of the "sine" driver (which is
    mono) served as L = the table, R = the table a quarter period on (slot 0) or L = R (slot 2); a null source is the
    "null" driver, and the model reads a twin of it on the host"""
    cm, orc = gpu, oracle
    Cn, block = 2, 1000
    grp = cm.Group(Cn, 6, block, queue_blocks=8)     # (not full: the engine has more streams than the group slots)
    assert grp.set_correlation(1) == 0
    assert cm.lib.coolmic_group_correlation(grp.ptr, 4, C.byref(cm.CorrResult())) == cm.ERROR_INVAL
    rc_s, table = orc.sine_table(48000)
    assert rc_s == 0 and len(table) == 48
    table = np.asarray(table, dtype=np.int16)
    drivers = ["sine", "null", "sine", "null"]
    setup = [([1000, 500], None), ([700, 700], None), ([2500, 900], [1, 0]), (None, None)]
    feeds, gs = [], []
    for i, drv in enumerate(drivers):
        if drv == "sine":
            frames = 8 * block
            x = np.empty((frames, 2), dtype=np.int16)
            x[:, 0] = np.tile(table, frames // 48 + 1)[:frames]
            x[:, 1] = np.tile(np.roll(table, -12 if i == 0 else 0), frames // 48 + 1)[:frames]
            h = cm.IoHandle.from_bytes(x.tobytes(), chunk=(0, 7, 1024, 0)[i])
            feeds.append({"raw": x.reshape(-1), "pos": 0})
            assert grp.add_stream(h) == i
            h.unref()
        else:
            dev = cm.Snddev(drv, 48000, Cn)
            h = dev.get_iohandle()
            assert grp.add_stream(h) == i
            h.unref(); dev.unref()
            twin = cm.Snddev(drv, 48000, Cn)
            feeds.append({"twin": twin, "handle": twin.get_iohandle()})
        gains, cmap = setup[i]
        if gains is None:
            assert grp.set_master_gain(i, 0, 0, None) == 0
            g = of.Gain()
        else:
            assert grp.set_master_gain(i, Cn, 1000, gains) == 0
            _, g = orc.gain(Cn, Cn, 1000, gains)
        assert grp.set_channel_map(i, cmap) == 0
        gs.append(g)
    N = len(drivers)
    assert grp.correlation_set_pairs([(1, 0)]) == 0 and grp.correlation_set_pairs([(0, 1)]) == 0
    assert grp.correlation_set_pairs([(0, 2)]) == cm.ERROR_INVAL
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    assert grp.set_eq(-1, coef) == cm.ERROR_INVAL    # the engine's INVAL, passed through

    def model(i, frames):
        f = feeds[i]
        if "raw" in f:
            raw = f["raw"][f["pos"] * Cn: (f["pos"] + frames) * Cn]
            f["pos"] += frames
        else:
            raw = _take(f["handle"], frames * Cn * 2)
        assert raw.size == frames * Cn
        return sums(_transform(orc, raw, Cn, gs[i], setup[i][1]), Cn)

    def vu_frames(k):
        """how many frames the pumps since the last call took from each source: the VU windows, closed at the same
        point, count them as well (a source may deliver less than a block; the table sources never do)"""
        vu, rc_vu = grp.vumeter_results()
        assert rc_vu == [0] * N
        n = [vu[i].frames for i in range(N)]
        assert all(0 < v <= k * block for v in n) and n[0] == n[2] == k * block
        return n

    # two pumps, then every window at once: the block in flight counts
    for _ in range(2):
        assert grp.pump() == N
    out, rc = grp.correlations()
    n = vu_frames(2)
    assert len(rc) == N and rc == [0] * N
    for i in range(N):
        _check(out[i], model(i, n[i]), n[i], Cn, what=("group", i))
    assert abs(out[0].correlation[0]) < 0.01 and out[0].balance_db[0] > 5.9       # quadrature, the left leg 6 dB up
    assert out[2].correlation[0] > 0.5                                            # L = R, one leg driven into saturation
    assert out[1].energy_a[0] == 0 and _bits(out[1].correlation[0]) == _bits(0.0)
    # empty windows: every rc INVAL, results left alone
    keep = bytes(out[2])
    out, rc = grp.correlations(out)
    assert rc == [cm.ERROR_INVAL] * N and bytes(out[2]) == keep
    # a single-slot call closes only that slot's window
    assert grp.pump() == N
    rc2, r2 = grp.correlation(2)
    assert rc2 == 0
    _check(r2, model(2, block), block, Cn, what="group, slot 2 alone")
    assert grp.correlation(2)[0] == cm.ERROR_INVAL
    assert grp.pump() == N
    out, rc = grp.correlations()
    n = vu_frames(2)
    assert rc == [0] * N
    for i in range(N):
        k = n[i] - block if i == 2 else n[i]
        _check(out[i], model(i, k), k, Cn, what=("group, after the single slot", i))
    # reset: one slot, all
    assert grp.pump() == N
    assert grp.correlation_reset(0) == 0
    assert grp.correlation_reset(4) == cm.ERROR_INVAL
    out, rc = grp.correlations()
    n = vu_frames(1)
    assert rc == [cm.ERROR_INVAL, 0, 0, 0]
    for i in range(N):
        want = model(i, n[i])
        if i:
            _check(out[i], want, n[i], Cn, what=("group, after reset(0)", i))
    assert grp.pump() == N
    assert grp.correlation_reset(-1) == 0
    assert grp.correlations()[1] == [cm.ERROR_INVAL] * N
    assert grp.set_correlation(0) == 0
    for f in feeds:
        if "twin" in f:
            f["handle"].unref(); f["twin"].unref()
    grp.unref()


# ---------------------------------------------------------------------------
# 8. the example


def test_batch_correlation_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_correlation"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_correlation.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert len(out) == 3
    assert out[0].startswith("L = R: ") and "correlation +1.000000" in out[0]
    assert out[1].startswith("L = -R: ") and "correlation -1.000000" in out[1]
    assert out[2].startswith("sine against its quarter period: ")
