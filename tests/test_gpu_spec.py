"""GPU: the spectrum meter through the batch ABI, the group, the Python mirror and the C example.

Bar: bit-exact.  The band sums are integers and EQUAL the model's (tests/spec_model.py: the specification in numpy
int64 with the library's tables, on the transformed stream orc.gain_apply(g, orc.chmap(map, raw, C), C) -- never another
run of the device code, nor the library's own reference); every double is bit-equal to the host formula of
include/coolmic_hip.h evaluated here with libm's log10 through ctypes.

Geometry the sizes below sit on: a block is N = 2^n frames, the hop N / 2; n = 8 unless stated, so N = 256, H = 128 and
a stream of 4103 frames completes 31 blocks and leaves 7 frames behind the last hop.  A workgroup takes one block; its
samples come from the stream's state (the N - 1 frames before the run) and from the run.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle_ffi as of
from spec_model import Model, octaves

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
N8, H8 = 256, 128

_libm = C.CDLL("libm.so.6")
_libm.log10.restype = C.c_double
_libm.log10.argtypes = [C.c_double]


def _bits(x):
    return struct.pack("<d", x)


def db(power, blocks):
    return 10.0 * _libm.log10(float(power) / (float(blocks) * 1649267441664.0)) if blocks else 0.0


_MODELS = {}


def model(cm, n=8):
    if n not in _MODELS:
        _MODELS[n] = Model(cm, n)
    return _MODELS[n]


def _check(r, m, y, Cn, frames, first, last, chans=None, edges=None, what="", rate=48000):
    """r against the model: y is the stream's transformed samples from its frame 0 (interleaved), the window summed
    the blocks [first, last) and accounted `frames` frames"""
    chans = list(chans) if chans is not None else ([0, 1] if Cn >= 2 else [0])
    edges = list(edges) if edges is not None else octaves(m.n)
    nb = len(edges) - 1
    assert (r.rate, r.channels, r.frames, r.blocks) == (rate, Cn, frames, last - first), what
    assert (r.fft_log2, r.bands, r.selected) == (m.n, nb, len(chans)), what
    assert [r.edges[i] for i in range(33)] == edges + [0] * (32 - nb), what
    assert [r.channel[i] for i in range(8)] == chans + [0] * (8 - len(chans)), what
    f = np.asarray(y, dtype=np.int64).reshape(-1, Cn)
    for c in range(8):
        want = m.bands(f[:, chans[c]], edges, first, last) if c < len(chans) else []
        want = want + [0] * (32 - len(want))
        got = [r.power[c][k] for k in range(32)]
        if c < len(chans):
            print("spec", what, "channel", chans[c], "got", got[:nb], "want", want[:nb])
        assert got == want, (what, c)
        for k in range(32):
            assert _bits(r.db[c][k]) == _bits(db(want[k], last - first) if c < len(chans) and k < nb else 0.0), (what, c, k)


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


def _batch(cm, streams=1, Cn=2, max_frames=4103, flags=None, n=8, edges=None, channels=None, configure=True):
    b = cm.Batch(streams, Cn, max_frames, flags=cm.VU if flags is None else flags)
    assert b.get_spectrum() == 0
    if configure:
        assert b.spec_configure(n, edges, channels) == 0
    assert b.set_spectrum(1) == 0
    assert b.get_spectrum() == 1
    return b


def _one(b, stream=0):
    rc, r = b.spec_result(stream)
    assert rc == 0
    return r


def _feed(b, s, x, Cn, cuts):
    """stream s of a batch of one: x in runs of the given lengths; a run of 0 frames is a run that gives the stream a
    count of 0 (a uniform run of 0 frames launches nothing) and then that one too"""
    pos = 0
    for k in cuts:
        if k:
            b.upload(s, x[Cn * pos: Cn * (pos + k)])
            b.run(k)
        else:
            b.run(1, [0])
            b.run(0)
        pos += k
    return pos


# ---------------------------------------------------------------------------
# 1. parity


@pytest.mark.parametrize("transform", ["identity", "general"])
def test_parity(gpu, oracle, transform):
    """3 stereo streams x 4103 frames of noise in one run: 31 blocks each, all of them from the run but for their
    first samples, which no state precedes"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(21)
    S, T = 3, 4103
    b = _batch(cm, S, configure=False)               # the defaults: n = 10 ...
    assert b.set_spectrum(0) == 0 and b.spec_configure(8) == 0 and b.set_spectrum(1) == 0    # ... and n = 8
    gains, cmap = (None, None) if transform == "identity" else ([750, 1250], [1, 0])
    g = _set(orc, b, -1, 2, gains, cmap)
    xs = [_noise(rng, T, 2) for _ in range(S)]
    for s in range(S):
        b.upload(s, xs[s])
    n0 = cm.lib.cmhip_debug_spec_count()
    b.run(T)
    assert cm.lib.cmhip_debug_spec_count() == n0 + 1
    out, rc = b.spec_results()
    m = model(cm)
    assert m.count(T) == 31
    for s in range(S):
        assert rc[s] == 0
        _check(out[s], m, _transform(orc, xs[s], 2, g, cmap), 2, T, 0, 31, what=(transform, s))
    b.close()


def test_the_default_geometry(gpu):
    """n = 10, channels 0 and 1, the bin octaves"""
    cm = gpu
    rng = np.random.default_rng(22)
    T = 1024 + 512 + 3
    x = _noise(rng, T, 2)
    b = _batch(cm, 1, max_frames=T, configure=False)
    b.upload(0, x)
    b.run(T)
    _check(_one(b), model(cm, 10), x, 2, T, 0, 2, what="defaults")
    b.close()


# ---------------------------------------------------------------------------
# 2. extremes, planted sines


def test_extremes(gpu):
    """full scale everywhere: DC, Nyquist, and impulses on a block's first and last sample and on each side of the
    run edge at frame 1000, one stream each; bands that hold every bin, DC included"""
    cm = gpu
    T, cut = 4103, 1000
    i = np.arange(T)
    sig = {
        "dc -32768": np.full(T, -32768), "dc 32767": np.full(T, 32767),
        "nyquist": np.where(i & 1, 32767, -32768), "nyquist inverted": np.where(i & 1, -32768, 32767),
    }
    for name, at in (("block 3's first", 3 * H8), ("block 3's last", 3 * H8 + N8 - 1), ("before the edge", cut - 1),
                     ("behind the edge", cut), ("the stream's first", 0), ("the last block's last", 30 * H8 + N8 - 1)):
        for v in (-32768, 32767):
            sig["%s %d" % (name, v)] = np.where(i == at, v, 0)
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 129]
    b = _batch(cm, len(sig), edges=edges)
    xs = {}
    for s, (name, mono) in enumerate(sig.items()):
        xs[s] = np.stack([mono, -mono - (mono == -32768)], axis=1).clip(-32768, 32767).astype(np.int16).reshape(-1)
    for lo, hi in ((0, cut), (cut, T)):
        for s in xs:
            b.upload(s, xs[s][2 * lo: 2 * hi])
        b.run(hi - lo)
    out, rc = b.spec_results()
    m = model(cm)
    for s, name in enumerate(sig):
        assert rc[s] == 0
        _check(out[s], m, xs[s], 2, T, 0, 31, edges=edges, what=name)
    # DC at -32768: X[0] is -2^29 but for the window's one clipped entry, 2^42 per block in the band of bin 0
    assert 31 * 2**42 * 0.999 < out[0].power[0][0] <= 31 * 2**42 and abs(out[0].db[0][0] - 10 * math.log10(2**42 / 1649267441664.)) < 0.01
    # Nyquist: the same in the band of bin 128
    assert 31 * 2**42 * 0.999 < out[2].power[0][8] <= 31 * 2**42
    b.close()


def test_planted_sines(gpu):
    """a full-scale sine in the middle of each octave band in turn, one stream per band: that band is the loudest,
    so none can hide behind another"""
    cm = gpu
    T = 4 * N8
    centres = [1, 3, 6, 12, 24, 48, 96, 128]          # (the last band is the Nyquist bin alone: a cosine there)
    b = _batch(cm, len(centres))
    xs = []
    for s, k0 in enumerate(centres):
        wave = np.cos if k0 == 128 else np.sin
        mono = np.rint(32767 * wave(2 * np.pi * k0 * np.arange(T) / N8)).astype(np.int16)
        xs.append(np.stack([mono, np.zeros(T, dtype=np.int16)], axis=1).reshape(-1))
        b.upload(s, xs[s])
    b.run(T)
    out, rc = b.spec_results()
    m = model(cm)
    for s, k0 in enumerate(centres):
        assert rc[s] == 0
        _check(out[s], m, xs[s], 2, T, 0, m.count(T), what=("sine at bin", k0))
        levels = [out[s].db[0][k] for k in range(8)]
        assert levels.index(max(levels)) == s, (k0, levels)
        if 6 <= k0 <= 96:                            # the three main-lobe bins lie inside the band: 0 dB
            assert abs(levels[s]) < 0.001, (k0, levels)
        assert all(out[s].power[1][k] == 0 and out[s].db[1][k] == -math.inf for k in range(8))    # the silent channel
    b.close()


# ---------------------------------------------------------------------------
# 3. cuts


CUTS = (1, 7, 127, 128, 129, 255, 256, 257, 1000, 0)


def test_cut_invariance(gpu, oracle):
    """one stream in runs of CUTS in several orders equals the single run: runs shorter than the hop that complete no
    block, runs that end on a block's last frame, and a run longer than 2 N ahead of short ones -- its blocks read the
    state the run before left while the run's own end becomes the next state"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(23)
    T = sum(CUTS)
    x = _noise(rng, T, 2)
    b = _batch(cm, 1, max_frames=T)
    g = _set(orc, b, 0, 2, [999, 1001], [1, 0])
    y = _transform(orc, x, 2, g, [1, 0])
    m = model(cm)
    assert _feed(b, 0, x, 2, [T]) == T
    whole = _one(b)
    _check(whole, m, y, 2, T, 0, m.count(T), what="one run")
    orders = [CUTS, CUTS[::-1], (1000, 1, 7, 0, 127, 128, 129, 255, 256, 257), (257, 0, 1, 1000, 7, 256, 127, 255, 129, 128),
              (7, 1, 127, 1000, 0, 128, 257, 129, 256, 255)]
    for order in orders:
        b.spec_reset(-1)
        assert _feed(b, 0, x, 2, order) == T
        cut = _one(b)
        _check(cut, m, y, 2, T, 0, m.count(T), what=("cut", order))
        assert bytes(cut) == bytes(whole), order
    b.close()


def test_ragged_counts(gpu, oracle):
    """five streams with counts of their own in every run, zeros among them; 32767 behind every count"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(24)
    S, F = 5, 700
    counts = [[0, 1, 127, 700, 300], [700, 0, 129, 1, 256], [255, 700, 0, 700, 0], [1, 513, 700, 0, 700],
              [700, 700, 700, 700, 1]]
    b = _batch(cm, S, max_frames=F)
    g = _set(orc, b, -1, 2, [1900, 310], None)
    fed = [np.zeros(0, dtype=np.int16) for _ in range(S)]
    for row in counts:
        for s, k in enumerate(row):
            x = np.full(F * 2, 32767, dtype=np.int16)
            x[:2 * k] = _noise(rng, k, 2)
            b.upload(s, x)
            fed[s] = np.concatenate([fed[s], x[:2 * k]])
        b.run(F, row)
    out, rc = b.spec_results()
    m = model(cm)
    for s in range(S):
        total = sum(row[s] for row in counts)
        assert rc[s] == 0 and m.count(total) >= 3
        _check(out[s], m, orc.gain_apply(g, fed[s], 2), 2, total, 0, m.count(total), what=("ragged", s))
    b.close()


# ---------------------------------------------------------------------------
# 4. windows


def test_windows(gpu):
    cm = gpu
    rng = np.random.default_rng(25)
    x = [_noise(rng, 2000, 2) for _ in range(2)]
    b = _batch(cm, 2, max_frames=300)
    m = model(cm)
    pos = [0, 0]

    def run(k):
        for s in range(2):
            b.upload(s, x[s][2 * pos[s]: 2 * (pos[s] + k)])
            pos[s] += k
        b.run(k)

    # a window without a block: INVAL, `out` untouched, the window kept
    run(200)
    sentinel = cm.SpecResult()
    C.memset(C.byref(sentinel), 0x5a, C.sizeof(sentinel))
    before = bytes(sentinel)
    assert b.spec_result(0, sentinel)[0] == cm.ERROR_INVAL and bytes(sentinel) == before
    out, rc = b.spec_results()
    assert rc == [cm.ERROR_INVAL] * 2
    # 300 frames: block 0; the result closes the window and keeps the state
    run(100)
    _check(_one(b, 0), m, x[0], 2, 300, 0, 1, what="block 0")
    assert b.spec_result(0)[0] == cm.ERROR_INVAL
    # block 1 covers frames 128..383: it straddles the close and lands in the later window
    run(100)
    _check(_one(b, 0), m, x[0], 2, 100, 1, 2, what="the straddling block")
    # 50 more complete nothing: INVAL, and the 50 frames stay accounted
    run(50)
    assert b.spec_result(0, sentinel)[0] == cm.ERROR_INVAL and bytes(sentinel) == before
    run(100)
    _check(_one(b, 0), m, x[0], 2, 150, 2, 3, what="after a window without a block")
    # stream 1 has had no result so far: its window holds everything
    out, rc = b.spec_results()
    assert rc == [cm.ERROR_INVAL, 0]
    _check(out[1], m, x[1], 2, 550, 0, 3, what="stream 1, all at once")
    # a reset re-anchors stream 0 at frame 0 of what follows; stream 1 goes on
    b.spec_reset(0)
    fresh = _noise(rng, 300, 2)
    b.upload(0, fresh)
    b.upload(1, x[1][2 * pos[1]: 2 * (pos[1] + 300)])
    pos[1] += 300
    b.run(300)
    out, rc = b.spec_results()
    assert rc == [0, 0]
    _check(out[0], m, fresh, 2, 300, 0, 1, what="after the reset")
    _check(out[1], m, x[1], 2, 300, 3, m.count(850), what="stream 1 beside the reset")
    # off and on again: empty windows at position 0
    assert b.set_spectrum(0) == 0 and b.spec_result(0, sentinel)[0] == cm.ERROR_INVAL and b.set_spectrum(1) == 0
    b.upload(0, fresh)
    b.upload(1, fresh)
    b.run(300)
    _check(_one(b, 1), m, fresh, 2, 300, 0, 1, what="after off and on")
    b.close()


# ---------------------------------------------------------------------------
# 5. sizes, channels, band tables


@pytest.mark.parametrize("n", [10, 12])
def test_sizes(gpu, oracle, n):
    """2 streams, 5 blocks each, in two runs"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(26 + n)
    N = 1 << n
    T = 3 * N + 5
    b = _batch(cm, 2, max_frames=T, n=n)
    g = _set(orc, b, -1, 2, [1200, 640], [1, 0])
    xs = [_noise(rng, T, 2) for _ in range(2)]
    for lo, hi in ((0, N + 17), (N + 17, T)):
        for s in range(2):
            b.upload(s, xs[s][2 * lo: 2 * hi])
        b.run(hi - lo)
    out, rc = b.spec_results()
    m = model(cm, n)
    assert m.count(T) == 5
    for s in range(2):
        assert rc[s] == 0
        _check(out[s], m, _transform(orc, xs[s], 2, g, [1, 0]), 2, T, 0, 5, what=(n, s))
    b.close()


CHANNEL_CASES = [(6, (5, 0, 3), [2, 0, 1, 5, 4, 3], [300, 2500, 1000, 999, 1, 65535]),
                 (16, (15, 0, 7, 8, 3, 12, 1, 10), None, list(range(400, 2000, 100))),
                 (1, (0,), None, [1500]),
                 (1, None, None, None),
                 (3, None, [2, 2, 0], None)]


@pytest.mark.parametrize("Cn,chans,cmap,gains", CHANNEL_CASES, ids=["6ch-3", "16ch-8", "mono", "mono-default", "3ch-default"])
def test_channels(gpu, oracle, Cn, chans, cmap, gains):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(27)
    S, T = 2, 1000
    b = _batch(cm, S, Cn, max_frames=T, channels=chans)
    g = _set(orc, b, -1, Cn, gains, cmap)
    xs = [_noise(rng, T, Cn) for _ in range(S)]
    for lo, hi in ((0, 333), (333, T)):
        for s in range(S):
            b.upload(s, xs[s][Cn * lo: Cn * hi])
        b.run(hi - lo)
    out, rc = b.spec_results()
    m = model(cm)
    for s in range(S):
        assert rc[s] == 0
        _check(out[s], m, _transform(orc, xs[s], Cn, g, cmap), Cn, T, 0, m.count(T), chans=chans, what=(Cn, chans, s))
    b.close()


def _tables(cm):
    return {"single bins": list(range(10, 43)), "everything": [0, 129], "32 bands": list(range(0, 132, 4)),
            "one bin at the top": [128, 129], "dc alone": [0, 1], "uneven": [0, 3, 4, 40, 41, 127, 129],
            "designed": cm.spec_design_bands(48000, 8, 1)}


@pytest.mark.parametrize("name", ["single bins", "everything", "32 bands", "one bin at the top", "dc alone", "uneven",
                                  "designed"])
def test_band_tables(gpu, name):
    cm = gpu
    edges = _tables(cm)[name]
    rng = np.random.default_rng(28)
    T = 1000
    x = _noise(rng, T, 2)
    b = _batch(cm, 1, max_frames=T, edges=edges)
    b.upload(0, x)
    b.run(T)
    m = model(cm)
    _check(_one(b), m, x, 2, T, 0, m.count(T), edges=edges, what=name)
    b.close()


# ---------------------------------------------------------------------------
# 6. refusals


def test_refusals(gpu):
    cm = gpu
    lib = cm.lib
    b = cm.Batch(2, 3, 300, flags=cm.VU)
    res = cm.SpecResult()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    before = bytes(res)
    e16 = lambda *v: (C.c_uint16 * len(v))(*v)       # noqa: E731
    ch8 = lambda *v: (C.c_ubyte * len(v))(*v)        # noqa: E731
    # NULL
    assert lib.cmhip_batch_set_spectrum(None, 1) == cm.ERROR_FAULT and lib.cmhip_batch_get_spectrum(None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_configure(None, 8, 0, None, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_configure(b.h, 8, 1, None, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_configure(b.h, 8, 0, None, 1, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_result(None, 0, C.byref(res)) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_result(b.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_results(b.h, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_spec_reset(None, 0) == cm.ERROR_FAULT
    # a batch without the meter
    assert lib.cmhip_batch_spec_result(b.h, 0, C.byref(res)) == cm.ERROR_INVAL and bytes(res) == before
    assert lib.cmhip_batch_spec_results(b.h, C.byref(res), None) == cm.ERROR_INVAL and bytes(res) == before
    assert lib.cmhip_batch_spec_reset(b.h, -1) == cm.ERROR_INVAL
    # bad geometry: nothing changes (the run below is held to the last good configuration)
    good = [0, 5, 129]
    assert b.spec_configure(8, good, (2, 0)) == 0
    for n in (0, 7, 13, 31):
        assert b.spec_configure(n, good, (2, 0)) == cm.ERROR_INVAL, n
    for bad in ([5, 5], [6, 5], [0, 130], [0, 5, 5, 9], [3, 2, 1], list(range(34))):
        assert lib.cmhip_batch_spec_configure(b.h, 8, len(bad) - 1, e16(*bad), 0, None) == cm.ERROR_INVAL, bad
    assert b.spec_configure(9, [0, 258]) == cm.ERROR_INVAL and b.spec_configure(9, [0, 257]) == 0
    assert b.spec_configure(8, good, (2, 0)) == 0
    for bad in ((3,), (0, 0), (0, 1, 2, 1), (255,)):
        assert b.spec_configure(8, good, bad) == cm.ERROR_INVAL, bad
    assert lib.cmhip_batch_spec_configure(b.h, 8, 0, None, 9, ch8(*range(9))) == cm.ERROR_INVAL
    # on: configure is BUSY, a stream out of range INVAL
    assert b.set_spectrum(1) == 0 and b.set_spectrum(1) == 0
    assert b.spec_configure(8, good, (2, 0)) == cm.ERROR_BUSY and b.spec_configure(10) == cm.ERROR_BUSY
    assert lib.cmhip_batch_spec_result(b.h, 2, C.byref(res)) == cm.ERROR_INVAL and bytes(res) == before
    assert lib.cmhip_batch_spec_reset(b.h, 2) == cm.ERROR_INVAL and lib.cmhip_batch_spec_reset(b.h, -2) == cm.ERROR_INVAL
    rng = np.random.default_rng(29)
    x = _noise(rng, 300, 3)
    b.upload(0, x)
    b.upload(1, x)
    b.run(300)
    _check(_one(b, 1), model(cm), x, 3, 300, 0, 1, chans=(2, 0), edges=good, what="the last good configuration")
    b.close()


def test_spectrum_and_equaliser_exclude_each_other(gpu):
    cm = gpu
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    e = cm.Batch(2, 2, 300, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    assert e.spec_configure(8) == 0 and e.set_spectrum(1) == 0
    assert e.set_eq(-1, coef) == cm.ERROR_INVAL      # sections while the meter is on
    assert e.set_eq(-1, []) == 0                     # (no sections stays allowed)
    assert e.set_spectrum(0) == 0
    assert e.set_eq(-1, coef) == 0
    assert e.set_spectrum(1) == cm.ERROR_INVAL and e.get_spectrum() == 0
    assert e.set_eq(-1, []) == 0
    assert e.set_spectrum(1) == 0
    x = _noise(np.random.default_rng(30), 300, 2)
    e.upload(0, x)
    e.upload(1, x)
    e.run(300)
    _check(_one(e, 0), model(cm), x, 2, 300, 0, 1, what="an EQ batch without sections")
    e.close()


# ---------------------------------------------------------------------------
# 7. beside the other meters, in place


def test_beside_the_other_meters(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(31)
    S, T = 3, 5000                                   # (a 100 ms sub-block of loudness is 4800 frames)
    xs = [_noise(rng, T, 2) for _ in range(S)]
    counts = [T, 0, 2049]
    m = model(cm)

    def run(tp, loud, co, sp):
        b = cm.Batch(S, 2, T, flags=cm.OUT_PCM | cm.VU)
        g = _set(orc, b, -1, 2, [800, 1300], [1, 0])
        assert b.set_true_peak(tp) == 0 and b.set_loudness(loud) == 0 and b.set_correlation(co) == 0
        assert b.spec_configure(8) == 0 and b.set_spectrum(sp) == 0
        n0 = cm.lib.cmhip_debug_spec_count()
        for k, fps in enumerate((None, counts)):
            for s in range(S):
                b.upload(s, xs[s])
            b.run(T, fps)
            assert cm.lib.cmhip_debug_spec_count() == n0 + (k + 1 if sp else 0)
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
        if sp:
            out, rc = b.spec_results()
            res["spec"] = [(rc[s], bytes(out[s])) for s in range(S)]
            for s in range(S):
                y = _transform(orc, xs[s], 2, g, [1, 0])
                y = np.concatenate([y, y[:counts[s] * 2]])
                _check(out[s], m, y, 2, T + counts[s], 0, m.count(T + counts[s]), what=("beside", s))
        vu, rc = b.vu_results()
        res["vu"] = [(rc[s], vu[s].as_dict()) for s in range(S)]
        res["pcm"] = [b.download(s, T).tobytes() for s in range(S)]
        b.close()
        return res

    together = run(1, 1, 1, 1)
    for alone in (run(1, 0, 0, 0), run(0, 1, 0, 0), run(0, 0, 1, 0), run(0, 0, 0, 1), run(0, 0, 0, 0)):
        for key, val in alone.items():
            assert together[key] == val, key


def test_in_place_pcm_batch(gpu, oracle):
    """the block kernel overwrites the slots the pass has read: queued ahead of it, the pass saw the input"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(32)
    S, T = 3, 4103
    b = _batch(cm, S, flags=cm.OUT_PCM | cm.VU | cm.INPLACE)
    g = _set(orc, b, -1, 2, [1700, 650], [1, 0])
    xs = [_noise(rng, T, 2) for _ in range(S)]
    for s in range(S):
        b.upload(s, xs[s])
    b.run(T)
    out, rc = b.spec_results()
    m = model(cm)
    for s in range(S):
        y = _transform(orc, xs[s], 2, g, [1, 0])
        assert np.array_equal(b.download(s, T), y), s
        assert rc[s] == 0
        _check(out[s], m, y, 2, T, 0, 31, what=("in place", s))
    b.close()


# ---------------------------------------------------------------------------
# 8. a group


def _take(handle, nbytes):
    got = b""
    while len(got) < nbytes:
        n, data = handle.read(nbytes - len(got))
        assert n > 0
        got += data
    return np.frombuffer(got, dtype=np.int16)


def test_group(gpu, oracle):
    """two table and two null sources, stereo, over pumped blocks of 1000 frames (the sources of
    tests/test_gpu_corr.py::test_group): the streams' positions run on from pump to pump, so each window is held to
    the blocks of the whole feed that completed in it"""
    cm, orc = gpu, oracle
    Cn, block = 2, 1000
    grp = cm.Group(Cn, 6, block, queue_blocks=8)     # (not full: the engine has more streams than the group slots)
    assert grp.spectrum_configure(8, None, (1, 0)) == 0
    assert grp.set_spectrum(1) == 0
    assert grp.spectrum_configure(8) == cm.ERROR_BUSY
    assert cm.lib.coolmic_group_spectrum(grp.ptr, 4, C.byref(cm.SpecResult())) == cm.ERROR_INVAL
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
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    assert grp.set_eq(-1, coef) == cm.ERROR_INVAL    # the engine's INVAL, passed through
    m = model(cm)
    ys = [np.zeros(0, dtype=np.int16) for _ in range(N)]     # the transformed feed so far, from the anchor
    done = [0] * N                                   # blocks earlier windows have taken

    def feed(i, frames):
        f = feeds[i]
        if "raw" in f:
            raw = f["raw"][f["pos"] * Cn: (f["pos"] + frames) * Cn]
            f["pos"] += frames
        else:
            raw = _take(f["handle"], frames * Cn * 2)
        assert raw.size == frames * Cn
        ys[i] = np.concatenate([ys[i], _transform(orc, raw, Cn, gs[i], setup[i][1])])

    def vu_frames(k):
        vu, rc_vu = grp.vumeter_results()
        assert rc_vu == [0] * N
        n = [vu[i].frames for i in range(N)]
        assert all(0 < v <= k * block for v in n) and n[0] == n[2] == k * block
        return n

    def held(r, i, frames, what):
        total = len(ys[i]) // Cn
        _check(r, m, ys[i], Cn, frames, done[i], m.count(total), chans=(1, 0), what=what)
        done[i] = m.count(total)

    # two pumps, then every window at once: the block in flight counts
    for _ in range(2):
        assert grp.pump() == N
    out, rc = grp.spectra()
    n = vu_frames(2)
    assert len(rc) == N and rc == [0] * N
    for i in range(N):
        feed(i, n[i])
        held(out[i], i, n[i], ("group", i))
    # the 1 kHz table: bin 5.33 of 256 at 48 kHz, the octave 4..7; the null source is silent
    assert max(range(8), key=lambda k: out[0].power[0][k]) == 2 and not any(out[1].power[0][k] for k in range(8))
    # empty windows: every rc INVAL, results left alone
    keep = bytes(out[2])
    out, rc = grp.spectra(out)
    assert rc == [cm.ERROR_INVAL] * N and bytes(out[2]) == keep
    # a single-slot call closes only that slot's window
    assert grp.pump() == N
    rc2, r2 = grp.spectrum(2)
    assert rc2 == 0
    feed(2, block)
    held(r2, 2, block, "group, slot 2 alone")
    assert grp.spectrum(2)[0] == cm.ERROR_INVAL
    assert grp.pump() == N
    out, rc = grp.spectra()
    n = vu_frames(2)
    assert rc == [0] * N
    for i in range(N):
        k = n[i] - block if i == 2 else n[i]
        feed(i, k)
        held(out[i], i, k, ("group, after the single slot", i))
    # reset: one slot re-anchors (its next window starts a stream of its own), then all
    assert grp.pump() == N
    assert grp.spectrum_reset(0) == 0
    assert grp.spectrum_reset(4) == cm.ERROR_INVAL
    out, rc = grp.spectra()
    n = vu_frames(1)
    assert rc == [cm.ERROR_INVAL, 0, 0, 0]
    for i in range(N):
        feed(i, n[i])
        if i:
            held(out[i], i, n[i], ("group, after reset(0)", i))
    ys[0], done[0] = ys[0][:0], 0
    assert grp.pump() == N
    out, rc = grp.spectra()
    n = vu_frames(1)
    assert rc == [0] * N
    for i in range(N):
        feed(i, n[i])
        held(out[i], i, n[i], ("group, re-anchored", i))
    assert grp.pump() == N
    assert grp.spectrum_reset(-1) == 0
    assert grp.spectra()[1] == [cm.ERROR_INVAL] * N
    assert grp.set_spectrum(0) == 0
    for f in feeds:
        if "twin" in f:
            f["handle"].unref(); f["twin"].unref()
    grp.unref()


# ---------------------------------------------------------------------------
# 9. the example


def test_batch_spectrum_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_spectrum"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_spectrum.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    tone = [ln for ln in lines if ln.startswith("1 kHz band")]
    hum = [ln for ln in lines if ln.startswith("50 Hz band")]
    assert len(tone) == 1 and len(hum) == 1
    assert abs(float(tone[0].split()[-2]) - -20.0) < 0.1, tone
    assert abs(float(hum[0].split()[-2]) - -60.0) < 0.1, hum
