"""GPU: loudness metering (ITU-R BS.1770 / EBU R128) through the batch ABI, the group and the Python mirror, against the
plain-Python model below -- the restatement of the specification in include/coolmic_hip.h: Python floats are IEEE
doubles, Python arithmetic is unfused, log10, tan and pow come from libm.  The model is never another run of the
device code.  The signal is the transformed stream: orc.gain_apply(g, orc.chmap(map, raw, C), C).

Bar: bit-exact.  Every sub-block sum and every result double is compared as struct.pack("<d", ...); the Tech 3341
sequences fed as real PCM are held to the +-0.1 LU that EBU Tech 3341 allows.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu

_libm = C.CDLL("libm.so.6")
for _n, _k in (("log10", 1), ("tan", 1), ("pow", 2)):
    getattr(_libm, _n).restype = C.c_double
    getattr(_libm, _n).argtypes = [C.c_double] * _k


def _bits(x):
    return struct.pack("<d", x)


def _hex(rows):
    return [[float(v).hex() for v in row] for row in rows]


# ---------------------------------------------------------------------------
# the model


def coefficients(rate):
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = _libm.tan(math.pi * f0 / rate)
    Vh = _libm.pow(10.0, G / 20.0)
    Vb = _libm.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
         2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = _libm.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def lufs(v):
    return -math.inf if v == 0 else -0.691 + 10.0 * _libm.log10(v)


def integrate(z):
    B = [(((z[i - 3] + z[i - 2]) + z[i - 1]) + z[i]) * 0.25 for i in range(3, len(z))]
    kept = [b for b in B if lufs(b) > -70.0]
    if not kept:
        return -math.inf, -math.inf, 0
    total = 0.0
    for b in kept:
        total += b
    thr = lufs(total / float(len(kept))) - 10.0
    kept = [b for b in kept if lufs(b) > thr]
    if not kept:
        return -math.inf, thr, 0
    total = 0.0
    for b in kept:
        total += b
    return lufs(total / float(len(kept))), thr, len(kept)


def _row_run(st, xs, coef, L):
    """one row (a channel of a stream): st = [u1, u2, y1, y2, v1, v2, e, pos], xs: the transformed samples (ints);
    returns the sums of the sub-blocks completed"""
    b0, b1, b2, a1, a2, d0, d1, d2, c1, c2 = coef
    u1, u2, y1, y2, v1, v2, e, pos = st
    out = []
    for x in xs:
        u = x / 32768.0
        f = (b0 * u + b1 * u1) + b2 * u2
        y = (f - a2 * y2) - a1 * y1
        u2 = u1
        u1 = u
        g = (d0 * y + d1 * y1) + d2 * y2
        v = (g - c2 * v2) - c1 * v1
        y2 = y1
        y1 = y
        v2 = v1
        v1 = v
        e = e + v * v
        pos += 1
        if pos == L:
            out.append(e)
            e = 0.0
            pos = 0
    st[:] = [u1, u2, y1, y2, v1, v2, e, pos]
    return out


class Model:
    """one stream"""

    def __init__(self, channels, rate, weights=None):
        self.C, self.rate = channels, rate
        self.L = (rate + 5) // 10
        self.coef = coefficients(rate)
        self.w = [1.0] * channels if weights is None else list(weights)
        self.reset()

    def reset(self):
        self.rows = [[0.0] * 7 + [0] for _ in range(self.C)]
        self.sums = []                           # per complete sub-block: [e_c]
        self.z = []
        self.frames = 0

    def run(self, y):
        y = np.asarray(y).astype(np.int64)
        done = [_row_run(self.rows[c], y[c::self.C].tolist(), self.coef, self.L) for c in range(self.C)]
        for j in range(len(done[0])):
            e = [done[c][j] for c in range(self.C)]
            total = 0.0
            for c in range(self.C):
                total += self.w[c] * e[c]
            self.sums.append(e)
            self.z.append(total / float(self.L))
        self.frames += y.size // self.C

    def result(self):
        z, n = self.z, len(self.z)
        mom = lufs((((z[n - 4] + z[n - 3]) + z[n - 2]) + z[n - 1]) * 0.25) if n >= 4 else -math.inf
        st = -math.inf
        if n >= 30:
            total = 0.0
            for v in z[n - 30:]:
                total += v
            st = lufs(total / 30.0)
        integ, thr, gated = integrate(z)
        return {"frames": self.frames, "blocks": n, "gated_blocks": gated, "momentary": mom, "short_term": st,
                "integrated": integ, "relative_threshold": thr}


def _check_raw(b, s, m, what, cap=30):
    got, done = b.loud_raw(s, cap)
    want = m.sums[-min(cap, 30):] if m.sums else []
    assert done == len(m.sums), (what, done, len(m.sums))
    assert got.shape == (len(want), m.C), (what, got.shape)
    if _hex(got.tolist()) != _hex(want):
        print("loudness sums", what, "got", _hex(got.tolist()), "want", _hex(want))
    assert [[_bits(v) for v in row] for row in got.tolist()] == [[_bits(v) for v in row] for row in want], what


def _check_result(r, m, what):
    want = m.result()
    assert (r.rate, r.channels) == (m.rate, m.C), what
    got = {k: getattr(r, k) for k in want}
    show = {k: (v.hex() if isinstance(v, float) else v) for k, v in got.items()}
    print("loudness result", what, show)
    for k, v in want.items():
        if isinstance(v, float):
            assert _bits(got[k]) == _bits(v), (what, k, got[k], v)
        else:
            assert got[k] == v, (what, k, got[k], v)
    return want


def _noise(rng, frames, Cn, amp=32768):
    return rng.integers(-amp, amp, size=frames * Cn, dtype=np.int64).astype(np.int16)


def _setup_streams(cm, orc, b, rng, S, Cn, maps):
    """per stream in turn: gains general / all below the scale / disabled / saturating; a channel map on every other
    group of four when `maps`"""
    params = []
    for s in range(S):
        kind = s % 4
        if kind == 0:
            gains = [int(v) for v in rng.integers(500, 3000, Cn)]
        elif kind == 1:
            gains = [int(v) for v in rng.integers(1, 1000, Cn)]
        elif kind == 2:
            gains = None
        else:
            gains = [int(v) for v in rng.integers(4000, 65536, Cn)]
        cmap = [int(v) for v in rng.integers(0, Cn, Cn)] if maps and (s // 4) % 2 == 0 else None
        if gains is not None:
            assert b.set_gain(s, Cn, 1000, gains) == 0
            rc, g = orc.gain(Cn, Cn, 1000, gains)
            assert rc == 0
        else:
            assert b.set_gain(s, 0, 0, None) == 0
            g = of.Gain()
        assert b.set_chmap(s, cmap) == 0
        params.append((g, cmap))
    return params


def _transform(orc, raw, Cn, g, cmap):
    x = np.asarray(raw, dtype=np.int16)
    if cmap is not None:
        x = orc.chmap(cmap, x, Cn)
    return orc.gain_apply(g, x, Cn)


def _flags(cm, form):
    f = 0
    for name in form.split("|"):
        f |= getattr(cm, name)
    return f


# ---------------------------------------------------------------------------
# 1. bit-exact sub-block sums

LITERAL_SUM = "0x1.3517c69b3f33ep+1"             # the model's value for [32767] + [0] * 4799 at 48 kHz, from the CPU


def test_literal_sub_block_sum(gpu):
    cm = gpu
    m = Model(1, 48000)
    x = np.array([32767] + [0] * 4799, dtype=np.int16)
    m.run(x)
    assert len(m.sums) == 1 and m.sums[0][0].hex() == LITERAL_SUM
    b = cm.Batch(1, 1, 4800, flags=cm.VU)
    assert b.get_loudness() == 0 and b.set_loudness(1) == 0 and b.get_loudness() == 1
    b.upload(0, x)
    b.run(4800)
    got, done = b.loud_raw(0)
    print("literal", got.tolist(), float.fromhex(LITERAL_SUM))
    assert done == 1 and got.shape == (1, 1)
    assert _bits(got[0, 0]) == _bits(float.fromhex(LITERAL_SUM))
    b.close()
    for rate in (7999, 384001):                  # refused at enable; the batch itself is fine
        b = cm.Batch(1, 1, 64, flags=cm.VU, rate=rate)
        assert b.set_loudness(1) == cm.ERROR_INVAL and b.get_loudness() == 0
        b.close()
    for rate in (8000, 384000):
        b = cm.Batch(1, 1, 64, flags=cm.VU, rate=rate)
        assert b.set_loudness(1) == 0
        b.close()


SHAPES = [(70, 1, False), (33, 2, True), (5, 3, False), (5, 6, True), (5, 16, False)]


@pytest.mark.parametrize("S,Cn,maps", SHAPES)
def test_random_full_range_blocks_against_the_model(gpu, oracle, S, Cn, maps):
    """rate 8000 (L = 800): 70 mono streams are one full wave of rows and a partial one; runs of 1, 799, 800, 801 and
    2403 frames, then ragged counts with 0 and one that ends exactly on a sub-block edge"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(100 * S + Cn)
    T = 2403
    b = cm.Batch(S, Cn, T, flags=cm.VU, rate=8000)
    assert b.set_loudness(1) == 0
    params = _setup_streams(cm, orc, b, rng, S, Cn, maps)
    models = [Model(Cn, 8000) for _ in range(S)]
    total = 1 + 799 + 800 + 801 + 2403
    edge = 800 - total % 800                                 # ends exactly on a sub-block edge
    ragged = [0, edge, T, 1, edge + 800, 397, edge - 1, edge + 1]
    plans = [(1, None), (799, None), (800, None), (801, None), (T, None), (T, [ragged[s % 8] for s in range(S)])]
    for k, (frames, fps) in enumerate(plans):
        for s in range(S):
            x = _noise(rng, frames, Cn)
            b.upload(s, x)
            n = frames if fps is None else fps[s]
            models[s].run(_transform(orc, x[:n * Cn], Cn, *params[s]))
        b.run(frames, fps)
        if k in (2, 3):                                      # 1600 frames: exactly two sub-blocks; then 2401
            for s in (0, S // 2, S - 1):
                _check_raw(b, s, models[s], (S, Cn, k, s))
    for s in range(S):
        _check_raw(b, s, models[s], (S, Cn, "end", s))
    assert len(models[1].sums) == (total + edge) // 800 and models[1].rows[0][7] == 0
    got, done = b.loud_raw(S - 1, 2)                         # a smaller cap: the trailing two
    assert done == len(models[S - 1].sums) and _hex(got.tolist()) == _hex(models[S - 1].sums[-2:])
    b.close()


def test_sums_do_not_depend_on_how_the_stream_is_cut(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(4000)
    x = _noise(rng, 4000, 2)
    m = Model(2, 8000)
    m.run(x)
    assert len(m.sums) == 5
    raws = []
    for cuts in ([4000], [7, 1593, 2400]):
        b = cm.Batch(1, 2, 4000, flags=cm.VU, rate=8000)
        assert b.set_loudness(1) == 0
        at = 0
        for n in cuts:
            b.upload(0, x[at * 2:(at + n) * 2])
            b.run(n)
            at += n
        _check_raw(b, 0, m, cuts)
        raws.append(b.loud_raw(0)[0].tobytes())
        b.close()
    assert raws[0] == raws[1]


def test_decay_is_not_flushed_to_zero(gpu):
    """full-scale noise, then zeros: the filters ring down through the whole double range; the tail sums are the
    model's bits -- denormal sums included -- and not zero while the model's are not"""
    cm = gpu
    rng = np.random.default_rng(77)
    m = Model(1, 8000)
    b = cm.Batch(1, 1, 8000, flags=cm.VU, rate=8000)
    assert b.set_loudness(1) == 0
    x = np.concatenate([_noise(rng, 800, 1), np.zeros(1600, dtype=np.int16)])
    b.upload(0, x)
    b.run(2400)
    m.run(x)
    _check_raw(b, 0, m, "two sub-blocks of zeros")
    got, _ = b.loud_raw(0)
    assert got[1, 0] > 0.0 and got[2, 0] > 0.0
    for _ in range(3):                                       # 24 more sub-blocks of zeros
        z = np.zeros(6400, dtype=np.int16)
        b.upload(0, z)
        b.run(6400)
        m.run(z)
    _check_raw(b, 0, m, "the whole decay")
    tail = [e[0] for e in m.sums]
    assert any(0.0 < v < 2.3e-308 for v in tail), tail       # the model passes through denormal sums ...
    got, _ = b.loud_raw(0)
    assert [v > 0.0 for v in got[:, 0].tolist()] == [v > 0.0 for v in tail]
    b.close()


def test_ring_is_drained_before_it_overflows(gpu):
    """max_frames 8192 at rate 8000: R = 48.  Runs without any result call pass R twice (the host drains on its own);
    then loud_raw after every third run, 30 sub-blocks apart: the concatenation is the model's sequence"""
    cm = gpu
    rng = np.random.default_rng(48)
    S = 2
    b = cm.Batch(S, 1, 8192, flags=cm.VU, rate=8000)
    assert b.set_loudness(1) == 0
    models = [Model(1, 8000) for _ in range(S)]

    def feed(frames, fps=None):
        for s in range(S):
            x = _noise(rng, frames, 1, amp=2000 + 30000 * s)
            b.upload(s, x)
            models[s].run(x[:frames if fps is None else fps[s]])
        b.run(frames, fps)

    for k in range(10):                                      # 81920 frames: 102 sub-blocks > 2 R, no result call
        feed(8192, None if k % 2 else [8192, 8192 - 37 * k])
    held = [len(models[s].sums) for s in range(S)]
    for s in range(S):
        assert held[s] > 96 - 3 * s
        # everything that depends on EVERY z_j the host took out of the ring on its own, bit for bit: one missed or
        # late drain, one overwritten slot, and integrated / threshold / gated_blocks over the 100-odd differ
        rc, r = b.loud_result(s)
        assert rc == 0
        _check_result(r, models[s], ("past R twice", s))
        _check_raw(b, s, models[s], ("past R twice", s))
    later = [[] for _ in range(S)]                           # the device's output alone
    for k in range(9):                                       # three runs are exactly 24000 frames: 30 sub-blocks
        feed((8192, 8192, 7616)[k % 3])
        if k % 3 == 2:
            for s in range(S):
                raw, done = b.loud_raw(s)
                assert done == len(models[s].sums) == held[s] + len(later[s]) + 30, (k, s, done)
                later[s] += raw.tolist()
    for s in range(S):
        assert len(later[s]) == 90
        assert _hex(later[s]) == _hex(models[s].sums[held[s]:]), s
        _check_result(b.loud_result(s)[1], models[s], ("the whole sequence", s))
    b.close()


# ---------------------------------------------------------------------------
# 2. results


def test_results_after_3_4_29_30_and_45_sub_blocks(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(45)
    S, Cn = 2, 2
    b = cm.Batch(S, Cn, 800, flags=cm.VU, rate=8000)
    assert b.set_loudness(1) == 0
    assert b.set_gain(1, 2, 1000, [700, 1300]) == 0
    _, g1 = orc.gain(2, 2, 1000, [700, 1300])
    params = [(of.Gain(), None), (g1, None)]
    models = [Model(Cn, 8000) for _ in range(S)]
    out, rc = b.loud_results()                               # before any frame: zeros and -inf
    assert rc == [0, 0]
    _check_result(out[0], models[0], "empty")
    # levels per sub-block: loud, quiet (the relative gate removes them) and near silence (the absolute gate)
    amps = [32768, 32768, 20000, 32768, 32768, 20000, 300, 300, 300, 300, 300, 300, 300, 2, 1, 2, 1, 20]
    for j in range(45):
        for s in range(S):
            x = _noise(rng, 800, Cn, amp=amps[(j + 4 * s) % len(amps)])
            b.upload(s, x)
            models[s].run(_transform(orc, x, Cn, *params[s]))
        b.run(800)
        if j + 1 in (3, 4, 29, 30, 45):
            out, rc = b.loud_results()
            assert rc == [0, 0]
            for s in range(S):
                want = _check_result(out[s], models[s], (j + 1, s))
                assert (want["momentary"] == -math.inf) == (j + 1 < 4)
                assert (want["short_term"] == -math.inf) == (j + 1 < 30)
                assert want["blocks"] == j + 1 and want["frames"] == 800 * (j + 1)
            again, _ = b.loud_results()                      # not destructive: twice in a row, identical
            assert bytes(again) == bytes(out)
            rc1, r1 = b.loud_result(1)
            assert rc1 == 0 and bytes(r1) == bytes(out[1])
    want = models[0].result()
    assert 0 < want["gated_blocks"] < 42 and want["integrated"] > want["relative_threshold"] > -70.0
    # resetting one stream leaves its neighbour's bits alone
    before = bytes(b.loud_result(1)[1])
    raw_before = b.loud_raw(1)[0].tobytes()
    b.loud_reset(0)
    models[0].reset()
    rc0, r0 = b.loud_result(0)
    assert rc0 == 0
    _check_result(r0, models[0], "after the reset")
    assert bytes(b.loud_result(1)[1]) == before and b.loud_raw(1)[0].tobytes() == raw_before
    for s in range(S):                                       # and both go on: history zero in stream 0, kept in 1
        x = _noise(rng, 800, Cn)
        b.upload(s, x)
        models[s].run(_transform(orc, x, Cn, *params[s]))
    b.run(800)
    for s in range(S):
        _check_raw(b, s, models[s], ("after the reset", s))
        _check_result(b.loud_result(s)[1], models[s], ("after the reset", s))
    # the contract's edges
    r = cm.LoudnessResult()
    assert cm.lib.cmhip_batch_loud_result(b.h, 2, C.byref(r)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_loud_result(b.h, 0, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_loud_reset(b.h, 2) == cm.ERROR_INVAL
    assert b.set_loudness(0) == 0 and b.get_loudness() == 0
    assert cm.lib.cmhip_batch_loud_result(b.h, 0, C.byref(r)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_loud_results(b.h, C.byref(r), None) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_loud_raw(b.h, 0, None, 0, None, None) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_loud_reset(b.h, -1) == cm.ERROR_INVAL
    assert b.set_loudness(1) == 0                            # on again: everything starts over
    models[1].reset()
    _check_result(b.loud_result(1)[1], models[1], "on again")
    b.close()


def test_channel_weights(gpu):
    cm = gpu
    rng = np.random.default_rng(51)
    w51 = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
    b = cm.Batch(2, 6, 1600, flags=cm.VU, rate=8000)
    one = (C.c_double * 6)(*w51)
    assert cm.lib.cmhip_batch_loud_set_weights(b.h, 0, one) == cm.ERROR_INVAL      # a batch without loudness
    assert b.set_loudness(1) == 0
    assert cm.lib.cmhip_batch_loud_set_weights(b.h, 0, None) == cm.ERROR_FAULT
    assert b.loud_set_weights(2, w51) == cm.ERROR_INVAL
    for bad in (-1.0, math.nan, math.inf):
        assert b.loud_set_weights(0, [1.0, 1.0, bad, 1.0, 1.0, 1.0]) == cm.ERROR_INVAL
    assert b.loud_set_weights(0, w51) == 0                   # stream 1 keeps the default, 1.0 everywhere
    models = [Model(6, 8000, w51), Model(6, 8000)]
    for k in range(3):
        for s in range(2):
            x = _noise(rng, 1600, 6)
            b.upload(s, x)
            models[s].run(x[:(1600 if s == 0 or k else 799) * 6])
        b.run(1600, None if k else [1600, 799])
        if k == 0:                                           # stream 1 holds no complete sub-block yet, stream 0 does
            assert b.loud_set_weights(0, w51) == cm.ERROR_BUSY
            assert b.loud_set_weights(-1, w51) == cm.ERROR_BUSY
            assert b.loud_set_weights(1, [1.0] * 6) == 0
    out, rc = b.loud_results()
    for s in range(2):
        _check_result(out[s], models[s], ("weights", s))
    assert _bits(out[0].momentary) != _bits(out[1].momentary)
    assert b.loud_set_weights(1, w51) == cm.ERROR_BUSY
    b.loud_reset(1)                                          # a reset stream takes new weights
    assert b.loud_set_weights(1, w51) == 0
    b.close()


def _tone(dbfs, seconds, rate=48000):
    n = int(round(seconds * rate))
    t = np.arange(n, dtype=np.float64)
    return 32768.0 * 10.0 ** (dbfs / 20.0) * np.sin(2.0 * math.pi * 1000.0 * t / rate)


def test_tech_3341_sequences_as_pcm(gpu):
    """EBU Tech 3341 cases 1, 3 and 5: a 48 kHz stereo 1 kHz sine (the levels are peak dBFS), three streams of one
    batch in 65536-frame runs with ragged counts; integrated loudness within +-0.1 LU of -23.0"""
    cm = gpu
    seqs = [[(-23, 20)], [(-36, 10), (-23, 60), (-36, 10)], [(-26, 20), (-20, 20.1), (-26, 20)]]
    pcm = []
    for seq in seqs:
        mono = np.rint(np.concatenate([_tone(db, sec) for db, sec in seq])).astype(np.int16)
        pcm.append(np.repeat(mono, 2))                       # the same sine in both channels
    T = 65536
    b = cm.Batch(3, 2, T, flags=cm.VU)
    assert b.set_loudness(1) == 0
    pos = [0, 0, 0]
    k = 0
    while any(pos[s] < pcm[s].size // 2 for s in range(3)):
        fps = []
        for s in range(3):
            n = min(T - (1000 * ((k + s) % 3) + 7 * s), pcm[s].size // 2 - pos[s])
            if n:
                b.upload(s, pcm[s][pos[s] * 2:(pos[s] + n) * 2])
            pos[s] += n
            fps.append(n)
        b.run(T, fps)
        k += 1
    out, rc = b.loud_results()
    for s in range(3):
        print("Tech 3341 as PCM", seqs[s], out[s].as_dict())
        assert out[s].frames == pcm[s].size // 2 and out[s].blocks == out[s].frames // 4800
        assert abs(out[s].integrated - (-23.0)) <= 0.1, (s, out[s].integrated)
    assert abs(out[0].momentary - (-23.0)) <= 0.1 and abs(out[0].short_term - (-23.0)) <= 0.1
    b.close()


# ---------------------------------------------------------------------------
# 3. nothing else moves

TP0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
TP1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
TPH = np.array([TP0, TP1, TP1[::-1], TP0[::-1]], dtype=np.int64)


def _true_peak(x):                               # one channel's transformed samples from zero history
    z = np.concatenate([np.zeros(11, dtype=np.int64), np.asarray(x, dtype=np.int64)])
    return max(int(np.abs(np.convolve(z, TPH[p])[11:11 + len(x)]).max()) for p in range(4))


FORMS = ["OUT_PCM|VU|INPLACE", "OUT_PCM|VU", "VU", "OUT_PCM|VU|HOSTPCM", "OUT_F32|VU"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Cn", [2, 6])
def test_everything_else_is_bit_equal_with_loudness_on(gpu, oracle, Cn, form):
    """two batches, the same runs, true peak on in both, loudness in one: PCM, float planes, VU and true-peak results
    are the same bits; loudness and true peak are each the model's; the batch that never enabled loudness launches no
    loudness pass"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(900 + Cn)
    S, T = 5, 1700
    flags = _flags(cm, form)
    count0 = cm.lib.cmhip_debug_loud_count()
    off = cm.Batch(S, Cn, T, flags=flags, rate=8000)
    assert off.set_true_peak(1) == 0
    prm = np.random.default_rng(17)
    params = _setup_streams(cm, orc, off, prm, S, Cn, True)
    plans = [(T, None), (T, [T, 0, 5, 801, 1])]
    data = [[_noise(rng, frames, Cn) for _ in range(S)] for frames, _ in plans]

    def drive(b):
        got = []
        for (frames, fps), xs in zip(plans, data):
            for s in range(S):
                b.upload(s, xs[s])
            b.run(frames, fps)
            for s in range(S):
                n = frames if fps is None else fps[s]
                if flags & cm.OUT_PCM:
                    got.append(b.download(s, n).tobytes())
                if flags & cm.OUT_F32 and n:
                    got += [b.download_f32(s, c, n).tobytes() for c in range(Cn)]
        vu, rc = b.vu_results()
        got += [rc] + [vu[s].as_dict() for s in range(S) if rc[s] == 0]
        tp, rc = b.tp_results()
        got += [rc] + [tp[s].as_dict() for s in range(S) if rc[s] == 0]
        return got, tp

    want, _ = drive(off)
    assert cm.lib.cmhip_debug_loud_count() == count0         # never enabled: no loudness pass
    off.close()
    on = cm.Batch(S, Cn, T, flags=flags, rate=8000)
    assert on.set_true_peak(1) == 0 and on.set_loudness(1) == 0
    prm = np.random.default_rng(17)
    assert [p[1] for p in _setup_streams(cm, orc, on, prm, S, Cn, True)] == [p[1] for p in params]
    got, tp = drive(on)
    assert cm.lib.cmhip_debug_loud_count() == count0 + 2
    assert got == want
    for s in range(S):
        m = Model(Cn, 8000)
        y = np.concatenate([_transform(orc, data[k][s][:(f if fps is None else fps[s]) * Cn], Cn, *params[s])
                            for k, (f, fps) in enumerate(plans)])
        m.run(y)
        _check_raw(on, s, m, (Cn, form, s))
        _check_result(on.loud_result(s)[1], m, (Cn, form, s))
        assert [tp[s].channel_peak[c] for c in range(Cn)] == [_true_peak(y[c::Cn]) for c in range(Cn)], (form, s)
    # off again: the block kernel and the true-peak pass alone
    assert on.set_loudness(0) == 0
    on.run(T)
    on.sync()
    assert cm.lib.cmhip_debug_loud_count() == count0 + 2
    on.close()


def test_loudness_and_equaliser_exclude_each_other(gpu):
    cm = gpu
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    e = cm.Batch(2, 1, 4800, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    assert e.set_loudness(1) == 0
    assert e.set_eq(-1, coef) == cm.ERROR_INVAL
    assert e.set_eq(-1, np.zeros(0, dtype=np.float32)) == 0  # no sections stay allowed, and the pass runs
    x = np.array([32767] + [0] * 4799, dtype=np.int16)
    e.upload(0, x)
    e.upload(1, x)
    e.run(4800)
    got, done = e.loud_raw(1)
    assert done == 1 and got[0, 0].hex() == LITERAL_SUM
    assert e.set_loudness(0) == 0
    assert e.set_eq(-1, coef) == 0
    assert e.set_loudness(1) == cm.ERROR_INVAL and e.get_loudness() == 0
    e.close()


# ---------------------------------------------------------------------------
# 4. a group


def test_group_loudnesses(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(808)
    Cn, N, block, rate = 2, 3, 1000, 8000
    grp = cm.Group(Cn, 8, block, queue_blocks=2, rate=rate)  # (not full: the engine has more streams than slots)
    r = cm.LoudnessResult()
    assert cm.lib.coolmic_group_loudness(grp.ptr, 0, C.byref(r)) == cm.ERROR_INVAL     # no slot yet
    assert grp.set_loudness(1) == 0
    wants, handles, params = [], [], []
    for i, frames in enumerate((4321, 2600, 1234)):          # ragged: the sources end in different pumps
        x = orc.lcg(6000 + i, frames * Cn)
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=(0, 7, 512)[i])
        assert grp.add_stream(src) == i
        src.unref()
        gains = [int(v) for v in rng.integers(100, 2500, Cn)]
        cmap = [1, 0] if i == 1 else None
        assert grp.set_master_gain(i, Cn, 1000, gains) == 0
        assert grp.set_channel_map(i, cmap) == 0
        _, g = orc.gain(Cn, Cn, 1000, gains)
        wants.append(_transform(orc, x, Cn, g, cmap))
        handles.append(grp.get_iohandle(i))
    assert cm.lib.coolmic_group_loudness(grp.ptr, N, C.byref(r)) == cm.ERROR_INVAL
    assert grp.loudness_set_weights(N, [1.0, 1.0]) == cm.ERROR_INVAL
    assert grp.loudness_set_weights(2, [1.0, 0.5]) == 0
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    assert grp.set_eq(-1, coef) == cm.ERROR_INVAL            # the engine's INVAL, passed through
    models = [Model(Cn, rate, [1.0, 0.5] if i == 2 else None) for i in range(N)]
    for _ in range(2):
        assert grp.pump() >= 0
    out, rc = grp.loudnesses()
    assert rc == [0] * N
    for i in range(N):
        n = out[i].frames                                    # what the two pumps took from the source
        assert 0 < n <= min(2 * block, wants[i].size // Cn)
        models[i].run(wants[i][:n * Cn])
        _check_result(out[i], models[i], ("group", i))
    again, _ = grp.loudnesses()
    assert bytes(again) == bytes(out)
    # the rest, drained through the readers; then slot by slot
    got = [b"" for _ in range(N)]
    active = set(range(N))
    guard = 0
    while active and guard < 100000:
        guard += 1
        for i in list(active):
            n, data = handles[i].read(8192)
            assert n >= 0
            got[i] += data
            if n == 0 and handles[i].eof() == 1:
                active.discard(i)
    assert not active
    for i in range(N):
        assert np.array_equal(np.frombuffer(got[i], np.int16), wants[i]), i
        models[i].run(wants[i][models[i].frames * Cn:])
        rc1, r1 = grp.loudness(i)
        assert rc1 == 0
        _check_result(r1, models[i], ("group, one slot", i))
    assert grp.loudness_set_weights(0, [1.0, 1.0]) == cm.ERROR_BUSY
    assert grp.loudness_reset(0) == 0
    models[0].reset()
    _check_result(grp.loudness(0)[1], models[0], "group, reset slot")
    _check_result(grp.loudness(1)[1], models[1], "group, its neighbour")
    for h in handles:
        h.unref()
    grp.unref()


def test_group_meters_in_c_prints_both_r128_meters(gpu, oracle, tmp_path):
    """examples/group_meters.c with "r128": its usual three lines, then true peak and loudness of the same two
    streams; every stream is the 48 kHz sine at unity gain, 40 blocks of 512 frames are four sub-blocks and a bit"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "libcoolmic-dsp_amd", "lib")
    exe = tmp_path / "group_meters"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "group_meters.c"), "-L", libdir, "-lcoolmic-dsp-hip", "-lpthread",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    streams, block, rounds = 3, 512, 40
    out = subprocess.run([str(exe), str(streams), str(block), str(rounds), "host", "r128"], check=True,
                         capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
    assert len(out) == 5, out
    rc_s, sine = oracle.sine_table(48000)
    assert rc_s == 0
    m = Model(1, 48000)
    m.run(np.tile(np.asarray(sine, dtype=np.int16), rounds * block // 48 + 1)[:rounds * block])
    want = m.result()
    assert want["blocks"] == 4
    for line, s in zip(out[3:], (0, streams - 1)):
        assert line.startswith("stream %d: true peak " % s), line
        assert line.endswith("loudness M %.2f S %.2f I %.2f LUFS (4 sub-blocks)"
                             % (want["momentary"], want["short_term"], want["integrated"])), (line, want)
