"""GPU: true-peak metering (ITU-R BS.1770 Annex 2, 4x oversampling) through the batch ABI, the group and the Python
mirror, against the integer model below and the literal values of the specification.

Bar: bit-exact.  Peaks are integers and equal the model's; every dBTP double is bit-equal to the host formula
20. * log10(peak / 268435456.) taken from libm.  The model is the numpy function `tp` -- never another run of the
device code.  The signal is the transformed stream: orc.gain_apply(g, orc.chmap(map, raw, C), C).
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu

P0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
P1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
H = np.array([P0, P1, P1[::-1], P0[::-1]], dtype=np.int64)
WORST = 542986257                                  # the largest value the filter can produce
WORST_PATTERN = np.array([32767 if P1[11 - j] >= 0 else -32768 for j in range(12)], dtype=np.int16)

_libm = C.CDLL("libm.so.6")
_libm.log10.restype = C.c_double
_libm.log10.argtypes = [C.c_double]


def tp(x, hist):      # x: one channel's transformed samples of a run, hist: 11 values; returns the run's max
    z = np.concatenate([hist, x]).astype(np.int64)
    return max(int(np.abs(np.convolve(z, H[p])[11:11 + len(x)]).max()) for p in range(4)) if len(x) else 0


def dbtp(peak):
    return 20. * _libm.log10(peak / 268435456.) if peak else -math.inf


def _bits(x):
    return struct.pack("<d", x)


class Model:
    """one stream: history per channel (kept over window closes), the open window's maxima and frame count"""

    def __init__(self, channels):
        self.C = channels
        self.reset()

    def reset(self):
        self.hist = [np.zeros(11, dtype=np.int64) for _ in range(self.C)]
        self.peak = [0] * self.C
        self.frames = 0

    def run(self, y):
        y = np.asarray(y, dtype=np.int64)
        for c in range(self.C):
            x = y[c::self.C]
            self.peak[c] = max(self.peak[c], tp(x, self.hist[c]))
            self.hist[c] = np.concatenate([self.hist[c], x])[-11:]
        self.frames += y.size // self.C

    def take(self):
        out = (list(self.peak), self.frames)
        self.peak = [0] * self.C
        self.frames = 0
        return out


def _check_result(r, peaks, frames, channels, what, rate=48000):
    assert (r.rate, r.channels, r.frames) == (rate, channels, frames), what
    got = [r.channel_peak[c] for c in range(channels)]
    print("true peak", what, "got", got, "want", peaks)
    assert got == peaks, what
    assert r.global_peak == max(peaks), what
    for c in range(channels):
        assert _bits(r.channel_dbtp[c]) == _bits(dbtp(peaks[c])), (what, c)
    assert _bits(r.global_dbtp) == _bits(dbtp(max(peaks))), what


def _mono(cm, max_frames=8192, flags=None):
    b = cm.Batch(1, 1, max_frames, flags=cm.VU if flags is None else flags)
    assert b.set_true_peak(1) == 0
    return b


def _feed(b, x, stream=0):
    x = np.asarray(x, dtype=np.int16)
    b.upload(stream, x)
    b.run(x.size // b.channels)


def _peak(b, stream=0):
    rc, r = b.tp_result(stream)
    assert rc == 0
    return r


# ---------------------------------------------------------------------------
# 1. the literal values of the specification


def test_literal_values(gpu):
    cm = gpu
    b = _mono(cm)
    for x, want in (([1] + [0] * 20, 7964), ([-32768] + [0] * 20, 260964352)):
        b.tp_reset()
        _feed(b, x)
        r = _peak(b)
        _check_result(r, [want], 21, 1, x[0])
    sine = [23170, 23170, -23170, -23170] * 1200
    b.tp_reset()
    _feed(b, sine)
    r = _peak(b)
    _check_result(r, [270996320], 4800, 1, "fs/4 sine")
    assert r.global_dbtp == float.fromhex("0x1.51cc5f944547ap-4")
    # the same input cut into a run of 5 frames and a run of 4795, one window
    b.tp_reset()
    _feed(b, sine[:5])
    _feed(b, sine[5:])
    _check_result(_peak(b), [270996320], 4800, 1, "sine in two runs")
    b.tp_reset()
    _feed(b, sine[:5])
    _check_result(_peak(b), [17562860], 5, 1, "the first run alone")
    # the largest value the filter can produce
    b.tp_reset()
    _feed(b, WORST_PATTERN)
    r = _peak(b)
    _check_result(r, [WORST], 12, 1, "worst case")
    assert r.global_dbtp > 6.11
    # history kept over the close, cleared by the reset
    b.tp_reset()
    _feed(b, [32767] * 40)
    _check_result(_peak(b), [299523147], 40, 1, "step")
    _feed(b, [32767] * 40)
    _check_result(_peak(b), [268853235], 40, 1, "step again, history kept")
    b.tp_reset()
    _feed(b, [32767] * 40)
    _check_result(_peak(b), [299523147], 40, 1, "after the reset")
    # silence: peak 0, -inf
    b.tp_reset()
    _feed(b, [0] * 100)
    r = _peak(b)
    _check_result(r, [0], 100, 1, "silence")
    assert r.global_dbtp == -math.inf
    assert cm.tp_dbtp(1 << 28) == 0.0 and cm.tp_dbtp(1) == -168.57679757182947
    b.close()


# ---------------------------------------------------------------------------
# 2. randomised blocks against the model

CHANNELS = [1, 2, 3, 4, 5, 6, 8, 12, 16]
FORMS = ["VU", "OUT_PCM|VU", "OUT_PCM|VU|INPLACE", "OUT_F32|VU"]


def _flags(cm, form):
    f = 0
    for name in form.split("|"):
        f |= getattr(cm, name)
    return f


def _setup_streams(cm, orc, b, rng, S, Cn):
    """per stream: gains general / all below the scale / disabled, with and without a channel map"""
    params = []
    for s in range(S):
        kind = s % 3
        if kind == 0:
            gains = [int(v) for v in rng.integers(500, 3000, Cn)]
        elif kind == 1:
            gains = [int(v) for v in rng.integers(1, 1000, Cn)]
        else:
            gains = None
        cmap = [int(v) for v in rng.integers(0, Cn, Cn)] if (s // 3) % 2 else None
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


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Cn", CHANNELS)
def test_random_blocks_against_the_model(gpu, oracle, Cn, form):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(1000 * Cn + FORMS.index(form))
    S, T = 7, 5000                                   # mono: 2 tiles of the kernel, stereo 3, other counts 5
    b = cm.Batch(S, Cn, T, flags=_flags(cm, form))
    assert b.get_true_peak() == 0
    assert b.set_true_peak(1) == 0
    assert b.get_true_peak() == 1
    params = _setup_streams(cm, orc, b, rng, S, Cn)
    models = [Model(Cn) for _ in range(S)]
    special = [0, 1, 10, 11, 12, T, T - 3]
    plans = [(T, None), (T, 1), (T, 3), (4099, None), (T, 5), (12, None)]
    for k, (frames, rot) in enumerate(plans):
        fps = None if rot is None else [special[(s + rot) % S] for s in range(S)]
        if k % 2 == 0:                               # GEN_NOISE and uploaded PCM in turn
            b.generate(cm.GEN_NOISE, 77 + k, frames, first_global=3 * k, global_step=1, frame_offset=k * T)
            b.sync()
            raws = [b.download_input(s, frames) for s in range(S)]
        else:
            raws = []
            for s in range(S):
                kind = ("full", "edges", "small")[(s + k) % 3]
                if kind == "full":
                    x = rng.integers(-32768, 32768, size=frames * Cn, dtype=np.int64).astype(np.int16)
                elif kind == "edges":
                    x = rng.choice(np.array([-32768, -32767, -1, 0, 1, 32766, 32767], dtype=np.int16), size=frames * Cn)
                else:
                    x = rng.integers(-5, 6, size=frames * Cn, dtype=np.int64).astype(np.int16)
                b.upload(s, x)
                raws.append(x)
        b.run(frames, fps)
        for s in range(S):
            n = frames if fps is None else fps[s]
            models[s].run(_transform(orc, raws[s][:n * Cn], Cn, *params[s]))
        if k in (1, 5):                              # results taken after some runs ...
            out, rc = b.tp_results()
            for s in range(S):
                peaks, fr = models[s].take()
                assert rc[s] == (0 if fr else cm.ERROR_INVAL), (k, s)
                if fr:
                    _check_result(out[s], peaks, fr, Cn, (Cn, form, k, s))
        elif k == 3:                                 # ... of some streams only ...
            for s in (0, 4, 5):
                peaks, fr = models[s].take()
                rc1, r = b.tp_result(s)
                assert rc1 == 0
                _check_result(r, peaks, fr, Cn, (Cn, form, k, s))
        # ... and not after others
    b.close()


# ---------------------------------------------------------------------------
# 3. the worst-case pattern around every boundary of the kernel


def _plant(total, Cn, ch, at):
    x = np.zeros(total * Cn, dtype=np.int16)
    x[at * Cn + ch: (at + 12) * Cn: Cn] = WORST_PATTERN
    return x


@pytest.mark.parametrize("Cn", [1, 2])
def test_worst_case_pattern_at_tile_and_slot_boundaries(gpu, Cn):
    """one stream per offset, all in one run: the pattern's last frame at every position in a band around each tile
    boundary (8 KiB: 4096 mono / 2048 stereo frames), around each lane's 128 bytes, and around the end of the slot's
    whole 16-byte vectors"""
    cm = gpu
    tile = 4096 // Cn
    total = 2 * tile + 150 + 5                       # ends in a partial vector
    starts = set()
    for edge in (0, 64 // Cn, tile, 2 * tile):
        starts |= set(range(max(0, edge - 30), edge + 20))
    starts |= set(range(total - 45, total - 11))     # the whole pattern still fits
    starts = sorted(s for s in starts if 0 <= s and s + 12 <= total)
    for ch in range(Cn):
        b = cm.Batch(len(starts), Cn, total, flags=cm.VU)
        assert b.set_true_peak(1) == 0
        for i, at in enumerate(starts):
            b.upload(i, _plant(total, Cn, ch, at))
        b.run(total)
        out, rc = b.tp_results()
        for i, at in enumerate(starts):
            assert rc[i] == 0
            want = [0] * Cn
            want[ch] = WORST                         # the other channel of a stereo stream stays 0
            _check_result(out[i], want, total, Cn, (Cn, ch, at))
        b.close()


@pytest.mark.parametrize("Cn", [1, 2])
def test_worst_case_pattern_split_across_two_runs(gpu, Cn):
    """the pattern's first `cut` frames end one run, the rest start the next: cut 1..11, after first runs of several
    lengths (the history is what carries it)"""
    cm = gpu
    firsts = [cut + lead for lead in (0, 1, 10, 11, 12, 4096 // Cn, 4096 // Cn + 3) for cut in range(1, 12)]
    cuts = [cut for _ in range(7) for cut in range(1, 12)]
    S = len(firsts)
    T = max(firsts) + 12
    for ch in range(Cn):
        b = cm.Batch(S, Cn, T, flags=cm.VU)
        assert b.set_true_peak(1) == 0
        second = []
        for s in range(S):
            n1, cut = firsts[s], cuts[s]
            x = _plant(n1 + 12 - cut, Cn, ch, n1 - cut)
            b.upload(s, x[:n1 * Cn])
            second.append(x[n1 * Cn:])
        b.run(max(firsts), firsts)
        for s in range(S):
            b.upload(s, second[s])
        n2 = [12 - cut for cut in cuts]
        b.run(max(n2), n2)
        out, rc = b.tp_results()
        for s in range(S):
            assert rc[s] == 0
            want = [0] * Cn
            want[ch] = WORST
            _check_result(out[s], want, firsts[s] + n2[s], Cn, (Cn, ch, firsts[s], cuts[s]))
        b.close()


# ---------------------------------------------------------------------------
# 4. the contract


def test_contract(gpu):
    cm = gpu
    b = cm.Batch(3, 2, 256, flags=cm.VU)
    r = cm.TruePeakResult()
    r.frames = 123
    # a batch without true peak
    assert cm.lib.cmhip_batch_tp_result(b.h, 0, C.byref(r)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_tp_results(b.h, C.byref(r), None) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_tp_reset(b.h, -1) == cm.ERROR_INVAL
    assert b.set_true_peak(1) == 0
    # before any frame: INVAL, out left alone
    assert cm.lib.cmhip_batch_tp_result(b.h, 0, C.byref(r)) == cm.ERROR_INVAL
    assert r.frames == 123
    assert cm.lib.cmhip_batch_tp_result(b.h, 3, C.byref(r)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_tp_result(b.h, 0, None) == cm.ERROR_FAULT
    out, rc = b.tp_results()
    assert rc == [cm.ERROR_INVAL] * 3
    step = np.repeat(np.array([32767], dtype=np.int16), 80)      # both channels: 40 frames of 32767
    for s in range(3):
        b.upload(s, step)
    b.run(40, [40, 0, 7])
    b.run(40, [40, 0, 0])
    # frames counts; tp_result of one stream leaves the others' windows open
    rc0, r0 = b.tp_result(0)
    assert rc0 == 0 and r0.frames == 80 and r0.channels == 2 and r0.rate == 48000
    assert b.tp_result(1)[0] == cm.ERROR_INVAL                   # no frame ever
    assert b.tp_result(0)[0] == cm.ERROR_INVAL                   # closed
    rc2, r2 = b.tp_result(2)
    assert rc2 == 0 and r2.frames == 7
    assert [r2.channel_peak[0], r2.channel_peak[1]] == [tp(np.full(7, 32767), np.zeros(11))] * 2
    # closing keeps the history ...
    b.run(40, [40, 0, 0])
    rc0, r0 = b.tp_result(0)
    assert rc0 == 0 and r0.frames == 40 and r0.channel_peak[0] == tp(np.full(40, 32767), np.full(11, 32767))
    assert r0.channel_peak[0] == 268853235
    # ... tp_reset of one stream clears it, and only there
    b.tp_reset(0)
    b.run(40, [40, 0, 40])
    assert b.tp_result(0)[1].channel_peak[0] == 299523147
    m = Model(2)
    m.run(step[:14])
    m.take()
    m.run(step)
    assert b.tp_result(2)[1].channel_peak[1] == m.peak[1]
    # turning it off discards window and history
    b.run(40)
    assert b.set_true_peak(0) == 0 and b.get_true_peak() == 0
    assert b.tp_result(0)[0] == cm.ERROR_INVAL
    assert b.set_true_peak(1) == 0
    assert b.tp_result(0)[0] == cm.ERROR_INVAL
    b.run(40)
    assert b.tp_result(0)[1].channel_peak[0] == 299523147
    b.close()
    # true peak and equaliser sections exclude each other; no sections stay allowed
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    e = cm.Batch(2, 1, 256, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    assert e.set_true_peak(1) == 0
    assert e.set_eq(-1, coef) == cm.ERROR_INVAL
    assert e.set_eq(-1, np.zeros(0, dtype=np.float32)) == 0
    e.upload(0, np.array([1] + [0] * 20, dtype=np.int16))
    e.upload(1, np.array([-32768] + [0] * 20, dtype=np.int16))
    e.run(21)
    out, rc = e.tp_results()
    assert rc == [0, 0] and [out[0].global_peak, out[1].global_peak] == [7964, 260964352]
    assert e.set_true_peak(0) == 0
    assert e.set_eq(-1, coef) == 0
    assert e.set_true_peak(1) == cm.ERROR_INVAL
    assert e.get_true_peak() == 0
    e.close()


# ---------------------------------------------------------------------------
# 5. nothing else changes with true peak on


@pytest.mark.parametrize("Cn", [1, 2, 6])
def test_pcm_floats_and_vu_unchanged_with_true_peak_on(gpu, oracle, Cn):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(500 + Cn)
    S, T = 6, 4500
    for form in FORMS:
        flags = _flags(cm, form)
        b = cm.Batch(S, Cn, T, flags=flags)
        assert b.set_true_peak(1) == 0
        params = _setup_streams(cm, orc, b, rng, S, Cn)
        vus = [orc.vu_new(Cn) for _ in range(S)]
        tp0, runs0 = cm.lib.cmhip_debug_tp_count(), cm.lib.cmhip_debug_run_count()
        for k, (frames, fps) in enumerate(((T, None), (T, [T, 0, 5, 4097, 1, 100]))):
            raws = []
            for s in range(S):
                x = rng.integers(-32768, 32768, size=frames * Cn, dtype=np.int64).astype(np.int16)
                b.upload(s, x)
                raws.append(x)
            b.run(frames, fps)
            for s in range(S):
                n = frames if fps is None else fps[s]
                want = _transform(orc, raws[s][:n * Cn], Cn, *params[s])
                if n:
                    orc.vu_accumulate(vus[s], want)
                if flags & cm.OUT_PCM:
                    assert np.array_equal(b.download(s, n), want), (Cn, form, k, s)
                if flags & cm.OUT_F32 and n:
                    planes = orc.to_f32_planar(want, Cn)
                    for c in range(Cn):
                        assert np.array_equal(b.download_f32(s, c, n), planes[c]), (Cn, form, k, s, c)
        assert cm.lib.cmhip_debug_tp_count() - tp0 == 2 and cm.lib.cmhip_debug_run_count() - runs0 == 2
        out, rc = b.vu_results()
        for s in range(S):
            rc_o, r_o = orc.vu_result(vus[s])
            assert rc[s] == rc_o
            if rc_o == 0:
                assert out[s].as_dict() == of.vu_result_dict(r_o), (Cn, form, s)
        # off again: the block kernel alone
        assert b.set_true_peak(0) == 0
        tp0, runs0 = cm.lib.cmhip_debug_tp_count(), cm.lib.cmhip_debug_run_count()
        b.run(T)
        b.sync()
        assert cm.lib.cmhip_debug_tp_count() == tp0 and cm.lib.cmhip_debug_run_count() == runs0 + 1
        b.close()


# ---------------------------------------------------------------------------
# 6. the flag-completion path


@pytest.mark.parametrize("Cn", [1, 2])
def test_host_resident_one_stream_batch_in_1k_blocks(gpu, oracle, Cn):
    """a one-stream CMHIP_HOSTPCM batch fed 1 KiB blocks: one-workgroup launches whose host spins on the completion
    word; the true-peak kernel runs ahead of the block kernel on the same stream"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(60 + Cn)
    frames = 512 // Cn                               # 1 KiB
    b = cm.Batch(1, Cn, frames, flags=cm.OUT_PCM | cm.VU | cm.HOSTPCM)
    assert b.set_true_peak(1) == 0
    gains = [int(v) for v in rng.integers(500, 2500, Cn)]
    assert b.set_gain(0, Cn, 1000, gains) == 0
    _, g = orc.gain(Cn, Cn, 1000, gains)
    m = Model(Cn)
    v = orc.vu_new(Cn)
    for k in range(40):
        x = rng.integers(-32768, 32768, size=frames * Cn, dtype=np.int64).astype(np.int16)
        b.upload(0, x)
        b.run(frames)
        want = orc.gain_apply(g, x, Cn)
        assert np.array_equal(b.download(0, frames), want), k
        m.run(want)
        orc.vu_accumulate(v, want)
        if k % 7 == 6:
            peaks, fr = m.take()
            rc, r = b.tp_result(0)
            assert rc == 0
            _check_result(r, peaks, fr, Cn, ("hostpcm", Cn, k))
    peaks, fr = m.take()
    out, rc = b.tp_results()
    assert rc == [0]
    _check_result(out[0], peaks, fr, Cn, ("hostpcm", Cn, "end"))
    rc_v, r_v = b.vu_result(0)
    rc_o, r_o = orc.vu_result(v)
    assert rc_v == rc_o == 0 and r_v.as_dict() == of.vu_result_dict(r_o)
    b.close()


# ---------------------------------------------------------------------------
# 7. a group


def test_group_true_peaks(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(707)
    Cn, N, block = 2, 64, 1000                       # block lengths that do not divide the inputs
    grp = cm.Group(Cn, 96, block, queue_blocks=2)    # (not full: the engine has more streams than the group slots)
    assert grp.set_true_peak(1) == 0
    r = cm.TruePeakResult()
    assert cm.lib.coolmic_group_true_peak(grp.ptr, N, C.byref(r)) == cm.ERROR_INVAL
    wants, handles = [], []
    for i in range(N):
        frames = int(rng.integers(1, 4321))
        x = orc.lcg(5000 + i, frames * Cn)
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=int(rng.choice([0, 3, 7, 512, 1024])))
        slot = grp.add_stream(src)
        src.unref()
        assert slot == i
        gains = [int(v) for v in rng.integers(100, 2500, Cn)]
        cmap = [int(v) for v in rng.integers(0, Cn, Cn)] if i % 2 else None
        assert grp.set_master_gain(slot, Cn, 1000, gains) == 0
        assert grp.set_channel_map(slot, cmap) == 0
        _, g = orc.gain(Cn, Cn, 1000, gains)
        wants.append(_transform(orc, x, Cn, g, cmap))
        handles.append(grp.get_iohandle(slot))
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    assert grp.set_eq(-1, coef) == cm.ERROR_INVAL    # the engine's INVAL, passed through
    # two blocks pumped, then every window at once.  What a window holds does not depend on how the stream was cut
    # into blocks (the history carries over exactly); how many frames the two pumps took from each source is what
    # the VU windows, asked between the same two pumps, count as well
    models = [Model(Cn) for _ in range(N)]
    pos = [0] * N
    for _ in range(2):
        assert grp.pump() >= 0
    out, rc = grp.true_peaks()
    vu, rc_vu = grp.vumeter_results()
    assert len(rc) == N
    for i in range(N):
        assert rc[i] == 0 and rc_vu[i] == 0
        n = vu[i].frames
        assert 0 < n <= min(2 * block, wants[i].size // Cn)
        models[i].run(wants[i][:n * Cn])
        pos[i] = n
        peaks, fr = models[i].take()
        _check_result(out[i], peaks, fr, Cn, ("group", i))
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
        models[i].run(wants[i][pos[i] * Cn:])
        peaks, fr = models[i].take()
        rc1, r1 = grp.true_peak(i)
        assert rc1 == (0 if fr else cm.ERROR_INVAL), i
        if fr:
            _check_result(r1, peaks, fr, Cn, ("group, one slot", i))
    for h in handles:
        h.unref()
    grp.unref()


# ---------------------------------------------------------------------------
# 8. full size once


def test_full_size(gpu, oracle):
    cm, orc = gpu, oracle
    S, Cn, T = 4096, 2, 65536
    b = cm.Batch(S, Cn, T, flags=cm.VU)
    assert b.set_true_peak(1) == 0
    assert b.set_gain(-1, 2, 1000, [750, 1250]) == 0
    assert b.set_chmap(-1, [1, 0]) == 0
    _, g = orc.gain(2, 2, 1000, [750, 1250])
    b.generate(cm.GEN_NOISE, 2024, T)
    b.sync()
    rng = np.random.default_rng(8)
    picked = sorted(set([0, 1, S - 1] + [int(v) for v in rng.integers(0, S, 61)]))
    while len(picked) < 64:
        picked = sorted(set(picked + [int(rng.integers(0, S))]))
    raws = {s: b.download_input(s, T) for s in picked}
    b.run(T)
    out, rc = b.tp_results()
    assert rc == [0] * S
    for s in range(S):
        assert out[s].frames == T and out[s].channels == 2
        assert out[s].global_peak == max(out[s].channel_peak[0], out[s].channel_peak[1]) > 0
    for s in picked:
        m = Model(2)
        m.run(_transform(orc, raws[s], 2, g, [1, 0]))
        _check_result(out[s], m.peak, T, 2, ("full size", s))
    b.close()
