"""GPU: the filter where it belongs -- a 40 Hz high-pass -> leveller -> limiter -> the slots of a batch, all on the
batch's stream with no synchronisation in between, over five ragged blocks of microphones with a DC offset.  Bar: every
stage's output equals its numpy model (the filter's from tests/test_gpu_iir.py, the leveller's and the limiter's from
their own test files) bit for bit, block by block, with every stage's state carried across the blocks; and the offset
that would have been levelled is gone: behind the filter the leveller sees the voice's level alone."""
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
MICS, MAXF, W_LOG2 = 3, 2000, 6
BLOCKS = [[700, 0, 333], [1, 2000, 1999], [2000, 7, 8], [0, 0, 1234], [1500, 1501, 1]]
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 4096


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_iir_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TI = _load("test_gpu_iir")             # Model
TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry
TA = _load("test_gpu_agc")             # Model, params


@pytest.mark.parametrize("channels", [1, 2])
def test_filter_leveller_limiter_batch(gpu, channels):
    cm = gpu
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(MICS, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    iir = cm.Filter(MICS, channels, 2, MAXF, hip_stream=b.hip_stream())
    agc = cm.Leveller(MICS, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    lim = cm.Limiter(MICS, channels, LOOKAHEAD_LOG2, HOLD, MAXF, threshold=THRESHOLD, drive=DRIVE,
                     hip_stream=b.hip_stream())
    assert iir.hip_stream() == agc.hip_stream() == lim.hip_stream() == b.hip_stream()
    # microphones 0 and 1: a 40 Hz low cut (mic 1 twice: fourth order); microphone 2 is left as it is
    cut = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0)
    filt = TI.Model(MICS, channels, 2)
    for s, k in ((0, 0), (1, 0), (1, 1)):
        iir.set(s, k, cut)
        filt.set(s, k, cut.as_tuple())
    p = TA.params(target=6000, gate=50, gain_min=256, gain_max=65535, rise=30000, fall=30000)
    agc.set(-1, cm.AgcParams(**p))
    levellers = [TA.Model(channels, W_LOG2, p) for _ in range(MICS)]
    hist = [np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16) for _ in range(MICS)]
    src, cutout, level = (cm.MappedPcm(types.SimpleNamespace(streams=MICS, stride=stride)) for _ in range(3))
    total = [sum(blk[s] for blk in BLOCKS) for s in range(MICS)]
    rng = np.random.default_rng(77)
    n = np.arange(max(total))
    voice = (900.0 * np.sin(2.0 * np.pi * n / 96.0)).astype(np.int64)
    signals = [np.clip(voice[:total[s], None] + 6000 + rng.integers(-60, 61, size=(total[s], channels)), -32768,
                       32767).astype(np.int16) for s in range(MICS)]
    try:
        at = [0] * MICS
        for k, counts in enumerate(BLOCKS):
            xs = [signals[s][at[s]:at[s] + c] for s, c in enumerate(counts)]
            at = [a + c for a, c in zip(at, counts)]
            src.array[:] = POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            cutout.array[:] = SENTINEL
            level.array[:] = SENTINEL
            frames = max(counts)
            iir.run(src.dev, stride, frames, cutout.dev, stride, counts)
            agc.run(cutout.dev, stride, frames, level.dev, stride, counts)
            lim.run(level.dev, stride, frames, b.dev_in, b.stride, counts)
            b.run(frames, counts)                    # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_cut = filt.run(xs)
            for s in range(MICS):
                c = counts[s]
                want_level = levellers[s].run(want_cut[s])
                want, _ = TL.model_lim(want_level, hist[s], THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
                hist[s] = TL.next_hist(hist[s], want_level)
                assert np.array_equal(cutout.array[s, :c * channels].reshape(-1, channels), want_cut[s]), ("filter", k, s)
                assert (cutout.array[s, c * channels:] == SENTINEL).all(), ("filter wrote past its count", k, s)
                assert np.array_equal(level.array[s, :c * channels].reshape(-1, channels), want_level), ("leveller", k, s)
                if c:
                    have = b.download(s, c).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, s)
                    assert rcs[s] == 0 and res[s].frames == c and abs(res[s].global_peak) <= THRESHOLD
            clips, overs = iir.state()
            assert clips.tolist() == filt.clips.tolist() and overs.tolist() == filt.overs.tolist()
            assert np.array_equal(iir.rows(), filt.rows()), ("filter state", k)
            gain, lv, aclips = agc.state()
            assert [(int(gain[s]), int(lv[s]), int(aclips[s])) for s in range(MICS)] == [m.state() for m in levellers]
        assert at == total
        # what the leveller saw: the voice's RMS (900 / sqrt 2 = 636) behind the low cut, the offset's 6000 without it
        assert all(550 < levellers[s].level < 720 for s in (0, 1)) and levellers[2].level > 5900
        assert levellers[0].a_hi > 4 * levellers[2].a_hi
    finally:
        for o in (lim, agc, iir, b):
            o.close()
        for a in (src, cutout, level):
            a.free()
