"""GPU: the noise suppressor where it belongs -- suppressor -> leveller -> limiter -> the slots of a batch, all on the
batch's stream with no synchronisation in between, over five ragged blocks.  Bar: every stage's PCM equals the composed
numpy models (the suppressor's from tests/denoise_model.py, the leveller's and the limiter's from their own test files)
bit for bit, block by block, with every state carried across the blocks.  The suppressor's delay is consumed by a
cmhip_delay_t of cmhip_denoise_delay() frames on a dry path: where the suppressor removes nothing (stream 2, at its
defaults) the two paths are equal to the bit, and elsewhere their difference is the removed part."""
import importlib.util
import os
import types

import numpy as np
import pytest

import denoise_model as DM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
S, MAXF, FFT_LOG2, W_LOG2 = 3, 2000, 8, 6
BLOCKS = [[700, 0, 333], [1, 2000, 1999], [2000, 7, 8], [0, 0, 1234], [1500, 1501, 1]]     # five ragged blocks
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 4096
MID = DM.params(floor=4125, over=64, rise_shift=1, fall_shift=2)


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_denoise_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry
TA = _load("test_gpu_agc")             # Model, params


@pytest.mark.parametrize("channels", [1, 2])
def test_suppressor_leveller_limiter_batch(gpu, channels):
    cm = gpu
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(S, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    hs = b.hip_stream()
    dn = cm.Denoiser(S, channels, FFT_LOG2, MAXF, hip_stream=hs)
    dry_line = cm.Delay(S, channels, dn.delay(), MAXF, delay=dn.delay(), hip_stream=hs)
    agc = cm.Leveller(S, channels, W_LOG2, MAXF, hip_stream=hs)
    lim = cm.Limiter(S, channels, LOOKAHEAD_LOG2, HOLD, MAXF, threshold=THRESHOLD, drive=DRIVE, hip_stream=hs)
    assert dn.hip_stream() == dry_line.hip_stream() == agc.hip_stream() == lim.hip_stream() == hs and dn.delay() == 255
    tab = DM.Tables(cm, FFT_LOG2)
    rng = np.random.default_rng(40 + channels)
    prof = rng.integers(1 << 18, 1 << 28, tab.H + 1).astype(np.uint64)
    cleaners = [DM.Stream(tab, channels) for _ in range(S)]
    for c in range(channels):
        dn.set_profile(0, c, prof)
        cleaners[0].set_profile(c, prof)
    dn.set(0, cm.DenoiseParams(**MID))
    cleaners[0].set(MID)
    dn.learn(1, True)
    cleaners[1].learn(True)
    # quiet streams brought up, at once: samples meet the leveller's clamp and the limiter's threshold
    plist = [TA.params(target=12000, gate=0, gain_min=1, gain_max=65535, rise=30000, fall=30000),
             TA.params(target=20000, gate=10, gain_min=1, gain_max=65535, rise=65535, fall=65535, initial=16384),
             TA.params(target=6000, gate=0, gain_min=1, gain_max=8192, rise=30000, fall=30000)]
    for s, p in enumerate(plist):
        agc.set(s, cm.AgcParams(**p))
    levellers = [TA.Model(channels, W_LOG2, p) for p in plist]
    hist = [np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16) for _ in range(S)]
    src, clean, dry, level = (cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride)) for _ in range(4))
    fed, total = [[] for _ in range(S)], [0] * S
    try:
        limited = removed = 0
        for k, counts in enumerate(BLOCKS):
            frames = max(counts)
            amp = 900 if k < 2 else 9000                                 # quiet while stream 1 learns
            xs = [rng.integers(-amp, amp + 1, size=(n, channels)).astype(np.int16) for n in counts]
            src.array[:] = POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            for a in (clean, dry, level):
                a.array[:] = SENTINEL
            if k == 2:                                                   # behind two queued blocks, no wait
                dn.learn(1, False)
                dn.set(1, cm.DenoiseParams(**MID))
                cleaners[1].learn(False)
                cleaners[1].set(MID)
            dn.run(src.dev, stride, frames, clean.dev, stride, counts)
            dry_line.run(src.dev, stride, frames, dry.dev, stride, counts)
            agc.run(clean.dev, stride, frames, level.dev, stride, counts)
            lim.run(level.dev, stride, frames, b.dev_in, b.stride, counts)
            b.run(frames, counts)                        # (no sync between the five: the order is the stream's)
            res, rcs = b.vu_results()
            for s in range(S):
                n = counts[s]
                fed[s].append(xs[s])
                total[s] += n
                want_clean = cleaners[s].run(xs[s])
                want_level = levellers[s].run(want_clean)
                want, _ = TL.model_lim(want_level, hist[s], THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
                hist[s] = TL.next_hist(hist[s], want_level)
                want_dry = np.concatenate([np.zeros((255, channels), dtype=np.int16)] + fed[s])[total[s] - n:total[s]]
                have_clean = clean.array[s, :n * channels].reshape(-1, channels)
                have_dry = dry.array[s, :n * channels].reshape(-1, channels)
                assert np.array_equal(have_clean, want_clean), ("suppressor", k, s)
                assert np.array_equal(have_dry, want_dry), ("dry path", k, s)
                assert np.array_equal(level.array[s, :n * channels].reshape(-1, channels), want_level), ("leveller", k, s)
                for a in (clean, dry, level):
                    assert (a.array[s, n * channels:] == SENTINEL).all(), ("written past its count", k, s)
                if s == 2:
                    assert np.array_equal(have_clean, have_dry)          # nothing removed: the delay alone
                else:
                    removed += int(np.abs(have_dry.astype(np.int64) - have_clean).sum())
                if n:
                    have = b.download(s, n).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, s)
                    assert np.abs(have.astype(np.int64)).max() <= THRESHOLD
                    assert rcs[s] == 0 and res[s].frames == n
                    limited += int(np.abs(want_level.astype(np.int64)).max() > THRESHOLD)
            clips, sat, learned = dn.state()
            assert [(int(clips[s]), int(sat[s]), int(learned[s])) for s in range(S)] == [m.state() for m in cleaners]
        assert limited > 0 and removed > 0 and cleaners[1].cnt > 0
        for s in range(S):
            for c in range(channels):
                q, g = dn.get_profile(s, c)
                assert g.tolist() == cleaners[s].rows[c].g and [int(v) for v in q] == cleaners[s].rows[c].np
    finally:
        for o in (lim, agc, dry_line, dn, b):
            o.close()
        for a in (src, clean, dry, level):
            a.free()
