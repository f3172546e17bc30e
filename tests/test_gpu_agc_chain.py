"""GPU: the leveller where it belongs -- bus -> leveller -> limiter -> the slots of a batch, all on the batch's stream
with no synchronisation in between, over five ragged blocks.  Bar: the batch's PCM equals the composed numpy models
(the bus's and the limiter's from their own test files, the leveller's from tests/test_gpu_agc.py) bit for bit, block
by block, with the leveller's and the limiter's state carried across the blocks; |y| <= threshold holds throughout,
although the leveller's gain above unity drives samples into its clamp."""
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
SOURCES, BUSES, MAXF, W_LOG2 = 4, 2, 2000, 6
BLOCKS = [[700, 0, 333, 1200], [1, 2000, 1999, 5], [2000, 7, 8, 0], [0, 0, 0, 1234], [1500, 1501, 1, 1999]]
SENDS = ([0, 0, 1, 1, 1], [0, 1, 1, 2, 3])            # bus 0: sources 0 and 1; bus 1: sources 1, 2 and 3
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 4096


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_agc_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TB = _load("test_gpu_bus")             # model_bus
TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry
TA = _load("test_gpu_agc")             # Model, params, enveloped


@pytest.mark.parametrize("channels", [1, 2])
def test_bus_leveller_limiter_batch(gpu, channels):
    cm = gpu
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(BUSES, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    bus = cm.Bus(SOURCES, BUSES, channels, channels, MAXF, 8, hip_stream=b.hip_stream())
    agc = cm.Leveller(BUSES, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    lim = cm.Limiter(BUSES, channels, LOOKAHEAD_LOG2, HOLD, MAXF, threshold=THRESHOLD, drive=DRIVE,
                     hip_stream=b.hip_stream())
    assert bus.hip_stream() == agc.hip_stream() == lim.hip_stream() == b.hip_stream()
    table = SENDS + (np.stack([8192 * np.eye(channels, dtype=np.int16)] * 5),)
    bus.set_routing(*table)
    # bus 0 is brought up to a modest level; bus 1 far too high, at once: its samples meet the leveller's clamp
    plist = [TA.params(target=6000, gate=0, gain_min=1, gain_max=8192, rise=30000, fall=30000),
             TA.params(target=20000, gate=10, gain_min=1, gain_max=65535, rise=65535, fall=65535, initial=16384)]
    for s, p in enumerate(plist):
        agc.set(s, cm.AgcParams(**p))
    levellers = [TA.Model(channels, W_LOG2, p) for p in plist]
    hist = [np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16) for _ in range(BUSES)]
    src, mixed, level = (cm.MappedPcm(types.SimpleNamespace(streams=n, stride=stride)) for n in (SOURCES, BUSES, BUSES))
    total = [sum(blk[s] for blk in BLOCKS) for s in range(SOURCES)]
    signals = [TA.enveloped(400 + s, total[s], channels, 1 << W_LOG2) // 2 for s in range(SOURCES)]
    try:
        at = [0] * SOURCES
        limited = 0
        for k, counts in enumerate(BLOCKS):
            xs = [signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)]
            at = [a + n for a, n in zip(at, counts)]
            src.array[:] = POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            mixed.array[:] = SENTINEL
            level.array[:] = SENTINEL
            got = bus.run(src.dev, stride, max(counts), mixed.dev, stride, counts)
            frames = int(got.max())
            agc.run(mixed.dev, stride, frames, level.dev, stride, got)
            lim.run(level.dev, stride, frames, b.dev_in, b.stride, got)
            b.run(frames, got)                       # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_mix = TB.model_bus(xs, table, BUSES, channels)
            assert got.tolist() == [y.shape[0] for y in want_mix]
            for s in range(BUSES):
                n = int(got[s])
                want_level = levellers[s].run(want_mix[s])
                want, _ = TL.model_lim(want_level, hist[s], THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
                hist[s] = TL.next_hist(hist[s], want_level)
                assert np.array_equal(mixed.array[s, :n * channels].reshape(-1, channels), want_mix[s]), ("bus", k, s)
                assert np.array_equal(level.array[s, :n * channels].reshape(-1, channels), want_level), ("leveller", k, s)
                assert (level.array[s, n * channels:] == SENTINEL).all(), ("leveller wrote past its count", k, s)
                if n:
                    have = b.download(s, n).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, s)
                    assert np.abs(have.astype(np.int64)).max() <= THRESHOLD
                    assert rcs[s] == 0 and res[s].frames == n and abs(res[s].global_peak) <= THRESHOLD
                    limited += int(np.abs(want_level.astype(np.int64)).max() > THRESHOLD)
            gain, lv, clips = agc.state()
            assert [(int(gain[s]), int(lv[s]), int(clips[s])) for s in range(BUSES)] == [m.state() for m in levellers]
        assert at == total and limited > 0
        assert levellers[1].clips > 0 and levellers[0].clips == 0      # the clamp was met, and only where it was meant to be
        assert (lim.min_gain() < 32768).any()
    finally:
        for o in (lim, agc, bus, b):
            o.close()
        for a in (src, mixed, level):
            a.free()
