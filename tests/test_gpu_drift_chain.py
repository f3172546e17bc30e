"""GPU: the drift stage where it belongs -- two sources -> drift -> bus -> limiter -> the slots of a batch, all on the
batch's stream with no synchronisation in between, over five ragged blocks.  Source 0 runs on its own clock: its delta
comes from the servo, fed with an elastic buffer's fill per block; source 1 is on the batch's clock (delta 0).  The
drift run's out_frames are the frames_per_stream of what follows.  Bar: the batch's PCM equals the composed numpy models
(the bus's and the limiter's from their own test files, the drift stage's from tests/drift_model.py) bit for bit, block
by block, with every stage's state carried across the blocks."""
import importlib.util
import os
import types

import numpy as np
import pytest

import drift_model as DM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
MAXF = 2000
BLOCKS = [[1200, 1190], [1, 0], [2000, 2000], [1234, 700], [1501, 5]]     # per block: the frames of the two sources
FILLS = [1100, 1300, 90000, 1024, 700]                                   # the elastic buffer's fill before each block
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 4096


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_drift_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TB = _load("test_gpu_bus")             # model_bus, noise
TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry


@pytest.mark.parametrize("channels", [1, 2])
def test_drift_bus_limiter_batch(gpu, channels):
    cm = gpu
    max_out = DM.out_frames(0, -DM.DELTA_MAX, MAXF)
    stride = (max_out * channels + 7) // 8 * 8 + 8
    b = cm.Batch(1, channels, max_out, flags=cm.OUT_PCM | cm.VU, rate=48000)
    H = cm.drift_design()
    drift = cm.Drift(2, channels, MAXF, hip_stream=b.hip_stream())
    assert drift.max_out_frames() == max_out
    bus = cm.Bus(2, 1, channels, channels, max_out, 2, hip_stream=b.hip_stream())
    lim = cm.Limiter(1, channels, LOOKAHEAD_LOG2, HOLD, max_out, threshold=THRESHOLD, drive=DRIVE,
                     hip_stream=b.hip_stream())
    assert drift.hip_stream() == bus.hip_stream() == lim.hip_stream() == b.hip_stream()
    table = ([0, 0], [0, 1], np.stack([12000 * np.eye(channels, dtype=np.int16)] * 2))
    bus.set_routing(*table)
    model = DM.DriftModel(2, channels, H)
    servo, servo_model = cm.Servo(1024, 15, 6), DM.ServoModel(1024, 15, 6)
    hist = np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16)
    src, fixed, mixed = (cm.MappedPcm(types.SimpleNamespace(streams=n, stride=stride)) for n in (2, 2, 1))
    total = [sum(blk[s] for blk in BLOCKS) for s in range(2)]
    signals = [TB.noise(900 + s, total[s], channels) for s in range(2)]
    try:
        at = [0, 0]
        deltas, limited = [], 0
        for k, counts in enumerate(BLOCKS):
            delta = servo.step(FILLS[k])
            assert delta == servo_model.step(FILLS[k])
            deltas.append(delta)
            drift.set(0, delta)
            model.set(0, delta)
            xs = [signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)]
            at = [a + n for a, n in zip(at, counts)]
            src.array[:] = POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            fixed.array[:] = SENTINEL
            mixed.array[:] = SENTINEL
            got = drift.run(src.dev, stride, max(counts), fixed.dev, stride, counts)
            got_bus = bus.run(fixed.dev, stride, int(got.max()), mixed.dev, stride, got)     # the counts as they came
            frames = int(got_bus.max())
            lim.run(mixed.dev, stride, frames, b.dev_in, b.stride, got_bus)
            b.run(frames, got_bus)                   # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_fixed = model.run(xs)
            assert got.tolist() == [y.shape[0] for y in want_fixed]
            want_mix = TB.model_bus(want_fixed, table, 1, channels)
            assert got_bus.tolist() == [want_mix[0].shape[0]] == [max(got.tolist())]
            want, _ = TL.model_lim(want_mix[0], hist, THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
            hist = TL.next_hist(hist, want_mix[0])
            for s in range(2):
                n = int(got[s]) * channels
                assert np.array_equal(fixed.array[s, :n].reshape(-1, channels), want_fixed[s]), ("drift", k, s)
                assert (fixed.array[s, n:] == SENTINEL).all(), ("drift wrote past its count", k, s)
                assert drift.get(s) == model.get(s)
            n = frames
            assert np.array_equal(mixed.array[0, :n * channels].reshape(-1, channels), want_mix[0]), ("bus", k)
            if n:
                have = b.download(0, n).reshape(-1, channels)
                assert np.array_equal(have, want), ("limiter", k)
                assert rcs[0] == 0 and res[0].frames == n
                limited += int(np.abs(want_mix[0].astype(np.int64)).max() > THRESHOLD)
        assert at == total and limited > 0
        # the servo moved: a fill above the target asked for more input per output, the huge one met the clamp
        assert deltas[0] > 0 and deltas[2] == DM.DELTA_MAX and deltas[4] < deltas[3]
        assert model.out_total[1] == total[1] and model.out_total[0] < total[0]
    finally:
        for o in (lim, bus, drift, b):
            o.close()
        for a in (src, fixed, mixed):
            a.free()
