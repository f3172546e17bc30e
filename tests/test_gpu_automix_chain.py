"""GPU: the automixer where it belongs -- automixer -> bus -> limiter -> the slots of a batch, all on the batch's stream
with no synchronisation in between, over five ragged blocks.  Four microphones of one group go to bus 0; a fifth stream
in no group, with counts of its own, passes the automixer as a copy and goes to bus 1.  Bar: the batch's PCM equals the
composed numpy models (the bus's and the limiter's from their own test files, the automixer's from
tests/automix_model.py) bit for bit, block by block, with the automixer's and the limiter's state carried across the
blocks."""
import importlib.util
import os
import types

import numpy as np
import pytest

import automix_model as AM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
MICS, SOURCES, BUSES, MAXF, W_LOG2 = 4, 5, 2, 2000, 6
BLOCKS = [[700, 1200], [1, 0], [2000, 1999], [0, 1234], [1501, 5]]       # per block: the group's count, the fifth stream's
SENDS = ([0, 0, 0, 0, 1], [0, 1, 2, 3, 4])            # bus 0: the four microphones; bus 1: the fifth stream
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 8192


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_automix_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TB = _load("test_gpu_bus")             # model_bus
TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry


@pytest.mark.parametrize("channels", [1, 2])
def test_automixer_bus_limiter_batch(gpu, channels):
    cm = gpu
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(BUSES, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    amx = cm.Automixer(SOURCES, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    bus = cm.Bus(SOURCES, BUSES, channels, channels, MAXF, 8, hip_stream=b.hip_stream())
    lim = cm.Limiter(BUSES, channels, LOOKAHEAD_LOG2, HOLD, MAXF, threshold=THRESHOLD, drive=DRIVE,
                     hip_stream=b.hip_stream())
    assert amx.hip_stream() == bus.hip_stream() == lim.hip_stream() == b.hip_stream()
    table = SENDS + (np.stack([16384 * np.eye(channels, dtype=np.int16)] * 5),)       # unity sends: the automixer keeps the sum in range
    bus.set_routing(*table)
    desk = AM.Desk(SOURCES, channels, W_LOG2)
    plist = [AM.params(), AM.params(attack=1, release=3), AM.params(weight=2048, floor=300, release=2), AM.params(floor=100),
             AM.params(weight=5)]
    for s, p in enumerate(plist):
        amx.set(s, cm.AutomixParams(**p))
        desk.set(s, p)
    for s in range(MICS):
        amx.set_group(s, 3)
        desk.set_group(s, 3)
    hist = [np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16) for _ in range(BUSES)]
    src, shared = (cm.MappedPcm(types.SimpleNamespace(streams=SOURCES, stride=stride)) for _ in range(2))
    mixed = cm.MappedPcm(types.SimpleNamespace(streams=BUSES, stride=stride))
    counts_of = lambda blk: [blk[0]] * MICS + [blk[1]]
    total = [sum(counts_of(blk)[s] for blk in BLOCKS) for s in range(SOURCES)]
    signals = [AM.spurts(700 + s, total[s], channels, 1 << W_LOG2, quiet_first=s % 2) // 2 for s in range(SOURCES)]
    try:
        at = [0] * SOURCES
        limited = shared_gain = 0
        for k, blk in enumerate(BLOCKS):
            counts = counts_of(blk)
            xs = [signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)]
            at = [a + n for a, n in zip(at, counts)]
            src.array[:] = POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            shared.array[:] = SENTINEL
            mixed.array[:] = SENTINEL
            amx.run(src.dev, stride, max(counts), shared.dev, stride, counts)
            got = bus.run(shared.dev, stride, max(counts), mixed.dev, stride, counts)
            frames = int(got.max())
            lim.run(mixed.dev, stride, frames, b.dev_in, b.stride, got)
            b.run(frames, got)                       # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_shared = desk.run(xs)
            want_mix = TB.model_bus(want_shared, table, BUSES, channels)
            assert got.tolist() == [y.shape[0] for y in want_mix]
            for s in range(SOURCES):
                n = counts[s] * channels
                assert np.array_equal(shared.array[s, :n].reshape(-1, channels), want_shared[s]), ("automixer", k, s)
                assert (shared.array[s, n:] == SENTINEL).all(), ("automixer wrote past its count", k, s)
            assert np.array_equal(want_shared[4], xs[4])                 # in no group: a copy
            for s in range(BUSES):
                n = int(got[s])
                want, _ = TL.model_lim(want_mix[s], hist[s], THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
                hist[s] = TL.next_hist(hist[s], want_mix[s])
                assert np.array_equal(mixed.array[s, :n * channels].reshape(-1, channels), want_mix[s]), ("bus", k, s)
                if n:
                    have = b.download(s, n).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, s)
                    assert np.abs(have.astype(np.int64)).max() <= THRESHOLD
                    assert rcs[s] == 0 and res[s].frames == n
                    limited += int(2 * np.abs(want_mix[s].astype(np.int64)).max() > THRESHOLD)
            gain, power, share = amx.state()
            assert (gain.tolist(), power.tolist(), share.tolist()) == desk.state()
            shared_gain += int(any(g not in (4096, p["floor"]) for g, p in zip(gain.tolist()[:MICS], plist)))
        assert at == total and limited > 0 and shared_gain > 0
        assert all(sq <= 2 ** 24 + 300 ** 2 + 100 ** 2 for sq, _ in desk.squares) and desk.squares
    finally:
        for o in (lim, bus, amx, b):
            o.close()
        for a in (src, shared, mixed):
            a.free()
