"""GPU: what the delay stage is for -- the published cmhip_*_delay() numbers put to use in two chains, each held to the
plain statement "the bus output is the input, delayed", bit for bit.

Mismatched bands: a band split (B = 2, T = 255) feeds band 0 through a dynamics object of smooth_log2 6 and band 1
through one of smooth_log2 8, both on the unity curve of creation; a Delay on band 0 of the difference of their delays
makes the two paths equal, a bus adds them at unity.  Parallel path: a source feeds a dynamics object and a Delay of
dyn.delay(); a bus adds the two at half weight each.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -21555
S = 3
BLOCKS = [[700, 0, 333], [1, 2000, 1999], [2000, 7, 8], [0, 0, 1234], [1500, 1501, 1]]     # five ragged blocks
MAXF = 2000


def pcm(cm, streams, stride):
    return cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=stride))


def noise(seed, frames, channels, scale):
    return np.random.default_rng(seed).integers(-scale, scale, size=(frames, channels)).astype(np.int16)


def delayed(fed, total, count, by, channels):
    """the last `count` frames of everything a stream was given (`fed`, `total` frames), `by` frames late"""
    z = np.concatenate([np.zeros((by, channels), dtype=np.int16)] + fed)
    return z[total - count:total]


@pytest.mark.parametrize("channels", [1, 2])
def test_bands_of_unequal_delay_add_up(gpu, channels):
    cm = gpu
    T, B = 255, 2
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    split = cm.BandSplit(S, channels, B, T, MAXF, rate=48000, crossover_hz=[1000.0])
    dyn0 = cm.Dynamics(S, channels, 6, 6, 0, MAXF)
    dyn1 = cm.Dynamics(S, channels, 6, 8, 0, MAXF)
    diff = dyn1.delay() - dyn0.delay()
    assert diff == 255 - 63 and split.delay() == 127
    delay = cm.Delay(S, channels, diff, MAXF, delay=diff)
    bus = cm.Bus(B * S, S, channels, channels, MAXF, B * S)
    bus.set_routing([s for b in range(B) for s in range(S)], [b * S + s for b in range(B) for s in range(S)],
                    [16384 * np.eye(channels, dtype=np.int16)] * (B * S))
    src, bands, comp, lined, out = (pcm(cm, n, stride) for n in (S, B * S, B * S, B * S, S))
    slot = stride * 2                                                    # bytes between slots
    try:
        fed, total = [[] for _ in range(S)], [0] * S
        for k, counts in enumerate(BLOCKS):
            frames = max(counts)
            xs = [noise(100 * k + s, n, channels, 8192) for s, n in enumerate(counts)]
            src.array[:] = 0x5a5a
            for s, x in enumerate(xs):
                src.array[s, :counts[s] * channels] = x.reshape(-1)
            out.array[:] = SENTINEL
            split.run(src.dev, stride, frames, bands.dev, stride, counts)
            split.sync()
            # band 0: dynamics (short ramp), then the delay that makes up the difference; band 1: dynamics (long ramp)
            dyn0.run(bands.dev, stride, frames, comp.dev, stride, counts)
            dyn0.sync()
            delay.run(comp.dev, stride, frames, lined.dev, stride, counts)
            delay.sync()
            dyn1.run(bands.dev + S * slot, stride, frames, lined.dev + S * slot, stride, counts)
            dyn1.sync()
            got = bus.run(lined.dev, stride, frames, out.dev, stride, counts * B)
            bus.sync()
            for s in range(S):
                fed[s].append(xs[s])
                total[s] += counts[s]
                want = delayed(fed[s], total[s], counts[s], split.delay() + 255, channels)
                n = counts[s] * channels
                assert got[s] == counts[s]
                assert np.array_equal(out.array[s, :n].reshape(-1, channels), want), ("block", k, "stream", s)
                assert (out.array[s, n:] == SENTINEL).all()
        assert (split.clips() == 0).all()
    finally:
        for o in (split, dyn0, dyn1, delay, bus):
            o.close()
        for a in (src, bands, comp, lined, out):
            a.free()


@pytest.mark.parametrize("channels", [1, 2])
def test_parallel_path_adds_up(gpu, channels):
    cm = gpu
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    dyn = cm.Dynamics(S, channels, 7, 7, 0, MAXF)
    D = dyn.delay()
    delay = cm.Delay(S, channels, D, MAXF, delay=D)
    bus = cm.Bus(2 * S, S, channels, channels, MAXF, 2 * S)
    bus.set_routing([s for b in range(2) for s in range(S)], [b * S + s for b in range(2) for s in range(S)],
                    [8192 * np.eye(channels, dtype=np.int16)] * (2 * S))
    src, both, out = pcm(cm, S, stride), pcm(cm, 2 * S, stride), pcm(cm, S, stride)
    slot = stride * 2
    try:
        fed, total = [[] for _ in range(S)], [0] * S
        for k, counts in enumerate(BLOCKS):
            frames = max(counts)
            xs = [noise(7000 + 100 * k + s, n, channels, 32768) for s, n in enumerate(counts)]
            src.array[:] = 0x5a5a
            for s, x in enumerate(xs):
                src.array[s, :counts[s] * channels] = x.reshape(-1)
            out.array[:] = SENTINEL
            dyn.run(src.dev, stride, frames, both.dev, stride, counts)            # the wet path: unity curve
            dyn.sync()
            delay.run(src.dev, stride, frames, both.dev + S * slot, stride, counts)   # the dry path, as late
            delay.sync()
            got = bus.run(both.dev, stride, frames, out.dev, stride, counts * 2)
            bus.sync()
            for s in range(S):
                fed[s].append(xs[s])
                total[s] += counts[s]
                want = delayed(fed[s], total[s], counts[s], D, channels)
                n = counts[s] * channels
                assert got[s] == counts[s]
                assert np.array_equal(out.array[s, :n].reshape(-1, channels), want), ("block", k, "stream", s)
                assert (out.array[s, n:] == SENTINEL).all()
    finally:
        for o in (dyn, delay, bus):
            o.close()
        for a in (src, both, out):
            a.free()
