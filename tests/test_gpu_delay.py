"""GPU: the delay stage (cmhip_delay_*, csrc/k_delay.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy model below of the arithmetic include/coolmic_hip.h specifies -- one list of all the
samples a stream was ever given, a delay d(n) per frame, the crossfade in int64 -- never another run of the device code;
what a run does not own of the output keeps its sentinel.  tests/test_delay_host.py runs the same model against its
emulation of the kernel's decomposition, without a GPU.

The tile comes from plan_delay: with t the plan's tile, counts are ragged over {0, 1, 7, 8, t-1, t, t+1, 2t+5} with
max_frames = 2t+5, delays step through {0, 1, 2, 3, 4, 7, 8, 9, t-1, t, t+1, max_delay} (for mono every misalignment of
the source), max_delay in {0, 9, t+1, 3t} -- the last longer than any run, so whole runs come from the ring -- and a case
runs until every stream has passed twice round its ring.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
CHANNELS = [1, 2, 3, 5, 6, 16]
RAMP_MAX = 1 << 20


def ramp_position(k, R):
    """cmhip_mix_ramp_position for arrays: p(k) = min(32768, (min(k, R) * ceil(2^32 / R)) >> 17), R >= 2"""
    inc = ((1 << 32) + R - 1) // R
    return np.minimum(32768, (np.minimum(np.asarray(k, dtype=np.int64), R) * inc) >> 17)


def crossfade(a, b, p):
    """the header's formula in int64: (a (32768 - p) + b p + 16384) >> 15"""
    a, b, p = (np.asarray(v, dtype=np.int64) for v in (a, b, p))
    N = a * (32768 - p) + b * p
    assert np.abs(N).max(initial=0) <= 2 ** 30
    return (N + 16384) >> 15


class Model:
    """one stream: every sample it was ever given, the delay per frame, set / ramp / reset as the header states them"""

    def __init__(self, channels, max_delay):
        self.C, self.max_delay = channels, max_delay
        self.x = np.zeros((max_delay, channels), dtype=np.int64)      # (frames before the first are zero)
        self.d1 = self.d0 = self.R = self.done = 0

    def ramping(self):
        return self.done < self.R

    def set(self, d):
        assert d <= self.max_delay
        self.d1 = self.d0 = d
        self.R = self.done = 0

    def ramp(self, d, R):
        """-> False where the library answers COOLMIC_ERROR_BUSY"""
        assert d <= self.max_delay and R <= RAMP_MAX
        if R < 2:
            self.set(d)
        elif self.ramping():
            return False
        else:
            self.d0, self.d1, self.R, self.done = self.d1, d, R, 0
        return True

    def get(self):
        return (self.d1, self.d0, self.done, self.R) if self.ramping() else (self.d1, self.d1, 0, 0)

    def reset(self):
        self.x[:] = 0

    def run(self, x):
        """x: int16 [F][C] -> int16 [F][C]"""
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.C)
        F, n0 = x.shape[0], self.x.shape[0]
        self.x = np.concatenate([self.x, x])
        n = n0 + np.arange(F)
        if self.ramping():
            p = ramp_position(self.done + 1 + np.arange(F), self.R)[:, None]
            y = crossfade(self.x[n - self.d0], self.x[n - self.d1], p)
            self.done = min(self.R, self.done + F)
            if not self.ramping():
                self.set(self.d1)
        else:
            y = self.x[n - self.d1]
        assert y.size == 0 or (y.min() >= -32768 and y.max() <= 32767)           # nothing saturates
        keep = self.max_delay                                                   # the state: the last max_delay frames
        self.x = self.x[self.x.shape[0] - keep:] if keep else self.x[:0]
        return y.astype(np.int16)


def noise(seed, frames, channels):
    """full-scale noise with planted frames of +32767 and -32768"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(frames, channels)).astype(np.int16)
    if frames:
        x[rng.integers(0, frames, size=frames // 16 + 1)] = 32767
        x[rng.integers(0, frames, size=frames // 16 + 1)] = -32768
    return x


def tile_of(cm, channels):
    p = cm.plan_delay(3, channels, 9, 64, 1)
    assert p.err == 0 and p.grid == 3 and p.fast == (1 if channels <= 2 else 0)
    return p.tile_frames


def counts_of(t):
    return [0, 1, 7, 8, t - 1, t, t + 1, 2 * t + 5]


def delays_of(t, max_delay):
    return [d for d in dict.fromkeys([0, 1, 2, 3, 4, 7, 8, 9, t - 1, t, t + 1, max_delay]) if d <= max_delay]


def max_delays_of(t):
    return [0, 9, t + 1, 3 * t]


class Rig:
    """a delay between two arrays of pinned, device-mapped host memory, and one model per stream"""

    def __init__(self, cm, streams, channels, max_delay, max_frames):
        self.cm, self.S, self.C = cm, streams, channels
        self.m = cm.Delay(streams, channels, max_delay, max_frames)
        assert self.m.max_delay() == max_delay
        self.ring = cm.plan_delay(streams, channels, max_delay, max_frames, 1).ring_frames
        self.in_stride = (max_frames * channels + 7) // 8 * 8 + 8            # wider than any run
        self.out_stride = (max_frames * channels + 7) // 8 * 8 + 16
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.models = [Model(channels, max_delay) for _ in range(streams)]
        self.given = [0] * streams                                           # frames per stream so far

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def set(self, stream, d):
        self.m.set(stream, d)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].set(d)

    def ramp(self, stream, d, R):
        """the library's answer must be the model's: BUSY when a named stream ramps, and then nothing changes"""
        names = list(range(self.S)) if stream < 0 else [stream]
        busy = R >= 2 and any(self.models[s].ramping() for s in names)
        rc = self.m.ramp_rc(stream, d, R)
        assert rc == (self.cm.ERROR_BUSY if busy else 0), (rc, busy)
        if not busy:
            for s in names:
                assert self.models[s].ramp(d, R)
        self.check_get()
        return not busy

    def reset(self, stream=-1):
        self.m.reset(stream)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].reset()

    def check_get(self):
        for s in range(self.S):
            assert self.m.get(s) == self.models[s].get(), s

    def run(self, xs, uniform=False):
        """xs: per stream int16 [F_s][C]; runs device and models, compares outputs and the untouched rest
        -> per stream the model's int16 [F_s][C]"""
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        frames = max(counts)
        self.src.array[:] = 0x5a5a
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        self.dst.array[:] = SENTINEL
        self.m.run(self.src.dev, self.in_stride, frames, self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = []
        for s, x in enumerate(xs):
            want = self.models[s].run(x)
            n = counts[s] * self.C
            row = self.dst.array[s]
            have = row[:n].reshape(-1, self.C)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(), "of", counts[s],
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (row[n:] == SENTINEL).all(), ("stream", s, "written past its count")
            self.given[s] += counts[s]
            wants.append(want)
        self.check_get()
        return wants


def rotate(counts, k, streams):
    """run k of a case: stream s gets count number k + 3 s of the list, so every stream meets every count"""
    return [counts[(k + 3 * s) % len(counts)] for s in range(streams)]


def test_refusals_of_a_real_object(gpu):
    """the checks tests/test_delay_host.py makes on an object without a device, on one with"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("test_delay_host_for_gpu", os.path.join(os.path.dirname(__file__), "test_delay_host.py"))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    d = gpu.Delay(3, 2, 9, 64)
    try:
        host.check_object_refusals(gpu, d)
    finally:
        d.close()


# ---------------------------------------------------------------------------
# steps

@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("which", range(4))
def test_steps_between_runs(gpu, which, channels):
    """every stream steps to another delay before every run, up and down, through ragged runs, until each has passed
    twice round its ring"""
    cm = gpu
    t = tile_of(cm, channels)
    max_delay = max_delays_of(t)[which]
    counts, delays = counts_of(t), delays_of(t, max_delay)
    S = 3 + which % 3
    rig = Rig(cm, S, channels, max_delay, 2 * t + 5)
    try:
        k = 0
        while min(rig.given) < 2 * rig.ring or k < 2 * len(delays):
            for s in range(S):
                rig.set(s, delays[(5 * k + 7 * s) % len(delays)])        # 5 and 7: up and down, all of them (12 at most)
            rig.run([noise(100 * k + s, n, channels) for s, n in enumerate(rotate(counts, k, S))])
            k += 1
            assert k < 200
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_step_up_reads_older_samples_and_reset_reads_zeros(gpu, channels):
    cm = gpu
    t = tile_of(cm, channels)
    max_delay = t + 1
    rig = Rig(cm, 3, channels, max_delay, 2 * t + 5)
    try:
        first = [noise(40 + s, t + 9, channels) for s in range(3)]
        rig.run(first)                                                   # d = 0: a copy
        rig.set(-1, max_delay)
        wants = rig.run([noise(50 + s, 2 * t + 5 - s, channels) for s in range(3)])
        for s in range(3):                                               # the step up reads what the first run put in
            assert np.array_equal(wants[s][:max_delay], first[s][t + 9 - max_delay:]), s
            assert np.abs(wants[s][:max_delay].astype(np.int64)).max() > 0
        rig.reset(1)
        wants = rig.run([noise(60 + s, t, channels) for s in range(3)], uniform=True)
        assert (wants[1] == 0).all() and (wants[0] != 0).any() and (wants[2] != 0).any()
        assert rig.m.get(1) == (max_delay, max_delay, 0, 0)              # the setting stays
        rig.set(-1, 0)
        rig.reset()
        rig.run([noise(70 + s, 8, channels) for s in range(3)])
    finally:
        rig.close()


def test_three_hundred_streams(gpu):
    cm = gpu
    channels, S = 2, 300
    t = tile_of(cm, channels)
    max_delay = t + 1
    counts, delays = counts_of(t), delays_of(t, max_delay)
    rng = np.random.default_rng(300)
    rig = Rig(cm, S, channels, max_delay, 2 * t + 5)
    try:
        for k in range(4):
            for s in range(S):
                rig.set(s, delays[int(rng.integers(len(delays)))])
            if k == 2:
                for s in range(0, S, 3):
                    rig.ramp(s, delays[int(rng.integers(len(delays)))], [2, 8, t + 1][s % 3])
            rig.run([noise(1000 * k + s, counts[int(rng.integers(len(counts)))], channels) for s in range(S)])
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# ramps

@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("R", ["2", "3", "8", "t+1", "32769"])
def test_ramps_across_cuts(gpu, R, channels):
    """crossfades up, down and on the spot (d0 = d1: the identity), across ragged cuts and runs of no frames; a second
    ramp is BUSY while one runs and changes nothing; cmhip_delay_get follows the ramp through every run"""
    cm = gpu
    t = tile_of(cm, channels)
    R = t + 1 if R == "t+1" else int(R)
    max_delay = 3 * t
    counts, delays = counts_of(t), delays_of(t, max_delay)
    S = 4
    rig = Rig(cm, S, channels, max_delay, 2 * t + 5)
    try:
        for s in range(S):
            rig.set(s, delays[-1 - s])
        rig.run([noise(s, t + 9, channels) for s in range(S)])           # something in every ring
        k, ramps, wanted = 0, 0, (S if R > 2 * t else 3 * S)             # (a long ramp takes many runs: one per stream)
        big = [2 * t + 5, 2 * t + 5, t + 1, 0]                           # long ramps: long runs, one stream idles in turn
        while ramps < wanted or any(m.ramping() for m in rig.models):
            for s in range(S):
                if not rig.models[s].ramping() and ramps < wanted:
                    kind = (ramps + s) % 3                               # 0: up, 1: down, 2: d0 = d1
                    d0 = rig.models[s].d1
                    ups = [d for d in delays if d > d0] or [d0]
                    downs = [d for d in delays if d < d0] or [d0]
                    target = d0 if kind == 2 else ups[(k + s) % len(ups)] if kind == 0 else downs[(k + s) % len(downs)]
                    assert rig.ramp(s, target, R)
                    ramps += 1
                elif rig.models[s].ramping() and k % 2:
                    assert not rig.ramp(s, delays[k % len(delays)], 5)   # BUSY: the model's state is compared in ramp()
            cs = rotate(big, k, S) if R > 2 * t else rotate(counts, k, S)
            rig.run([noise(500 + 10 * k + s, n, channels) for s, n in enumerate(cs)])
            k += 1
            assert k < 1000
        for s in range(S):
            assert rig.m.get(s)[2:] == (0, 0)
        rig.run([noise(900 + s, 7, channels) for s in range(S)])         # behind the ramps: the target, exactly
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 16])
def test_identity_ramp_is_the_delayed_input(gpu, channels):
    cm = gpu
    t = tile_of(cm, channels)
    rig = Rig(cm, 3, channels, t + 1, 2 * t + 5)
    try:
        rig.set(-1, 9)
        fed = [noise(s, t, channels) for s in range(3)]
        rig.run(fed)
        assert rig.ramp(-1, 9, t + 1)
        xs = [noise(10 + s, t - s, channels) for s in range(3)]
        wants = rig.run(xs)
        for s in range(3):
            z = np.concatenate([fed[s], xs[s]])
            assert np.array_equal(wants[s], z[t - 9:t - 9 + t - s]), s
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_full_scale_square_wave_through_a_ramp(gpu, channels):
    """a square wave of period 2 d puts -32768 on one tap and 32767 on the other for the whole ramp"""
    cm = gpu
    t = tile_of(cm, channels)
    d = 8
    rig = Rig(cm, 3, channels, d, 2 * t + 5)
    try:
        def square(first, frames):
            n = first + np.arange(frames)
            return np.where((n // d) % 2 == 0, -32768, 32767).astype(np.int16)[:, None].repeat(channels, axis=1)

        rig.run([square(0, t + 3)] * 3)
        for s, R in enumerate([2, 8, t + 1]):
            assert rig.ramp(s, d, R)
        wants = rig.run([square(t + 3, 2 * t + 5)] * 3)
        for s, R in enumerate([2, 8, t + 1]):
            w = wants[s].astype(np.int64)
            assert w.min() == -32768 and w.max() == 32767
            inside = w[:R - 1]
            assert ((inside > -32768) & (inside < 32767)).any(), s      # the fade passes through the middle
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_set_cancels_a_ramp(gpu, channels):
    cm = gpu
    t = tile_of(cm, channels)
    rig = Rig(cm, 3, channels, t + 1, 2 * t + 5)
    try:
        rig.run([noise(s, t + 1, channels) for s in range(3)])
        assert rig.ramp(-1, t + 1, 4 * t)
        rig.run([noise(10 + s, [t - 1, 0, 7][s], channels) for s in range(3)])
        assert rig.m.get(0) == (t + 1, 0, t - 1, 4 * t) and rig.m.get(1) == (t + 1, 0, 0, 4 * t)
        rig.set(0, 3)                                                    # ends the ramp and steps
        assert rig.m.get(0) == (3, 3, 0, 0) and rig.m.get(2) == (t + 1, 0, 7, 4 * t)
        assert rig.ramp(0, 7, 3) and not rig.ramp(2, 1, 2) and not rig.ramp(-1, 1, 2)
        assert rig.ramp(2, 1, 1)                                         # R = 1 is a set: never BUSY
        rig.run([noise(20 + s, t + 1, channels) for s in range(3)])
        rig.run([noise(30 + s, 2 * t + 5, channels) for s in range(3)], uniform=True)
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# cuts

@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_output_does_not_depend_on_the_cuts(gpu, channels):
    """the same streams, sets and ramps at the same frames: once in long runs, once in many ragged ones"""
    cm = gpu
    t = tile_of(cm, channels)
    max_delay, total = t + 1, 3 * (2 * t + 5)
    xs = [noise(77 + s, total, channels) for s in range(3)]
    events = {0: ("set", 7), t + 9: ("ramp", t + 1, t + 1), 2 * t + 5: ("cut",), 3 * t + 2: ("set", 2),
              3 * t + 10: ("ramp", 9, 8), 4 * t + 5: ("cut",), 5 * t + 8: ("cut",)}

    def play(cuts):
        rig = Rig(cm, 3, channels, max_delay, 2 * t + 5)
        try:
            out, at, due = [[] for _ in range(3)], 0, dict(events)
            for n in cuts:
                ev = due.pop(at, None)                                   # (once: a cut of no frames stays at its frame)
                if ev and ev[0] == "set":
                    rig.set(-1, ev[1])
                elif ev and ev[0] == "ramp":
                    assert rig.ramp(-1, ev[1], ev[2])
                for s, w in enumerate(rig.run([x[at:at + n] for x in xs])):
                    out[s].append(w)
                at += n
            assert at == total
            return [np.concatenate(o) for o in out]
        finally:
            rig.close()

    edges = sorted(events) + [total]
    long_cuts = [b - a for a, b in zip(edges, edges[1:])]
    ragged = []
    for n in long_cuts:                                                  # each long run cut again: 1, 0, 7, 8, t - 1, the rest
        rest = n
        for c in (1, 0, 7, 8, t - 1):
            if c <= rest:
                ragged.append(c)
                rest -= c
        ragged.append(rest)
    assert sum(ragged) == total and max(long_cuts) <= 2 * t + 5
    a, b = play(long_cuts), play(ragged)
    for s in range(3):
        assert np.array_equal(a[s], b[s]), s
