"""GPU: the band split (cmhip_split_*, csrc/k_split.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy model below of the arithmetic include/coolmic_hip.h specifies -- int64, per-stream
history, clip counters -- never another run of the device code.  Tables are taken from the library
(cmhip_split_design), or are the test's own where the test is about a table: a designed filter's outer taps are next to
nothing, so whatever a kernel does wrong at the ends of a filter, in the oldest history frames or at a group boundary
adds little to its sums.  dense_table() gives every tap weight.  tests/test_split_host.py runs the same cases through
its emulation of the kernel's decomposition, without a GPU.

The tile comes from plan_split: with t the plan's tile, the streams' counts are ragged over
{0, 1, D, T-1, T, t-1, t, t+1, 2t+5}, three streams in three consecutive runs, so every stream also carries history
from one run into the next.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
RATE = 48000
CROSSOVERS = {2: [1000.0], 3: [300.0, 3000.0], 8: [100.0, 200.0, 400.0, 800.0, 1600.0, 3200.0, 6400.0]}
S = 3


class Model:
    """one stream: r_b = (sum_k g_b[k] x[n-k] + 2^(q_b-1)) >> q_b, y_b = sat16(r_b), y_last = sat16(x[n-D] - sum r_b)"""

    def __init__(self, g, q, channels):
        self.g, self.q, self.C = np.asarray(g, dtype=np.int64), [int(v) for v in q], channels
        self.nf, self.T = self.g.shape
        self.D = (self.T - 1) // 2
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.T - 1, self.C), dtype=np.int64)
        self.clips = np.zeros(self.nf + 1, dtype=np.int64)

    def run(self, x):
        """x: int16 [F][C] -> int16 [B][F][C]; history and clip counters move on"""
        T, D = self.T, self.D
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.C)
        F = x.shape[0]
        z = np.concatenate([self.hist, x])
        r = np.zeros((self.nf + 1, F, self.C), dtype=np.int64)
        r[self.nf] = z[T - 1 - D:T - 1 - D + F]
        for b in range(self.nf):
            for c in range(self.C):
                acc = np.convolve(z[:, c], self.g[b])[T - 1:T - 1 + F] if F else np.zeros(0, dtype=np.int64)
                assert acc.dtype == np.int64 and (acc.size == 0 or np.abs(acc).max() < 2 ** 41)
                r[b, :, c] = (acc + (1 << (self.q[b] - 1))) >> self.q[b]
            r[self.nf] -= r[b]
        y = np.clip(r, -32768, 32767)
        self.clips += (y != r).sum(axis=(1, 2))
        self.hist = z[z.shape[0] - (T - 1):]
        return y.astype(np.int16)


def counts_for(t, T):
    D = (T - 1) // 2
    return [0, 1, D, T - 1, T, t - 1, t, t + 1, 2 * t + 5]


def runs_for(t, T):
    """three runs of three streams over the nine counts: stream s gets counts s, 3 + s, 6 + s"""
    c = counts_for(t, T)
    return [c[0:3], c[3:6], c[6:9]]


def noise(seed, frames, channels, scale=32768):
    rng = np.random.default_rng(seed)
    x = rng.integers(-scale, scale, size=(frames, channels)).astype(np.int16)
    if scale == 32768 and frames:
        x[rng.integers(0, frames, size=frames // 16 + 1)] = 32767              # full-scale frames here and there
        x[rng.integers(0, frames, size=frames // 16 + 1)] = -32768
    return x


def dense_table(bands, T, seed):
    """every tap non-zero, random signs, each q_b random in 14..20; the magnitudes of a filter lie in [A/2, A] with A
    chosen so that r_b has an RMS near 3000 on full-scale noise: most outputs stay unsaturated, and a wrong sum shows"""
    rng = np.random.default_rng(seed)
    q = rng.integers(14, 21, size=bands - 1).astype(np.uint8)
    g = np.zeros((bands - 1, T), dtype=np.int16)
    for b in range(bands - 1):
        A = int(min(32767, max(2, 0.21 * 2.0 ** int(q[b]) / np.sqrt(T))))
        g[b] = rng.integers(-(-A // 2), A + 1, size=T) * rng.choice([-1, 1], size=T)
    assert (g != 0).all()
    return g, q


_designed = {}


def designed(cm, bands, T):
    if (bands, T) not in _designed:
        _designed[(bands, T)] = cm.split_design(RATE, bands, CROSSOVERS[bands], T)
    return _designed[(bands, T)]


class Rig:
    """a band split between two arrays of pinned, device-mapped host memory, and one model per stream"""

    def __init__(self, cm, streams, channels, g, q, max_frames):
        self.cm, self.S, self.C = cm, streams, channels
        self.g, self.q = np.asarray(g, dtype=np.int16), np.asarray(q, dtype=np.uint8)
        self.B, self.T = self.g.shape[0] + 1, self.g.shape[1]
        self.m = cm.BandSplit(streams, channels, self.B, self.T, max_frames, table=(self.g, self.q))
        assert self.m.delay() == (self.T - 1) // 2
        tg, tq = self.m.get_table()
        assert np.array_equal(tg, self.g) and np.array_equal(tq, self.q)
        self.in_stride = (max_frames * channels + 7) // 8 * 8 + 8          # wider than any run
        self.out_stride = (max_frames * channels + 7) // 8 * 8 + 16
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=self.B * streams, stride=self.out_stride))
        self.models = [Model(self.g, self.q, channels) for _ in range(streams)]

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def run(self, xs, uniform=False):
        """xs: per stream int16 [F_s][C]; runs device and models, compares the bands and the untouched rest
        -> per stream the model's int16 [B][F_s][C]"""
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
            for b in range(self.B):
                row = self.dst.array[b * self.S + s]
                have = row[:n].reshape(-1, self.C)
                bad = np.argwhere(have != want[b])
                assert bad.size == 0, ("stream", s, "band", b, "first mismatch (frame, channel)", bad[0].tolist(),
                                       "got", int(have[tuple(bad[0])]), "want", int(want[b][tuple(bad[0])]))
                assert (row[n:] == SENTINEL).all(), ("stream", s, "band", b, "written past its count")
            wants.append(want)
        return wants

    def check_clips(self):
        want = np.array([m.clips for m in self.models], dtype=np.int64) % 2 ** 32
        got = self.m.clips()
        assert np.array_equal(got.astype(np.int64), want), (got.tolist(), want.tolist())
        return want

    def reset(self, stream=-1):
        self.m.reset(stream)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].reset()


def tile_of(cm, channels, bands, T):
    p = cm.plan_split(S, channels, bands, T, 1)
    assert p.err == 0 and p.grid == S and p.fast == (1 if channels <= 2 else 0)
    return p.tile_frames


# ---------------------------------------------------------------------------
# designed tables: the bands add up, by themselves and through a real bus

@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("bands", [2, 3, 8])
@pytest.mark.parametrize("T", [3, 31, 255, 1023])
def test_designed_tables_reconstruct(gpu, T, bands, channels):
    cm = gpu
    g, q = designed(cm, bands, T)
    t = tile_of(cm, channels, bands, T)
    D = (T - 1) // 2
    runs = runs_for(t, T)
    rig = Rig(cm, S, channels, g, q, 2 * t + 5)
    bus = cm.Bus(bands * S, S, channels, channels, 2 * t + 5, bands * S)
    bus.set_routing([s for b in range(bands) for s in range(S)], [b * S + s for b in range(bands) for s in range(S)],
                    [16384 * np.eye(channels, dtype=np.int16)] * (bands * S))
    summed = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    try:
        fed = [np.zeros((D, channels), dtype=np.int16) for _ in range(S)]        # every stream's input so far, behind D zeros
        for k, counts in enumerate(runs):
            xs = [noise(1000 * T + 10 * k + s, n, channels, scale=8192) for s, n in enumerate(counts)]
            wants = rig.run(xs)
            summed.array[:] = SENTINEL
            got = bus.run(rig.dst.dev, rig.out_stride, max(counts), summed.dev, rig.out_stride, counts * bands)
            bus.sync()
            for s in range(S):
                before = fed[s].shape[0] - D
                fed[s] = np.concatenate([fed[s], xs[s]])
                delayed = fed[s][before:before + counts[s]]
                assert np.array_equal(wants[s].astype(np.int64).sum(axis=0), delayed), ("model", s)
                assert got[s] == counts[s]
                n = counts[s] * channels
                assert np.array_equal(summed.array[s, :n].reshape(-1, channels), delayed), ("bus", s)
                assert (summed.array[s, n:] == SENTINEL).all()
        assert all((m.clips == 0).all() for m in rig.models)         # the condition of exact reconstruction, on the model
        assert (rig.check_clips() == 0).all()
    finally:
        summed.free()
        bus.close()
        rig.close()


@pytest.mark.parametrize("T,bands,channels", [(3, 2, 1), (31, 3, 2), (255, 8, 1), (1023, 3, 2)])
def test_constant_input(gpu, T, bands, channels):
    cm = gpu
    g, q = designed(cm, bands, T)
    t = tile_of(cm, channels, bands, T)
    rig = Rig(cm, S, channels, g, q, t + T)
    try:
        consts = [[12345, -32768][:channels], [-7, 32767][:channels], [32767, 1][:channels]]
        xs = [np.tile(np.array(c, dtype=np.int16), (t + T - s, 1)) for s, c in enumerate(consts)]
        wants = rig.run(xs)
        for s, want in enumerate(wants):
            assert np.array_equal(want[0, T - 1:], xs[s][T - 1:]), s
            assert (want[1:, T - 1:] == 0).all(), s
        rig.check_clips()
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# dense tables: every tap, the int64 path, the int32 edge

def edge_tables(kind, T):
    """-> (g int16 [B-1][T], q uint8 [B-1])"""
    if kind == "max":                  # all taps +32767 / all -32767: groups of two taps, sums near 2^40
        return (np.array([[32767] * T, [-32767] * T], dtype=np.int16), np.array([20, 17], dtype=np.uint8))
    if kind == "one-group":            # sum |g| = 65535 exactly, q = 14: one group each; all negative, all positive, mixed
        mag = np.full(T, 65535 // T, dtype=np.int64)
        mag[: 65535 - int(mag.sum())] += 1
        assert mag.sum() == 65535
        sign = np.where(np.arange(T) % 3 == 0, -1, 1)
        return (np.array([-mag, mag, mag * sign], dtype=np.int16), np.array([14, 14, 14], dtype=np.uint8))
    if kind == "min-pairs":            # pairs of -32768: a pair's sum reaches +2^31 against two samples of -32768
        g = np.full((1, T), -32768, dtype=np.int16)
        g[0, 5] = 17
        return g, np.array([19], dtype=np.uint8)
    raise ValueError(kind)


def edge_input(kind, g, seed, frames, channels):
    """full-scale noise with stretches that reach the edge: all -32768, and the sign-matched pattern of filter 2"""
    x = noise(seed, frames, channels)
    T = g.shape[1]
    if frames >= 3 * T:
        x[T // 2:T // 2 + 2 * T] = -32768
        if kind == "one-group":
            # output n = frames - 1 of filter 2 meets x[n-k] = -32768 where g[k] < 0 and 32767 where g[k] > 0, and the
            # frame before it the opposite signs
            pat = np.where(g[2][::-1] < 0, -32768, 32767).astype(np.int16)
            x[frames - T:] = pat[:, None]
            x[frames - 2 * T:frames - T] = np.where(pat < 0, 32767, -32768).astype(np.int16)[:, None]
    return x


DENSE = [("dense", 3, 2, 1), ("dense", 31, 3, 2), ("dense", 255, 8, 1), ("dense", 255, 3, 2), ("dense", 1023, 3, 2),
         ("dense", 1023, 2, 1), ("max", 1023, 3, 1), ("max", 255, 3, 2), ("one-group", 31, 4, 1), ("one-group", 255, 4, 2),
         ("min-pairs", 31, 2, 1), ("min-pairs", 1023, 2, 2)]


def dense_case(kind, T, bands, seed):
    return dense_table(bands, T, seed) if kind == "dense" else edge_tables(kind, T)


@pytest.mark.parametrize("kind,T,bands,channels", DENSE)
def test_dense_tables(gpu, kind, T, bands, channels):
    cm = gpu
    g, q = dense_case(kind, T, bands, 77 + T + bands)
    assert g.shape[0] == bands - 1
    t = tile_of(cm, channels, bands, T)
    rig = Rig(cm, S, channels, g, q, 2 * t + 5)
    try:
        total = 0
        for k, counts in enumerate(runs_for(t, T)):
            xs = [edge_input(kind, g, 500 + 10 * k + s, n, channels) for s, n in enumerate(counts)]
            assert any((x == -32768).any() for x in xs)
            for want in rig.run(xs):
                total += want.size
        clips = rig.check_clips()
        assert clips.sum() > 0                                           # the counters are exercised ...
        if kind == "dense":
            assert clips.sum() < 0.25 * total                            # ... and most outputs show their sums
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# cuts, zero-frame runs, resets

@pytest.mark.parametrize("T,bands,channels", [(31, 3, 1), (255, 2, 2), (1023, 3, 1)])
def test_cuts_do_not_matter(gpu, T, bands, channels):
    cm = gpu
    g, q = dense_table(bands, T, 9 + T)
    t = tile_of(cm, channels, bands, T)
    D = (T - 1) // 2
    cuts = [1] * 5 + [D, T - 2, 1, 1, T - 1, T, 0, t + 1, 2, D, 1, 1, 1, T - 2, 3]
    N = sum(cuts)
    x = [noise(40 + s, N, channels) for s in range(S)]
    whole = Rig(cm, S, channels, g, q, N)
    parts = Rig(cm, S, channels, g, q, t + T + 8)
    assert len(cuts) % 2 == 0
    try:
        want = whole.run(x, uniform=True)
        want_clips = whole.check_clips()
        at = [0] * S
        got = [[] for _ in range(S)]
        for k, n in enumerate(cuts):
            # streams 0 and 2 are cut as listed; stream 1 sits out every even run (a stream with 0 frames keeps its
            # history) and takes both runs' frames in the odd one
            take = [n, 0 if k % 2 == 0 else cuts[k - 1] + n, n]
            for s, y in enumerate(parts.run([x[s][at[s]:at[s] + take[s]] for s in range(S)])):
                got[s].append(y)
                at[s] += take[s]
        for s in range(S):
            assert np.array_equal(np.concatenate(got[s], axis=1), want[s]), s
        assert np.array_equal(parts.check_clips(), want_clips)
    finally:
        whole.close()
        parts.close()


def test_zero_frame_streams_and_resets(gpu):
    cm = gpu
    T, bands, channels = 255, 3, 2
    g, q = dense_table(bands, T, 4)
    rig = Rig(cm, S, channels, g, q, 600)
    try:
        rig.run([noise(1 + s, 600, channels) for s in range(S)])
        rig.run([noise(11, 300, channels), np.zeros((0, channels), dtype=np.int16), noise(13, 7, channels)])
        rig.run([np.zeros((0, channels), dtype=np.int16), noise(22, 100, channels), np.zeros((0, channels), dtype=np.int16)])
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride) == 0     # a run of nothing
        rig.run([noise(31 + s, 50, channels) for s in range(S)])
        assert rig.check_clips().sum() > 0
        rig.reset(1)                                                    # one stream: history and counters
        assert (rig.check_clips()[1] == 0).all() and rig.check_clips()[0].sum() > 0
        rig.run([noise(41 + s, 200, channels) for s in range(S)])
        rig.check_clips()
        rig.reset()                                                     # all of them
        assert (rig.check_clips() == 0).all()
        rig.run([noise(51 + s, 200, channels) for s in range(S)])
        before = rig.check_clips()
        assert before.sum() > 0 and np.array_equal(rig.m.clips(clear=True).astype(np.int64), before)
        assert (rig.m.clips() == 0).all()                               # read and cleared in one round trip
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# channel forms and the grid

@pytest.mark.parametrize("channels", [3, 6, 16])
def test_any_channel_count(gpu, channels):
    cm = gpu
    T, bands = 63, 3
    g, q = dense_table(bands, T, 100 + channels)
    t = tile_of(cm, channels, bands, T)
    rig = Rig(cm, S, channels, g, q, 2 * t + 5)
    try:
        for k, counts in enumerate(runs_for(t, T)):
            rig.run([noise(700 + 10 * k + s, n, channels) for s, n in enumerate(counts)])
        rig.check_clips()
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_many_streams(gpu, channels):
    cm = gpu
    T, bands, streams = 15, 3, 300
    g, q = dense_table(bands, T, 3)
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 400, size=streams).tolist()
    counts[0], counts[-1] = 399, 398
    rig = Rig(cm, streams, channels, g, q, 400)
    try:
        rig.run([noise(s, n, channels) for s, n in enumerate(counts)])
        rig.run([noise(900 + s, n, channels) for s, n in enumerate(reversed(counts))])
        rig.check_clips()
    finally:
        rig.close()
