"""GPU: clock-drift compensation (cmhip_drift_*, csrc/k_drift.hip) through the C ABI and the Python mirror.

Bar: bit-exact against tests/drift_model.py, the numpy model of the arithmetic include/coolmic_hip.h specifies -- never
another run of the device code.  The tables are dense (every |h| in [3B/4, B], random signs): a designed table's edge
taps are 2-3 units and would let a mistake at the ends of the filter -- the oldest history frame, the oldest frame of a
tile's halo, the last tap pair -- through; full-scale noise goes in, and every case asserts that under a tenth of the
model's outputs are saturated.  What makes a case reach its path (the table in LDS or read through the caches, the
number of tiles) is asserted from the plan (tests/test_drift_host.py runs an emulation of the kernel over the same kind
of cases without a GPU)."""
import types

import numpy as np
import pytest

import drift_model as DM

pytestmark = pytest.mark.gpu
ONE, DMAX = DM.ONE, DM.DELTA_MAX
SENTINEL = -21555                                 # what the output slots hold before a run
SATURATED_MAX = 0.10


def noise(rng, frames, channels):
    x = rng.integers(-32768, 32768, size=(frames, channels))
    if frames >= 16:
        x[rng.integers(0, frames, size=frames // 16)] = 32767            # full-scale frames here and there
        x[rng.integers(0, frames, size=frames // 16)] = -32768
    return x.astype(np.int16)


class Slots:
    """two arrays of pinned, device-mapped host memory: a run's input and output slots"""

    def __init__(self, cm, streams, in_stride, out_stride):
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=out_stride))

    def free(self):
        self.src.free()
        self.dst.free()


class Rig:
    """a drift stage between slots, and the model"""

    def __init__(self, cm, streams, channels, H, max_in, slots=1):
        self.cm, self.S, self.C, self.H = cm, streams, channels, np.asarray(H, dtype=np.int16)
        self.d = cm.Drift(streams, channels, max_in, table=self.H)
        self.phi, self.T = self.d.geometry()
        assert (1 << self.phi, self.T) == self.H.shape
        self.max_out = self.d.max_out_frames()
        assert self.max_out == DM.out_frames(0, -DMAX, max_in)
        self.in_stride = (max_in * channels + 7) // 8 * 8
        self.out_stride = (self.max_out * channels + 7) // 8 * 8 + 8
        self.slots = [Slots(cm, streams, self.in_stride, self.out_stride) for _ in range(slots)]
        self.model = DM.DriftModel(streams, channels, self.H)

    def close(self):
        self.d.close()
        for sl in self.slots:
            sl.free()

    def set(self, s, delta):
        self.d.set(s, delta)
        self.model.set(s, delta)

    def seek(self, s, frac):
        self.d.seek(s, frac)
        self.model.seek(s, frac)

    def reset(self, s=-1):
        self.d.reset(s)
        self.model.reset(s)

    def queue(self, xs, slot=0, frames=None, uniform=False):
        """one run queued (no wait): -> what check() needs"""
        sl = self.slots[slot]
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        frames = max(counts) if frames is None else frames
        sl.src.array[:] = 0x5a5a
        for s, x in enumerate(xs):
            sl.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        sl.dst.array[:] = SENTINEL
        got = self.d.run(sl.src.dev, self.in_stride, frames, sl.dst.dev, self.out_stride, None if uniform else counts)
        want = self.model.run(xs)
        for s in range(self.S):
            assert got[s] == want[s].shape[0], (s, got[s], want[s].shape[0])
            assert self.d.get(s) == self.model.get(s), s
        return sl, want

    def check(self, queued):
        sl, want = queued
        outs = []
        for s in range(self.S):
            n = want[s].size
            have = sl.dst.array[s, :n].reshape(-1, self.C)
            bad = np.argwhere(have != want[s])
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(), "of", want[s].shape,
                                   "got", int(have[tuple(bad[0])]), "want", int(want[s][tuple(bad[0])]))
            assert (sl.dst.array[s, n:] == SENTINEL).all(), ("stream", s, "written past its count")
            outs.append(have.copy())
        return outs

    def run(self, xs, frames=None, uniform=False):
        q = self.queue(xs, 0, frames, uniform)
        self.d.sync()
        return self.check(q)

    def saturated_share(self):
        return self.model.saturated / max(self.model.outputs, 1)


def ragged(F, T):
    """per-stream counts of one run: a full stream, one with nothing, one frame, T - 2 frames, F - 1 frames"""
    return [F, 0, 1, T - 2, F - 1]


def plan_of(cm, rig, counts):
    """the plan of the run that gives the streams these counts, from the model's positions BEFORE the run"""
    most = max(DM.out_frames(rig.model.pos[s], rig.model.delta[s], counts[s]) for s in range(rig.S))
    return cm.plan_drift(rig.S, rig.C, rig.phi, rig.T, max(most, 1))


# ---------------------------------------------------------------------------
# channel forms x counts: every kernel, ragged counts, three runs on one history and position

DELTAS5 = [858993, -DMAX, DMAX, 1, -1]
SEEKS5 = [0, 1, ONE - 1, (5 << 25) - 1, 5 << 25]                 # ... and both sides of a row boundary (phi = 7)


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 6, 16])
def test_channel_forms_and_counts(gpu, channels):
    rng = np.random.default_rng(100 + channels)
    T, F = 32, 2300
    rig = Rig(gpu, 5, channels, DM.dense_table(rng, 7, T), F)
    try:
        for s in range(5):
            rig.set(s, DELTAS5[s])
            rig.seek(s, SEEKS5[s])
        first = ragged(F, T)
        p = plan_of(gpu, rig, first)
        assert p.table_lds == 1 and p.fast == (channels <= 2) and p.chunks >= 2
        assert p.tile_out == (2048 if channels <= 6 else 512)
        for counts in (first, first[::-1], first[2:] + first[:2]):
            rig.run([noise(rng, n, channels) for n in counts], frames=F)
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# delta x position

GRID_DELTAS = [0, 1, -1, DMAX, -DMAX, 12345, -7654321, 4294967]
# phi = 5: a row is 2^27 wide, a step of mu 2^12
GRID_SEEKS = [0, 1, ONE - 1, (3 << 27) - 1, 3 << 27, (3 << 27) + (1 << 12) - 1, (3 << 27) + (1 << 12)]


@pytest.mark.parametrize("channels", [1, 2])
def test_delta_and_position_grid(gpu, channels):
    rng = np.random.default_rng(200 + channels)
    S, F = len(GRID_DELTAS) * len(GRID_SEEKS), 300
    rig = Rig(gpu, S, channels, DM.dense_table(rng, 5, 8), F)
    try:
        for i, d in enumerate(GRID_DELTAS):
            for j, f in enumerate(GRID_SEEKS):
                rig.set(i * len(GRID_SEEKS) + j, d)
                rig.seek(i * len(GRID_SEEKS) + j, f)
        rig.run([noise(rng, F, channels) for _ in range(S)], uniform=True)
        rig.run([noise(rng, F - (s % 3), channels) for s in range(S)])
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_runs_without_an_output_and_with_one_more(gpu, channels):
    rng = np.random.default_rng(300 + channels)
    rig = Rig(gpu, 2, channels, DM.dense_table(rng, 6, 8), 255)
    try:
        rig.set(0, DMAX)
        rig.seek(0, ONE - 1)
        rig.set(1, -DMAX)
        counts = []
        for F in (1, 1, 1, 255):
            before = [rig.model.out_total[s] for s in range(2)]
            rig.run([noise(rng, F, channels), noise(rng, 255 if F == 255 else 0, channels)], frames=F)
            counts.append([rig.model.out_total[s] - before[s] for s in range(2)])
        # stream 0: its second frame arrives and gives nothing (pos was 2^32 - 1 + 2^24); stream 1: 255 in, 256 out
        assert [c[0] for c in counts[:3]] == [1, 0, 1] and counts[3][1] == 256
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# halos: T = 64 over a history that is only partly filled, the table read through the caches and from LDS

HALO_RUNS = [14, 1, 0, 14, 40, 50, 2300]


@pytest.mark.parametrize("channels,phi", [(1, 5), (2, 5), (2, 8), (3, 6), (16, 8)])
def test_halos(gpu, channels, phi):
    rng = np.random.default_rng(400 + channels + phi)
    rig = Rig(gpu, 2, channels, DM.dense_table(rng, phi, 64), max(HALO_RUNS))
    try:
        rig.set(0, -DMAX)
        rig.set(1, DMAX)
        rig.seek(1, ONE - 1)
        seen = set()
        # two streams: the list, and the list rotated by one run -- a different fill of the history per run
        for a, b in zip(HALO_RUNS, HALO_RUNS[1:] + HALO_RUNS[:1]):
            p = plan_of(gpu, rig, [a, b])
            most = max(DM.out_frames(rig.model.pos[s], rig.model.delta[s], n) for s, n in enumerate((a, b)))
            assert p.table_lds == (1 if 2 * min(most, p.tile_out) >= (1 << phi) + 1 else 0)
            seen.add((p.table_lds, p.chunks > 1))
            rig.run([noise(rng, a, channels), noise(rng, b, channels)])
        assert {(0, False), (1, True)} <= seen                       # short runs: global; the long one: LDS, 2+ tiles
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# cut invariance, set between runs, identity

@pytest.mark.parametrize("channels", [1, 2, 5])
def test_cut_invariance_and_set_between_runs(gpu, channels):
    rng = np.random.default_rng(500 + channels)
    F = 3000
    H = DM.dense_table(rng, 7, 16)
    x = noise(rng, F, channels)
    cuts = ([F], [1, 2047, 0, 952], [700, 33, 15, 1, 1, 2250])
    rig = Rig(gpu, len(cuts), channels, H, F)
    try:
        rig.set(-1, -3210987)
        rig.seek(-1, 987654321)
        at = [0] * len(cuts)
        outs = [[] for _ in cuts]
        for r in range(max(len(c) for c in cuts)):
            xs = []
            for i, c in enumerate(cuts):
                n = c[r] if r < len(c) else 0
                xs.append(x[at[i]:at[i] + n])
                at[i] += n
            for i, o in enumerate(rig.run(xs)):
                outs[i].append(o)
        whole = [np.concatenate(o) for o in outs]
        assert at == [F] * len(cuts) and whole[0].shape[0] == DM.out_frames(987654321, -3210987, F)
        assert (whole[0] == whole[1]).all() and (whole[0] == whole[2]).all()
        # a set between runs: the model's piecewise steps
        for d in (4294967, -DMAX, 0, DMAX):
            rig.set(1, d)
            rig.run([noise(rng, n, channels) for n in (500, 777, 0)])
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


@pytest.mark.parametrize("channels,T", [(1, 4), (2, 32), (6, 64)])
def test_identity(gpu, channels, T):
    """every row the unit at tap T/2, delta 0: the input delayed by T/2 frames, bit for bit"""
    rng = np.random.default_rng(600 + channels)
    F = 1000
    rig = Rig(gpu, 1, channels, DM.unit_table(5, T), F)
    try:
        x = noise(rng, 2 * F, channels)
        y = np.concatenate([rig.run([x[:F]])[0], rig.run([x[F:]])[0]])
        assert y.shape == x.shape and not y[:T // 2].any() and (y[T // 2:] == x[:2 * F - T // 2]).all()
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# set, seek and reset behind queued runs

def test_control_is_ordered_behind_queued_runs(gpu):
    rng = np.random.default_rng(700)
    S, F = 3, 2100
    rig = Rig(gpu, S, 2, DM.dense_table(rng, 7, 32), F, slots=4)
    try:
        rig.set(-1, 2000000)
        queued = [rig.queue([noise(rng, F, 2) for _ in range(S)], slot=0)]
        rig.set(0, -DMAX)                                            # behind run 0, in front of run 1
        rig.seek(1, ONE - 1)
        rig.reset(2)
        queued.append(rig.queue([noise(rng, F - s, 2) for s in range(S)], slot=1))
        rig.reset(-1)
        rig.set(2, DMAX)
        queued.append(rig.queue([noise(rng, 40 + s, 2) for s in range(S)], slot=2))
        rig.seek(-1, 1 << 31)
        queued.append(rig.queue([noise(rng, F, 2) for _ in range(S)], slot=3))
        rig.d.sync()
        for q in queued:
            rig.check(q)
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# scale

def test_scale_300_stereo_streams(gpu):
    rng = np.random.default_rng(800)
    S = 300
    rig = Rig(gpu, S, 2, DM.dense_table(rng, 7, 32), 200)
    try:
        for s in range(S):
            rig.set(s, int(rng.integers(-DMAX, DMAX + 1)))
            rig.seek(s, int(rng.integers(0, ONE)))
        rig.run([noise(rng, 200, 2) for _ in range(S)], uniform=True)
        rig.run([noise(rng, s % 65, 2) for s in range(S)], frames=64)
        rig.run([noise(rng, 200, 2) for _ in range(S)], uniform=True)
        assert rig.saturated_share() < SATURATED_MAX
    finally:
        rig.close()


def test_designed_default_runs(gpu):
    """cmhip_drift_new's own table, held against the model with the table cmhip_drift_design returns"""
    rng = np.random.default_rng(900)
    d = gpu.Drift(2, 2, 1024)
    try:
        assert d.geometry() == (7, 32)
    finally:
        d.close()
    rig = Rig(gpu, 2, 2, gpu.drift_design(), 1024)
    try:
        rig.set(0, gpu.drift_ppm(200.0))
        rig.set(1, gpu.drift_ppm(-3000.0))
        for _ in range(2):
            rig.run([noise(rng, 1024, 2) // 2 for _ in range(2)])
    finally:
        rig.close()
