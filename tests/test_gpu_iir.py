"""GPU: the filter stage (cmhip_iir_*, csrc/k_iir.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy int64 model below of the arithmetic include/coolmic_hip.h specifies -- every row walked
frame by frame, section by section -- in output, `clips`, `overs` and the continued state of every section, never
another run of the device code; what a run does not own of the output keeps its sentinel.  tests/test_iir_host.py runs
the same model against its emulation of the two kernels' decompositions, without a GPU.

Shapes: with B the tile's frames (read from the plan) the run lengths are ragged over {0, 1, 2, 7, 8, 9, B-1, B, B+1,
2B+1}, dealt so that every stream meets every length; 33 streams fill a wave partly and 70 leave a workgroup's last
streams missing.  The input is full-range noise with stretches of +-full scale and a DC offset, and the streams'
sections go round a palette that holds real designs, coefficients at +-2^28 and unity; the model's trace says that
every branch is taken.
"""
import collections
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past a stream's count
ONE = 1 << 26
V_MAX = 2 ** 31 - 1
UNITY = (ONE, 0, 0, 0, 0)
BRANCHES = ("over_pos", "over_neg", "clip_pos", "clip_neg", "neg_rem", "pos_rem", "no_rem")


class Model:
    """S streams of C channels through N sections as the header states it: int64 arrays over the rows, one frame at a
    time.  coef int64 [S][N][5]; st int64 [S][C][N][5] = u1, u2, v1, v2, e"""

    def __init__(self, streams, channels, sections):
        self.S, self.C, self.N = streams, channels, sections
        self.coef = np.tile(np.array(UNITY, dtype=np.int64), (streams, sections, 1))
        self.st = np.zeros((streams, channels, sections, 5), dtype=np.int64)
        self.clips = np.zeros(streams, dtype=np.int64)
        self.overs = np.zeros(streams, dtype=np.int64)
        self.trace = collections.Counter()

    def set(self, stream, section, sec):
        self.coef[slice(None) if stream < 0 else stream, section] = np.array(sec, dtype=np.int64)

    def reset(self, stream=-1):
        self.st[slice(None) if stream < 0 else stream] = 0

    def rows(self):
        return self.st.reshape(self.S * self.C, self.N, 5).astype(np.int32)

    def run(self, xs):
        """xs: per stream int16 [F_s][C] -> per stream int16 [F_s][C]"""
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, self.C) for x in xs]
        counts = np.array([x.shape[0] for x in xs])
        F = int(counts.max()) if len(xs) else 0
        X = np.zeros((self.S, F, self.C), dtype=np.int64)
        for s, x in enumerate(xs):
            X[s, :counts[s]] = x
        Y = np.zeros_like(X)
        t = self.trace
        for f in range(F):
            act = (counts > f)[:, None]                              # [S][1]
            u = X[:, f, :] << 12
            assert np.abs(u).max() <= 2 ** 27
            for k in range(self.N):
                c = self.coef[:, k, :, None]                         # [S][5][1]
                st = self.st[:, :, k, :]                             # [S][C][5], a view
                assert max(int(np.abs(u).max()), int(np.abs(st[..., :4]).max())) <= V_MAX and np.abs(c).max() <= 2 ** 28
                acc = c[:, 0] * u + c[:, 1] * st[..., 0] + c[:, 2] * st[..., 1] - c[:, 3] * st[..., 2] - c[:, 4] * st[..., 3]
                acc += st[..., 4]
                assert np.abs(acc).max() < 2 ** 62
                e = acc & (ONE - 1)
                q = acc >> 26                                        # arithmetic: floor
                v = np.clip(q, -V_MAX, V_MAX)
                t["over_pos"] += int(((q > V_MAX) & act).sum())
                t["over_neg"] += int(((q < -V_MAX) & act).sum())
                t["neg_rem"] += int(((acc < 0) & (e != 0) & act).sum())
                t["pos_rem"] += int(((acc > 0) & (e != 0) & act).sum())
                t["no_rem"] += int(((e == 0) & act).sum())
                self.overs += ((v != q) & act).sum(axis=1)
                new = np.stack([u, st[..., 0], v, st[..., 2], e], axis=-1)
                self.st[:, :, k, :] = np.where(act[..., None], new, st)
                u = v
            r = (u + 2048) >> 12
            y = np.clip(r, -32768, 32767)
            t["clip_pos"] += int(((r > 32767) & act).sum())
            t["clip_neg"] += int(((r < -32768) & act).sum())
            self.clips += ((y != r) & act).sum(axis=1)
            Y[:, f, :] = y
        return [Y[s, :counts[s]].astype(np.int16) for s in range(self.S)]


# ---------------------------------------------------------------------------
# inputs and cases

BIG = 1 << 28


def palette(cm, k):
    """section number k of the round: real designs, the coefficient range's corners, unity"""
    return [
        lambda: cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0).as_tuple(),
        lambda: cm.iir_design(cm.IIR_LOWSHELF, 48000.0, 1000.0, 0.7, 12.0).as_tuple(),
        lambda: (BIG, BIG, BIG, 0, 0),                                           # gain 12: the second of these overflows
        lambda: cm.iir_design(cm.IIR_PEAK, 44100.0, 3000.0, 2.0, -9.0).as_tuple(),
        lambda: UNITY,
        lambda: cm.iir_design(cm.IIR_HIGHPASS1, 48000.0, 20.0).as_tuple(),
        lambda: (-BIG, BIG, -BIG, (1 << 27) - 2, ONE - 1),                       # on the triangle's edge
        lambda: cm.iir_design(cm.IIR_NOTCH, 48000.0, 50.0, 8.0).as_tuple(),
        lambda: cm.iir_design(cm.IIR_LOWPASS, 8000.0, 3400.0).as_tuple(),
        lambda: (BIG, -BIG, BIG, -((1 << 27) - 2), ONE - 1),
        lambda: cm.iir_design(cm.IIR_HIGHSHELF, 48000.0, 8000.0, 0.7, 12.0).as_tuple(),
        lambda: cm.iir_design(cm.IIR_LOWPASS1, 48000.0, 3183.1).as_tuple(),
    ][k % 12]()


def noise(seed, frames, channels):
    """full-range noise on a DC offset with stretches of both full scales"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-20000, 20001, size=(frames, channels)) + int(rng.integers(-9000, 9001))
    at = 0
    while at < frames:
        n = int(rng.integers(3, 40))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            x[at:at + n] = 32767
        elif kind == 1:
            x[at:at + n] = -32768
        at += n + int(rng.integers(5, 60))
    return np.clip(x, -32768, 32767).astype(np.int16)


def run_lengths(B):
    return [B + 1, 0, 1, B - 1, 2 * B + 1, B, 9, 2, 7, 8]


def rotate(lengths, k, streams):
    """run k of a case: stream s gets length number k + 3 s of the list, so every stream meets every length"""
    return [lengths[(k + 3 * s) % len(lengths)] for s in range(streams)]


def stride_of(max_frames, channels, extra):
    return (max_frames * channels + 7) // 8 * 8 + extra


class Rig:
    """a filter between two arrays of pinned, device-mapped host memory, and the model"""

    def __init__(self, cm, streams, channels, sections, max_frames, secs=None):
        self.cm, self.S, self.C, self.N = cm, streams, channels, sections
        self.m = cm.Filter(streams, channels, sections, max_frames)
        self.in_stride = stride_of(max_frames, channels, 8)                  # wider than any run
        self.out_stride = stride_of(max_frames, channels, 16)
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.model = Model(streams, channels, sections)
        if secs is not None:                                                 # secs(s, k) -> five integers
            for s in range(streams):
                for k in range(sections):
                    self.set(s, k, secs(s, k))

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def set(self, stream, section, sec):
        self.m.set(stream, section, self.cm.IirSection(*sec))
        self.model.set(stream, section, sec)
        for s in (range(self.S) if stream < 0 else [stream]):
            assert self.m.get(s, section).as_tuple() == tuple(sec)

    def reset(self, stream=-1):
        self.m.reset(stream)
        self.model.reset(stream)

    def fill(self, xs):
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        self.src.array[:] = POISON
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        self.dst.array[:] = SENTINEL
        return counts

    def check_state(self):
        clips, overs = self.m.state()
        assert clips.tolist() == self.model.clips.tolist(), "clips"
        assert overs.tolist() == self.model.overs.tolist(), "overs"
        have, want = self.m.rows(), self.model.rows()
        bad = np.argwhere(have != want)
        assert bad.size == 0, ("state: first mismatch (row, section, field)", bad[0].tolist(), have[tuple(bad[0])],
                               want[tuple(bad[0])])

    def check_output(self, wants):
        for s, want in enumerate(wants):
            n = want.size
            row = self.dst.array[s]
            have = row[:n].reshape(-1, self.C)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(), "of", want.shape[0],
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (row[n:] == SENTINEL).all(), ("stream", s, "written past its count")

    def run(self, xs, uniform=False):
        """xs: per stream int16 [F_s][C]; runs device and model, compares outputs, the untouched rest and the state
        -> per stream the model's int16 [F_s][C]"""
        counts = self.fill(xs)
        self.m.run(self.src.dev, self.in_stride, max(counts), self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = self.model.run(xs)
        self.check_output(wants)
        self.check_state()
        return wants


def tile_frames(cm, channels, sections):
    return cm.plan_iir(1, channels, sections, 1).tile


def model_case(cm, streams, channels, sections, seed, runs=None):
    """the signals, the sections and the cuts of a model-equality case"""
    lengths = run_lengths(tile_frames(cm, channels, sections))
    runs = len(lengths) if runs is None else runs
    cuts = [rotate(lengths, k, streams) for k in range(runs)]
    total = [sum(c[s] for c in cuts) for s in range(streams)]
    signals = [noise(seed + s, total[s], channels) for s in range(streams)]
    return signals, (lambda s, k: palette(cm, s + 5 * k)), cuts


def play(cm, streams, channels, sections, signals, secs, cuts, max_frames, between=None):
    """the streams' signals through a fresh filter, cut as `cuts` says (per run: a count per stream); between(rig, k)
    is called in front of run k -> (per stream the output, (clips, overs, rows), the model)"""
    rig = Rig(cm, streams, channels, sections, max_frames, secs)
    try:
        at = [0] * streams
        out = [[] for _ in range(streams)]
        for k, counts in enumerate(cuts):
            if between:
                between(rig, k)
            wants = rig.run([signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)])
            for s, n in enumerate(counts):
                out[s].append(wants[s])
                at[s] += n
        clips, overs = rig.m.state()
        return [np.concatenate(o) for o in out], (clips.tolist(), overs.tolist(), rig.m.rows()), rig.model
    finally:
        rig.close()


# every channel count with every section count at 33 streams (a wave partly filled); 1 and 70 streams (a workgroup's
# last streams missing) where the forms differ: mono and stereo at NP = 1, 2, 4, 8, and the any-channel-count kernel
MODEL_CASES = ([(33, c, n) for c in (1, 2, 3, 5, 6, 16) for n in (1, 2, 3, 4, 5, 8)] +
               [(1, 1, 1), (1, 2, 3), (1, 2, 8), (1, 3, 2), (1, 16, 8), (1, 5, 5)] +
               [(70, 1, 1), (70, 1, 5), (70, 2, 2), (70, 2, 8), (70, 3, 4), (70, 16, 1), (70, 6, 8)])


@pytest.mark.parametrize("streams,channels,sections", MODEL_CASES)
def test_equals_the_model(gpu, streams, channels, sections):
    B = tile_frames(gpu, channels, sections)
    signals, secs, cuts = model_case(gpu, streams, channels, sections, 100 * channels + sections,
                                     runs=None if streams == 1 else 4)
    _, _, model = play(gpu, streams, channels, sections, signals, secs, cuts, 2 * B + 1)
    if streams >= 33 and sections >= 2:           # the whole palette: every branch was taken
        assert all(model.trace[b] > 0 for b in BRANCHES), model.trace
        assert (model.overs > 0).any() and (model.clips > 0).any()
        assert sections > 2 or (model.overs == 0).any()


@pytest.mark.parametrize("channels,sections", [(1, 1), (1, 8), (2, 3), (2, 4), (3, 2), (16, 5)])
def test_output_does_not_depend_on_the_cuts(gpu, channels, sections):
    """the same streams in two runs and in many ragged ones that include 0- and 1-frame runs, with a set of one
    stream's sections and a reset of another stream at the same frame in both: identical output, counters and state"""
    B, S = tile_frames(gpu, channels, sections), 9
    half = 2 * B + 1
    signals = [noise(50 + s, 2 * half, channels) for s in range(S)]
    secs = lambda s, k: palette(gpu, s + 5 * k)

    def ragged(total):
        lengths, cuts, left, k = run_lengths(B // 2), [], [total] * S, 0
        while any(left):
            counts = [min(n, left[s]) for s, n in enumerate(rotate(lengths, k, S))]
            left = [a - b for a, b in zip(left, counts)]
            cuts.append(counts)
            k += 1
        return cuts

    first = ragged(half)
    many = first + ragged(half)
    assert len(many) > 8 and any(0 in c for c in many) and any(1 in c for c in many)

    def at_the_middle(middle):
        def between(rig, k):
            if k == middle:
                rig.set(2, 0, palette(gpu, 7))
                rig.set(-1, sections - 1, palette(gpu, 3))
                rig.reset(4)
        return between

    a, state_a, _ = play(gpu, S, channels, sections, signals, secs, [[half] * S] * 2, half, at_the_middle(1))
    b, state_b, _ = play(gpu, S, channels, sections, signals, secs, many, half, at_the_middle(len(first)))
    for s in range(S):
        assert np.array_equal(a[s], b[s]), s
    assert state_a[:2] == state_b[:2] and np.array_equal(state_a[2], state_b[2])


# ---------------------------------------------------------------------------
# edges

@pytest.mark.parametrize("channels", [1, 2, 5])
def test_largest_coefficients_on_full_scale(gpu, channels):
    """three sections of b = +-2^28 (a gain of 12 each) on +-32768: the second and third meet the inner clamp on both
    sides, with a1, a2 on the triangle's edge |acc| comes near 2^62; the model asserts that it stays below"""
    B = tile_frames(gpu, channels, 3)
    secs = lambda s, k: [(BIG, BIG, BIG, 0, 0), (-BIG, -BIG, -BIG, 0, 0),
                         (BIG, BIG, BIG, -((1 << 27) - 2), ONE - 1)][(k + s) % 3]
    rig = Rig(gpu, 3, channels, 3, 2 * B + 1, secs)
    try:
        n = np.arange(2 * B + 1)
        square = np.where((n // 11) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
        wants = rig.run([square, -1 - square, square[:B + 3]])
        t = rig.model.trace
        assert t["over_pos"] > 0 and t["over_neg"] > 0 and t["clip_pos"] > 0 and t["clip_neg"] > 0, t
        assert all(w.min() == -32768 and w.max() == 32767 for w in wants)
        clips, overs = rig.m.state(clear=True)
        assert (clips > 0).all() and (overs > 0).all()
        assert rig.m.state()[0].tolist() == [0] * 3 and rig.m.state()[1].tolist() == [0] * 3      # cleared
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_a_12_db_shelf_on_full_scale_meets_the_output_clamp(gpu, channels):
    B = tile_frames(gpu, channels, 1)
    shelf = gpu.iir_design(gpu.IIR_LOWSHELF, 48000.0, 1000.0, 0.7, 12.0).as_tuple()
    rig = Rig(gpu, 2, channels, 1, 2 * B + 1, lambda s, k: shelf)
    try:
        n = np.arange(2 * B + 1)
        slow = np.where((n // 50) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
        rig.run([slow, slow // 8])
        assert rig.model.clips[0] > 0 and rig.model.clips[1] == 0 and rig.model.overs.tolist() == [0, 0]
        assert rig.model.trace["clip_pos"] > 0 and rig.model.trace["clip_neg"] > 0
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_floor_not_truncation_on_negative_sums(gpu, channels):
    """a high-pass on a negative signal: negative acc with a remainder in most frames, where a shift that rounds
    towards zero would give another v"""
    B = tile_frames(gpu, channels, 2)
    hp = gpu.iir_design(gpu.IIR_HIGHPASS, 48000.0, 40.0).as_tuple()
    rig = Rig(gpu, 2, channels, 2, 2 * B + 1, lambda s, k: hp)
    try:
        x = -np.abs(noise(5, 2 * B + 1, channels).astype(np.int32)).clip(1, 32768)
        rig.run([x.astype(np.int16), (x // 3).astype(np.int16)])
        assert rig.model.trace["neg_rem"] > B
    finally:
        rig.close()


@pytest.mark.parametrize("channels,sections", [(1, 1), (1, 3), (2, 8), (5, 2), (16, 8)])
def test_unity_sections_give_the_input_back(gpu, channels, sections):
    """the object's state at creation: a copy, bit for bit, full scale included"""
    B = tile_frames(gpu, channels, sections)
    rig = Rig(gpu, 3, channels, sections, 2 * B + 1)
    try:
        for k in range(3):
            xs = [noise(10 * k + s, n, channels) for s, n in enumerate(rotate(run_lengths(B), 4 + k, 3))]
            wants = rig.run(xs)
            for x, y in zip(xs, wants):
                assert np.array_equal(x, y)
        clips, overs = rig.m.state()
        assert clips.tolist() == [0, 0, 0] and overs.tolist() == [0, 0, 0]
        assert not rig.m.rows()[:, :, 4].any()                               # no remainder: every acc is u << 26
    finally:
        rig.close()


@pytest.mark.parametrize("channels,sections", [(1, 2), (1, 3), (2, 5), (2, 8), (3, 7)])
def test_a_single_section_equals_the_cascade_padded_with_unity(gpu, channels, sections):
    """an N = 1 object and an N-section object whose other sections are unity give the same output, wherever in the
    cascade the one section sits"""
    B = tile_frames(gpu, channels, sections)
    hp = gpu.iir_design(gpu.IIR_HIGHPASS, 48000.0, 300.0, 1.3).as_tuple()
    xs = [noise(70 + s, n, channels) for s, n in enumerate((2 * B + 1, B + 1, 9))]
    outs = []
    for n, where in ((1, 0), (sections, 0), (sections, sections - 1), (sections, sections // 2)):
        rig = Rig(gpu, 3, channels, n, 2 * B + 1)
        try:
            rig.set(-1, where, hp)
            outs.append(rig.run(xs))
        finally:
            rig.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("channels", [1, 3])
def test_set_behind_a_queued_run_needs_no_wait(gpu, channels):
    """run A, a set, run B with no host wait in between: run A keeps the old sections, run B takes the new ones"""
    B, S, N = tile_frames(gpu, channels, 2), 3, 2
    rig = Rig(gpu, S, channels, N, 2 * B + 1, lambda s, k: palette(gpu, s + k))
    src_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride))
    dst_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    try:
        xa = [noise(90 + s, n, channels) for s, n in enumerate((B + 3, 2 * B + 1, 7))]
        xb = [noise(95 + s, n, channels) for s, n in enumerate((2 * B + 1, 1, B))]
        ca, cb = rig.fill(xa), [x.shape[0] for x in xb]
        src_b.array[:] = POISON
        for s, x in enumerate(xb):
            src_b.array[s, :x.size] = x.reshape(-1)
        dst_b.array[:] = SENTINEL
        new = gpu.iir_design(gpu.IIR_LOWPASS, 48000.0, 500.0).as_tuple()
        rig.m.run(rig.src.dev, rig.in_stride, max(ca), rig.dst.dev, rig.out_stride, ca)
        rig.m.set(1, 0, gpu.IirSection(*new))
        rig.m.set(2, 1, gpu.IirSection(*new))
        rig.m.run(src_b.dev, rig.in_stride, max(cb), dst_b.dev, rig.out_stride, cb)
        rig.m.sync()
        rig.check_output(rig.model.run(xa))
        rig.model.set(1, 0, new)
        rig.model.set(2, 1, new)
        rig.dst.array[:] = dst_b.array
        rig.check_output(rig.model.run(xb))
        rig.check_state()
    finally:
        src_b.free()
        dst_b.free()
        rig.close()


def test_refusals_of_a_real_object(gpu):
    """the checks tests/test_iir_host.py makes on an object without a device, on one with"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("test_iir_host_for_gpu", os.path.join(os.path.dirname(__file__), "test_iir_host.py"))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    d = gpu.Filter(3, 2, 2, 64)
    try:
        host.check_object_refusals(gpu, d)
    finally:
        d.close()
