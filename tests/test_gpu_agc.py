"""GPU: the leveller (cmhip_agc_*, csrc/k_agc.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy model below of the arithmetic include/coolmic_hip.h specifies -- a stream walked window
by window in int64 with Python's own integer root -- in output, clip counts and cmhip_agc_state, never another run of the
device code; what a run does not own of the output keeps its sentinel.  tests/test_agc_host.py runs the same model
against its emulation of the three kernels' decomposition, without a GPU.

Shapes: with W = 2^w the run lengths are ragged over {0, 1, W-1, W, W+1, 5W+3, ...} with max_frames = 5W+3, dealt so
that every stream meets every length and the streams' positions differ: window edges fall at every offset of a 16-byte
vector.  The input is random under per-stream envelopes that step between amplitudes of about 30 and 30 000, and the
streams' parameters go round a palette chosen so that every branch of the step is taken; the model's trace says so.
"""
import collections
import copy
import math
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past a stream's count
PARAM_NAMES = ("target", "gate", "gain_min", "gain_max", "rise", "fall", "initial")
BRANCHES = ("gate", "rise", "rise_reaches", "fall", "fall_reaches", "clamp_min", "clamp_max", "frozen_up", "frozen_down",
            "holds")


def params(**kw):
    """a parameter set as a dict: the creation defaults (a copy) with `kw` over them"""
    p = dict(target=3277, gate=33, gain_min=4096, gain_max=4096, rise=0, fall=0, initial=4096)
    p.update(kw)
    assert set(p) == set(PARAM_NAMES)
    return p


def step(A, L, p, trace=None):
    """the header's step(A, L) in Python integers; trace: a Counter of the branches taken"""
    t = trace if trace is not None else collections.Counter()
    if L == 0 or L < p["gate"]:
        t["gate"] += 1
        return A
    D = (p["target"] << 12) // L
    assert D < 2 ** 27
    if D < p["gain_min"]:
        t["clamp_min"] += 1
    if D > p["gain_max"]:
        t["clamp_max"] += 1
    D = min(max(D, p["gain_min"]), p["gain_max"])
    if D > A and p["rise"]:
        assert A * p["rise"] < 2 ** 32
        new = min(D, A + max(1, (A * p["rise"]) >> 16))
        t["rise_reaches" if new == D else "rise"] += 1
        return new
    if D < A and p["fall"]:
        new = max(D, A - max(1, (A * p["fall"]) >> 16))
        t["fall_reaches" if new == D else "fall"] += 1
        return new
    t["frozen_up" if D > A else "frozen_down" if D < A else "holds"] += 1
    return A


class Model:
    """one stream as the header states it: frames counted since creation or reset, the open window's sums, the two gain
    nodes in force, the last level, the clip counter"""

    def __init__(self, channels, w, p=None):
        self.C, self.w, self.W = channels, w, 1 << w
        self.p = dict(p) if p else params()
        self.clips = 0
        self.trace = collections.Counter()
        self.nodes = []                           # every A[k+1] the stream computed, in order (A[0] in front)
        self.reset()

    def reset(self):
        self.n = 0
        self.sums = np.zeros(self.C, dtype=np.int64)
        self.a_lo = self.a_hi = None
        self.level = 0

    def set(self, p):
        self.p = dict(p)

    def state(self):
        """-> (gain, level, clips) as cmhip_agc_state reports them"""
        return (self.p["initial"] if self.n == 0 else self.a_hi), self.level, self.clips

    def run(self, x):
        """x: int16 [F][C] -> int16 [F][C]"""
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.C)
        F = x.shape[0]
        y = np.zeros((F, self.C), dtype=np.int64)
        f = 0
        while f < F:
            j = self.n & (self.W - 1)
            if self.n == 0:
                self.a_lo = self.a_hi = self.p["initial"]
                self.level = 0
                self.sums[:] = 0
                self.nodes += [self.a_lo, self.a_hi]
            elif j == 0:                          # frame k W, k >= 1
                self.a_lo, self.a_hi = self.a_hi, step(self.a_hi, self.level, self.p, self.trace)
                self.nodes.append(self.a_hi)
            m = min(F - f, self.W - j)
            seg = x[f:f + m]
            prod = (self.a_hi - self.a_lo) * (j + np.arange(m, dtype=np.int64))
            assert np.abs(prod).max() < 2 ** 30
            g = self.a_lo + (prod >> self.w)
            assert g.min() >= 1 and g.max() <= 65535
            v = seg * g[:, None] + 2048
            assert np.abs(v).max() < 2 ** 31
            v >>= 12
            yy = np.clip(v, -32768, 32767)
            self.clips += int((yy != v).sum())
            y[f:f + m] = yy
            self.sums += (seg * seg).sum(axis=0)
            self.n += m
            f += m
            if self.n & (self.W - 1) == 0:        # the window is complete
                E = int(self.sums.max())
                assert E <= 2 ** 44
                self.level = math.isqrt(E >> self.w)
                assert 0 <= self.level <= 32768
                self.sums[:] = 0
        return y.astype(np.int16)


# ---------------------------------------------------------------------------
# inputs and cases

def palette(k):
    """parameter set k of the round: together they take every branch of the step under the envelopes below"""
    return [
        params(gate=100, gain_min=256, gain_max=65535, rise=20000, fall=30000),      # quiet: gated; loud: falls
        params(gate=0, gain_min=1, gain_max=65535, rise=65535, fall=65535),          # clamps at the top, reaches at once
        params(gate=0, gain_min=2048, gain_max=8192, rise=3000, fall=3000),          # both clamps, slow moves
        params(gate=0, gain_min=1, gain_max=65535, rise=0, fall=9000),               # frozen upwards
        params(gate=0, gain_min=1, gain_max=65535, rise=9000, fall=0, initial=20000),  # frozen downwards
        params(),                                                                    # a copy
        params(target=32767, gate=0, gain_min=1, gain_max=65535, rise=1, fall=1, initial=65535),   # max(1, ...)
        params(target=300, gate=20, gain_min=1, gain_max=65535, rise=6132, fall=1960, initial=1),
    ][k % 8]


def enveloped(seed, frames, channels, W):
    """random samples under an envelope that steps between amplitudes of about 30 and 30 000 every 2 or 3 windows"""
    rng = np.random.default_rng(seed)
    x = np.zeros((frames, channels), dtype=np.int64)
    at, loud = 0, bool(seed & 1)
    while at < frames:
        n = int(rng.integers(2, 4)) * W + int(rng.integers(0, 5))
        amp = int(rng.integers(25000, 30001)) if loud else int(rng.integers(20, 41))
        n = min(n, frames - at)
        x[at:at + n] = rng.integers(-amp, amp + 1, size=(n, channels))
        at += n
        loud = not loud
    return x.astype(np.int16)


def run_lengths(W):
    return [W + 1, 0, 1, W - 1, 5 * W + 3, W, 9, 2 * W + 5, 3, 5 * W + 3, 5 * W + 3]


def rotate(lengths, k, streams):
    """run k of a case: stream s gets length number k + 3 s of the list, so every stream meets every length"""
    return [lengths[(k + 3 * s) % len(lengths)] for s in range(streams)]


def stride_of(max_frames, channels, extra):
    return (max_frames * channels + 7) // 8 * 8 + extra


class Rig:
    """a leveller between two arrays of pinned, device-mapped host memory, and one model per stream"""

    def __init__(self, cm, streams, channels, w, max_frames, plist=None):
        self.cm, self.S, self.C, self.w = cm, streams, channels, w
        self.m = cm.Leveller(streams, channels, w, max_frames)
        self.in_stride = stride_of(max_frames, channels, 8)                 # wider than any run
        self.out_stride = stride_of(max_frames, channels, 16)
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.models = [Model(channels, w) for _ in range(streams)]
        if plist is not None:
            for s in range(streams):
                self.set(s, plist[s])

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def set(self, stream, p, check=True):
        self.m.set(stream, self.cm.AgcParams(**p))
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].set(p)
            if check:
                assert self.m.get(s).as_dict() == p

    def reset(self, stream=-1):
        self.m.reset(stream)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].reset()

    def fill(self, xs):
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        self.src.array[:] = POISON
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        self.dst.array[:] = SENTINEL
        return counts

    def check_state(self):
        gain, level, clips = self.m.state()
        want = [m.state() for m in self.models]
        assert gain.tolist() == [v[0] for v in want], "gain"
        assert level.tolist() == [v[1] for v in want], "level"
        assert clips.tolist() == [v[2] for v in want], "clips"

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
        """xs: per stream int16 [F_s][C]; runs device and models, compares outputs, the untouched rest and the state
        -> per stream the model's int16 [F_s][C]"""
        counts = self.fill(xs)
        self.m.run(self.src.dev, self.in_stride, max(counts), self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = [m.run(x) for m, x in zip(self.models, xs)]
        self.check_output(wants)
        self.check_state()
        return wants


def play(cm, streams, channels, w, signals, plist, cuts):
    """the streams' signals through a fresh leveller, cut as `cuts` says (per run: a count per stream)
    -> (per stream the output, the final state, the models)"""
    rig = Rig(cm, streams, channels, w, 5 * (1 << w) + 3, plist)
    try:
        at = [0] * streams
        out = [[] for _ in range(streams)]
        for counts in cuts:
            wants = rig.run([signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)])
            for s, n in enumerate(counts):
                out[s].append(wants[s])
                at[s] += n
        gain, level, clips = rig.m.state()
        return [np.concatenate(o) for o in out], (gain.tolist(), level.tolist(), clips.tolist()), rig.models
    finally:
        rig.close()


def model_case(streams, channels, w, seed):
    """the signals, parameters and cuts of a model-equality case: every stream meets every run length once"""
    W = 1 << w
    lengths = run_lengths(W)
    total = sum(lengths)
    assert total >= 8 * W
    signals = [enveloped(seed + 2 * s + (s // 8 & 1), total, channels, W) for s in range(streams)]
    plist = [palette(s) for s in range(streams)]
    cuts = [rotate(lengths, k, streams) for k in range(len(lengths))]
    return signals, plist, cuts


# S = 70 is more than one wave of k_agc_step's lanes, 300 more than one workgroup of them; C = 1, 2 are the fast
# kernels, 3, 6 and 16 the any-channel-count ones
MODEL_CASES = ([(1, c, w) for c in (1, 2, 3, 6, 16) for w in (6, 8)] +
               [(3, c, 6) for c in (1, 2, 3, 6, 16)] + [(3, 1, 8), (3, 2, 8)] +
               [(70, 1, 6), (70, 2, 8), (70, 3, 6), (70, 16, 6), (300, 2, 6), (300, 1, 8), (300, 6, 6)])


@pytest.mark.parametrize("streams,channels,w", MODEL_CASES)
def test_equals_the_model(gpu, streams, channels, w):
    signals, plist, cuts = model_case(streams, channels, w, 1000 * w + 10 * channels)
    _, _, models = play(gpu, streams, channels, w, signals, plist, cuts)
    for m in models:
        assert m.n == len(signals[0]) and m.n >= 8 * m.W
    if streams >= 8:                              # the whole palette: every branch of the step was taken by some stream
        trace = sum((m.trace for m in models), collections.Counter())
        assert all(trace[b] > 0 for b in BRANCHES), trace
        assert sum(m.clips for m in models) > 0 and any(m.clips == 0 for m in models)


@pytest.mark.parametrize("channels,w", [(1, 6), (2, 6), (3, 6), (16, 8), (2, 8)])
def test_output_does_not_depend_on_the_cuts(gpu, channels, w):
    """the same streams in the fewest runs and in many ragged ones: identical output, clips and state"""
    W, S = 1 << w, 9
    total = 4 * (5 * W + 3)
    signals = [enveloped(50 + s, total, channels, W) for s in range(S)]
    plist = [palette(s) for s in range(S)]
    long_cuts = [[5 * W + 3] * S] * 4
    lengths, ragged, left, k = run_lengths(W), [], [total] * S, 0
    while any(left):
        counts = [min(n, left[s]) for s, n in enumerate(rotate(lengths, k, S))]
        left = [a - b for a, b in zip(left, counts)]
        ragged.append(counts)
        k += 1
    assert len(ragged) > 2 * len(long_cuts) and any(0 in counts for counts in ragged)
    a, state_a, _ = play(gpu, S, channels, w, signals, plist, long_cuts)
    b, state_b, _ = play(gpu, S, channels, w, signals, plist, ragged)
    for s in range(S):
        assert np.array_equal(a[s], b[s]), s
    assert state_a == state_b


# ---------------------------------------------------------------------------
# extremes

FAST_FALL = dict(target=32767, gate=0, gain_min=1, gain_max=65535, rise=65535, fall=65535, initial=65535)


@pytest.mark.parametrize("channels", [1, 16])
def test_constant_full_scale_at_the_longest_window(gpu, channels):
    """constant -32768 at w = 14: E = 2^44, L = 32768, the nodes run 65535, 65535, 4095, and every sample of the first
    two windows clips"""
    w, W = 14, 1 << 14
    rig = Rig(gpu, 1, channels, w, 3 * W, [params(**FAST_FALL)])
    try:
        x = np.full((3 * W, channels), -32768, dtype=np.int16)
        want = rig.run([x], uniform=True)[0]
        m = rig.models[0]
        assert m.nodes == [65535, 65535, 4095, 4095] and m.level == 32768
        assert m.clips == 2 * W * channels
        assert (want[:2 * W] == -32768).all() and (want[2 * W:] == (-32768 * 4095 + 2048) >> 12).all()
        gain, level, clips = rig.m.state(clear_clips=True)
        assert (gain[0], level[0], clips[0]) == (4095, 32768, 2 * W * channels)
        assert rig.m.state()[2][0] == 0                                      # cleared
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_the_issues_figures_at_w_6(gpu, channels):
    """constant -32768 at w = 6: all 128 frames of the first two windows clip; then the square wave of amplitude 300
    reaches the gain (3277 << 12) / 300 = 44741 exactly, stays there and comes out at +-3277 with no clip"""
    W = 64
    rig = Rig(gpu, 2, channels, 6, 5 * W + 3)
    try:
        rig.set(0, params(**FAST_FALL))
        rig.set(1, params(target=3277, gate=0, gain_min=1, gain_max=65535, rise=20000, fall=20000))
        n = np.arange(5 * W + 3)
        square = np.where((n // 5) % 2 == 0, 300, -300).astype(np.int16)[:, None].repeat(channels, axis=1)
        full = np.full((5 * W + 3, channels), -32768, dtype=np.int16)
        for _ in range(8):
            wants = rig.run([full, square], uniform=True)
        assert rig.models[0].nodes[:3] == [65535, 65535, 4095]
        first = Model(channels, 6, params(**FAST_FALL))
        first.run(full[:2 * W])
        assert first.clips == 128 * channels
        m = rig.models[1]
        assert m.clips == 0 and m.level == 300 and m.a_hi == 44741 and m.nodes[-8:] == [44741] * 8
        assert set(np.unique(wants[1]).tolist()) == {-3277, 3277}
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_silence_leaves_the_gain_alone(gpu, channels):
    W = 64
    rig = Rig(gpu, 3, channels, 6, 5 * W + 3, [palette(1), palette(0), palette(4)])
    try:
        for k in range(3):
            wants = rig.run([np.zeros((n, channels), dtype=np.int16) for n in (5 * W + 3, W + 1, 2 * W + k)])
            assert all((w == 0).all() for w in wants)
        gain, level, clips = rig.m.state()
        assert gain.tolist() == [palette(1)["initial"], palette(0)["initial"], palette(4)["initial"]]
        assert level.tolist() == [0, 0, 0] and clips.tolist() == [0, 0, 0]
        assert all(m.trace["gate"] == sum(m.trace.values()) > 0 for m in rig.models)
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_largest_gain_on_full_scale_clamps_both_ways(gpu, channels):
    W = 64
    rig = Rig(gpu, 2, channels, 6, 5 * W + 3)
    try:
        rig.set(-1, params(gate=0, gain_min=65535, gain_max=65535, rise=65535, fall=65535, initial=65535))
        rng = np.random.default_rng(channels)
        xs = [rng.choice(np.array([-32768, 32767, 2047, 2048, -2048, -2049, 0], dtype=np.int16), size=(n, channels))
              for n in (5 * W + 3, 3 * W + 1)]
        wants = rig.run(xs)
        for x, y in zip(xs, wants):
            assert y.min() == -32768 and y.max() == 32767
        assert all(m.clips > 0 for m in rig.models)                      # (the counts are compared in run)
    finally:
        rig.close()


@pytest.mark.parametrize("channels,w", [(1, 6), (2, 8), (5, 6), (16, 6)])
def test_unity_parameters_give_the_input_back(gpu, channels, w):
    """gain_min = gain_max = initial = 4096, the object's state at creation: a copy, bit for bit, full scale included"""
    W = 1 << w
    rig = Rig(gpu, 3, channels, w, 5 * W + 3)
    try:
        rng = np.random.default_rng(w + channels)
        for k in range(3):
            xs = [rng.integers(-32768, 32768, size=(n, channels)).astype(np.int16)
                  for n in rotate(run_lengths(W), 4 + k, 3)]
            for x in xs:
                x[::7] = -32768
                x[3::11] = 32767
            wants = rig.run(xs)
            for x, y in zip(xs, wants):
                assert np.array_equal(x, y)
        assert rig.m.state()[2].tolist() == [0, 0, 0]
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# set, reset, refusals

@pytest.mark.parametrize("channels", [1, 2, 3])
def test_set_behind_a_queued_run_needs_no_wait(gpu, channels):
    """run A, set, run B with no host wait in between: run A keeps the old parameters, run B takes the new ones from
    each stream's next window edge on; copies of the models that never see the set show that it mattered"""
    W, S = 64, 3
    rig = Rig(gpu, S, channels, 6, 5 * W + 3, [palette(1)] * S)
    src_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride))
    dst_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    try:
        sig = [enveloped(90 + s, 12 * W, channels, W) for s in range(S)]
        first, second = [3 * W + 5, 2 * W, W - 1], [5 * W + 3, 4 * W + 1, 5 * W]
        rig.run([sig[s][:n] for s, n in enumerate(first)])
        at = [n + W + 3 for n in first]                                  # where run B begins
        xa = [sig[s][first[s]:at[s]] for s in range(S)]
        xb = [sig[s][at[s]:at[s] + second[s]] for s in range(S)]
        new = params(target=1000, gate=0, gain_min=100, gain_max=5000, rise=65535, fall=65535, initial=100)
        rig.fill(xa)
        src_b.array[:] = POISON
        for s, x in enumerate(xb):
            src_b.array[s, :x.size] = x.reshape(-1)
        dst_b.array[:] = SENTINEL
        # the device: run A, the set on streams 0 and 2, run B -- and only then a wait
        rig.m.run(rig.src.dev, rig.in_stride, W + 3, rig.dst.dev, rig.out_stride)
        for s in (0, 2):
            rig.m.set(s, gpu.AgcParams(**new))
        rig.m.run(src_b.dev, rig.in_stride, max(second), dst_b.dev, rig.out_stride, second)
        rig.m.sync()
        # the models: run A with the old parameters, then the set, then run B
        rig.check_output([m.run(x) for m, x in zip(rig.models, xa)])
        unset = copy.deepcopy(rig.models)
        for s in (0, 2):
            rig.models[s].set(new)
        want_b = [m.run(x) for m, x in zip(rig.models, xb)]
        rig.dst.array[:] = dst_b.array
        rig.check_output(want_b)
        rig.check_state()
        without = [m.run(x) for m, x in zip(unset, xb)]
        assert np.array_equal(without[1], want_b[1])
        for s in (0, 2):
            edge = -at[s] % W                                            # the stream's next window edge in run B
            assert 0 < edge < second[s]
            assert np.array_equal(without[s][:edge], want_b[s][:edge]), s                # not before it ...
            assert not np.array_equal(without[s][edge:], want_b[s][edge:]), s            # ... but from it on
    finally:
        src_b.free()
        dst_b.free()
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_reset_starts_a_stream_afresh(gpu, channels):
    W, S = 64, 3
    plist = [palette(1), palette(0), palette(2)]
    rig = Rig(gpu, S, channels, 6, 5 * W + 3, plist)
    try:
        sig = [enveloped(30 + s, 11 * W, channels, W) for s in range(S)]
        rig.run([sig[s][:3 * W + 7 + s] for s in range(S)])              # every stream inside an open window
        before = [m.state() for m in rig.models]
        rig.reset(1)
        assert rig.models[1].state()[:2] == (plist[1]["initial"], 0)
        rig.check_state()                                                # the others untouched, the clip counter kept
        assert [m.state() for m in rig.models][0] == before[0] and [m.state() for m in rig.models][2] == before[2]
        wants = rig.run([sig[s][3 * W + 7 + s:8 * W] for s in range(S)])
        fresh = Model(channels, 6, plist[1])
        assert np.array_equal(wants[1], fresh.run(sig[1][3 * W + 8:8 * W]))      # position 0, no sums carried
        rig.reset()
        rig.run([sig[s][8 * W:8 * W + 2 * W + s] for s in range(S)])
        assert all(m.n == 2 * W + s for s, m in enumerate(rig.models))
    finally:
        rig.close()


def test_refusals_of_a_real_object(gpu):
    """the checks tests/test_agc_host.py makes on an object without a device, on one with"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("test_agc_host_for_gpu", os.path.join(os.path.dirname(__file__), "test_agc_host.py"))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    d = gpu.Leveller(3, 2, 6, 64)
    try:
        host.check_object_refusals(gpu, d)
    finally:
        d.close()
