"""GPU: the automixer (cmhip_automix_*, csrc/k_automix.hip) through the C ABI and the Python mirror.

Bar: bit-exact against tests/automix_model.py -- the arithmetic include/coolmic_hip.h specifies, a desk walked group by
group and window by window in Python integers, written from the header's text -- in output, gains, powers and shares,
never another run of the device code; what a run does not own of the output keeps its sentinel.
tests/test_automix_host.py runs the same model against its emulation of the two lane-per-stream kernels, without a GPU.

Shapes: with W = 2^w the run lengths are 1, W-1, W, W+1, 2W+3, 0 and max_frames = 5W+3, rotated per group so that
groups differ and members agree.  The signals are talk spurts with whole silent windows (a group's sum of 0) and
stretches of constant full scale (m = 2^30); the palette takes every branch, the model's trace says so.
"""
import copy
import importlib.util
import os
import types

import numpy as np
import pytest

import automix_model as AM

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past a stream's count


def stride_of(max_frames, channels, extra):
    return (max_frames * channels + 7) // 8 * 8 + extra


class Rig:
    """an automixer between two arrays of pinned, device-mapped host memory, and the model of the whole desk"""

    def __init__(self, cm, streams, channels, w, max_frames, hip_stream=None):
        self.cm, self.S, self.C, self.w = cm, streams, channels, w
        self.m = cm.Automixer(streams, channels, w, max_frames, hip_stream=hip_stream)
        self.in_stride = stride_of(max_frames, channels, 8)                 # wider than any run
        self.out_stride = stride_of(max_frames, channels, 16)
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.desk = AM.Desk(streams, channels, w)

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def set(self, stream, p):
        self.m.set(stream, self.cm.AutomixParams(**p))
        self.desk.set(stream, p)
        for s in (range(self.S) if stream < 0 else [stream]):
            assert self.m.get(s).as_dict() == p

    def set_group(self, stream, group):
        self.m.set_group(stream, group)
        self.desk.set_group(stream, group)
        assert self.m.get_group(stream) == group

    def reset(self, stream=-1):
        self.m.reset(stream)
        self.desk.reset(stream)

    def fill(self, xs, src=None, dst=None):
        src, dst = src or self.src, dst or self.dst
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        src.array[:] = POISON
        for s, x in enumerate(xs):
            src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        dst.array[:] = SENTINEL
        return counts

    def check_state(self):
        gain, power, share = self.m.state()
        want = self.desk.state()
        assert gain.tolist() == want[0], "gain"
        assert power.tolist() == want[1], "power"
        assert share.tolist() == want[2], "share"

    def check_output(self, wants, dst=None):
        for s, want in enumerate(wants):
            n = want.size
            row = (dst or self.dst).array[s]
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
        wants = self.desk.run(xs)
        self.check_output(wants)
        self.check_state()
        return wants


def case_rig(cm, channels, w):
    rig = Rig(cm, AM.CASE_STREAMS, channels, w, 5 * (1 << w) + 3)
    for s in range(AM.CASE_STREAMS):
        rig.set(s, AM.palette(s))
        if AM.CASE_GROUPS[s] >= 0:
            rig.set_group(s, AM.CASE_GROUPS[s])
    return rig


def play(rig, signals, cuts):
    """the streams' signals through the rig, cut as `cuts` says -> (per stream the output, the final state)"""
    at = [0] * rig.S
    out = [[] for _ in range(rig.S)]
    for counts in cuts:
        wants = rig.run([signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)])
        for s, n in enumerate(counts):
            out[s].append(wants[s])
            at[s] += n
    return [np.concatenate(o) for o in out], tuple(v.tolist() for v in rig.m.state())


@pytest.mark.parametrize("channels,w", AM.CASE_SHAPES)
def test_equals_the_model(gpu, channels, w):
    """S = 7: groups {0, 1, 2} and {3, 4}, stream 5 in no group, {6} alone under group id S - 1; output, gains, powers
    and shares after every run"""
    signals, cuts = AM.case(channels, w)
    rig = case_rig(gpu, channels, w)
    try:
        out, _ = play(rig, signals, cuts)
        assert all(t.n == len(signals[0]) for t in rig.desk.st)
        assert np.array_equal(out[5], signals[5])
        assert all(rig.desk.trace[b] > 0 for b in AM.BRANCHES), rig.desk.trace
        assert all(sq <= 2 ** 24 for sq, bare in rig.desk.squares if bare) and any(bare for _, bare in rig.desk.squares)
    finally:
        rig.close()


@pytest.mark.parametrize("channels,w", [(1, 6), (3, 6), (2, 8)])
def test_output_does_not_depend_on_the_cuts(gpu, channels, w):
    """the same streams under the case's ragged cuts and in the fewest runs: identical output and state"""
    W = 1 << w
    signals, cuts = AM.case(channels, w)
    total = len(signals[0])
    long_cuts, left = [], total
    while left:
        long_cuts.append([min(left, 5 * W + 3)] * AM.CASE_STREAMS)
        left -= long_cuts[-1][0]
    assert len(long_cuts) < len(cuts) - 2
    outs = []
    for c in (cuts, long_cuts):
        rig = case_rig(gpu, channels, w)
        try:
            outs.append(play(rig, signals, c))
        finally:
            rig.close()
    for s in range(AM.CASE_STREAMS):
        assert np.array_equal(outs[0][0][s], outs[1][0][s]), s
    assert outs[0][1] == outs[1][1]


def square(frames, channels, amp=8000, half=5):
    n = np.arange(frames)
    return np.where((n // half) % 2 == 0, amp, -amp).astype(np.int16)[:, None].repeat(channels, axis=1)


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_the_issues_figures(gpu, channels):
    """n members with equal input each get isqrt(2^24 / n): 4096, 2896, 2364, 2048; against members at digital silence
    one talker gets 4096 and the silent ones their floor"""
    W = 64
    for n, want in ((1, 4096), (2, 2896), (3, 2364), (4, 2048)):
        rig = Rig(gpu, 4, channels, 6, 4 * W)
        try:
            for s in range(n):
                rig.set_group(s, 2)
            xs = [square(4 * W, channels) for _ in range(4)]
            ys = rig.run(xs, uniform=True)
            gain, power, share = rig.m.state()
            assert gain.tolist() == [want] * n + [4096] * (4 - n) and share.tolist() == gain.tolist()
            assert power.tolist() == [(8000 * 8000) << 8] * n + [0] * (4 - n)
            if n > 1:
                assert set(np.unique(ys[0][3 * W:]).tolist()) == {(8000 * want + 2048) >> 12, (-8000 * want + 2048) >> 12}
        finally:
            rig.close()
    rig = Rig(gpu, 4, channels, 6, 3 * W)
    try:
        for s in range(4):
            rig.set(s, AM.params(floor=100 * s))
            rig.set_group(s, 3)
        rig.run([square(3 * W, channels)] + [np.zeros((3 * W, channels), dtype=np.int16)] * 3, uniform=True)
        assert rig.m.state()[0].tolist() == [4096, 100, 200, 300]
    finally:
        rig.close()


@pytest.mark.parametrize("channels,w", [(1, 6), (2, 8), (5, 6), (16, 6)])
def test_copies(gpu, channels, w):
    """streams in no group, and a group of one from its third window on, give the input back, full scale included"""
    W = 1 << w
    rig = Rig(gpu, 3, channels, w, 5 * W + 3)
    try:
        rig.set(1, AM.params(initial=0, floor=0))
        rig.set_group(1, 0)
        rng = np.random.default_rng(w + channels)
        seen = 0
        for k, n in enumerate([W + 1, 5 * W + 3, 0, 2 * W + 5]):
            xs = [rng.integers(-32768, 32768, size=(n, channels)).astype(np.int16) for _ in range(3)]
            for x in xs:
                x[::7] = -32768
                x[3::11] = 32767
            wants = rig.run(xs)
            for s in (0, 2):
                assert np.array_equal(xs[s], wants[s])
            lo = max(0, 2 * W - seen)                                    # the group of one: from frame 2 W on
            assert np.array_equal(xs[1][lo:], wants[1][lo:])
            if k == 0:
                assert not wants[1][:W].any()                            # (and its first window at initial 0: silence)
            seen += n
    finally:
        rig.close()


def test_one_group_of_300_streams(gpu):
    """several workgroups of the lane-per-stream kernels add into one group's sums: 300 mono streams, 3 windows"""
    W, S = 64, 300
    rig = Rig(gpu, S, 1, 6, 3 * W)
    try:
        for s in range(S):
            rig.set_group(s, 299)
        rig.set(7, AM.params(weight=1000, floor=50, attack=1))
        rng = np.random.default_rng(300)
        amps = rng.integers(0, 30000, size=S)
        xs = [rng.integers(-int(a), int(a) + 1, size=(3 * W, 1)).astype(np.int16) for a in amps]
        rig.run([x[:W + 9] for x in xs])
        rig.run([x[W + 9:] for x in xs], uniform=True)
        gain = rig.m.state()[0].astype(np.int64)
        # (one floor, 50, is not 0; the loudest of 300 has at least 1 / 300 of the sum: isqrt(2^24 / 300) = 236)
        assert (gain ** 2).sum() - 50 ** 2 <= 2 ** 24 and gain.max() >= 236
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# set, set_group, reset, refusals

@pytest.mark.parametrize("channels", [1, 2, 3])
def test_set_behind_a_queued_run_needs_no_wait(gpu, channels):
    """run A, set, run B with no host wait in between: run A's windows keep the old parameters, run B's take the new"""
    W, S = 64, 3
    rig = Rig(gpu, S, channels, 6, 5 * W + 3)
    src_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride))
    dst_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    try:
        for s in range(S):
            rig.set_group(s, 1)
        sig = [AM.spurts(90 + s, 12 * W, channels, W, quiet_first=0) + (s + 1) * square(12 * W, channels, amp=900) for s in range(S)]
        rig.run([x[:3 * W + 5] for x in sig])
        xa = [x[3 * W + 5:5 * W + 8] for x in sig]
        xb = [x[5 * W + 8:10 * W] for x in sig]
        new = AM.params(weight=300, floor=1500, attack=0, release=0, initial=7)
        rig.fill(xa)
        rig.fill(xb, src_b, dst_b)
        # the device: run A, the set on stream 0, run B -- and only then a wait
        rig.m.run(rig.src.dev, rig.in_stride, 2 * W + 3, rig.dst.dev, rig.out_stride)
        rig.m.set(0, gpu.AutomixParams(**new))
        rig.m.run(src_b.dev, rig.in_stride, 5 * W - 8, dst_b.dev, rig.out_stride)
        rig.m.sync()
        # the model: run A with the old parameters, then the set, then run B
        rig.check_output(rig.desk.run(xa))
        unset = copy.deepcopy(rig.desk)
        rig.desk.set(0, new)
        want_b = rig.desk.run(xb)
        rig.check_output(want_b, dst_b)
        rig.check_state()
        without = unset.run(xb)
        assert any(not np.array_equal(a, b) for a, b in zip(without, want_b))            # the set mattered
    finally:
        src_b.free()
        dst_b.free()
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_set_group_and_reset_restart_whole_groups(gpu, channels):
    W = 64
    signals, _ = AM.case(channels, 6)
    rig = case_rig(gpu, channels, 6)
    try:
        at = 0

        def go(n, per=None):
            nonlocal at
            counts = per or [n] * 7
            rig.run([signals[s][at:at + c] for s, c in enumerate(counts)])
            at += n

        go(3 * W + 7)                                                    # every stream inside an open window
        rig.reset(4)                                                     # group {3, 4} restarts, nobody else
        assert rig.desk.st[3].n == 0 and rig.desk.st[0].n == 3 * W + 7
        rig.check_state()
        go(W + 1)
        rig.set_group(2, 1)                                              # {0, 1, 2} and {3, 4} both restart: {0, 1}, {2, 3, 4}
        assert [t.n for t in rig.desk.st] == [0, 0, 0, 0, 0, 4 * W + 8, 4 * W + 8]
        rig.check_state()
        go(2 * W + 3, [2 * W + 3, 2 * W + 3, 5, 5, 5, 0, W])             # the new groups on clocks of their own
        rig.set_group(5, 6)                                              # the stream in no group joins {6}: both restart
        rig.set_group(0, -1)                                             # 0 leaves: {1} restarts, 0 becomes a copy
        rig.check_state()
        go(2 * W)
        rig.reset()
        assert all(t.n == 0 for t in rig.desk.st)
        go(W + 3)
    finally:
        rig.close()


def _host():
    spec = importlib.util.spec_from_file_location("test_automix_host_for_gpu", os.path.join(os.path.dirname(__file__), "test_automix_host.py"))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    return host


def test_refusals_of_a_real_object(gpu):
    """the checks tests/test_automix_host.py makes on an object without a device, on one with; a refused run in
    between two runs changes nothing"""
    d = gpu.Automixer(3, 2, 6, 64)
    try:
        _host().check_object_refusals(gpu, d)
    finally:
        d.close()
    W = 64
    rig = Rig(gpu, 3, 1, 6, 2 * W)
    try:
        for s in (0, 2):
            rig.set_group(s, 0)
        x = [square(4 * W, 1, amp=1000 * (s + 1)) for s in range(3)]
        rig.run([v[:W + 5] for v in x])
        before = rig.dst.array.copy()
        rc = rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W, rig.dst.dev, rig.out_stride, np.array([9, 9, 8], dtype=np.uint32))
        assert rc == gpu.ERROR_INVAL and "stream 0 has 9 frames" in gpu.last_error() and "has 8" in gpu.last_error()
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W, rig.dst.dev, 8) == gpu.ERROR_INVAL
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride) == 0          # a run of no frames
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride, np.zeros(3, dtype=np.uint32)) == 0
        rig.m.sync()
        assert np.array_equal(rig.dst.array, before)
        rig.check_state()
        rig.run([v[W + 5:3 * W] for v in x])
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# the stage contract (tests/test_gpu_stage_contract.py holds the other nine stages to it)

def test_readbacks_are_complete_and_repeatable(gpu):
    W = 64
    rig = Rig(gpu, 2, 2, 6, 3 * W)
    try:
        rig.set_group(0, 0)
        rig.set_group(1, 0)
        rig.run([square(3 * W, 2, amp=a) for a in (3000, 5000)], uniform=True)
        a, b = rig.m.state(), rig.m.state()
        assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[0].tolist() != [4096, 4096]
    finally:
        rig.close()


def test_stream_ownership(gpu):
    """an object made without a stream has one of its own; one made on a caller's stream reports that stream and leaves
    it usable when it goes"""
    W = 64
    big = gpu.Batch(2, 2, 4096, flags=gpu.OUT_PCM | gpu.VU)
    try:
        st = big.hip_stream()
        own, lent = Rig(gpu, 2, 1, 6, 2 * W), Rig(gpu, 2, 1, 6, 2 * W, hip_stream=st)
        try:
            assert own.m.hip_stream() not in (0, st) and lent.m.hip_stream() == st
            for r in (own, lent):
                r.set_group(0, 1)
                r.set_group(1, 1)
                r.run([square(2 * W, 1, amp=a) for a in (700, 9000)])
            lent.m.close()
            big.generate(gpu.GEN_NOISE, 1, 4096)
            big.run(4096)
            big.sync()
            own.run([square(W, 1, amp=a) for a in (9000, 700)])
        finally:
            own.close()
            lent.close()
    finally:
        big.close()


def test_create_and_close_without_a_run(gpu):
    """creation queues the object's first fills on its stream; close() without a run waits for them and returns, and a
    second object of the same shape runs as the model says"""
    gpu.Automixer(5, 3, 7, 1000).close()
    rig = Rig(gpu, 5, 3, 7, 1000)
    try:
        for s in range(4):
            rig.set_group(s, 4)
        rng = np.random.default_rng(1)
        for n in (1000, 333):
            rig.run([rng.integers(-3000 * (s + 1), 3000 * (s + 1), size=(n, 3)).astype(np.int16) for s in range(5)])
    finally:
        rig.close()
