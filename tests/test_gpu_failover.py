"""GPU: the failover switch (cmhip_failover_*, csrc/k_failover.hip) through the C ABI and the Python mirror.

Bar: bit-exact against tests/failover_model.py -- the arithmetic include/coolmic_hip.h specifies, walked window by window
in Python integers, written from the header's text -- in output, plan state, counters, levels and `switches` after every
run, never another run of the device code; what a run does not own of the output keeps its sentinel, and the input past
a count is poison.  tests/test_failover_host.py runs the same model against its emulation of the step kernel's walk,
without a GPU.

Shapes: w = 6 (and 7 once), run lengths 1, W-1, W, W+1, 2W+3, 0 and max_frames = 5W+3, rotated per output; S = 6 inputs,
O = 5 outputs with K in 1, 2, 4, input 5 the backup of three outputs, input 4 read by nobody; strides wider than the run.
The counter saturation is the one branch no device run reaches (65535 windows): tests/test_failover_host.py plants it.
"""
import types

import numpy as np
import pytest

import failover_model as FM

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past the run's frames


def stride_of(max_frames, channels, extra):
    return (max_frames * channels + 7) // 8 * 8 + extra


class Rig:
    """a switch between two arrays of pinned, device-mapped host memory, and the model of it"""

    def __init__(self, cm, streams, outputs, channels, w, max_frames, hip_stream=None):
        self.cm, self.S, self.O, self.C, self.w = cm, streams, outputs, channels, w
        self.m = cm.Failover(streams, outputs, channels, w, max_frames, hip_stream=hip_stream)
        self.in_stride = stride_of(max_frames, channels, 8)                 # wider than any run
        self.out_stride = stride_of(max_frames, channels, 16)
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=outputs, stride=self.out_stride))
        self.model = FM.Switch(streams, outputs, channels, w)

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def params(self, p):
        return self.cm.failover_params(self.w, **p)

    def set(self, output, p):
        self.m.set(output, self.params(p))
        self.model.set(output, p)
        for o in (range(self.O) if output < 0 else [output]):
            assert self.m.get(o).as_dict() == p

    def set_sources(self, output, streams):
        self.m.set_sources(output, streams)
        self.model.set_sources(output, streams)
        assert self.m.get_sources(output) == list(streams) and self.m.get(output).force == -1

    def reset(self, output=-1):
        self.m.reset(output)
        self.model.reset(output)

    def fill(self, slots, src=None, dst=None):
        src, dst = src or self.src, dst or self.dst
        src.array[:] = POISON
        for s, x in enumerate(slots):
            x = np.asarray(x, dtype=np.int16).reshape(-1)
            src.array[s, :x.size] = x
        dst.array[:] = SENTINEL

    def check_state(self):
        have, want = self.m.state(), self.model.state()
        for k, name in (("from", "fr"), ("to", "to"), ("fade_window", "fade_window"), ("switches", "switches"),
                        ("live_run", "live_run"), ("dead_run", "dead_run"), ("level", "level")):
            assert have[k].tolist() == want[name], (k, have[k].tolist(), want[name])

    def check_output(self, wants, dst=None):
        for o, want in enumerate(wants):
            n = want.size
            row = (dst or self.dst).array[o]
            have = row[:n].reshape(-1, self.C)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("output", o, "first mismatch (frame, channel)", bad[0].tolist(), "of", want.shape[0],
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (row[n:] == SENTINEL).all(), ("output", o, "written past its count")

    def run(self, slots, counts, uniform=False):
        """slots: per input int16 [frames][C]; counts per output; runs device and model, compares outputs, the
        untouched rest and the state -> per output the model's int16 [count][C]"""
        self.fill(slots)
        self.m.run(self.src.dev, self.in_stride, max(counts), self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = self.model.run(slots, counts)
        self.check_output(wants)
        self.check_state()
        return wants


# ---------------------------------------------------------------------------
# the case: FM.case_script's runs, sets, new lists and resets, played to device and model (tests/test_failover_host.py
# plays it to the model alone first, and asks for every branch there)

def play(rig, ops):
    for op in ops:
        if op[0] == "run":
            rig.run(op[1], op[2])
        elif op[0] == "set":
            rig.set(op[1], op[2])
        elif op[0] == "sources":
            rig.set_sources(op[1], op[2])
        else:
            rig.reset(op[1])


@pytest.mark.parametrize("channels,w", FM.CASE_SHAPES)
def test_equals_the_model(gpu, channels, w):
    """output, plan state, counters, levels and switches after every run of the case"""
    ops = FM.case_script(channels, w)
    rig = Rig(gpu, FM.CASE_STREAMS, FM.CASE_OUTPUTS, channels, w, 5 * (1 << w) + 3)
    try:
        play(rig, ops)
        assert all(rig.model.trace[b] > 0 for b in FM.BRANCHES), rig.model.trace
        assert sum(rig.model.state()["switches"]) > 10
    finally:
        rig.close()


def uniform_case(channels, w, windows):
    W = 1 << w
    return FM.case_signals(channels, w, windows * W)


def cut_up(total, lens):
    cuts, left, i = [], total, 0
    while left:
        n = min(left, lens[i % len(lens)])
        i += 1
        if n:
            cuts.append(n)
            left -= n
    return cuts


@pytest.mark.parametrize("channels,w", [(1, 6), (3, 6), (2, 7)])
def test_output_does_not_depend_on_the_cuts(gpu, channels, w):
    """one signal under three cut sequences -- ragged, whole windows, the fewest runs -- with the sets at the same
    frames: equal output and state"""
    W = 1 << w
    total = 40 * W
    sig = uniform_case(channels, w, 40)
    at_set = 17 * W + 5
    results = []
    for lens in ([1, W - 1, W, W + 1, 2 * W + 3, 5 * W + 3], [W], [5 * W + 3]):
        rig = Rig(gpu, FM.CASE_STREAMS, FM.CASE_OUTPUTS, channels, w, 5 * W + 3)
        try:
            for o in range(FM.CASE_OUTPUTS):
                rig.set_sources(o, FM.CASE_SOURCES[o])
                rig.set(o, FM.case_params(w, o))
            outs, at = [[] for _ in range(rig.O)], 0
            for part, stop in ((0, at_set), (1, total)):
                if part:
                    rig.set(0, dict(FM.case_params(w, 0), fade_log2=w, fail_windows=1))
                    rig.set(1, dict(FM.case_params(w, 1), force=3))
                for n in cut_up(stop - at, lens):
                    ys = rig.run([x[at:at + n] for x in sig], [n] * rig.O, uniform=True)
                    at += n
                    for o, y in enumerate(ys):
                        outs[o].append(y)
            results.append(([np.concatenate(o) for o in outs], rig.model.state(), {k: v.tolist() for k, v in rig.m.state().items()}))
        finally:
            rig.close()
    for other in results[1:]:
        for o in range(FM.CASE_OUTPUTS):
            assert np.array_equal(results[0][0][o], other[0][o]), o
        assert results[0][1] == other[1] and results[0][2] == other[2]
    assert sum(results[0][1]["switches"]) > 5


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_thresholds_are_exact(gpu, channels):
    """windows whose m is exactly quiet^2 are not live, windows with quiet^2 + 1 are; full scale is m = 2^30"""
    w, W = 6, 64
    rig = Rig(gpu, 2, 1, channels, w, 4 * W)
    try:
        rig.set_sources(0, [0, 1])
        ones = np.ones((W, channels), dtype=np.int16)
        twos = np.zeros((W, channels), dtype=np.int16)
        twos[::2] = 2
        short = twos.copy()
        short[0] = 0                                                      # E = 2 W - 4: m = 1
        full = np.full((W, channels), -32768, dtype=np.int16)
        x0 = np.concatenate([ones, twos, short, full])
        x1 = np.concatenate([-ones, ones, ones, ones])
        rig.set(0, FM.params(w, quiet=(1, 0, 33, 33), fail_windows=9, return_windows=9))
        rig.run([x0[:2 * W + 7], x1[:2 * W + 7]], [2 * W + 7])
        st = rig.m.state()
        assert st["level"][0].tolist() == [2, 1, 0, 0]
        # window 0 (m = 1 = quiet^2) was dead, window 1 (m = 2) live -- of candidate 1 (quiet 0, m = 1) both live
        assert st["live_run"][0].tolist()[:2] == [1, 2] and st["dead_run"][0].tolist()[:2] == [0, 0]
        rig.run([x0[2 * W + 7:], x1[2 * W + 7:]], [2 * W - 7])
        st = rig.m.state()
        assert st["level"][0].tolist() == [1 << 30, 1, 0, 0]
        # (the counters hold what the last edge processed left: window 2, m = 1, dead again)
        assert st["live_run"][0].tolist()[:2] == [0, 3] and st["dead_run"][0].tolist()[:2] == [1, 0]
    finally:
        rig.close()


@pytest.mark.parametrize("channels,w", [(1, 6), (2, 8), (5, 6), (16, 6)])
def test_copies(gpu, channels, w):
    """K = 1, and an output that stays on its source, give the input back bit for bit, full scale included"""
    W = 1 << w
    rig = Rig(gpu, 3, 3, channels, w, 5 * W + 3)
    try:
        rig.set_sources(2, [1, 0])                                        # the main source never dies: steady on input 1
        rng = np.random.default_rng(5)
        for n in (5 * W + 3, 1, W + 1, 2 * W - 1):
            xs = [rng.integers(-32768, 32768, size=(n, channels)).astype(np.int16) for _ in range(3)]
            xs[0][n // 2:] = 0
            ys = rig.run(xs, [n, n, n])
            assert np.array_equal(ys[0], xs[0]) and np.array_equal(ys[1], xs[1]) and np.array_equal(ys[2], xs[1])
        assert rig.m.state()["switches"].tolist() == [0, 0, 0]
    finally:
        rig.close()


@pytest.mark.parametrize("channels,w", [(3, 9), (2, 11), (1, 12)])
def test_windows_of_several_tiles(gpu, channels, w):
    """w above the tile's size (256 frames for any channel count, 1024 stereo, 2048 mono): a window's tiles share one
    plan word, and a fade's position runs on through them"""
    W = 1 << w
    rig = Rig(gpu, 2, 2, channels, w, 2 * W + 77)
    try:
        rig.set_sources(0, [0, 1])
        rig.set_sources(1, [1, 0])
        rig.set(0, FM.params(w, fade_log2=w + 1))
        rig.set(1, FM.params(w, quiet=(20000, 33, 33, 33)))                # its main source never counts as live
        rng = np.random.default_rng(w)
        sig = [rng.integers(-9000, 9001, size=(7 * W, channels)).astype(np.int16) for _ in range(2)]
        sig[0][W + 5:4 * W] = 0
        at = 0
        for n in (W + 3, 2 * W + 77, 1, W - 81, 2 * W, W):
            rig.run([x[at:at + n] for x in sig], [n, max(n - 9, 0)])
            at += n
        assert at == 7 * W and rig.model.state()["switches"] == [2, 1]
    finally:
        rig.close()


def test_more_outputs_than_a_workgroup_of_step_lanes(gpu):
    """300 outputs with lists drawn from 7 inputs, two ragged runs"""
    w, W, O, S = 6, 64, 300, 7
    rig = Rig(gpu, S, O, 2, w, 3 * W)
    try:
        rng = np.random.default_rng(300)
        for o in range(O):
            k = int(rng.integers(1, 5))
            rig.set_sources(o, [int(v) for v in rng.permutation(S)[:k]])
            rig.set(o, FM.params(w, quiet=tuple(int(v) for v in rng.integers(0, 3000, size=4)),
                                 fail_windows=int(rng.integers(1, 3)), return_windows=int(rng.integers(1, 3)),
                                 fade_log2=w + int(rng.integers(0, 2))))
        sig = [FM.spurts(70 + s, 9 * W, 2, W, amp=4000) for s in range(S)]
        at = 0
        for n in (3 * W, 2 * W + 9, 3 * W, W - 9):
            counts = [int(v) for v in rng.integers(0, n + 1, size=O)]
            counts[0] = n
            rig.run([x[at:at + n] for x in sig], counts)
            at += n
        assert sum(rig.model.state()["switches"]) > 50
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_calls_behind_queued_runs_need_no_wait(gpu, channels):
    """run A, a set, a new list and a reset, run B, with no host wait in between: run A keeps the old settings, run B
    takes the new"""
    w, W, S, O = 6, 64, 4, 3
    rig = Rig(gpu, S, O, channels, w, 5 * W + 3)
    src_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride))
    dst_b = gpu.MappedPcm(types.SimpleNamespace(streams=O, stride=rig.out_stride))
    try:
        for o in range(O):
            rig.set_sources(o, [o, 3])
            rig.set(o, FM.params(w, quiet=(500, 500, 500, 500), fade_log2=w + 1))
        sig = [FM.spurts(40 + s, 12 * W, channels, W) for s in range(S)]
        sig[3] = FM.spurts(44, 12 * W, channels, 16 * W)                 # the backup: one long spurt
        sig[3][:] = np.where(sig[3] == 0, 7000, sig[3])
        n0, na, nb = 3 * W + 5, 2 * W + 3, 5 * W - 8
        rig.run([x[:n0] for x in sig], [n0] * O)
        xa = [x[n0:n0 + na] for x in sig]
        xb = [x[n0 + na:n0 + na + nb] for x in sig]
        rig.fill(xa)
        rig.fill(xb, src_b, dst_b)
        # the device: run A, the calls, run B -- and only then a wait
        rig.m.run(rig.src.dev, rig.in_stride, na, rig.dst.dev, rig.out_stride)
        rig.m.set(0, rig.params(FM.params(w, quiet=(500, 500, 500, 500), force=1)))
        rig.m.set_sources(1, [3, 2, 1])
        rig.m.reset(2)
        rig.m.run(src_b.dev, rig.in_stride, nb, dst_b.dev, rig.out_stride)
        rig.m.sync()
        # the model: run A with the old settings, then the calls, then run B
        rig.check_output(rig.model.run(xa, [na] * O))
        rig.model.set(0, FM.params(w, quiet=(500, 500, 500, 500), force=1))
        rig.model.set_sources(1, [3, 2, 1])
        rig.model.reset(2)
        rig.check_output(rig.model.run(xb, [nb] * O), dst_b)
        rig.check_state()
        assert rig.model.out[0].plan[1] == 1 and rig.model.out[2].n == nb
    finally:
        src_b.free()
        dst_b.free()
        rig.close()


def test_refusals_and_an_empty_run(gpu):
    """a refused run between two runs changes nothing; a run of no frames is fine; switches clears on demand"""
    w, W = 6, 64
    rig = Rig(gpu, 2, 2, 1, w, 2 * W)
    try:
        rig.set_sources(0, [0, 1])
        x = [FM.spurts(3, 4 * W, 1, W), np.full((4 * W, 1), 900, dtype=np.int16)]
        rig.run([v[:W + 5] for v in x], [W + 5, 9])
        before = rig.dst.array.copy()
        bad = np.array([2 * W + 1, 0], dtype=np.uint32)
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W, rig.dst.dev, rig.out_stride, bad) == gpu.ERROR_INVAL
        assert "frames_per_output[0]" in gpu.last_error()
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W + 1, rig.dst.dev, rig.out_stride) == gpu.ERROR_INVAL
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W, rig.dst.dev, 8) == gpu.ERROR_INVAL
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 2 * W, rig.src.dev, rig.out_stride) == gpu.ERROR_INVAL
        assert rig.m.run_rc(0, rig.in_stride, 2 * W, rig.dst.dev, rig.out_stride) == gpu.ERROR_FAULT
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride) == 0
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride, np.zeros(2, dtype=np.uint32)) == 0
        rig.m.sync()
        assert np.array_equal(rig.dst.array, before)
        rig.check_state()
        rig.run([v[W + 5:3 * W] for v in x], [2 * W - 5, 2 * W - 5])
        n = rig.m.state(clear=True)["switches"].tolist()
        assert n == rig.model.state()["switches"] and rig.m.state()["switches"].tolist() == [0, 0]
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# the stage contract (tests/test_gpu_stage_contract.py holds the other stages to it)

def test_readbacks_are_complete_and_repeatable(gpu):
    w, W = 6, 64
    rig = Rig(gpu, 2, 1, 2, w, 4 * W)
    try:
        rig.set_sources(0, [0, 1])
        x = [np.zeros((4 * W, 2), dtype=np.int16), np.full((4 * W, 2), 5000, dtype=np.int16)]
        rig.run(x, [4 * W], uniform=True)
        a, b = rig.m.state(), rig.m.state()
        assert all(np.array_equal(a[k], b[k]) for k in a) and a["to"].tolist() == [1] and a["switches"].tolist() == [1]
    finally:
        rig.close()


def test_stream_ownership_and_creation_without_a_run(gpu):
    """an object made without a stream has one of its own; one made on a caller's stream reports that stream and leaves
    it usable when it goes; close() without a run returns"""
    w, W = 6, 64
    gpu.Failover(5, 7, 3, 7, 1000).close()
    big = gpu.Batch(2, 2, 4096, flags=gpu.OUT_PCM | gpu.VU)
    try:
        st = big.hip_stream()
        own, lent = Rig(gpu, 2, 2, 1, w, 2 * W), Rig(gpu, 2, 2, 1, w, 2 * W, hip_stream=st)
        try:
            assert own.m.hip_stream() not in (0, st) and lent.m.hip_stream() == st
            x = [FM.spurts(8, 2 * W, 1, W), np.full((2 * W, 1), -700, dtype=np.int16)]
            for r in (own, lent):
                r.set_sources(0, [0, 1])
                r.run(x, [2 * W, 2 * W])
            lent.m.close()
            big.generate(gpu.GEN_NOISE, 1, 4096)
            big.run(4096)
            big.sync()
            own.run([v[:W] for v in x], [W, 5])
        finally:
            own.close()
            lent.close()
    finally:
        big.close()
