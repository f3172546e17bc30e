"""GPU: the noise suppressor (cmhip_denoise_*, csrc/k_denoise.hip) through the C ABI and the Python mirror.

Bar: bit-exact against tests/denoise_model.py, the numpy model of the arithmetic include/coolmic_hip.h specifies, after
every run: the output, what a run does not own of it (it keeps its sentinel), clips, sat, learned_blocks, and g and Np of
every row through cmhip_denoise_get_profile -- never another run of the device code.  tests/test_denoise_host.py runs the
same model against its emulation of the kernel's decomposition, without a GPU.

Shapes: N = 2^n, H = N / 2.  The scenario of most cases: quiet noise while the streams learn, then learning off, a
suppressing parameter set and a loud signal; cut into runs of 1, 0, H - 1, N + 3 and the rest, dealt round the streams
so that every run's counts are ragged and one of them is 0.
"""
import types

import numpy as np
import pytest

import denoise_model as DM

pytestmark = pytest.mark.gpu
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past a stream's count
MID = DM.params(floor=4125, over=64, rise_shift=1, fall_shift=2)


def stride_of(max_frames, channels, extra):
    return (max_frames * channels + 7) // 8 * 8 + extra


class Rig:
    """a suppressor between two arrays of pinned, device-mapped host memory, and one model per stream"""

    def __init__(self, cm, streams, channels, n, max_frames):
        self.cm, self.S, self.C, self.n = cm, streams, channels, n
        self.tab = DM.Tables(cm, n)
        self.m = cm.Denoiser(streams, channels, n, max_frames)
        assert self.m.delay() == self.tab.N - 1
        self.in_stride = stride_of(max_frames, channels, 8)                 # wider than any run
        self.out_stride = stride_of(max_frames, channels, 16)
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.models = [DM.Stream(self.tab, channels) for _ in range(streams)]

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def each(self, stream):
        return range(self.S) if stream < 0 else [stream]

    def set(self, stream, p):
        self.m.set(stream, self.cm.DenoiseParams(**p))
        for s in self.each(stream):
            self.models[s].set(p)
            assert self.m.get(s).as_dict() == p

    def learn(self, stream, on):
        self.m.learn(stream, on)
        for s in self.each(stream):
            self.models[s].learn(on)

    def reset(self, stream=-1):
        self.m.reset(stream)
        for s in self.each(stream):
            self.models[s].reset()

    def set_profile(self, stream, channel, profile):
        self.m.set_profile(stream, channel, profile)
        self.models[stream].set_profile(channel, profile)

    def fill(self, xs, src=None, dst=None):
        src = self.src if src is None else src
        dst = self.dst if dst is None else dst
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        src.array[:] = POISON
        for s, x in enumerate(xs):
            src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        dst.array[:] = SENTINEL
        return counts

    def check_state(self):
        clips, sat, learned = self.m.state()
        want = [m.state() for m in self.models]
        assert clips.tolist() == [v[0] for v in want], "clips"
        assert sat.tolist() == [v[1] for v in want], "sat"
        assert learned.tolist() == [v[2] for v in want], "learned_blocks"
        for s, m in enumerate(self.models):
            for c, row in enumerate(m.rows):
                q, g = self.m.get_profile(s, c)
                assert g.tolist() == row.g, ("g", s, c)
                assert [int(v) for v in q] == row.np, ("Np", s, c)

    def check_output(self, wants, dst=None):
        dst = self.dst if dst is None else dst
        for s, want in enumerate(wants):
            n = want.size
            row = dst.array[s]
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
        wants = [m.run(np.asarray(x).reshape(-1, self.C)) for m, x in zip(self.models, xs)]
        self.check_output(wants)
        self.check_state()
        return wants


def scenario_signal(seed, N, channels, quiet=3, loud=4, extra=37):
    """quiet noise (amplitude 400) for quiet * N frames, then loud (30000) for loud * N + extra"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-400, 401, size=(quiet * N, channels))
    b = rng.integers(-30000, 30001, size=(loud * N + extra, channels))
    return np.concatenate((a, b)).astype(np.int16)


def dealt(lengths, streams):
    """runs of a phase: stream s gets the lengths rotated by s, so every run's counts are ragged"""
    k = len(lengths)
    return [[lengths[(r + s) % k] for s in range(streams)] for r in range(k)]


def scenario(cm, streams, channels, n, cut, seed):
    """learn over the quiet part, then MID over the loud part; cut: False -- a run per phase; True -- runs of 1, 0, H - 1,
    N + 3 and the rest per phase, dealt round the streams -> (per stream the concatenated output, the final state)"""
    tab_N = 1 << n
    H = tab_N // 2
    sig = [scenario_signal(seed + s, tab_N, channels) for s in range(streams)]
    L1, L2 = 3 * tab_N, 4 * tab_N + 37
    phases = []
    for L in (L1, L2):
        phases.append(dealt([1, 0, H - 1, tab_N + 3, L - (tab_N + H + 3)], streams) if cut else [[L] * streams])
    rig = Rig(cm, streams, channels, n, max(L1, L2))
    try:
        at = [0] * streams
        out = [[] for _ in range(streams)]
        for k, runs in enumerate(phases):
            if k == 0:
                rig.learn(-1, True)
            else:
                rig.learn(-1, False)
                rig.set(-1, MID)
            assert not cut or any(0 in counts for counts in runs)            # and a stream that gets nothing
            for counts in runs:
                assert not cut or len(set(counts)) > 1 or streams == 1       # ragged
                wants = rig.run([sig[s][at[s]:at[s] + c] for s, c in enumerate(counts)])
                for s, c in enumerate(counts):
                    out[s].append(wants[s])
                    at[s] += c
        assert at == [L1 + L2] * streams
        m = rig.models[0]
        assert m.cnt == (L1 - tab_N) // H + 1 and any(g != DM.UNITY for g in m.rows[0].g)
        state = [m.state() for m in rig.models]
        return [np.concatenate(o) for o in out], state
    finally:
        rig.close()


# ---------------------------------------------------------------------------

def test_defaults_are_the_input_delayed(gpu):
    """(a) n = 8, S = 3, C = 2, 7 H + 37 frames at the creation defaults: the input N - 1 frames later, bit for bit,
    full scale included, and every counter zero"""
    n, N, H = 8, 256, 128
    F = 7 * H + 37
    rig = Rig(gpu, 3, 2, n, F)
    try:
        rng = np.random.default_rng(8)
        xs = [rng.integers(-32768, 32768, size=(F, 2)).astype(np.int16) for _ in range(3)]
        for x in xs:
            x[::7] = -32768
            x[3::11] = 32767
        wants = rig.run(xs, uniform=True)
        for x, y in zip(xs, wants):
            assert np.array_equal(y[N - 1:], x[:F - (N - 1)]) and not y[:N - 1].any()
        clips, sat, learned = rig.m.state()
        assert not clips.any() and not sat.any() and not learned.any()
    finally:
        rig.close()


def test_learned_noise_then_signal_in_one_run_and_cut(gpu):
    """(b) n = 8, S = 3, C = 2: the phases in one run each, and cut into runs of 1, 0, H - 1, N + 3 and the rest with
    ragged counts; the concatenations, the counters and the state are equal"""
    a, sa = scenario(gpu, 3, 2, 8, False, 100)
    b, sb = scenario(gpu, 3, 2, 8, True, 100)
    for s in range(3):
        assert np.array_equal(a[s], b[s]), s
    assert sa == sb


@pytest.mark.parametrize("channels", [1, 3, 16])
def test_channel_counts(gpu, channels):
    """(c) C in {1, 3, 16} at S = 2, cut"""
    scenario(gpu, 2, channels, 8, True, 200 + channels)


@pytest.mark.parametrize("n", [9, 10, 11, 12])
def test_every_block_size(gpu, n):
    """(d) S = 2, C = 1, 4 N + 5 frames in two runs: a random profile through set_profile on stream 0 with MID, stream 1
    learns under a slower parameter set"""
    N = 1 << n
    F = 4 * N + 5
    rig = Rig(gpu, 2, 1, n, F)
    try:
        rng = np.random.default_rng(n)
        prof = rng.integers(0, 1 << 36, N // 2 + 1).astype(np.uint64)
        prof[::3] = 0
        prof[1] = 1 << 52
        rig.set_profile(0, 0, prof)
        rig.set(0, MID)
        rig.set(1, DM.params(floor=1000, over=40, rise_shift=3, fall_shift=0))
        rig.learn(1, True)
        xs = [rng.integers(-9000, 9001, size=(F, 1)).astype(np.int16) for _ in range(2)]
        rig.run([x[:N + 3] for x in xs], uniform=True)
        rig.run([xs[0][N + 3:], xs[1][N + 3:F - 7]])
        assert rig.models[1].cnt == (F - 7 - N) // (N // 2) + 1
        assert all(any(g != DM.UNITY for g in m.rows[0].g) for m in rig.models)
    finally:
        rig.close()


def test_three_hundred_streams(gpu):
    """(e) 300 streams x 1 channel x 3 H + 1 frames at n = 8: more rows than a wave of workgroups, two blocks each"""
    n, N, H, S = 8, 256, 128, 300
    F = 3 * H + 1
    rig = Rig(gpu, S, 1, n, F)
    try:
        rng = np.random.default_rng(300)
        rig.set(-1, MID)
        rig.learn(-1, True)
        rig.learn(7, False)
        xs = [rng.integers(-3000 - 90 * s, 3001 + 90 * s, size=(F if s % 9 else F - 1 - s % 5, 1)).astype(np.int16) for s in range(S)]
        rig.run(xs)
        assert [m.cnt for m in rig.models[:9]] == [2, 2, 2, 2, 2, 2, 2, 0, 2]
    finally:
        rig.close()


def test_calls_queued_behind_runs_need_no_wait(gpu):
    """(f) run, set, learn on, run, learn off, set_profile, run, reset, run -- and only then a wait; the refusals in between
    (BUSY while the stream learns, INVAL) change nothing"""
    n, N, H, S, C = 8, 256, 128, 3, 2
    F = N + H + 9
    rig = Rig(gpu, S, C, n, F)
    extra = [(gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride)),
              gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))) for _ in range(3)]
    bufs = [(rig.src, rig.dst)] + extra
    try:
        rng = np.random.default_rng(66)
        prof = (rng.integers(0, 1 << 30, N // 2 + 1).astype(np.uint64)) << np.uint64(8)
        too_big = prof.copy()
        too_big[5] = (1 << 52) + 1
        runs = [[rng.integers(-20000, 20001, size=(c, C)).astype(np.int16) for c in counts]
                for counts in ([F, F - 3, N], [F, H, F - 1], [N + 1, F, F], [F, F, 0])]
        for (src, dst), xs in zip(bufs, runs):
            rig.fill(xs, src, dst)
        counts = [[len(x) for x in xs] for xs in runs]

        def go(k):
            rig.m.run(bufs[k][0].dev, rig.in_stride, max(counts[k]), bufs[k][1].dev, rig.out_stride, counts[k])

        # the device: everything queued back to back
        go(0)
        rig.m.set(0, gpu.DenoiseParams(**MID))
        rig.m.set(2, gpu.DenoiseParams(**DM.params(floor=0, over=255)))
        rig.m.learn(1, True)
        rig.m.learn(2, True)
        assert rig.m.set_profile_rc(1, 0, prof) == gpu.ERROR_BUSY
        go(1)
        rig.m.learn(2, False)
        rig.m.set_profile(2, 1, prof)
        rig.m.set_profile(0, 0, prof)
        assert rig.m.set_profile_rc(0, 1, too_big) == gpu.ERROR_INVAL
        assert rig.m.set_rc(0, gpu.denoise_params(rise_shift=9)) == gpu.ERROR_INVAL
        go(2)
        rig.m.reset(0)
        rig.m.learn(1, False)
        go(3)
        rig.m.sync()
        # the models: the same calls in the same order
        M = rig.models
        wants = [[m.run(x) for m, x in zip(M, runs[0])]]
        M[0].set(MID)
        M[2].set(DM.params(floor=0, over=255))
        M[1].learn(True)
        M[2].learn(True)
        wants.append([m.run(x) for m, x in zip(M, runs[1])])
        M[2].learn(False)
        M[2].set_profile(1, prof)
        M[0].set_profile(0, prof)
        wants.append([m.run(x) for m, x in zip(M, runs[2])])
        M[0].reset()
        M[1].learn(False)
        wants.append([m.run(x) for m, x in zip(M, runs[3])])
        for k in range(4):
            rig.check_output(wants[k], bufs[k][1])
        rig.check_state()
        assert M[1].cnt > 0 and M[2].cnt > 0 and rig.m.get(0).as_dict() == MID
        # the reset mattered: stream 0's last run begins with N - 1 zeros
        assert not wants[3][0][:N - 1].any() and wants[2][0][:N - 1].any()
    finally:
        for a, b in extra:
            a.free()
            b.free()
        rig.close()


def saturating_case(tab, seed):
    """a random binary mask of removed bins and the block of +- full scale whose signs follow the mask's zero-phase
    kernel mirrored about the block's centre: the inverse transform's largest output, at the centre"""
    N, H = tab.N, tab.H
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 2, H + 1)
    h = np.fft.irfft(mask.astype(float), N)
    k = h[(N // 2 - np.arange(N)) % N]
    x = np.where(k >= 0, 32767, -32768).astype(np.int16)
    return np.where(mask == 1, 1 << 52, 0).astype(np.uint64), x


def test_saturation_of_the_inverse_transform(gpu):
    """(g) n = 10, seed 0 (found on the model: sat = 1 with a weighted L1 of 8.9 against the 8x headroom; at n = 8 and 9 the
    best of 60 seeds reach 4.9 and 6.6 and nothing saturates -- tests/cpp/denoise_plan_test.cpp holds sat32 there)"""
    n, N = 10, 1024
    rig = Rig(gpu, 2, 1, n, 2 * N)
    try:
        prof, x = saturating_case(rig.tab, 0)
        rig.set(-1, DM.params(floor=0))
        rig.set_profile(1, 0, prof)
        blk = np.concatenate((x, np.zeros(N, dtype=np.int16))).reshape(-1, 1)
        rig.run([blk, blk], uniform=True)
        assert rig.models[1].sat > 0 and rig.models[0].sat == 0
        assert rig.models[1].clips > 0                                   # x - r leaves int16 where r opposes x
        clips, sat, _ = rig.m.state(clear=True)
        assert sat[1] == rig.models[1].sat
        assert not rig.m.state()[0].any() and not rig.m.state()[1].any()                # cleared
    finally:
        rig.close()


def test_a_row_does_not_depend_on_its_neighbours(gpu):
    """(h) one loud row among silent ones, everything suppressing: the silent rows stay silent to the bit, and the loud
    row's output is what it is alone"""
    n, N, H, S, C = 8, 256, 128, 3, 3
    F = 3 * N + 11
    rig = Rig(gpu, S, C, n, F)
    try:
        rng = np.random.default_rng(12)
        prof = rng.integers(1 << 20, 1 << 30, H + 1).astype(np.uint64)
        for s in range(S):
            for c in range(C):
                rig.set_profile(s, c, prof)
        rig.set(-1, MID)
        loud = rng.integers(-32768, 32768, size=F).astype(np.int16)
        xs = [np.zeros((F, C), dtype=np.int16) for _ in range(S)]
        xs[1][:, 1] = loud
        wants = rig.run(xs, uniform=True)
        for s in range(S):
            for c in range(C):
                if (s, c) != (1, 1):
                    assert not wants[s][:, c].any()
        alone = DM.Stream(rig.tab, 1, MID)
        alone.set_profile(0, prof)
        assert np.array_equal(alone.run(loud.reshape(-1, 1))[:, 0], wants[1][:, 1]) and wants[1][:, 1].any()
    finally:
        rig.close()


def test_refusals_of_a_real_object(gpu):
    """the checks tests/test_denoise_host.py makes on an object without a device, on one with"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("test_denoise_host_for_gpu", os.path.join(os.path.dirname(__file__), "test_denoise_host.py"))
    host = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host)
    d = gpu.Denoiser(3, 2, 8, 64)
    try:
        host.check_object_refusals(gpu, d)
    finally:
        d.close()
