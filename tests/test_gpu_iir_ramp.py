"""GPU: the filter's coefficient ramps (cmhip_iir_ramp, csrc/k_iirramp.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy int64 model below of what include/coolmic_hip.h specifies -- every frame of every
section with a section c(p) of its own, the frame's arithmetic that of tests/test_gpu_iir.py's model -- in output,
`clips`, `overs`, the continued state of every section, and what cmhip_iir_get and cmhip_iir_ramp_state answer after
every run; what a run does not own of the output keeps its sentinel.  Never another run of the device code.
tests/test_iir_ramp_host.py runs the same model against an emulation of the two ramp kernels, without a GPU.

Shapes: B the plan's tile.  Run lengths ragged over {0, 1, 2, 7, 8, 9, B-1, B, B+1, 2B+1}, dealt as tests/test_gpu_iir.py
deals them; ramp lengths over {2, 3, B-1, B, B+1, 2B+1, 5B+7} and one of 2^20 that is only begun; ramps start in front of
different runs on different streams and sections, so that they end inside a tile, on a tile's edge and runs later, are
retargeted on the way, and share a launch with sections at rest.  The model's trace says what was met."""
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, tag):
    spec = importlib.util.spec_from_file_location(name + tag, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_iir", "_for_iir_ramp")         # the frame's arithmetic, the palette, the rig
ONE, BIG, V_MAX = TG.ONE, TG.BIG, TG.V_MAX
P_ONE = 32768
RAMP_MAX = 1 << 20
RAMP_BRANCHES = ("in_ramp", "past_end", "at_rest", "retarget", "b1_clamped")
# two ends between which the unclamped b1 passes 2^28: s moves from 2^28 + 6 to 2^28 while b0 and b2 truncate to 0
CORNER_A, CORNER_B = (3, BIG, 3, 0, 0), (0, BIG, 0, 0, 0)


# ---------------------------------------------------------------------------
# the specification in numpy

def position(n, R):
    """p(n), the mixer's: int64 arrays -> int64"""
    n, R = np.asarray(n, dtype=np.int64), np.asarray(R, dtype=np.int64)
    safe = np.maximum(R, 2)
    inc = ((1 << 32) + safe - 1) // safe
    p = np.minimum((np.minimum(n, safe) * inc) >> 17, P_ONE)
    return np.where(n == 0, 0, np.where(R < 2, P_ONE, p))


def ramp_section(c0, c1, p, trace=None, act=None):
    """c(p): c0, c1 int64 [..., 5], p int64 [...] -> int64 [..., 5]"""
    c0, c1, p = np.asarray(c0, dtype=np.int64), np.asarray(c1, dtype=np.int64), np.asarray(p, dtype=np.int64)
    q = P_ONE - p

    def trunc(x0, x1):
        N = x0 * q + x1 * p
        assert np.abs(N).max(initial=0) < 2 ** 45
        return np.sign(N) * (np.abs(N) >> 15)

    b0, b2, a1 = (trunc(c0[..., i], c1[..., i]) for i in (0, 2, 3))
    a2 = -((-(c0[..., 4] * q + c1[..., 4] * p)) >> 15)
    s = trunc(c0[..., :3].sum(axis=-1), c1[..., :3].sum(axis=-1))
    raw = s - b0 - b2
    b1 = np.clip(raw, -BIG, BIG)
    if trace is not None:
        trace["b1_clamped"] += int(((raw != b1) & act).sum())
    return np.stack([b0, b1, b2, a1, a2], axis=-1)


class RampModel(TG.Model):
    """tests/test_gpu_iir.py's model with a ramp per (stream, section): c0, c1 int64 [S][N][5], done, R int64 [S][N]"""

    def __init__(self, streams, channels, sections):
        super().__init__(streams, channels, sections)
        self.c0 = self.coef.copy()
        self.c1 = self.coef                                      # (the base's coef is the target)
        self.done = np.zeros((streams, sections), dtype=np.int64)
        self.R = np.zeros((streams, sections), dtype=np.int64)

    def now(self, s, k):
        """the section in force -> five ints"""
        if self.done[s, k] < self.R[s, k]:
            return tuple(int(v) for v in ramp_section(self.c0[s, k], self.c1[s, k], position(self.done[s, k], self.R[s, k])))
        return tuple(int(v) for v in self.c1[s, k])

    def ramp_state(self, s, k):
        return int(self.done[s, k]), int(self.R[s, k])

    def set(self, stream, section, sec):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.c0[s, section] = self.c1[s, section] = np.array(sec, dtype=np.int64)
            self.done[s, section] = self.R[s, section] = 0

    def ramp(self, stream, section, sec, frames):
        if frames < 2:
            return self.set(stream, section, sec)
        for s in (range(self.S) if stream < 0 else [stream]):
            if self.done[s, section] < self.R[s, section]:
                self.trace["retarget"] += 1
            self.c0[s, section] = np.array(self.now(s, section), dtype=np.int64)
            self.c1[s, section] = np.array(sec, dtype=np.int64)
            self.done[s, section], self.R[s, section] = 0, frames

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
        ramping = self.done < self.R                                 # [S][N] at the run's start
        for f in range(F):
            act = (counts > f)[:, None]                              # [S][1]
            n = self.done + f + 1
            p = np.where(ramping, position(n, self.R), P_ONE)        # [S][N]
            t["in_ramp"] += int((ramping & (n < self.R) & act).sum())
            t["past_end"] += int((ramping & (n > self.R) & act).sum())
            t["at_rest"] += int((~ramping & act).sum())
            coef = ramp_section(self.c0, self.c1, p, t, act)         # [S][N][5]
            u = X[:, f, :] << 12
            for k in range(self.N):
                c = coef[:, k, :, None]                              # [S][5][1]
                st = self.st[:, :, k, :]                             # [S][C][5]
                assert max(int(np.abs(u).max()), int(np.abs(st[..., :4]).max())) <= V_MAX and np.abs(c).max() <= 2 ** 28
                acc = c[:, 0] * u + c[:, 1] * st[..., 0] + c[:, 2] * st[..., 1] - c[:, 3] * st[..., 2] - c[:, 4] * st[..., 3]
                acc += st[..., 4]
                assert np.abs(acc).max() < 2 ** 62
                e = acc & (ONE - 1)
                q = acc >> 26                                        # arithmetic: floor
                v = np.clip(q, -V_MAX, V_MAX)
                self.overs += ((v != q) & act).sum(axis=1)
                new = np.stack([u, st[..., 0], v, st[..., 2], e], axis=-1)
                self.st[:, :, k, :] = np.where(act[..., None], new, st)
                u = v
            r = (u + 2048) >> 12
            y = np.clip(r, -32768, 32767)
            self.clips += ((y != r) & act).sum(axis=1)
            Y[:, f, :] = y
        self.done = np.where(ramping, np.minimum(self.done + counts[:, None], self.R), self.done)
        over = ramping & (self.done >= self.R)
        self.c0[over] = self.c1[over]
        self.done[over] = self.R[over] = 0
        return [Y[s, :counts[s]].astype(np.int16) for s in range(self.S)]


# ---------------------------------------------------------------------------
# the rig

class RampRig(TG.Rig):
    """tests/test_gpu_iir.py's rig over the ramp model (or, model=, over any other): every run also checks what get and
    ramp_state answer"""

    def __init__(self, cm, streams, channels, sections, max_frames, secs=None, model=None):
        super().__init__(cm, streams, channels, sections, max_frames)
        self.model = model or RampModel(streams, channels, sections)
        self.mirror = isinstance(self.model, RampModel)
        if secs is not None:
            for s in range(streams):
                for k in range(sections):
                    self.set(s, k, secs(s, k))

    def ramp(self, stream, section, sec, frames):
        self.m.ramp(stream, section, self.cm.IirSection(*sec), frames)
        if self.mirror:
            self.model.ramp(stream, section, sec, frames)
            self.check_mirror(range(self.S) if stream < 0 else [stream], [section])

    def check_mirror(self, streams=None, sections=None):
        for s in (range(self.S) if streams is None else streams):
            for k in (range(self.N) if sections is None else sections):
                assert self.m.get(s, k).as_tuple() == self.model.now(s, k), ("get", s, k)
                assert self.m.ramp_state(s, k) == self.model.ramp_state(s, k), ("ramp_state", s, k)

    def run(self, xs, uniform=False):
        wants = super().run(xs, uniform)
        if self.mirror:
            self.check_mirror()
        return wants


def ramp_lengths(B):
    return [2, 3, B - 1, B, B + 1, 2 * B + 1, 5 * B + 7, RAMP_MAX]


def ends(cm, k):
    """end number k of the round: the palette of tests/test_gpu_iir.py and the two corner sections"""
    return (CORNER_A, CORNER_B)[k % 14 - 12] if k % 14 >= 12 else TG.palette(cm, k % 14)


def schedule(cm, rig, k, B):
    """what happens in front of run k: ramps of every length on some (stream, section), a set that ends a ramp on
    others, a corner pair on every eleventh stream's section 0; every fifth stream and what the rules leave out rest"""
    lengths = ramp_lengths(B)
    for s in range(rig.S):
        if s % 5 == 4:
            continue
        for sec in range(rig.N):
            if s % 11 == 0 and sec == 0:
                if k == 0:
                    rig.set(s, 0, CORNER_A)
                elif k == 1:
                    rig.ramp(s, 0, CORNER_B, B + 1)
                continue
            if (s + sec + k) % 7 == 3:
                rig.set(s, sec, ends(cm, s + sec + 2 * k))
            elif (s + 2 * sec + k) % 3 == 0:
                rig.ramp(s, sec, ends(cm, s + 5 * sec + 3 * k + 1), lengths[(s + sec + 3 * k) % len(lengths)])


def play(cm, streams, channels, sections, signals, secs, cuts, max_frames, between=None):
    """tests/test_gpu_iir.py's play over the ramp rig -> (per stream the output, (clips, overs, rows), the model)"""
    rig = RampRig(cm, streams, channels, sections, max_frames, secs)
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


SHAPES = [(1, 1), (1, 2), (2, 3), (2, 4), (1, 8), (2, 8), (3, 2), (6, 8), (16, 5)]


@pytest.mark.parametrize("streams", [1, 33, 70])
@pytest.mark.parametrize("channels,sections", SHAPES)
def test_equals_the_model(gpu, streams, channels, sections):
    B = TG.tile_frames(gpu, channels, sections)
    runs = 10 if streams == 1 else 5
    signals, secs, cuts = TG.model_case(gpu, streams, channels, sections, 300 * channels + sections, runs=runs)
    _, _, model = play(gpu, streams, channels, sections, signals, secs, cuts, 2 * B + 1,
                       lambda rig, k: schedule(gpu, rig, k, B))
    t = model.trace
    assert t["in_ramp"] > 0 and t["b1_clamped"] > 0, t
    if streams >= 33:
        assert all(t[b] > 0 for b in RAMP_BRANCHES), t
        assert (model.R == RAMP_MAX).any() and (model.done[model.R == RAMP_MAX] > 0).all()      # the long one: only begun


@pytest.mark.parametrize("channels,sections", [(1, 1), (1, 8), (2, 3), (3, 2), (16, 5)])
def test_output_does_not_depend_on_the_cuts(gpu, channels, sections):
    """the same streams in two runs and in many ragged ones that include 0- and 1-frame runs; ramps at the start, and
    in the middle a retarget, a set that ends a ramp and a reset, at the same frames in both: identical output,
    counters and state (and each equals the model)"""
    B, S = TG.tile_frames(gpu, channels, sections), 9
    half = 2 * B + 1
    signals = [TG.noise(150 + s, 2 * half, channels) for s in range(S)]
    secs = lambda s, k: TG.palette(gpu, s + 5 * k)

    def ragged(total):
        lengths, cuts, left, k = TG.run_lengths(B // 2), [], [total] * S, 0
        while any(left):
            counts = [min(n, left[s]) for s, n in enumerate(TG.rotate(lengths, k, S))]
            left = [a - b for a, b in zip(left, counts)]
            cuts.append(counts)
            k += 1
        return cuts

    first = ragged(half)
    many = first + ragged(half)
    assert len(many) > 8 and any(0 in c for c in many) and any(1 in c for c in many)
    last = sections - 1

    def at(middle):
        def between(rig, k):
            if k == 0:
                rig.ramp(1, 0, TG.palette(gpu, 7), 3 * B)              # still running at the middle: retargeted there
                rig.ramp(2, last, TG.palette(gpu, 1), 5 * B + 7)       # ... ended by a set there
                rig.ramp(3, 0, TG.palette(gpu, 8), B + 1)              # over before the middle
                rig.ramp(5, last, TG.palette(gpu, 0), 4 * B + 2)       # runs through the middle, ends past it
                rig.ramp(-1, sections // 2, TG.palette(gpu, 10), 2 * B)
            if k == middle:
                rig.ramp(1, 0, TG.palette(gpu, 3), B - 1)
                rig.set(2, last, TG.palette(gpu, 5))
                rig.ramp(6, 0, TG.palette(gpu, 6), 7)
                rig.reset(4)
                rig.reset(5)
        return between

    a, state_a, model = play(gpu, S, channels, sections, signals, secs, [[half] * S] * 2, half, at(1))
    b, state_b, _ = play(gpu, S, channels, sections, signals, secs, many, half, at(len(first)))
    assert model.trace["retarget"] > 0 and model.trace["past_end"] > 0
    for s in range(S):
        assert np.array_equal(a[s], b[s]), s
    assert state_a[:2] == state_b[:2] and np.array_equal(state_a[2], state_b[2])


@pytest.mark.parametrize("channels,sections", [(1, 2), (5, 3)])
def test_a_stream_given_no_frames_does_not_advance(gpu, channels, sections):
    B = TG.tile_frames(gpu, channels, sections)
    rig = RampRig(gpu, 3, channels, sections, 2 * B + 1, lambda s, k: TG.palette(gpu, s + k))
    try:
        rig.ramp(-1, 0, TG.palette(gpu, 3), B + 5)
        rig.run([TG.noise(1, 9, channels), TG.noise(2, 0, channels), TG.noise(3, B, channels)])
        assert [rig.m.ramp_state(s, 0) for s in range(3)] == [(9, B + 5), (0, B + 5), (B, B + 5)]
        before = [rig.m.get(s, 0).as_tuple() for s in range(3)]
        assert rig.m.run_rc(rig.src.dev, rig.in_stride, 0, rig.dst.dev, rig.out_stride) == 0       # a run of no frames
        rig.run([TG.noise(4, 0, channels)] * 3)
        assert [rig.m.get(s, 0).as_tuple() for s in range(3)] == before
        rig.run([TG.noise(5, 1, channels), TG.noise(6, B + 5, channels), TG.noise(7, 0, channels)])
        assert [rig.m.ramp_state(s, 0) for s in range(3)] == [(10, B + 5), (0, 0), (B, B + 5)]
        rig.run([TG.noise(8, 2 * B + 1, channels)] * 3)
        assert [rig.m.ramp_state(s, 0) for s in range(3)] == [(0, 0)] * 3
    finally:
        rig.close()


@pytest.mark.parametrize("channels,sections,frames", [(1, 1, 1), (2, 4, 0), (3, 2, 1)])
def test_a_ramp_of_one_frame_is_a_set(gpu, channels, sections, frames):
    """the device through cmhip_iir_ramp(..., 0 or 1), the model -- that of tests/test_gpu_iir.py, which knows no ramps --
    through set: bit for bit, also where the call ends a ramp that runs"""
    B = TG.tile_frames(gpu, channels, sections)
    rig = RampRig(gpu, 3, channels, sections, 2 * B + 1, lambda s, k: TG.palette(gpu, s + k),
                  model=TG.Model(3, channels, sections))
    try:
        for r in range(3):
            for s in range(3):
                sec = TG.palette(gpu, 2 * r + s + 1)
                rig.m.ramp(s, r % sections, gpu.IirSection(*sec), frames)
                rig.model.set(s, r % sections, sec)
                assert rig.m.get(s, r % sections).as_tuple() == sec and rig.m.ramp_state(s, r % sections) == (0, 0)
            rig.run([TG.noise(20 + 3 * r + s, n, channels) for s, n in enumerate((B + 1, 9, 2 * B + 1))])
        long_one = TG.palette(gpu, 8)
        rig.m.ramp(-1, 0, gpu.IirSection(*long_one), 4 * B)              # a ramp that the next call ends with a step
        rig.m.ramp(-1, 0, gpu.IirSection(*TG.palette(gpu, 3)), frames)
        rig.model.set(-1, 0, TG.palette(gpu, 3))
        rig.run([TG.noise(40 + s, B + 2, channels) for s in range(3)])
    finally:
        rig.close()


@pytest.mark.parametrize("channels,sections", [(1, 1), (2, 3), (2, 8), (5, 4)])
def test_a_ramp_between_equal_ends_is_the_plain_filter(gpu, channels, sections):
    """every section ramps to the section it has: the ramp kernels run, and the output, the counters and the state are
    those of the model that knows no ramps"""
    B, S = TG.tile_frames(gpu, channels, sections), 5
    secs = lambda s, k: TG.palette(gpu, s + 5 * k)
    rig = RampRig(gpu, S, channels, sections, 2 * B + 1, secs, model=TG.Model(S, channels, sections))
    try:
        for r in range(3):
            for s in range(S):
                for k in range(sections):
                    rig.m.ramp(s, k, gpu.IirSection(*secs(s, k)), (3, 2 * B + 1, RAMP_MAX)[(s + k + r) % 3])
            assert rig.m.ramp_state(0, 0)[1] >= 2
            rig.run([TG.noise(60 + 5 * r + s, n, channels) for s, n in enumerate(TG.rotate(TG.run_lengths(B), r, S))])
    finally:
        rig.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_ramps_behind_a_queued_run_need_no_wait(gpu, channels):
    """run A, two ramps and a retarget, run B with no host wait in between: run A keeps the old sections, run B ramps"""
    B, S, N = TG.tile_frames(gpu, channels, 2), 3, 2
    rig = RampRig(gpu, S, channels, N, 2 * B + 1, lambda s, k: TG.palette(gpu, s + k))
    src_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.in_stride))
    dst_b = gpu.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.out_stride))
    try:
        xa = [TG.noise(90 + s, n, channels) for s, n in enumerate((B + 3, 2 * B + 1, 7))]
        xb = [TG.noise(95 + s, n, channels) for s, n in enumerate((2 * B + 1, 1, B))]
        ca, cb = rig.fill(xa), [x.shape[0] for x in xb]
        src_b.array[:] = TG.POISON
        for s, x in enumerate(xb):
            src_b.array[s, :x.size] = x.reshape(-1)
        dst_b.array[:] = TG.SENTINEL
        new = gpu.iir_design(gpu.IIR_LOWPASS, 48000.0, 500.0).as_tuple()
        rig.m.run(rig.src.dev, rig.in_stride, max(ca), rig.dst.dev, rig.out_stride, ca)
        moves = [(1, 0, TG.palette(gpu, 9), 2 * B), (2, 1, new, B - 1), (1, 0, new, B + 1)]
        for s, k, sec, frames in moves:
            rig.m.ramp(s, k, gpu.IirSection(*sec), frames)
        rig.m.run(src_b.dev, rig.in_stride, max(cb), dst_b.dev, rig.out_stride, cb)
        rig.m.sync()
        rig.check_output(rig.model.run(xa))
        for s, k, sec, frames in moves:
            rig.model.ramp(s, k, sec, frames)
        rig.dst.array[:] = dst_b.array
        rig.check_output(rig.model.run(xb))
        rig.check_state()
        rig.check_mirror()
        assert rig.m.ramp_state(1, 0) == (1, B + 1) and rig.m.ramp_state(2, 1) == (0, 0)
    finally:
        src_b.free()
        dst_b.free()
        rig.close()


def test_refusals_change_nothing_on_a_real_object(gpu):
    host = _load("test_iir_ramp_host", "_for_gpu")
    d = gpu.Filter(3, 2, 2, 64)
    try:
        host.check_ramp_refusals(gpu, d)
    finally:
        d.close()


# ---------------------------------------------------------------------------
# the chain of tests/test_gpu_iir_chain.py with a low-cut ramp in the middle

@pytest.mark.parametrize("channels", [1, 2])
def test_filter_leveller_limiter_batch_with_a_low_cut_ramp(gpu, channels):
    """a 40 Hz high-pass -> leveller -> limiter -> the slots of a batch on one stream with no synchronisation in
    between, five ragged blocks; in front of the third block the low cuts ramp to 120 Hz over 2500 frames, which ends
    in different blocks on different microphones: every stage equals its model, block by block"""
    cm = gpu
    TC = _load("test_gpu_iir_chain", "_for_iir_ramp")
    TL, TA = TC.TL, TC.TA
    MICS, MAXF, W_LOG2, BLOCKS = TC.MICS, TC.MAXF, TC.W_LOG2, TC.BLOCKS
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(MICS, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    iir = cm.Filter(MICS, channels, 2, MAXF, hip_stream=b.hip_stream())
    agc = cm.Leveller(MICS, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    lim = cm.Limiter(MICS, channels, TC.LOOKAHEAD_LOG2, TC.HOLD, MAXF, threshold=TC.THRESHOLD, drive=TC.DRIVE,
                     hip_stream=b.hip_stream())
    cut = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 40.0)
    higher = cm.iir_design(cm.IIR_HIGHPASS, 48000.0, 120.0)
    filt = RampModel(MICS, channels, 2)
    for s, k in ((0, 0), (1, 0), (1, 1)):
        iir.set(s, k, cut)
        filt.set(s, k, cut.as_tuple())
    p = TA.params(target=6000, gate=50, gain_min=256, gain_max=65535, rise=30000, fall=30000)
    agc.set(-1, cm.AgcParams(**p))
    levellers = [TA.Model(channels, W_LOG2, p) for _ in range(MICS)]
    hist = [np.zeros((TL.geometry(TC.LOOKAHEAD_LOG2, TC.HOLD)[3], channels), dtype=np.int16) for _ in range(MICS)]
    src, cutout, level = (cm.MappedPcm(types.SimpleNamespace(streams=MICS, stride=stride)) for _ in range(3))
    total = [sum(blk[s] for blk in BLOCKS) for s in range(MICS)]
    rng = np.random.default_rng(78)
    n = np.arange(max(total))
    voice = (900.0 * np.sin(2.0 * np.pi * n / 96.0)).astype(np.int64)
    signals = [np.clip(voice[:total[s], None] + 6000 + rng.integers(-60, 61, size=(total[s], channels)), -32768,
                       32767).astype(np.int16) for s in range(MICS)]
    try:
        at = [0] * MICS
        for k, counts in enumerate(BLOCKS):
            if k == 2:
                for s, sec in ((0, 0), (1, 0), (1, 1)):
                    iir.ramp(s, sec, higher, 2500)
                    filt.ramp(s, sec, higher.as_tuple(), 2500)
            xs = [signals[s][at[s]:at[s] + c] for s, c in enumerate(counts)]
            at = [a + c for a, c in zip(at, counts)]
            src.array[:] = TG.POISON
            for s, x in enumerate(xs):
                src.array[s, :x.size] = x.reshape(-1)
            cutout.array[:] = TG.SENTINEL
            level.array[:] = TG.SENTINEL
            frames = max(counts)
            iir.run(src.dev, stride, frames, cutout.dev, stride, counts)
            agc.run(cutout.dev, stride, frames, level.dev, stride, counts)
            lim.run(level.dev, stride, frames, b.dev_in, b.stride, counts)
            b.run(frames, counts)                    # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_cut = filt.run(xs)
            for s in range(MICS):
                c = counts[s]
                want_level = levellers[s].run(want_cut[s])
                want, _ = TL.model_lim(want_level, hist[s], TC.THRESHOLD, TC.DRIVE, TC.LOOKAHEAD_LOG2, TC.HOLD)
                hist[s] = TL.next_hist(hist[s], want_level)
                assert np.array_equal(cutout.array[s, :c * channels].reshape(-1, channels), want_cut[s]), ("filter", k, s)
                assert (cutout.array[s, c * channels:] == TG.SENTINEL).all(), ("filter wrote past its count", k, s)
                assert np.array_equal(level.array[s, :c * channels].reshape(-1, channels), want_level), ("leveller", k, s)
                if c:
                    have = b.download(s, c).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, s)
                    assert rcs[s] == 0 and res[s].frames == c
            clips, overs = iir.state()
            assert clips.tolist() == filt.clips.tolist() and overs.tolist() == filt.overs.tolist()
            assert np.array_equal(iir.rows(), filt.rows()), ("filter state", k)
            for s in range(MICS):
                for sec in range(2):
                    assert iir.get(s, sec).as_tuple() == filt.now(s, sec) and iir.ramp_state(s, sec) == filt.ramp_state(s, sec)
            gain, lv, aclips = agc.state()
            assert [(int(gain[s]), int(lv[s]), int(aclips[s])) for s in range(MICS)] == [m.state() for m in levellers]
        assert at == total and filt.trace["in_ramp"] > 0 and filt.trace["past_end"] > 0
        assert iir.get(0, 0).as_tuple() == higher.as_tuple() and iir.ramp_state(1, 1) == (7 + 1501, 2500)
    finally:
        for o in (lim, agc, iir, b):
            o.close()
        for a in (src, cutout, level):
            a.free()
