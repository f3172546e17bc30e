"""GPU: the mix bus's send ramps (cmhip_bus_ramp_sends, csrc/k_busramp.hip) against a numpy model in int64 of the
arithmetic include/coolmic_hip.h states ("send ramps"), bit for bit: every kernel form with ramps that end inside the
first tile, cross tile edges and outlive a run, per-bus counts with a bus at 0, sends of one bus at different positions
of different ramps with a retarget and a step, cuts, the group split taken from both ends of every ramp, wide buses,
the way back to the plain kernels, the mixer's ramp on one send, the order of a ramp with the runs, and refusals that
change nothing.  Input slots hold a poison value past every count; output slots are pre-filled with a sentinel that
must survive past every bus's count.  (tests/test_bus_ramp_host.py takes the model from here; the rig, the noise and
the dense sends come from tests/test_gpu_bus.py, the ramp's formulas from tests/test_gpu_mix_ramp.py.)"""
import ctypes as C
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, alias):
    spec = importlib.util.spec_from_file_location(alias, os.path.join(ROOT, "tests", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TB = _load("test_gpu_bus.py", "test_gpu_bus_for_ramps")            # the bus's rig, model and dense sends
TR = _load("test_gpu_mix_ramp.py", "test_gpu_mix_ramp_for_bus")    # ramp_position, ramp_weight, RampModel
noise, dense_sends, SENTINEL, SATURATED_MAX = TB.noise, TB.dense_sends, TB.SENTINEL, TB.SATURATED_MAX
RAMP_MAX = 1 << 20
FAST = sorted(TB.FAST)
ANY = [(3, 2), (6, 2), (5, 5), (16, 16)]


# ---------------------------------------------------------------------------
# the specification in numpy

class BusRampModel:
    """a bus object's table with a ramp state (tests/test_gpu_mix_ramp.py's RampModel) per send, in the caller's order;
    a send's clock is its BUS's output count"""

    def __init__(self, buses, ci, co):
        self.B, self.CI, self.CO = buses, ci, co
        self.set([], [], np.zeros((0, co, ci), dtype=np.int16))

    def set(self, bus, stream, W):
        W = np.asarray(W, dtype=np.int64).reshape(len(bus), self.CO, self.CI)
        self.bus, self.stream = list(bus), list(stream)
        self.sends = [TR.RampModel(w) for w in W]

    def ramp(self, first, W, R):
        W = np.asarray(W, dtype=np.int64).reshape(-1, self.CO, self.CI)
        for j, w in enumerate(W):
            self.sends[first + j].ramp(w, R)                     # (R < 2: a step)

    def targets(self):
        return np.array([s.w1 for s in self.sends], dtype=np.int16).reshape(-1, self.CO, self.CI)

    def state(self, j):
        return self.sends[j].state()

    def run(self, xs):
        """xs: per stream int16 [F_s][C_in] -> per bus int16 [F_b][C_out]; every ramping send moves on by F_b"""
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, self.CI) for x in xs]
        outs = []
        for b in range(self.B):
            js = [j for j in range(len(self.bus)) if self.bus[j] == b]
            F = max([xs[self.stream[j]].shape[0] for j in js], default=0)
            acc = np.zeros((F, self.CO), dtype=np.int64)
            for j in js:
                mod, x = self.sends[j], xs[self.stream[j]]
                c = x.shape[0]
                if mod.ramping():
                    p = TR.ramp_position(mod.done + 1 + np.arange(c), mod.R)
                    W = TR.ramp_weight(mod.w0[None], mod.w1[None], p[:, None, None])         # [c][C_out][C_in]
                    assert c == 0 or np.abs(W).sum(axis=2).max() <= 65535                    # the row bound, every frame
                    q = np.einsum("foc,fc->fo", W, x)
                    mod.done = min(mod.R, mod.done + F)          # by the BUS's count, whatever the stream's
                else:
                    q = x @ mod.w1.T
                assert q.size == 0 or np.abs(q).max() < 2 ** 31
                acc[:c] += q
            outs.append(np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16))
        return outs


class Rig(TB.Rig):
    """tests/test_gpu_bus.py's rig with a BusRampModel beside the bus"""

    def __init__(self, cm, streams, buses, ci, co, max_frames, max_sends):
        super().__init__(cm, streams, buses, ci, co, max_frames, max_sends)
        self.model = BusRampModel(buses, ci, co)

    def set(self, bus, stream, W):
        super().set(bus, stream, W)
        self.model.set(bus, stream, W)

    def ramp(self, first, W, R):
        self.m.ramp_sends(first, W, R)
        self.model.ramp(first, W, R)
        assert np.array_equal(self.m.get_routing()[2], self.model.targets())     # read-back: the targets

    def check_state(self):
        for j in range(len(self.model.sends)):
            done, total, w = self.m.ramp_state(j)
            d, r, wm = self.model.state(j)
            assert (done, total) == (d, r), ("send", j, (done, total), (d, r))
            assert np.array_equal(w, wm), ("send", j)

    def play(self, xs, frames=None, uniform=False):
        """a run of the device and of the model, compared; then the states compared -> the model's outputs"""
        wants = self.model.run(xs)
        self.run(xs, frames=frames, uniform=uniform, wants=wants)
        self.check_state()
        return wants

    def output(self, b, n):
        return self.dst.array[b, :n * self.CO].reshape(-1, self.CO).copy()


def saturated_share(ys):
    return sum(TB.saturated(y) for y in ys) / max(1, sum(y.size for y in ys))


# ---------------------------------------------------------------------------
# 1. every form: ramps that end inside the first tile, cross tile edges, outlive a run; per-bus counts

STREAMS, BUSES = 5, 3
BUS, STREAM = [0, 1, 0, 0, 1, 0, 1], [0, 2, 1, 3, 4, 0, 3]       # bus 2 has no sends; stream 0 twice in bus 0
RAMPS = [2, 7, 1000, 3000]


def run_forms(cm, ci, co, R, nt):
    fast = (ci, co) in TB.FAST
    plan = cm.plan_busramp(BUSES, ci, co, 1)
    assert plan.fast == (1 if fast else 0)
    t = plan.tile_frames
    F = 5000 if (ci, co) == (1, 1) else 2600                     # about 2.5 tiles of the mono / stereo forms
    assert not fast or 2 * t < F < 3 * t
    n = len(BUS)
    W0 = dense_sends(ci, co, n, 4, 9000 + 100 * ci + co)
    W1 = dense_sends(ci, co, n, 4, 9500 + 100 * ci + co)
    xs = [noise(300 * ci + co + 11 * s, F, ci) for s in range(STREAMS)]
    rig = Rig(cm, STREAMS, BUSES, ci, co, F, n + 1)
    cm.lib.cmhip_test_bus_nt_loads(rig.m.h, nt)
    rig.set(BUS, STREAM, W0)
    rig.ramp(0, W1[0:2], R)                                      # sends 0 and 1 (two buses): R frames
    rig.ramp(3, W1[3:6], R + 5)                                  # sends 3 .. 5: R + 5; sends 2 and 6 stay at rest
    ys = []
    for counts in ([F, F - 3, min(t, F) + 5, 1, 0],              # ragged last vectors; bus 1 shorter than bus 0
                   [40, 40, 0, 0, 0],                            # bus 1 produces 0 frames: its sends keep their positions
                   [F, 33, F - 8, 0, 9]):
        ys += rig.play([x[:c] for x, c in zip(xs, counts)])
    ys += rig.play(xs, uniform=True)                             # full vectors and tiles everywhere
    assert [y.shape[0] for y in ys[:6]] == [F, min(t, F) + 5, 0, 40, 0, 0]
    assert saturated_share(ys) < SATURATED_MAX
    assert all(rig.m.ramp_state(j)[:2] == (0, 0) for j in range(n))              # 3 F + 40 frames: every ramp has ended
    rig.close()


@pytest.mark.parametrize("R", RAMPS)
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("ci,co", FAST)
def test_fast_forms(gpu, ci, co, nt, R):
    run_forms(gpu, ci, co, R, nt)


@pytest.mark.parametrize("R", RAMPS)
@pytest.mark.parametrize("ci,co", ANY)
def test_any_forms(gpu, ci, co, R):
    run_forms(gpu, ci, co, R, 0)


# ---------------------------------------------------------------------------
# 2. sends of one bus at different positions of different ramps; a retarget and a step mid-ramp

@pytest.mark.parametrize("ci,co", [(2, 2), (1, 2), (6, 2)])
def test_independent_sends(gpu, ci, co):
    cm = gpu
    W = [dense_sends(ci, co, 4, 4, 9900 + 10 * ci + co + i) for i in range(4)]
    xs = [noise(7700 + ci + s, 1500, ci) for s in range(4)]
    rig = Rig(cm, 4, 1, ci, co, 1500, 4)
    rig.set([0] * 4, [0, 1, 2, 3], W[0])
    rig.ramp(0, W[1][0:1], 3000)
    ys = rig.play([x[:700] for x in xs])
    rig.ramp(1, W[1][1:2], 300)                                  # started at another run, with another R
    rig.ramp(3, W[1][3:4], 2000)
    assert [rig.m.ramp_state(j)[:2] for j in range(4)] == [(700, 3000), (0, 300), (0, 0), (0, 2000)]
    ys += rig.play([x[700:1400] for x in xs])                    # send 1 ends inside this run
    assert [rig.m.ramp_state(j)[:2] for j in range(4)] == [(1400, 3000), (0, 0), (0, 0), (700, 2000)]
    rig.ramp(0, W[2][0:1], 900)                                  # a retarget: from the matrix in force, n restarts
    rig.ramp(3, W[2][3:4], 0)                                    # a step mid-ramp
    assert [rig.m.ramp_state(j)[:2] for j in range(4)] == [(0, 900), (0, 0), (0, 0), (0, 0)]
    ys += rig.play([x[:500] for x in xs])
    rig.ramp(3, W[3][3:4], 1)                                    # ramp_frames 1 is a step as well
    ys += rig.play(xs)                                           # send 0 ends after 400 more frames
    assert all(rig.m.ramp_state(j)[:2] == (0, 0) for j in range(4))
    assert np.array_equal(rig.m.get_routing()[2], np.stack([W[2][0], W[1][1], W[0][2], W[3][3]]))
    assert saturated_share(ys) < SATURATED_MAX
    rig.close()


# ---------------------------------------------------------------------------
# 3. cuts: the concatenated output does not depend on how the run sequence was cut

CUTS_FREE = ([3000], [1, 7, 0, 392, 8, 1092, 0, 900, 600])                   # ramps requested at frame 0 only
CUTS_AT_400 = ([400, 2600], [1, 7, 0, 392, 8, 1092, 0, 900, 600])            # ... and a retarget and a step at frame 400


@pytest.mark.parametrize("ci,co", [(2, 2), (2, 1), (3, 2)])
@pytest.mark.parametrize("cuts", [CUTS_FREE, CUTS_AT_400], ids=["one-run", "ops-at-400"])
def test_cuts(gpu, ci, co, cuts):
    cm = gpu
    W = [dense_sends(ci, co, 3, 3, 8800 + 10 * ci + co + i) for i in range(3)]
    xs = [noise(8700 + ci + s, 3000 - 100 * s, ci) for s in range(3)]        # the streams end at different frames
    outs = []
    for cut in cuts:
        assert sum(cut) == 3000
        rig = Rig(cm, 3, 2, ci, co, max(cut), 3)
        rig.set([0, 0, 1], [0, 1, 2], W[0])
        rig.ramp(0, W[1][0:1], 700)
        rig.ramp(2, W[1][2:3], 2500)
        got, at, moved = [[], []], 0, cuts is CUTS_FREE
        for i, n in enumerate(cut):
            if at == 400 and not moved:
                rig.ramp(0, W[2][0:1], 1000)
                rig.ramp(1, W[2][1:2], 0)
                moved = True
            part = [x[at:at + n] for x in xs]
            wants = rig.model.run(part)
            # (a run of no frames: once with frames = 0, which launches nothing, once with frames = 8 and every count at
            # 0, which launches the kernels)
            rig.run(part, frames=n if n or i == 2 else 8, wants=wants)
            rig.check_state()
            for b in range(2):
                got[b].append(rig.output(b, wants[b].shape[0]))
            at += n
        assert moved
        rig.close()
        outs.append([np.concatenate(g) for g in got])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert outs[0][0].shape[0] == 3000 and outs[0][1].shape[0] == 2800
    assert saturated_share(outs[0]) < SATURATED_MAX


# ---------------------------------------------------------------------------
# 4. both ends of the split: groups compiled from the targets alone wrap an int32

def test_both_ends_of_the_split_mono(gpu):
    """table {30000, 30000, 2000} on constant 32767: send 0 ramps slowly to 2000, then send 2 quickly to 30000.  The
    targets sum to 62000, one int32 group; the weights in force to about 90000, and 90000 * 32767 > 2^31: a wrapped
    accumulator gives -32768 where the sum, saturated, is 32767"""
    cm = gpu
    xs = [np.full((64, 1), 32767, dtype=np.int16) for _ in range(3)]
    rig = Rig(cm, 3, 1, 1, 1, 64, 3)
    rig.set([0, 0, 0], [0, 1, 2], [[[30000]], [[30000]], [[2000]]])
    assert cm.bus_compile(1, 3, 1, 1, [0] * 3, [0, 1, 2], [[[2000]], [[30000]], [[30000]]])[2].sum() == 1   # one group
    rig.ramp(0, [[[2000]]], 4000)
    ys = rig.play([x[:8] for x in xs])
    rig.ramp(2, [[[30000]]], 2)
    ys += rig.play(xs)
    ys += rig.play(xs)
    assert rig.m.ramp_state(0)[:2] == (136, 4000) and int(rig.m.ramp_state(0)[2][0, 0]) > 29000
    assert all((y == 32767).all() for y in ys)
    rig.close()


def test_both_ends_of_the_split_stereo(gpu):
    """the same with rows: {32000, 32000, 1534} per row, 65534 at rest and in the targets, about 96000 in force"""
    cm = gpu
    big, small = [[16000, 16000], [16000, 16000]], [[767, 767], [767, 767]]
    xs = [np.full((64, 2), 32767, dtype=np.int16) for _ in range(3)]
    rig = Rig(cm, 3, 1, 2, 2, 64, 3)
    rig.set([0, 0, 0], [0, 1, 2], [big, big, small])
    assert cm.bus_compile(1, 3, 2, 2, [0] * 3, [0, 1, 2], [small, big, big])[2].sum() == 1
    rig.ramp(0, [small], 4000)
    ys = rig.play([x[:8] for x in xs])
    rig.ramp(2, [big], 2)
    ys += rig.play(xs)
    ys += rig.play(xs)
    assert all((y == 32767).all() for y in ys)
    # and downwards: every weight negated gives -32768 throughout
    rig.set([0, 0, 0], [0, 1, 2], -np.array([big, big, small]))
    rig.ramp(0, -np.array([small]), 4000)
    ys = rig.play([x[:8] for x in xs])
    rig.ramp(2, -np.array([big]), 2)
    ys += rig.play(xs)
    assert all((y == -32768).all() for y in ys)
    rig.close()


# ---------------------------------------------------------------------------
# 5. wide buses: several int32 groups at rest, one send ramping -- the int64 path with a ramp inside

@pytest.mark.parametrize("ci,co", [(1, 1), (2, 2), (1, 2), (3, 2)])
def test_wide_buses(gpu, ci, co):
    cm = gpu
    rng = np.random.default_rng(640 + 10 * ci + co)
    n, F = 7, 2300

    def rows40000():                                             # (mono: an entry is a row, 32767 at most)
        mag = np.full((n, co, ci), 40000 // ci)
        mag[:, :, 0] += 40000 - mag.sum(axis=2)
        return (np.minimum(mag, 32767) * rng.choice([-1, 1], size=(n, co, ci))).astype(np.int16)

    W0, W1 = rows40000(), rows40000()
    xs = [noise(6400 + ci + s, F - 5 * s, ci) >> 4 for s in range(n)]
    rig = Rig(cm, n, 2, ci, co, F, n)
    rig.set([0, 0, 0, 0, 0, 1, 1], list(range(n)), W0)
    flags = cm.bus_compile(2, n, ci, co, [0, 0, 0, 0, 0, 1, 1], list(range(n)), W0)[2]
    assert flags.sum() == (4 if ci == 1 else 7)                  # no two such sends share a group (mono: no three)
    rig.ramp(2, W1[2:3], 1500)
    rig.ramp(6, W1[6:7], 3000)
    ys = rig.play(xs)
    ys += rig.play(xs)
    assert saturated_share(ys) == 0                              # (a saturated output would hide a wrong sum)
    assert [rig.m.ramp_state(j)[:2] for j in (2, 6)] == [(0, 0), (0, 0)]
    rig.close()


# ---------------------------------------------------------------------------
# 6. back to the plain kernels; set_routing mid-ramp; one ramping send against the mixer's ramp

def test_ended_ramps_leave_a_plain_bus(gpu):
    cm = gpu
    W0, W1 = dense_sends(2, 2, 5, 3, 5100), dense_sends(2, 2, 5, 3, 5200)
    bus, stream = [0, 1, 0, 1, 0], [0, 1, 2, 0, 1]
    xs = [noise(5300 + s, 2500, 2) for s in range(3)]
    plain = Rig(cm, 3, 2, 2, 2, 2500, 5)
    ramped = Rig(cm, 3, 2, 2, 2, 2500, 5)
    plain.set(bus, stream, W1)
    ramped.set(bus, stream, W0)
    for j in range(5):
        ramped.ramp(j, W1[j:j + 1], 100 + 37 * j)
    ramped.play([x[:300] for x in xs])
    assert all(ramped.m.ramp_state(j)[:2] == (0, 0) for j in range(5))
    got = ramped.m.get_routing()
    assert got[0].tolist() == bus and got[1].tolist() == stream and np.array_equal(got[2], W1)
    a = plain.run(xs)
    ramped.run(xs, wants=a)
    assert np.array_equal(plain.dst.array, ramped.dst.array)
    # set_routing mid-ramp steps and clears every ramp
    ramped.ramp(0, W0[0:5], 5000)
    ramped.play([x[:100] for x in xs])
    assert all(ramped.m.ramp_state(j)[:2] == (100, 5000) for j in range(5))
    ramped.set(bus[:4], stream[:4], W1[:4])
    assert all(ramped.m.ramp_state(j)[:2] == (0, 0) for j in range(4))
    plain.set(bus[:4], stream[:4], W1[:4])
    a = plain.run(xs)
    ramped.play(xs)
    assert np.array_equal(plain.dst.array, ramped.dst.array)
    plain.close()
    ramped.close()


@pytest.mark.parametrize("ci,co", [(1, 1), (2, 2), (2, 1), (6, 2)])
def test_one_send_equals_the_mixers_ramp(gpu, ci, co):
    """device against device: cmhip_mix_ramp_matrix with the same matrices and counts"""
    cm = gpu
    A, Bm, Cm = (TB.TM.dense_matrix(ci, co, 4100 + 10 * ci + co + i) for i in range(3))
    x = noise(4200 + ci, 2700, ci)
    rig = Rig(cm, 1, 1, ci, co, 2700, 1)
    rig.set([0], [0], [A])
    mixer = cm.Mixer(1, ci, co, 2700, matrix=A)
    ref = cm.MappedPcm(types.SimpleNamespace(streams=1, stride=rig.out_stride))
    rig.ramp(0, [Bm], 3100)
    mixer.ramp_matrix(0, Bm, 3100)
    for n, retarget in ((2700, False), (9, True), (2613, False)):
        if retarget:
            rig.ramp(0, [Cm], 1200)
            mixer.ramp_matrix(0, Cm, 1200)
        rig.play([x[:n]])
        ref.array[:] = SENTINEL
        mixer.run(rig.src.dev, rig.in_stride, n, ref.dev, rig.out_stride, [n])
        mixer.sync()
        assert np.array_equal(rig.dst.array, ref.array)
        assert rig.m.ramp_state(0)[:2] == mixer.ramp_state(0)[:2]
    mixer.close()
    ref.free()
    rig.close()


# ---------------------------------------------------------------------------
# 7. a ramp is ordered with the runs by the stream alone

def test_ordering_without_synchronisation(gpu):
    cm = gpu
    S, F = 4, 3000
    xs = [noise(6100 + s, F - 7 * s, 2) for s in range(S)]
    bus, stream = [0, 1, 0, 1, 1], [0, 1, 2, 3, 0]
    W0, W1 = dense_sends(2, 1, 5, 3, 63), dense_sends(2, 1, 5, 3, 64)
    rig = Rig(cm, S, 2, 2, 1, F, 5)
    rig.set(bus, stream, W0)
    counts = rig.fill(xs)
    outs = [rig.dst] + [cm.MappedPcm(types.SimpleNamespace(streams=2, stride=rig.out_stride)) for _ in range(2)]
    for o in outs:
        o.array[:] = SENTINEL
    m = rig.m
    m.run(rig.src.dev, rig.in_stride, F, outs[0].dev, rig.out_stride, counts)        # run, ramp, run, step, run: no sync
    w = W1[1:4].copy()
    assert cm.lib.cmhip_bus_ramp_sends(m.h, 1, 3, w.ctypes.data, 4000) == 0
    w[:] = 32767                                                 # the caller's array is free on return
    m.run(rig.src.dev, rig.in_stride, F, outs[1].dev, rig.out_stride, counts)
    m.ramp_sends(4, W1[4:5], 0)
    m.run(rig.src.dev, rig.in_stride, F, outs[2].dev, rig.out_stride, counts)
    m.sync()                                                     # (the only synchronisation)
    first = rig.model.run(xs)                                    # the first run used the old weights
    assert all(np.array_equal(a, b) for a, b in zip(first, TB.model_bus(xs, (bus, stream, W0), 2, 1)))
    rig.check(outs[0].array, first)
    rig.model.ramp(1, W1[1:4], 4000)
    rig.check(outs[1].array, rig.model.run(xs))
    rig.model.ramp(4, W1[4:5], 0)
    rig.check(outs[2].array, rig.model.run(xs))
    rig.check_state()
    assert not np.array_equal(outs[0].array, outs[1].array) and not np.array_equal(outs[1].array, outs[2].array)
    for o in outs[1:]:
        o.free()
    rig.close()


# ---------------------------------------------------------------------------
# 8. refusals change nothing: the next run is what it would have been

def test_refusals(gpu):
    cm = gpu
    W0, W1 = dense_sends(2, 1, 3, 2, 73), dense_sends(2, 1, 3, 2, 74)
    xs = [noise(7300 + s, 600 - s, 2) for s in range(3)]
    for started in (False, True):                # (before the ramps' state exists, and while ramps run)
        rig = Rig(cm, 3, 2, 2, 1, 600, 4)
        rig.set([0, 1, 1], [0, 1, 2], W0)
        m = rig.m
        if started:
            rig.ramp(0, W1[0:2], 500)
            rig.play([x[:100] for x in xs])
        rig.dst.array[:] = SENTINEL
        before = [m.ramp_state(j) for j in range(3)]
        table = m.get_routing()
        heavy = [[[-32768, -32768]]]
        assert m.ramp_sends_rc(2, W1[0:2], 100) == cm.ERROR_INVAL                        # first + count above the sends
        assert m.ramp_sends_rc(4, W1[0:1], 100) == cm.ERROR_INVAL
        assert cm.lib.cmhip_bus_ramp_sends(m.h, 4, 0, None, 100) == cm.ERROR_INVAL
        assert cm.lib.cmhip_bus_ramp_sends(m.h, 1, C.c_size_t(-1).value, W1.ctypes.data, 100) == cm.ERROR_INVAL
        assert m.ramp_sends_rc(0, W1[0:1], RAMP_MAX + 1) == cm.ERROR_INVAL
        assert m.ramp_sends_rc(0, heavy, 100) == cm.ERROR_INVAL                          # a row of 65536
        assert m.ramp_sends_rc(0, heavy, 0) == cm.ERROR_INVAL                            # ... as a step too
        assert m.ramp_sends_rc(0, np.concatenate([W1[0:1], heavy]), 100) == cm.ERROR_INVAL
        assert cm.lib.cmhip_bus_ramp_sends(m.h, 0, 1, None, 100) == cm.ERROR_FAULT
        assert cm.lib.cmhip_bus_ramp_sends(None, 0, 1, W1.ctypes.data, 100) == cm.ERROR_FAULT
        a, b = C.c_uint32(77), C.c_uint32(77)
        assert cm.lib.cmhip_bus_ramp_state(m.h, 3, C.byref(a), C.byref(b), None) == cm.ERROR_INVAL
        assert cm.lib.cmhip_bus_ramp_state(m.h, 0, None, C.byref(b), None) == cm.ERROR_FAULT
        assert cm.lib.cmhip_bus_ramp_state(m.h, 0, C.byref(a), None, None) == cm.ERROR_FAULT
        assert cm.lib.cmhip_bus_ramp_state(None, 0, C.byref(a), C.byref(b), None) == cm.ERROR_FAULT
        assert (a.value, b.value) == (77, 77)
        assert cm.lib.cmhip_bus_ramp_state(m.h, 0, C.byref(a), C.byref(b), None) == 0    # W_now may be NULL
        assert cm.lib.cmhip_bus_ramp_sends(m.h, 3, 0, None, 100) == 0                    # count == 0: accepted, nothing done
        m.sync()
        assert (rig.dst.array == SENTINEL).all()
        for j in range(3):
            now = m.ramp_state(j)
            assert now[:2] == before[j][:2] == ((100, 500) if started and j < 2 else (0, 0))
            assert np.array_equal(now[2], before[j][2])
        assert all(np.array_equal(x, y) for x, y in zip(table, m.get_routing()))
        rig.play(xs)                             # the next run is the model's: the running ramps went on unharmed
        assert m.ramp_sends_rc(2, W1[2:3], RAMP_MAX) == 0 and m.ramp_state(2)[:2] == (0, RAMP_MAX)
        rig.close()
