"""GPU: every stage object's two promises of include/coolmic_hip.h, held behind a BUSY stream.

1. test_counts_are_free_on_return: tests/test_gpu_programme_chain.py's test of that name for the run paths added since
   -- the dynamics stage (mean, keyed, RMS), the true-peak limiter, the release stage (both detectors), the band split,
   the delay, the leveller and the filter.  The object is parked behind a backlog of some 10 ms on the same stream; ONE
   pinned counts array is refilled between the runs; hipStreamQuery must answer hipErrorNotReady after run 2, so run 1's
   copy provably had not executed when its array changed.  Four more runs follow without a synchronisation, so the
   counts ring (CountsRing, csrc/cmhip_stage.h, four blocks) wraps: run 5's take() waits on the host for run 1's copy,
   which is the documented behaviour and the reason why the proof is taken after run 2.  Three of the kinds write
   records (delay: count, position, taps, ramp place; leveller: count, position, parameters) or a table (filter: the
   coefficients, in run 1 only) into the block themselves.
2. test_changes_queue_behind_pending_runs: run A, a change (set, ramp, move, reset -- per kind below), run B into a second
   array, all behind the same backlog, hipStreamQuery == hipErrorNotReady after run B is queued: run A was still pending
   when the change was made.  Run A must be the model's with the old settings and state, run B the model's with the new.
   Where a call takes a caller's table that the header calls free on return (cmhip_dyn_set_curve, cmhip_mix_set_matrix,
   cmhip_mix_ramp_matrix, cmhip_bus_set_routing, cmhip_bus_ramp_sends) the call is made through cm.lib with a buffer
   the test owns, and the buffer is overwritten with other valid values as soon as the call returns.
   The bus makes its two changes in two cases: its table travels from ONE pinned staging area, and the header says that
   a second table change may wait ON THE HOST until the first one's copy has executed -- behind a backlog that wait is
   the backlog, and the proof that run A was pending could not be taken after it.

Expected output is always the numpy model of the per-stage test files, never another run of the device code; the
sentinel must stand past every count; the stage's observable state must be the model's.  The counts of two successive
runs differ in every stream and every one of them is valid for every run: a wrong count gives a wrong output, never an
access out of bounds.  `frames` is the stage's tile (from its plan hook) and 64 frames, so the longer counts pass a
tile edge."""
import copy
import ctypes as C
import importlib.util
import os
import time
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("queue_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TD, TK, TRMS = _load("test_gpu_dyn"), _load("test_gpu_dyn_key"), _load("test_gpu_dyn_rms")
TTP, TREL, TSP = _load("test_gpu_limtp"), _load("test_gpu_limrel"), _load("test_gpu_split")
TDL, TA, TI = _load("test_gpu_delay"), _load("test_gpu_agc"), _load("test_gpu_iir")
TL, TR, TBR = _load("test_gpu_lim"), _load("test_gpu_mix_ramp"), _load("test_gpu_bus_ramp")
TB = TBR.TB
SENTINEL = TL.SENTINEL
assert all(t.SENTINEL == SENTINEL for t in (TD, TSP, TDL, TA, TI))

CS = 8                                            # streams of the object under test
# The backlog, as in tests/test_gpu_programme_chain.py: uniform runs of a batch of 1024 stereo streams x 65536 frames,
# about 0.08 ms each, 128 of them some 10 ms -- several times what the host needs to queue them and the calls behind
# them.  BACKLOG_RUNS_OF names the kinds whose host set-up between the backlog and the proof needs a longer one.
BACKLOG_STREAMS, BACKLOG_FRAMES, BACKLOG_RUNS = 1024, 65536, 128
BACKLOG_RUNS_OF = {}
HIP_ERROR_NOT_READY = 600


def run_counts(frames, group):
    """the counts of six runs with no synchronisation: X, Y, Z1 .. Z4.  Streams of one group (`group` neighbours) share
    theirs, groups differ; two successive runs differ in every stream; every count is valid for every run"""
    v = [s // group * group for s in range(CS)]
    runs = [[100 + k for k in v], [frames - k for k in v], [37 + 5 * k for k in v], [frames - 9 - 2 * k for k in v],
            [3 + 7 * k for k in v], [frames // 2 + 11 * k for k in v]]
    for c in runs:
        assert all(0 < n <= frames for n in c) and len(set(c)) == CS // group
    for c, d in zip(runs, runs[1:]):
        assert all(n != m for n, m in zip(c, d))
    return runs


def _mapped(cm, streams, stride):
    return cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=stride))


def _own(values, dtype):
    """a buffer the test owns, for a call through cm.lib"""
    return np.array(values, dtype=dtype, order="C", copy=True).reshape(-1)


class _Stage:
    """an object under test on the backlog's stream between one input array and output arrays, all pinned and
    device-mapped, and its model.  part 1: the set-up of test_counts_are_free_on_return; part 2: that of
    test_changes_queue_behind_pending_runs.  model(counts) -> per output slot int16 [frames][co], the model moved on;
    state(): the device's observable state is the model's; change(), model_change(): part 2's change, there and here --
    apart, so that no model runs on the host while the backlog drains"""
    C = 2
    group = {1: 1, 2: 1}                          # streams that share a count, per part
    out_slots = CS
    CHANGED = [1, 4]                              # the output slots whose run B is another without part 2's change

    def open(self, cm, tile, signal):
        self.cm, self.tile, self.F = cm, tile, max(208, tile + 64)
        self.ci = self.co = self.C
        self.s_in = (self.F * self.C + 7) // 8 * 8
        self.s_out = (self.F * self.C + 7) // 8 * 8 + 8
        self.src = _mapped(cm, CS, self.s_in)
        self.x = [signal(s) for s in range(CS)]
        for s in range(CS):
            assert self.x[s].shape == (self.F, self.C)
            self.src.array[s, :self.F * self.C] = self.x[s].reshape(-1)

    def outs(self, n):
        return [_mapped(self.cm, self.out_slots, self.s_out) for _ in range(n)]

    def run(self, counts, out):
        self.o.run(self.src.dev, self.s_in, self.F, out.dev, self.s_out, counts)

    def cut(self, counts):
        return [self.x[s][:n] for s, n in enumerate(counts)]

    def close(self):
        self.o.close()
        self.src.free()


# ---- the dynamics stage: plain upload()

class _Dyn(_Stage):
    detector, keyed = None, False
    a, b, H = 6, 6, 0

    def __init__(self, cm, st, part):
        plan = cm.plan_dynrms if self.detector else cm.plan_dyn
        self.open(cm, plan(CS, self.C, self.a, self.b, self.H, 1).tile_frames, lambda s: TD.signal(600 + s, self.F, self.C))
        self.T = TD.design(**TD.DENSE_CURVE)                         # a compressing, gating curve
        assert np.array_equal(cm.dyn_design(comp_threshold_db=-18, comp_ratio=4, comp_knee_db=6, gate_threshold_db=-45,
                                            gate_ratio=2, gate_range_db=40), self.T)
        self.o = cm.Dynamics(CS, self.C, self.a, self.b, self.H, self.F, curve=self.T, hip_stream=st,
                             detector=self.detector)
        self.m = TK.KeyModel(CS, self.C, self.a, self.b, self.H, detector=self.detector or TK.MEAN)
        self.m.set(-1, self.T)
        if self.keyed:                                               # s keyed by s ^ 1: each other's key
            for s in range(CS):
                self.o.set_key(s, s ^ 1)
                self.m.set_key(s, s ^ 1)

    def model(self, counts):
        return self.m.run(self.cut(counts))

    def state(self):
        assert self.o.min_gain().tolist() == self.m.gmin, "min_gain"
        assert min(self.m.gmin) < TD.UNITY                           # (the curve did something)

    T2 = TD.design(ct=-30.0, R=8.0, K=3.0, gt=-50.0, Re=3.0, rng=20.0)

    def set_curve(self, stream, T):
        """through cm.lib with a table the test owns, overwritten at once: the header calls it free on return"""
        buf = _own(T, np.uint16)
        assert self.cm.lib.cmhip_dyn_set_curve(self.o.h, stream, buf.ctypes.data) == 0
        buf[:] = TD.flat(12345)

    def change(self):
        self.set_curve(1, self.T2)
        self.o.reset(4)

    def model_change(self):
        self.m.set(1, self.T2)
        self.m.reset(4)

    def check_change(self):
        assert np.array_equal(self.o.get_curve(1), self.T2) and np.array_equal(self.o.get_curve(0), self.T)


class _DynKey(_Dyn):
    """cmhip_dyn_run refuses a stream whose count differs from its key's: counts equal within a pair (part 2: within
    the four streams of an old and a new pair)"""
    keyed, C = True, 1
    group = {1: 2, 2: 4}
    CHANGED = [0, 2, 5]

    def change(self):
        for s, k in ((0, 2), (2, 0)):                                # 0 <-> 2 now; 1 -> 0 and 3 -> 2 as before
            self.o.set_key(s, k)
        self.set_curve(5, self.T2)

    def model_change(self):
        for s, k in ((0, 2), (2, 0)):
            self.m.set_key(s, k)
        self.m.set(5, self.T2)

    def check_change(self):
        assert [self.o.get_key(s) for s in range(CS)] == [2, 0, 0, 2, 5, 4, 7, 6]
        assert np.array_equal(self.o.get_curve(5), self.T2)


class _DynRms(_Dyn):
    detector = TK.RMS


# ---- the limiter: the sample detector, the true-peak detector, the release stage over both

class _Lim(_Stage):
    detector, rho = None, None
    a, H = 6, 100

    def plan(self, cm):
        return cm.plan_lim(CS, self.C, self.a, self.H, 1)

    def new_model(self):
        return TL.Model(CS, self.C, self.a, self.H)

    def __init__(self, cm, st, part):
        self.open(cm, self.plan(cm).tile_frames, lambda s: TL.bursts(600 + s, self.F, self.C))
        self.o = cm.Limiter(CS, self.C, self.a, self.H, self.F, hip_stream=st, detector=self.detector,
                            release_log2=self.rho)
        self.m = self.new_model()
        assert self.o.delay() == self.m.D
        for s in range(CS):                                          # per stream another threshold and drive
            self.set(s, 12000 - 500 * s, 4096 + 512 * s)

    def set(self, stream, T, drive):
        self.o.set(stream, T, drive)
        self.m.set(stream, T, drive)

    def model(self, counts):
        return self.m.run(self.cut(counts))

    def state(self):
        assert self.o.min_gain().tolist() == self.m.gmin, "min_gain"
        assert max(self.m.gmin) < TL.UNITY                           # (every stream was limited)

    def change(self):
        self.o.set(1, 20000, 8192)
        self.o.reset(4)

    def model_change(self):
        self.m.set(1, 20000, 8192)
        self.m.reset(4)

    def check_change(self):
        assert [self.o.get(s) for s in range(CS)] == [tuple(p) for p in self.m.par]


class _LimTp(_Lim):
    C = 1

    def __init__(self, cm, st, part):
        self.detector = cm.LIM_DETECT_TRUE_PEAK
        super().__init__(cm, st, part)

    def plan(self, cm):
        return cm.plan_limtp(CS, self.C, self.a, self.H, 1)

    def new_model(self):
        return TTP.MH.ModelTp(CS, self.C, self.a, self.H)


class _LimRel(_Lim):
    rho, det = 9, TREL.SAMPLE

    def __init__(self, cm, st, part):
        self.detector = self.det
        super().__init__(cm, st, part)
        assert self.o.release() == self.rho and self.o.detector() == self.det

    def plan(self, cm):
        return cm.plan_limrel(self.det, CS, self.C, self.a, self.H, self.rho, 1)

    def new_model(self):
        return TREL.RH.ModelRel(self.det, CS, self.C, self.a, self.H, self.rho)


class _LimRelTp(_LimRel):
    det, C = TREL.TRUE_PEAK, 1


# ---- the band split: counts select B * S output slots, band-major

class _Split(_Stage):
    bands, taps = 3, 31
    out_slots = 3 * CS
    CHANGED = [3, CS + 3, 2 * CS + 3]

    def __init__(self, cm, st, part):
        self.open(cm, cm.plan_split(CS, self.C, self.bands, self.taps, 1).tile_frames,
                  lambda s: TSP.noise(600 + s, self.F, self.C))
        g, q = TSP.dense_table(self.bands, self.taps, 77)
        self.o = cm.BandSplit(CS, self.C, self.bands, self.taps, self.F, table=(g, q), hip_stream=st)
        self.models = [TSP.Model(g, q, self.C) for _ in range(CS)]

    def model(self, counts):
        ys = [m.run(x) for m, x in zip(self.models, self.cut(counts))]           # per stream [B][F][C]
        return [ys[s][b] for b in range(self.bands) for s in range(CS)]

    def state(self):
        want = np.array([m.clips for m in self.models], dtype=np.int64)
        assert np.array_equal(self.o.clips().astype(np.int64), want), "clips"

    def change(self):
        self.o.reset(3)

    def model_change(self):
        assert self.models[3].hist.any()                             # (run A left a history to lose)
        self.models[3].reset()

    def check_change(self):
        assert self.models[3].hist.any() and self.models[2].hist.any()           # (run B left both a history)


# ---- the delay: the block holds records (count, position, both taps, ramp place)

class _Delay(_Stage):
    C, MAX_DELAY = 1, 300
    CHANGED = [0, 1, 3, 5]

    def __init__(self, cm, st, part):
        self.open(cm, cm.plan_delay(CS, self.C, self.MAX_DELAY, 4096, 1).tile_frames,
                  lambda s: TDL.noise(600 + s, self.F, self.C))
        self.o = cm.Delay(CS, self.C, self.MAX_DELAY, self.F, hip_stream=st)
        self.models = [TDL.Model(self.C, self.MAX_DELAY) for _ in range(CS)]
        self.R = 6 * self.F + 1000                                   # a ramp that spans every run of the test
        assert self.R <= TDL.RAMP_MAX
        for s in range(CS):                                          # a delay of its own per stream
            self.set(s, 10 + 30 * s)
        for s in (range(CS) if part == 1 else [3]):                  # part 1: every stream inside a ramp over all runs
            self.ramp(s, 290 - 35 * s, self.R)

    def set(self, s, d):
        self.o.set(s, d)
        self.models[s].set(d)

    def ramp(self, s, d, R):
        self.o.ramp(s, d, R)
        assert self.models[s].ramp(d, R)

    def model(self, counts):
        return [m.run(x) for m, x in zip(self.models, self.cut(counts))]

    def state(self):
        for s, m in enumerate(self.models):
            assert self.o.get(s) == m.get(), ("get", s)

    def change(self):
        self.o.set(0, 77)                                            # a step
        self.o.ramp(1, 200, 500)                                     # a ramp that ends inside run B
        self.o.set(3, 40)                                            # a step that cancels the running ramp
        self.o.reset(5)

    def model_change(self):
        self.models[0].set(77)
        assert self.models[1].ramp(200, 500) and self.models[3].ramping()
        self.models[3].set(40)
        self.models[5].reset()

    def check_change(self):
        assert not any(m.ramping() for m in self.models)


# ---- the leveller: the block holds records (count, position, parameters)

class _Agc(_Stage):
    W_LOG2 = 6
    CHANGED = [0, 2, 4]

    def __init__(self, cm, st, part):
        self.open(cm, 1 << cm.plan_agc(CS, self.C, self.W_LOG2, 4096, 1).tile_log2,
                  lambda s: TA.enveloped(600 + s, self.F, self.C, 1 << self.W_LOG2))
        self.o = cm.Leveller(CS, self.C, self.W_LOG2, self.F, hip_stream=st)
        self.models = [TA.Model(self.C, self.W_LOG2) for _ in range(CS)]
        for s in range(CS):                                          # parameters of its own per stream
            self.set(s, TA.palette(s))

    def set(self, s, p):
        self.o.set(s, self.cm.AgcParams(**p))
        self.models[s].set(p)

    def model(self, counts):
        return [m.run(x) for m, x in zip(self.models, self.cut(counts))]

    def state(self):
        gain, level, clips = self.o.state()
        want = [m.state() for m in self.models]
        assert gain.tolist() == [v[0] for v in want], "gain"
        assert level.tolist() == [v[1] for v in want], "level"
        assert clips.tolist() == [v[2] for v in want], "clips"

    NEW = {0: TA.params(target=1000, gate=0, gain_min=100, gain_max=5000, rise=65535, fall=65535, initial=100),
           2: TA.palette(6)}

    def change(self):
        for s, p in self.NEW.items():
            self.o.set(s, self.cm.AgcParams(**p))
        self.o.reset(4)

    def model_change(self):
        for s, p in self.NEW.items():
            self.models[s].set(p)
        self.models[4].reset()

    def check_change(self):
        assert [self.o.get(s).as_dict() for s in range(CS)] == [m.p for m in self.models]


# ---- the filter: run 1 carries the table behind its counts, run 2 does not

class _Iir(_Stage):
    C, SECTIONS = 1, 2
    CHANGED = [0, 1, 2, 4, 5, 6, 7]               # (stream 3 had section 0's new coefficients before)

    def __init__(self, cm, st, part):
        self.open(cm, cm.plan_iir(CS, self.C, self.SECTIONS, 1).tile, lambda s: TI.noise(600 + s, self.F, self.C))
        self.o = cm.Filter(CS, self.C, self.SECTIONS, self.F, hip_stream=st)
        self.m = TI.Model(CS, self.C, self.SECTIONS)
        for s in range(CS):                                          # two sections of its own per stream
            for k in range(self.SECTIONS):
                self.set(s, k, TI.palette(cm, s + 5 * k))

    def set(self, s, k, sec):
        self.o.set(s, k, self.cm.IirSection(*sec))
        self.m.set(s, k, sec)

    def model(self, counts):
        return self.m.run(self.cut(counts))

    def state(self):
        clips, overs = self.o.state()
        assert clips.tolist() == self.m.clips.tolist(), "clips"
        assert overs.tolist() == self.m.overs.tolist(), "overs"
        have, want = self.o.rows(), self.m.rows()
        bad = np.argwhere(have != want)
        assert bad.size == 0, ("rows: first mismatch (row, section, field)", bad[0].tolist())

    def change(self):
        self.new = TI.palette(self.cm, 8), TI.palette(self.cm, 3)
        self.o.set(2, 1, self.cm.IirSection(*self.new[0]))           # one section of one stream
        self.o.set(-1, 0, self.cm.IirSection(*self.new[1]))          # one section of all streams
        self.o.reset(5)

    def model_change(self):
        self.m.set(2, 1, self.new[0])
        self.m.set(-1, 0, self.new[1])
        self.m.reset(5)

    def check_change(self):
        for s in range(CS):
            for k in range(self.SECTIONS):
                assert self.o.get(s, k).as_tuple() == tuple(int(v) for v in self.m.coef[s, k]), (s, k)


# ---- part 2 alone: the mixer and the bus (part 1 has them in tests/test_gpu_programme_chain.py)

class _Mix(_Stage):
    def __init__(self, cm, st, part):
        self.open(cm, 4096, lambda s: TR.noise(600 + s, self.F, self.C))
        self.o = cm.Mixer(CS, 2, 2, self.F, hip_stream=st)
        w0 = [TR.dense_matrix(2, 2, 700 + s) for s in range(CS)]
        for s, w in enumerate(w0):
            self.o.set_matrix(s, w)
        self.models = [TR.RampModel(w) for w in w0]

    def model(self, counts):
        return [m.run(x) for m, x in zip(self.models, self.cut(counts))]

    def state(self):
        for s, m in enumerate(self.models):
            done, total, w = self.o.ramp_state(s)
            assert (done, total) == m.state()[:2] and np.array_equal(w, m.state()[2]), ("ramp state", s)

    def change(self):
        lib = self.cm.lib
        w1, w2 = TR.dense_matrix(2, 2, 901), TR.dense_matrix(2, 2, 902)
        other = _own(TR.dense_matrix(2, 2, 903), np.int16)
        buf = _own(w1, np.int16)
        assert lib.cmhip_mix_set_matrix(self.o.h, 1, buf.ctypes.data) == 0
        buf[:] = other
        buf = _own(w2, np.int16)
        assert lib.cmhip_mix_ramp_matrix(self.o.h, 4, buf.ctypes.data, 3000) == 0
        buf[:] = other
        self.w1, self.w2 = w1, w2

    def model_change(self):
        self.models[1].set(self.w1)
        self.models[4].ramp(self.w2, 3000)

    def check_change(self):
        assert np.array_equal(self.o.get_matrix(1), self.w1) and np.array_equal(self.o.get_matrix(4), self.w2)
        assert not any(m.ramping() for m in self.models)             # (the ramp ended inside run B)


class _Bus(_Stage):
    """set_routing: the whole table from the caller's three arrays"""
    out_slots = 2
    CHANGED = [0, 1]

    def __init__(self, cm, st, part):
        self.open(cm, 4096, lambda s: TB.noise(600 + s, self.F, self.C))
        self.o = cm.Bus(CS, 2, 2, 2, self.F, CS, hip_stream=st)
        self.m = TBR.BusRampModel(2, 2, 2)
        table = ([s % 2 for s in range(CS)], list(range(CS)), TB.dense_sends(2, 2, CS, CS // 2, 900))
        self.o.set_routing(*table)
        self.m.set(*table)
        self.got, self.want = [], []

    def run(self, counts, out):
        self.got.append(self.o.run(self.src.dev, self.s_in, self.F, out.dev, self.s_out, counts).tolist())

    def model(self, counts):
        ys = self.m.run(self.cut(counts))
        self.want.append([y.shape[0] for y in ys])
        return ys

    def state(self):
        assert self.got == self.want, "out_frames"
        for j in range(len(self.m.sends)):
            done, total, w = self.o.ramp_state(j)
            d, r, wm = self.m.state(j)
            assert (done, total) == (d, r) and np.array_equal(w, wm), ("send", j)

    def change(self):
        bus, strm = [s // 4 for s in range(CS - 1)], list(range(CS - 1, 0, -1))   # seven sends, another order
        w = TB.dense_sends(2, 2, CS - 1, 4, 910)
        b, s, wb = _own(bus, np.uint32), _own(strm, np.uint32), _own(w, np.int16)
        assert self.cm.lib.cmhip_bus_set_routing(self.o.h, len(bus), b.ctypes.data, s.ctypes.data, wb.ctypes.data) == 0
        b[:] = 1
        s[:] = 0
        wb[:] = _own(TB.dense_sends(2, 2, CS - 1, 4, 911), np.int16)
        self.new = bus, strm, w

    def model_change(self):
        self.m.set(*self.new)

    def check_change(self):
        assert np.array_equal(self.o.get_routing()[2], self.m.targets())


class _BusRamp(_Bus):
    """ramp_sends: three sends from the caller's array, a ramp that ends inside run B"""

    def change(self):
        w = TB.dense_sends(2, 2, 3, CS // 2, 920)
        buf = _own(w, np.int16)
        assert self.cm.lib.cmhip_bus_ramp_sends(self.o.h, 2, 3, buf.ctypes.data, 3000) == 0
        buf[:] = _own(TB.dense_sends(2, 2, 3, CS // 2, 921), np.int16)
        self.new = w

    def model_change(self):
        self.m.ramp(2, self.new, 3000)

    def check_change(self):
        super().check_change()
        assert not any(s.ramping() for s in self.m.sends)            # (the ramps ended inside run B)


COUNTS_KINDS = {"dyn": _Dyn, "dyn_key": _DynKey, "dyn_rms": _DynRms, "limtp": _LimTp, "limrel": _LimRel,
                "limrel_tp": _LimRelTp, "split": _Split, "delay": _Delay, "agc": _Agc, "iir": _Iir}
CHANGE_KINDS = dict(COUNTS_KINDS, lim=_Lim, mix=_Mix, bus_routing=_Bus, bus_ramp=_BusRamp)


# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def backlog(gpu):
    big = gpu.Batch(BACKLOG_STREAMS, 2, BACKLOG_FRAMES, flags=gpu.OUT_PCM | gpu.VU)
    # hipStreamQuery of the runtime the ENGINE is linked to, looked up through the engine's own handle (a process may
    # hold a second HIP runtime that knows nothing of the engine's streams)
    query = gpu.lib.hipStreamQuery
    query.argtypes = [C.c_void_p]
    query.restype = C.c_int
    yield big, query
    big.close()


def _check_runs(u, outs, wants_of_runs):
    for i, wants in enumerate(wants_of_runs):
        assert len(wants) == u.out_slots
        for slot, want in enumerate(wants):
            want = np.asarray(want).reshape(-1, u.co)
            have = outs[i].array[slot, :want.size].reshape(-1, u.co)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("run", i + 1, "slot", slot, "first mismatch (frame, channel)", bad[0].tolist(), "of",
                                   want.shape[0], "frames: got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (outs[i].array[slot, want.size:] == SENTINEL).all(), ("run", i + 1, "slot", slot, "written past its count")


def _pinned_counts(cm):
    ptr = cm.lib.cmhip_host_alloc(4 * CS)                            # ONE pinned array for the counts of every run
    assert ptr
    counts = np.frombuffer((C.c_uint32 * CS).from_address(ptr), dtype=np.uint32)
    assert np.ascontiguousarray(counts, dtype=np.uint32).ctypes.data == ptr      # (the mirror passes it on as it is)
    return ptr, counts


@pytest.mark.parametrize("kind", list(COUNTS_KINDS))
def test_counts_are_free_on_return(gpu, backlog, kind):
    """With CountsRing::take() handing out block 0 without a wait (one block, as before the ring) every one of these
    kinds failed on an MI355X at run 1, slot 0: delay and agc on the output (another run's position, taps and
    parameters), the eight others on the sentinel past the count (run 1 wrote as many frames as a later run's counts
    say).  On the ring as it is the stream was still busy in every case: queued in 0.5-1.8 ms, drained after
    10.6-12.0 ms, 6.8-20.7 x."""
    cm = gpu
    big, stream_query = backlog
    st = big.hip_stream()
    u = COUNTS_KINDS[kind](cm, st, 1)
    outs, ptr = [], None
    try:
        assert u.o.hip_stream() == st
        runs = run_counts(u.F, u.group[1])
        assert max(runs[1]) > u.tile                                 # some stream has more than one tile
        outs += u.outs(len(runs))
        for o in outs:
            o.array[:] = SENTINEL
        ptr, counts = _pinned_counts(cm)
        big.sync()
        t0 = time.perf_counter()
        for _ in range(BACKLOG_RUNS_OF.get(kind, BACKLOG_RUNS)):
            big.run(BACKLOG_FRAMES)
        counts[:] = runs[0]
        u.run(counts, outs[0])
        counts[:] = runs[1]
        u.run(counts, outs[1])
        state = stream_query(st)
        t1 = time.perf_counter()
        for i in (2, 3):
            counts[:] = runs[i]
            u.run(counts, outs[i])
        counts[:] = runs[4]
        u.run(counts, outs[4])                                       # (its take() waits for run 1's copy: the backlog is through)
        t2 = time.perf_counter()
        counts[:] = runs[5]
        u.run(counts, outs[5])
        big.sync()                                                   # (the only synchronisation)
        t3 = time.perf_counter()
        print("counts %s: frames %d (tile %d), queued in %.2f ms, the stream drained after %.2f ms: margin %.1f x, "
              "hipStreamQuery %d, all six runs done after %.2f ms"
              % (kind, u.F, u.tile, 1e3 * (t1 - t0), 1e3 * (t2 - t0), (t2 - t0) / (t1 - t0), state, 1e3 * (t3 - t0)))
        # the proof that run 1's copy had not executed when the array changed; without it the test proves nothing
        assert state == HIP_ERROR_NOT_READY, "set-up failure: the backlog had drained before run 2 was queued (%d)" % state
        _check_runs(u, outs, [u.model(c) for c in runs])
        u.state()
    finally:                                 # (before the backlog's stream goes, whatever the outcome)
        u.close()
        for o in outs:
            o.free()
        if ptr:
            cm.lib.cmhip_host_free(ptr)


@pytest.mark.parametrize("kind", list(CHANGE_KINDS))
def test_changes_queue_behind_pending_runs(gpu, backlog, kind):
    cm = gpu
    big, stream_query = backlog
    st = big.hip_stream()
    u = CHANGE_KINDS[kind](cm, st, 2)
    outs, ptr = [], None
    try:
        assert u.o.hip_stream() == st
        runs = run_counts(u.F, u.group[2])[:2]
        outs += u.outs(2)
        for o in outs:
            o.array[:] = SENTINEL
        ptr, counts = _pinned_counts(cm)
        big.sync()
        t0 = time.perf_counter()
        for _ in range(BACKLOG_RUNS_OF.get(kind, BACKLOG_RUNS)):
            big.run(BACKLOG_FRAMES)
        counts[:] = runs[0]
        u.run(counts, outs[0])                                       # run A
        u.change()                                                   # ... the change
        counts[:] = runs[1]
        u.run(counts, outs[1])                                       # run B
        state = stream_query(st)
        t1 = time.perf_counter()
        big.sync()
        t2 = time.perf_counter()
        print("change %s: frames %d, queued in %.2f ms, the stream drained after %.2f ms: margin %.1f x, hipStreamQuery %d"
              % (kind, u.F, 1e3 * (t1 - t0), 1e3 * (t2 - t0), (t2 - t0) / (t1 - t0), state))
        # the proof that run A was still pending when the change was made; without it the test proves nothing
        assert state == HIP_ERROR_NOT_READY, "set-up failure: the backlog had drained before run B was queued (%d)" % state
        want_a = u.model(runs[0])                                    # the model: run A, the change, run B
        unset = {k: copy.deepcopy(v) for k, v in vars(u).items() if k in ("m", "models", "want")}
        u.model_change()
        want_b = u.model(runs[1])
        # copies of the models that never see the change show that it mattered, in every slot it names
        ours = {k: getattr(u, k) for k in unset}
        vars(u).update(unset)
        without = u.model(runs[1])
        vars(u).update(ours)
        assert [i for i, (w, v) in enumerate(zip(want_b, without)) if not np.array_equal(w, v)] == u.CHANGED
        _check_runs(u, outs, [want_a, want_b])
        u.state()
        u.check_change()
    finally:                                 # (before the backlog's stream goes, whatever the outcome)
        u.close()
        for o in outs:
            o.free()
        if ptr:
            cm.lib.cmhip_host_free(ptr)
