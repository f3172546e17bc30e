"""GPU: what the nine stage objects beside a batch have in common -- reset, a refused run, a run of no frames, the
synchronous readbacks, the ownership of the stream, creation and its end -- held side by side for every kind.

The per-stage files pin each stage's numbers and tests/test_gpu_stage_queue.py its ordering behind a busy stream; this
file pins the contract around them, which the stages' host code keeps in one copy (csrc/cmhip_stage.h).  The objects,
signals and numpy models are test_gpu_stage_queue's (COUNTS_KINDS, CHANGE_KINDS), loaded the way that file loads the
per-stage files; the resampler joins them with the model of tests/test_gpu_src.py.  Expected output is always a model's,
never another run of the device code.

Shapes: 8 streams, 1 or 2 channels, frames of the stage's tile + 64, ragged counts that differ between successive runs.
Every refused call is one the library refuses on the host before anything is launched.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("contract_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Q, TS = _load("test_gpu_stage_queue"), _load("test_gpu_src")
CS, SENTINEL = Q.CS, Q.SENTINEL
assert TS.SENTINEL == SENTINEL
MID = 3                                           # the single stream a reset names


class _Src(Q._Stage):
    """the resampler, 3 -> 2 with weight at every tap: fewer frames leave than enter, so the output slots of the other
    kinds hold them; r = (frames so far) mod 3 moves with every count"""
    L, M, T = 2, 3, 16

    def __init__(self, cm, st, part):
        tile = cm.plan_src(CS, self.C, self.L, self.M, self.T, 4096).tile_in
        self.open(cm, tile, lambda s: TS.noise(600 + s, self.F, self.C))
        H = TS.dense_table(self.L, self.T, 77)
        self.o = cm.Resampler(CS, self.C, 48000, 32000, self.F, table=(self.L, self.M, H), hip_stream=st)
        self.models = [TS.Model(self.L, self.M, H, self.C) for _ in range(CS)]
        self.got, self.want = [], []

    def run(self, counts, out):
        self.got.append(self.o.run(self.src.dev, self.s_in, self.F, out.dev, self.s_out, counts).tolist())

    def model(self, counts):
        ys = [m.run(x) for m, x in zip(self.models, self.cut(counts))]
        self.want.append([y.shape[0] for y in ys])
        return ys

    def state(self):
        assert self.got == self.want, "out_frames"


KINDS = dict(Q.CHANGE_KINDS, src=_Src)
# the kinds with two slots of history (src, lim*, dyn*, split) and the others that have a reset
RESET_KINDS = ["src", "lim", "limtp", "limrel", "dyn", "dyn_rms", "split", "delay", "agc", "iir"]
RUN_KINDS = RESET_KINDS + ["mix", "bus_routing"]
NINE = ["src", "mix", "bus_routing", "lim", "dyn", "split", "delay", "agc", "iir"]       # one kind per C object


def model_reset(u, stream):
    if hasattr(u, "m"):
        u.m.reset(stream)
    else:
        for s in (range(CS) if stream < 0 else [stream]):
            u.models[s].reset()


class Rig:
    """a kind's object on a stream of its own (or `st`), runs with the counts of test_gpu_stage_queue.run_counts, and
    the comparison of every run so far with the model"""

    def __init__(self, cm, kind, st=None):
        self.cm, self.u = cm, KINDS[kind](cm, st, 1)
        runs = Q.run_counts(self.u.F, self.u.group[1])
        self.counts = [runs[i] for i in (0, 1, 3, 5)]                # (the four with at least 100 frames in every stream)
        assert max(self.counts[1]) > self.u.tile                     # some stream has more than one tile
        self.outs, self.ran, self.wants = [], [], []

    def run(self):
        """the next run of the list, on the device alone"""
        c = self.counts[len(self.ran)]
        out = self.u.outs(1)[0]
        out.array[:] = SENTINEL
        self.outs.append(out)
        self.u.run(np.array(c, dtype=np.uint32), out)
        self.ran.append(c)

    def refused(self, frames, out_stride, counts):
        """a run the host must refuse -> the error number (the output array is the last run's: nothing may touch it)"""
        u = self.u
        rc = u.o.run_rc(u.src.dev, u.s_in, frames, self.outs[-1].dev, out_stride, counts)
        return rc[0] if isinstance(rc, tuple) else rc

    def check(self, events=()):
        """every run against the model, which moves over the runs it has not seen; events: {index of a run: what the
        model does before it}, then the observable state"""
        self.u.o.sync()
        for i in range(len(self.wants), len(self.ran)):
            for act in dict(events).get(i, []):
                act()
            self.wants.append(self.u.model(self.ran[i]))
        Q._check_runs(self.u, self.outs, self.wants)
        if hasattr(self.u.o, "min_gain"):                            # (the kind's state() without its demand that every
            assert self.u.o.min_gain().tolist() == self.u.m.gmin     # stream's meter has moved: a reset puts it back)
        else:
            self.u.state()

    def close(self):
        self.u.close()
        for o in self.outs:
            o.free()


@pytest.fixture
def rig(gpu):
    made = []

    def make(kind, st=None):
        made.append(Rig(gpu, kind, st))
        return made[-1]

    yield make
    for r in made:
        r.close()


@pytest.mark.parametrize("before", [1, 2])
@pytest.mark.parametrize("kind", RESET_KINDS)
def test_reset_at_both_parities(rig, kind, before):
    """after one run and after two (the two slots of a history change places with every run): reset of one stream, a
    run, reset of every stream, a run.  A reset stream continues as a model started afresh, every other one as a model
    that was never reset"""
    r = rig(kind)
    for _ in range(before):
        r.run()
    r.u.o.reset(MID)
    r.run()
    r.u.o.reset(-1)
    r.run()
    r.check({before: [lambda: model_reset(r.u, MID)], before + 1: [lambda: model_reset(r.u, -1)]})


@pytest.mark.parametrize("kind", RUN_KINDS)
def test_refused_run_changes_nothing(gpu, rig, kind):
    """a run, two refused calls, a run: the second run is the model's second -- neither the history's parity nor a
    mirror moved with a refusal, and nothing was written"""
    r = rig(kind)
    u = r.u
    r.run()
    u.o.sync()
    before = r.outs[0].array.copy()
    above = np.array(r.counts[1], dtype=np.uint32)
    above[MID] = u.F + 1
    assert r.refused(u.F, u.s_out, above) == gpu.ERROR_INVAL
    assert "frames_per_stream[%d] above frames" % MID in gpu.last_error()
    assert r.refused(u.F, 8, np.array(r.counts[1], dtype=np.uint32)) == gpu.ERROR_INVAL
    assert "out_stride 8 below" in gpu.last_error()
    r.run()
    r.check()
    assert np.array_equal(r.outs[0].array, before)


@pytest.mark.parametrize("kind", RUN_KINDS)
def test_run_of_no_frames(gpu, rig, kind):
    """a run of 0 frames returns 0 and is no run: the next one is the model's second"""
    r = rig(kind)
    r.run()
    assert r.refused(0, r.u.s_out, None) == 0
    assert r.refused(0, r.u.s_out, np.zeros(CS, dtype=np.uint32)) == 0
    r.run()
    r.check()


def _read_min_gain(o, clear):
    return [o.min_gain(reset=clear)]


def _read_clips(o, clear):
    return [o.clips(clear=clear)]


def _read_agc(o, clear):
    return list(o.state(clear_clips=clear))


def _read_iir(o, clear):
    return list(o.state(clear=clear))


# kind -> (the read, per array: its value after a clearing read, None where the read clears nothing of it)
READBACKS = {"lim": (_read_min_gain, [Q.TL.UNITY]), "limtp": (_read_min_gain, [Q.TL.UNITY]),
             "limrel": (_read_min_gain, [Q.TL.UNITY]), "dyn": (_read_min_gain, [Q.TD.UNITY]),
             "dyn_rms": (_read_min_gain, [Q.TD.UNITY]), "split": (_read_clips, [0]), "agc": (_read_agc, [None, None, 0]),
             "iir": (_read_iir, [0, 0])}


@pytest.mark.parametrize("kind", list(READBACKS))
def test_readbacks(rig, kind):
    """min_gain, clips, state: a read without clear leaves the values, a read with clear returns them and leaves the
    initial ones, complete on return; the values are the model's"""
    read, initial = READBACKS[kind]
    r = rig(kind)
    r.run()
    r.run()
    r.check()                                                        # (the model's values, with no clear)
    first = read(r.u.o, False)
    for a, init in zip(first, initial):
        if init is not None:
            assert (a != init).any(), "the signal leaves nothing to clear"
    again = read(r.u.o, False)
    cleared = read(r.u.o, True)
    after = read(r.u.o, False)
    for a, b, c, d, init in zip(first, again, cleared, after, initial):
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.array_equal(d, a if init is None else np.full_like(a, init))


@pytest.mark.parametrize("kind", NINE)
def test_stream_ownership(gpu, rig, kind):
    """an object made without a stream has one of its own; one made on a caller's stream reports that stream and leaves
    it usable when it goes"""
    big = gpu.Batch(CS, 2, 4096, flags=gpu.OUT_PCM | gpu.VU)
    try:
        st = big.hip_stream()
        own, lent = rig(kind), rig(kind, st)
        assert own.u.o.hip_stream() not in (0, st)
        assert lent.u.o.hip_stream() == st
        for r in (own, lent):
            r.run()
            r.check()
        lent.u.o.close()
        big.generate(gpu.GEN_NOISE, 1, 4096)
        big.run(4096)
        big.sync()
        own.run()
        own.check()
    finally:
        big.close()


@pytest.mark.parametrize("kind", NINE)
def test_create_and_close_without_a_run(rig, kind):
    """creation queues the object's first fills on its stream; close() without a run waits for them and returns, and a
    second object of the same shape runs as the model says"""
    rig(kind).u.o.close()
    r = rig(kind)
    r.run()
    r.run()
    r.check()
