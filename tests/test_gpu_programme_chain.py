"""GPU: the programme chain as one chain, block by block -- source -> rate (cmhip_src_t) -> width (cmhip_mix_t, with
matrix ramps) -> sum (cmhip_bus_t) -> limit (cmhip_lim_t) -> batch (VU, true peak, loudness) -- and the contract that a
run's frames_per_stream array is free when the call returns.

1. test_chain: all five objects on the batch's stream, one set of intermediate arrays reused by every block, every
   stage's counts the previous stage's out_frames, fourteen ragged blocks and two ramp_matrix calls queued without a
   synchronisation; after the one sync every block's PCM, the sentinel past every count, every out_frames the host
   returned, the ramp state, the gain-reduction meter and the three meters are held to the composition of the numpy
   models the per-object tests already have -- never to another run of the device code.  Every stage carries state from
   run to run (the resampler's r and history, a ramp's position, the limiter's two history slots, the meters), and two
   stages compute the next stage's counts on the host from a mirror.
2. test_counts_are_free_on_return: the counts of a run live in ONE pinned array (cmhip_host_alloc) that the host
   refills for the next run while the first is still queued behind a backlog.  hipMemcpyAsync from pinned memory reads
   the host array when the stream reaches the copy; each object must therefore have taken its copy before it returned.

(tests/test_programme_chain_host.py takes the chain's inputs and its model from here and holds the model alone to its
own properties, without a GPU.)"""
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
    spec = importlib.util.spec_from_file_location("chain_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TS, TR, TB, TL = _load("test_gpu_src"), _load("test_gpu_mix_ramp"), _load("test_gpu_bus"), _load("test_gpu_lim")
TTP, TLD = _load("test_gpu_truepeak"), _load("test_gpu_loudness")
SENTINEL, POISON, UNITY = TL.SENTINEL, TB.POISON, TL.UNITY

# ---------------------------------------------------------------------------
# the chain: its shape, its inputs and its model (numpy alone)

STREAMS, BUSES = 6, 2                             # streams 0-2 -> bus 0, streams 3-5 -> bus 1
RATE_IN, RATE_OUT = 44100, 48000
LOOKAHEAD_LOG2, HOLD = 6, 100
# per-block input counts, one list per bus: the streams of a bus share theirs (only then is the block-wise sum the sum
# of the whole signals), the two buses differ (every run is ragged across streams and buses).  Blocks of 0, 1 and 7
# frames -- below the limiter's history of 226 frames and the resampler's filter -- right behind long ones, counts on
# both sides of the limiter's 4096-frame tile, a stream with 0 frames beside one with thousands.
CUTS = ([4410, 1, 7, 0, 4097, 441, 8192, 3, 5000, 2, 6000, 4411, 0, 8000],
        [1, 4410, 0, 7, 441, 8191, 4097, 5000, 3, 6000, 2, 0, 4411, 8192])
MAX_IN = 8192
RAMPS = {2: 3000, 5: 20000}                       # before block r: every stream ramps to a new matrix over R frames
# fast: the mono / stereo kernels throughout; any: the any-channel-count kernels throughout.  Threshold and drive are
# chosen so that the MODEL meets the dense conditions of tests/test_gpu_lim.py (tests/test_programme_chain_host.py
# holds it to them); the batch's gains are at or below the scale, so the threshold bounds the device's own output.
VARIANTS = {
    "fast": dict(ci=1, co=2, threshold=8000, drive=8192, gains=[750, 1000]),
    "any": dict(ci=3, co=6, threshold=12000, drive=8192, gains=[750, 1000, 900, 1000, 500, 999]),
}
GAIN_SCALE = 1000


def bus_of(stream):
    return stream // (STREAMS // BUSES)


def routing(co):
    """-> (bus [n], stream [n], W [n][co][co]): every stream sent to its bus at 8192 on the diagonal"""
    w = np.zeros((STREAMS, co, co), dtype=np.int16)
    for c in range(co):
        w[:, c, c] = 8192
    return [bus_of(s) for s in range(STREAMS)], list(range(STREAMS)), w


def matrices(variant, stage):
    """the streams' matrices int16 [co][ci], weights within +-9000: stage 0 at creation, 1 and 2 the ramps' targets"""
    v = VARIANTS[variant]
    rng = np.random.default_rng(4000 + 100 * v["ci"] + stage)
    return [rng.integers(-9000, 9001, size=(v["co"], v["ci"])).astype(np.int16) for _ in range(STREAMS)]


def sources(variant):
    """per stream int16 [F][ci]: the limiter tests' bursts over quiet noise, as long as the stream's bus's cuts"""
    ci = VARIANTS[variant]["ci"]
    return [TL.bursts(9000 + 10 * ci + s, sum(CUTS[bus_of(s)]), ci) for s in range(STREAMS)]


class ChainModel:
    """the five stages' models behind each other, state and all"""

    def __init__(self, table, variant):
        L, M, T, H = table
        v = VARIANTS[variant]
        self.v, self.co = v, v["co"]
        self.src = [TS.Model(L, M, H, v["ci"]) for _ in range(STREAMS)]
        self.ramp = [TR.RampModel(w) for w in matrices(variant, 0)]
        self.table = routing(v["co"])
        self.lim = TL.Model(BUSES, v["co"], LOOKAHEAD_LOG2, HOLD)
        self.lim.set(-1, v["threshold"], v["drive"])
        self.mixed, self.summed = [], []             # every mixer and bus output, for the dense conditions

    def ramp_all(self, targets, R):
        for m, w in zip(self.ramp, targets):
            m.ramp(w, R)

    def run(self, xs):
        """xs: per stream int16 [F_s][ci] -> (the resampler's counts [S], the bus's counts [B], per bus the limiter's
        output int16 [F_b][co])"""
        ys = [m.run(x) for m, x in zip(self.src, xs)]
        zs = [m.run(y) for m, y in zip(self.ramp, ys)]
        sums = TB.model_bus(zs, self.table, BUSES, self.co)
        outs = self.lim.run(sums)
        self.mixed += zs
        self.summed += sums
        return [y.shape[0] for y in ys], [u.shape[0] for u in sums], outs


_cases = {}


def chain_case(cm, variant):
    """the inputs and, block by block, what the model gives -- computed once, never changed"""
    if variant in _cases:
        return _cases[variant]
    table = TS.table(cm, RATE_IN, RATE_OUT)
    xs = sources(variant)
    model = ChainModel(table, variant)
    pos = [0] * STREAMS
    blocks = []
    for r in range(len(CUTS[0])):
        if r in RAMPS:
            model.ramp_all(matrices(variant, 1 if r == 2 else 2), RAMPS[r])
        counts = [CUTS[bus_of(s)][r] for s in range(STREAMS)]
        ins = [xs[s][pos[s]:pos[s] + counts[s]] for s in range(STREAMS)]
        pos = [p + n for p, n in zip(pos, counts)]
        src_counts, bus_counts, outs = model.run(ins)
        blocks.append(types.SimpleNamespace(counts=counts, ins=ins, src_counts=src_counts, bus_counts=bus_counts,
                                            outs=outs))
    assert pos == [x.shape[0] for x in xs]
    case = types.SimpleNamespace(variant=variant, v=VARIANTS[variant], table=table, xs=xs, blocks=blocks, model=model)
    _cases[variant] = case
    return case


def programme(case, b):
    """bus b's limiter output over all blocks, int16 [F][co]"""
    return np.concatenate([blk.outs[b] for blk in case.blocks])


# ---------------------------------------------------------------------------
# 1. the chain on the device

def _mapped(cm, streams, stride):
    return cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=stride))


def _stride(frames, channels):
    return (frames * channels + 7) // 8 * 8 + 8


@pytest.mark.parametrize("variant", ["fast", "any"])
def test_chain(gpu, oracle, variant):
    from oracle import oracle_ffi
    cm = gpu
    case = chain_case(cm, variant)
    v, ci, co = case.v, case.v["ci"], case.v["co"]
    L, M, T, H = case.table
    S, B, T_lim = STREAMS, BUSES, v["threshold"]
    max_out = MAX_IN * L // M + 1

    objects, arrays = [], []
    try:
        batch = cm.Batch(B, co, max_out, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, rate=RATE_OUT)
        objects.append(batch)
        assert batch.set_gain(-1, co, GAIN_SCALE, v["gains"]) == 0
        assert batch.set_true_peak(1) == 0 and batch.set_loudness(1) == 0
        st = batch.hip_stream()
        src = cm.Resampler(S, ci, RATE_IN, RATE_OUT, MAX_IN, hip_stream=st)
        objects.append(src)
        mix = cm.Mixer(S, ci, co, max_out, hip_stream=st)
        objects.append(mix)
        bus = cm.Bus(S, B, co, co, max_out, S, hip_stream=st)
        objects.append(bus)
        lim = cm.Limiter(B, co, LOOKAHEAD_LOG2, HOLD, max_out, threshold=T_lim, drive=v["drive"], hip_stream=st)
        objects.append(lim)
        assert src.hip_stream() == mix.hip_stream() == bus.hip_stream() == lim.hip_stream() == st
        assert src.max_out_frames() == max_out and (cm.plan_lim(B, co, LOOKAHEAD_LOG2, HOLD, 1).tile_frames == 4096)
        assert cm.plan_mix(S, ci, co, 1).fast == cm.plan_bus(B, co, co, 1).fast == (1 if variant == "fast" else 0)
        for s, w in enumerate(matrices(variant, 0)):
            mix.set_matrix(s, w)
        bus.set_routing(*routing(co))

        # ONE set of intermediate arrays in device memory, reused by every block and never cleared in between
        s_in, s_a, s_b, s_c = (MAX_IN * ci + 7) // 8 * 8, _stride(max_out, ci), _stride(max_out, co), _stride(max_out, co)
        d_a = cm.DeviceWords((S * s_a * 2 + 7) // 8)     # the resampler's output
        d_b = cm.DeviceWords((S * s_b * 2 + 7) // 8)     # the mixer's
        d_c = cm.DeviceWords((B * s_c * 2 + 7) // 8)     # the bus's
        d_d = cm.DeviceWords((B * batch.stride * 2 + 7) // 8)        # the limiter's: the batch's input slots
        arrays += [d_a, d_b, d_c, d_d]
        # every block's sources and every block's result in pinned, device-mapped arrays of their own
        feeds, results = [], []
        for blk in case.blocks:
            feed, res = _mapped(cm, S, s_in), cm.MappedPcm(batch)
            feed.array[:] = POISON
            for s, x in enumerate(blk.ins):
                feed.array[s, :x.size] = x.reshape(-1)
            res.array[:] = SENTINEL
            feeds.append(feed)
            results.append(res)
            arrays += [feed, res]

        # the host loop: block after block, no wait anywhere
        got_src, got_bus = [], []
        for r, blk in enumerate(case.blocks):
            if r in RAMPS:
                for s, w in enumerate(matrices(variant, 1 if r == 2 else 2)):
                    mix.ramp_matrix(s, w, RAMPS[r])
            k = src.run(feeds[r].dev, s_in, max(blk.counts), d_a.dev, s_a, blk.counts)
            mix.run(d_a.dev, s_a, int(k.max()), d_b.dev, s_b, k)
            kb = bus.run(d_b.dev, s_b, int(k.max()), d_c.dev, s_c, k)
            lim.run(d_c.dev, s_c, int(kb.max()), d_d.dev, batch.stride, kb)
            batch.run_slots(int(kb.max()), d_d.dev, results[r].dev, kb)
            got_src.append(k.tolist())
            got_bus.append(kb.tolist())
        batch.sync()                                                 # (the only synchronisation)

        # every out_frames the host returned
        assert got_src == [blk.src_counts for blk in case.blocks]
        assert got_bus == [blk.bus_counts for blk in case.blocks]
        # every block's PCM, the sentinel past every count, the ceiling on the device's own output
        _, g = oracle.gain(co, co, GAIN_SCALE, v["gains"])
        pcm = [[] for _ in range(B)]
        for r, blk in enumerate(case.blocks):
            for b in range(B):
                want = oracle.gain_apply(g, blk.outs[b].reshape(-1), co)
                have = results[r].array[b, :want.size]
                bad = np.flatnonzero(have != want)
                assert bad.size == 0, ("block", r, "bus", b, "first mismatch (frame, channel)", divmod(int(bad[0]), co),
                                       "got", int(have[bad[0]]), "want", int(want[bad[0]]), "of", want.size // co)
                assert (results[r].array[b, want.size:] == SENTINEL).all(), ("block", r, "bus", b, "written past its count")
                assert np.abs(have.astype(np.int64)).max(initial=0) <= T_lim, ("block", r, "bus", b, "above the ceiling")
                pcm[b].append(want)
        # the state at the end: ramps, the gain-reduction meter
        for s, m in enumerate(case.model.ramp):
            done, total, w = mix.ramp_state(s)
            assert (done, total) == m.state()[:2] and np.array_equal(w, m.state()[2]), ("ramp state", s)
        assert lim.min_gain().tolist() == case.model.lim.gmin
        # the meters over the whole programme
        vu, vu_rc = batch.vu_results()
        tp, tp_rc = batch.tp_results()
        ld, ld_rc = batch.loud_results()
        for b in range(B):
            y = np.concatenate(pcm[b])
            w = oracle.vu_new(co)
            oracle.vu_accumulate(w, y)
            _, want = oracle.vu_result(w)
            assert vu_rc[b] == 0 and oracle_ffi.vu_result_dict(want) == vu[b].as_dict(), ("VU", b)
            assert abs(vu[b].global_peak) <= T_lim
            m = TTP.Model(co)
            m.run(y)
            peaks, frames = m.take()
            assert tp_rc[b] == 0
            TTP._check_result(tp[b], peaks, frames, co, "chain bus %d" % b)
            m = TLD.Model(co, RATE_OUT)
            m.run(y)
            assert ld_rc[b] == 0
            TLD._check_result(ld[b], m, "chain bus %d" % b)
    finally:                                 # (the four that borrow the batch's stream go before the batch, whatever the outcome)
        for o in reversed(objects):
            o.close()
        for o in arrays:
            o.free()


# ---------------------------------------------------------------------------
# 2. frames_per_stream is free on return

CS, CF = 8, 4096                                  # the object under test: 8 streams of at most 4096 frames
X = [100 + s for s in range(CS)]                  # run 1's counts
Y = [CF - s for s in range(CS)]                   # run 2's: both valid for either run, whichever the device sees
Z = [37 + 5 * s for s in range(CS)]               # run 3's, after the sync: the state the first two left is the model's
# The backlog: uniform runs of a batch of 1024 stereo streams x 65536 frames on the same stream.  README gives 0.33 ms
# for the 4096-stream form of this run (2 x 2.1 GB of traffic), so about 0.08 ms each here: 128 of them keep the stream
# busy for some 10 ms, several times what the host needs to queue them and the two runs behind them (about 1 ms).
BACKLOG_STREAMS, BACKLOG_FRAMES, BACKLOG_RUNS = 1024, 65536, 128
HIP_ERROR_NOT_READY = 600


class _Under:
    """an object under test between one input array and output arrays, all pinned and device-mapped, and its model"""
    out_slots = CS

    def outs(self, cm):
        return [_mapped(cm, self.out_slots, self.s_out) for _ in range(3)]

    def extra(self, runs):
        pass

    def close(self):
        self.o.close()
        self.src.free()

    def fill(self, cm, ci):
        self.s_in = (CF * ci + 7) // 8 * 8
        self.src = _mapped(cm, CS, self.s_in)
        self.x = [TS.noise(600 + s, CF, ci) for s in range(CS)]
        for s in range(CS):
            self.src.array[s, :CF * ci] = self.x[s].reshape(-1)


class _UnderBatch(_Under):
    def __init__(self, cm, oracle, st):
        self.o = cm.Batch(CS, 2, CF, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, hip_stream=st)
        assert self.o.set_gain(-1, 2, 1000, [750, 1250]) == 0
        self.fill(cm, 2)
        assert self.o.stride == self.s_in
        self.s_out, self.co = self.s_in, 2
        _, self.g = oracle.gain(2, 2, 1000, [750, 1250])
        self.oracle = oracle

    def run(self, counts, out):
        self.o.run_slots(CF, self.src.dev, out.dev, counts)

    def model(self, counts):
        return [self.oracle.gain_apply(self.g, self.x[s][:n].reshape(-1), 2).reshape(-1, 2) for s, n in enumerate(counts)]

    def extra(self, runs):
        res, rcs = self.o.vu_results()               # the windows counted what the device saw
        assert [r.frames for r in res] == [sum(c[s] for c in runs) for s in range(CS)]


class _UnderSrc(_Under):
    def __init__(self, cm, oracle, st):
        L, M, T, H = TS.table(cm, RATE_IN, RATE_OUT)
        self.o = cm.Resampler(CS, 2, RATE_IN, RATE_OUT, CF, hip_stream=st)
        self.fill(cm, 2)
        self.s_out, self.co = _stride(self.o.max_out_frames(), 2), 2
        self.models = [TS.Model(L, M, H, 2) for _ in range(CS)]
        self.got = []

    def run(self, counts, out):
        self.got.append(self.o.run(self.src.dev, self.s_in, CF, out.dev, self.s_out, counts).tolist())

    def model(self, counts):
        return [m.run(self.x[s][:n]) for s, (m, n) in enumerate(zip(self.models, counts))]

    def extra(self, runs):
        L, M = self.models[0].L, self.models[0].M
        want, r = [], [0] * CS
        for counts in runs:
            want.append([-(-(r[s] + n) * L // M) - -(-r[s] * L // M) for s, n in enumerate(counts)])
            r = [(r[s] + n) % M for s, n in enumerate(counts)]
        assert self.got == want, "out_frames"


class _UnderMix(_Under):
    def __init__(self, cm, oracle, st):
        self.o = cm.Mixer(CS, 2, 2, CF, hip_stream=st)
        self.fill(cm, 2)
        self.s_out, self.co = _stride(CF, 2), 2
        w0 = [TR.dense_matrix(2, 2, 700 + s) for s in range(CS)]
        for s, w in enumerate(w0):
            self.o.set_matrix(s, w)
        self.models = [TR.RampModel(w) for w in w0]
        for s in range(CS):                          # every stream inside a ramp over all three runs
            w1 = TR.dense_matrix(2, 2, 800 + s)
            self.o.ramp_matrix(s, w1, 20000)
            self.models[s].ramp(w1, 20000)

    def run(self, counts, out):
        self.o.run(self.src.dev, self.s_in, CF, out.dev, self.s_out, counts)

    def model(self, counts):
        return [m.run(self.x[s][:n]) for s, (m, n) in enumerate(zip(self.models, counts))]

    def extra(self, runs):
        for s in range(CS):
            done, total, _ = self.o.ramp_state(s)
            assert (done, total) == (sum(c[s] for c in runs), 20000), ("ramp state", s)


class _UnderLim(_Under):
    def __init__(self, cm, oracle, st):
        self.o = cm.Limiter(CS, 2, LOOKAHEAD_LOG2, HOLD, CF, threshold=12000, drive=4096, hip_stream=st)
        self.fill(cm, 2)
        self.s_out, self.co = _stride(CF, 2), 2
        self.m = TL.Model(CS, 2, LOOKAHEAD_LOG2, HOLD)
        self.m.set(-1, 12000, 4096)

    def run(self, counts, out):
        self.o.run(self.src.dev, self.s_in, CF, out.dev, self.s_out, counts)

    def model(self, counts):
        return self.m.run([self.x[s][:n] for s, n in enumerate(counts)])

    def extra(self, runs):
        assert self.o.min_gain().tolist() == self.m.gmin


class _UnderBus(_Under):
    """the control: cmhip_bus_run has always copied its counts"""
    out_slots = 2

    def __init__(self, cm, oracle, st):
        self.o = cm.Bus(CS, 2, 2, 2, CF, CS, hip_stream=st)
        self.fill(cm, 2)
        self.s_out, self.co = _stride(CF, 2), 2
        self.table = ([s % 2 for s in range(CS)], list(range(CS)), TB.dense_sends(2, 2, CS, CS // 2, 900))
        self.o.set_routing(*self.table)
        self.got = []

    def run(self, counts, out):
        self.got.append(self.o.run(self.src.dev, self.s_in, CF, out.dev, self.s_out, counts).tolist())

    def model(self, counts):
        return TB.model_bus([self.x[s][:n] for s, n in enumerate(counts)], self.table, 2, 2)

    def extra(self, runs):
        assert self.got == [[max(c[s] for s in range(b, CS, 2)) for b in range(2)] for c in runs], "out_frames"


UNDER = {"batch": _UnderBatch, "src": _UnderSrc, "mix": _UnderMix, "lim": _UnderLim, "bus": _UnderBus}


@pytest.fixture(scope="module")
def backlog(gpu):
    big = gpu.Batch(BACKLOG_STREAMS, 2, BACKLOG_FRAMES, flags=gpu.OUT_PCM | gpu.VU)
    # hipStreamQuery of the runtime the ENGINE is linked to, looked up through the engine's own handle: a process may
    # hold a second HIP runtime (torch brings a copy of its own), and that one knows nothing of the engine's streams --
    # its first call initialises it for tens of milliseconds and answers hipErrorNoDevice
    query = gpu.lib.hipStreamQuery
    query.argtypes = [C.c_void_p]
    query.restype = C.c_int
    yield big, query
    big.close()


@pytest.mark.parametrize("kind", list(UNDER))
def test_counts_are_free_on_return(gpu, oracle, backlog, kind):
    """Before the objects copied their counts (CountsRing, csrc/cmhip_internal.h) this failed on an MI355X for batch,
    src, mix and lim alike -- run 1 wrote as many frames as run 2's counts say -- and passed for the bus, which always
    copied; the stream was still busy in every case (queued in 0.5-2.1 ms, drained after 10.7-12.4 ms: 5.8-23.8 x)."""
    cm = gpu
    big, stream_query = backlog
    st = big.hip_stream()
    u = UNDER[kind](cm, oracle, st)
    outs, ptr = [], None
    try:
        assert u.o.hip_stream() == st
        outs += u.outs(cm)
        for o in outs:
            o.array[:] = SENTINEL
        ptr = cm.lib.cmhip_host_alloc(4 * CS)                        # ONE pinned array for the counts of every run
        assert ptr
        counts = np.frombuffer((C.c_uint32 * CS).from_address(ptr), dtype=np.uint32)
        assert np.ascontiguousarray(counts, dtype=np.uint32).ctypes.data == ptr      # (the mirror passes it on as it is)
        big.sync()
        t0 = time.perf_counter()
        for _ in range(BACKLOG_RUNS):
            big.run(BACKLOG_FRAMES)
        counts[:] = X
        u.run(counts, outs[0])
        counts[:] = Y
        u.run(counts, outs[1])
        state = stream_query(st)
        t1 = time.perf_counter()
        big.sync()
        t2 = time.perf_counter()
        print("counts %s: queued in %.2f ms, the stream drained after %.2f ms: margin %.1f x, hipStreamQuery %d"
              % (kind, 1e3 * (t1 - t0), 1e3 * (t2 - t0), (t2 - t0) / (t1 - t0), state))
        # the proof that run 1's copy had not executed when the array changed; without it the test proves nothing
        assert state == HIP_ERROR_NOT_READY, "set-up failure: the backlog had drained before run 2 was queued (%d)" % state
        counts[:] = Z
        u.run(counts, outs[2])
        big.sync()
        for i, c in enumerate((X, Y, Z)):
            wants = u.model(c)
            for s, want in enumerate(wants):
                have = outs[i].array[s, :want.size].reshape(-1, u.co)
                bad = np.argwhere(have != want.reshape(-1, u.co))
                assert bad.size == 0, ("run", i + 1, "slot", s, "first mismatch (frame, channel)", bad[0].tolist(), "of",
                                       want.size // u.co, "frames")
                assert (outs[i].array[s, want.size:] == SENTINEL).all(), ("run", i + 1, "slot", s, "written past its count")
        u.extra([X, Y, Z])
    finally:                                 # (before the backlog's stream goes, whatever the outcome)
        u.close()
        for o in outs:
            o.free()
        if ptr:
            cm.lib.cmhip_host_free(ptr)
