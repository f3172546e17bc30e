"""GPU: the mix bus (cmhip_bus_*, csrc/k_bus.hip) against a numpy model in int64 of the arithmetic include/coolmic_hip.h
states, bit for bit: both kernel forms over dense per-send matrices with 1 .. 64 sends per bus and streams of mixed
lengths, buses of several int32 groups, the literal values of the one rounding after the sum, a single send against
cmhip_mix_run on the device, vector and tile edges of a short send under a long one, 300 buses of mix-minus, the order
of set_routing with the runs, refusals that launch nothing, bus -> batch on one stream, and the C example.  Input slots
hold a poison value past every count; output slots are pre-filled with a sentinel that must survive past every bus's
count.  (tests/test_bus_host.py takes the model and the tables from here.)"""
import functools
import importlib.util
import math
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
SENTINEL = -21555                                 # what the output slots hold before a run
POISON = 0x5a5a                                   # what the input slots hold past a stream's count
SATURATED_MAX = 0.25              # of a dense case's outputs in the MODEL: a saturated output hides a wrong sum


def _mix_tests():
    spec = importlib.util.spec_from_file_location("test_gpu_mix_for_bus", os.path.join(ROOT, "tests", "test_gpu_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TM = _mix_tests()                  # the full-scale noise, the mixer's model and its dense matrices
noise = TM.noise


def model_bus(xs, table, buses, co):
    """xs: per stream int16 [F_s][C_in]; table: (bus [n], stream [n], W [n][C_out][C_in]) -> per bus int16 [F_b][C_out]:
    p_j exact, acc = sum of the bus's p_j in int64, ONE rounding: sat16((acc + 8192) >> 14); F_b the largest count among
    the bus's sends' streams (0 without sends); a shorter send is silent past its own count"""
    bus, stream, W = table
    if len(bus) == 0:
        return [np.zeros((0, co), dtype=np.int16) for _ in range(buses)]
    W = np.asarray(W, dtype=np.int64).reshape(len(bus), co, -1)
    xs = [np.asarray(x, dtype=np.int64).reshape(-1, W.shape[2]) for x in xs]
    outs = []
    for b in range(buses):
        js = [j for j in range(len(bus)) if bus[j] == b]
        F = max([xs[stream[j]].shape[0] for j in js], default=0)
        acc = np.zeros((F, co), dtype=np.int64)
        for j in js:
            p = xs[stream[j]] @ W[j].T
            assert p.size == 0 or np.abs(p).max() < 2 ** 31
            acc[:p.shape[0]] += p
        outs.append(np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16))
    return outs


def saturated(y):
    return int(((y == 32767) | (y == -32768)).sum())


def dense_sends(ci, co, n, k, seed):
    """n matrices for buses of k sends: every |w| in [3B/4, B], B = min(65535 // C_in, 8192, floor(16384 /
    sqrt(k * C_in))), random signs -- no entry a kernel could skip unnoticed, and a sum that mostly stays in int16"""
    B = min(65535 // ci, 8192, int(math.floor(16384 / math.sqrt(k * ci))))
    rng = np.random.default_rng(seed)
    w = rng.integers(3 * B // 4, B + 1, size=(n, co, ci)) * rng.choice([-1, 1], size=(n, co, ci))
    assert np.abs(w).sum(axis=2).max() <= 65535
    return w.astype(np.int16)


def heavy_sends(ci, co, n, seed):
    """n matrices whose every row has sum |w| in (32768, 65535] (mono: |w| = 32767): no two of them share an int32
    group (mono: no three)"""
    rng = np.random.default_rng(seed)
    if ci == 1:
        mag = np.full((n, co, ci), 32767)
    else:
        mag = rng.integers(-(-32769 // ci), 65535 // ci + 1, size=(n, co, ci))
        assert (mag.sum(axis=2) > 32768).all() and (mag.sum(axis=2) <= 65535).all()
    return (mag * rng.choice([-1, 1], size=(n, co, ci))).astype(np.int16)


class Rig:
    """a bus object between two arrays of pinned, device-mapped host memory"""

    def __init__(self, cm, streams, buses, ci, co, max_frames, max_sends):
        self.cm, self.S, self.B, self.CI, self.CO = cm, streams, buses, ci, co
        self.m = cm.Bus(streams, buses, ci, co, max_frames, max_sends)
        self.in_stride = (max_frames * ci + 7) // 8 * 8
        self.out_stride = (max_frames * co + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=buses, stride=self.out_stride))
        self.table = ([], [], np.zeros((0, co, ci), dtype=np.int16))

    def set(self, bus, stream, W):
        self.m.set_routing(bus, stream, W)
        self.table = (list(bus), list(stream), np.asarray(W, dtype=np.int16).reshape(-1, self.CO, self.CI))
        got = self.m.get_routing()
        assert self.m.sends() == len(bus) and got[0].tolist() == list(bus) and got[1].tolist() == list(stream)
        assert np.array_equal(got[2], self.table[2])

    def close(self):
        self.m.close()
        self.src.free()
        self.dst.free()

    def fill(self, xs):
        counts = [np.asarray(x).reshape(-1, self.CI).shape[0] for x in xs]
        self.src.array[:] = POISON
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.CI] = np.asarray(x, dtype=np.int16).reshape(-1)
        return counts

    def run(self, xs, frames=None, uniform=False, wants=None):
        """xs: per stream int16 [F_s][C_in]; runs the device and the model, compares outputs, counts and the untouched
        rest; -> the model's outputs"""
        counts = self.fill(xs)
        frames = max(counts) if frames is None else frames
        assert not uniform or all(n == frames for n in counts)
        self.dst.array[:] = SENTINEL
        got = self.m.run(self.src.dev, self.in_stride, frames, self.dst.dev, self.out_stride, None if uniform else counts)
        self.m.sync()
        wants = model_bus(xs, self.table, self.B, self.CO) if wants is None else wants
        assert got.tolist() == [w.shape[0] for w in wants], "out_frames"
        self.check(self.dst.array, wants)
        return wants

    def check(self, array, wants):
        for b, want in enumerate(wants):
            n = want.size
            have = array[b, :n].reshape(-1, self.CO)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("bus", b, "first mismatch (frame, channel)", bad[0].tolist(),
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (array[b, n:] == SENTINEL).all(), ("bus", b, "written past its count")


# ---------------------------------------------------------------------------
# 1. both forms: dense matrices per send, K sends per bus, long and short streams in every bus

PAIRS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (6, 2), (5, 3), (16, 16)]
FAST = {(1, 1), (1, 2), (2, 1), (2, 2)}
KS = [1, 2, 3, 17, 64]
STREAMS, BUSES = 10, 6


def forms_counts(t):
    """two streams per count of {2t + 13, t, t - 1, 1, 0}: stream s has count class s // 2"""
    return [c for c in (2 * t + 13, t, t - 1, 1, 0) for _ in range(2)]


def forms_table(k):
    """bus b < 4: k sends whose streams' count classes cycle through b .. 4 (long and short ones mixed; the bus's own
    count is that of class b), streams repeating once k passes what there is; bus 4: k sends of count-0 streams only;
    bus 5: no sends.  The sends are given interleaved over the buses, not sorted."""
    bus, stream = [], []
    for i in range(k):
        for b in range(5):
            cls = b + i % (5 - b)
            bus.append(b)
            stream.append(2 * cls + (i // (5 - b)) % 2)
    return bus, stream


@functools.lru_cache(maxsize=None)
def forms_case(ci, co, t, k, heavy=False):
    """the table, full-length inputs and the model's outputs of the ragged and of the uniform run, and the share of
    saturated outputs -- computed once, never changed"""
    frames = 2 * t + 13
    bus, stream = forms_table(k)
    seed = 100000 * ci + 1000 * co + k
    W = heavy_sends(ci, co, len(bus), seed) if heavy else dense_sends(ci, co, len(bus), k, seed)
    xs = [noise(200 * ci + co + 7 * s, frames, ci) for s in range(STREAMS)]
    if heavy:
        xs = [x >> 4 for x in xs]
    table = (bus, stream, W)
    ragged = model_bus([x[:n] for x, n in zip(xs, forms_counts(t))], table, BUSES, co)
    full = model_bus(xs, table, BUSES, co)
    outs = sum(y.size for y in full + ragged)
    share = sum(saturated(y) for y in full + ragged) / outs
    return table, xs, full, ragged, share


def run_forms(cm, ci, co, k, heavy):
    plan = cm.plan_bus(BUSES, ci, co, 1)
    assert plan.fast == (1 if (ci, co) in FAST else 0)
    t = plan.tile_frames
    table, xs, full, ragged, share = forms_case(ci, co, t, k, heavy)
    counts = forms_counts(t)
    assert [w.shape[0] for w in ragged] == [counts[0], counts[2], counts[4], counts[6], 0, 0]
    assert [w.shape[0] for w in full] == [counts[0]] * 5 + [0]
    rig = Rig(cm, STREAMS, BUSES, ci, co, counts[0], len(table[0]))
    rig.set(*table)
    rig.run([x[:n] for x, n in zip(xs, counts)], wants=ragged)
    rig.run(xs, uniform=True, wants=full)                        # a second run on the same object: there is no state
    rig.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ci,co", PAIRS)
def test_forms(gpu, ci, co, k):
    t = gpu.plan_bus(BUSES, ci, co, 1).tile_frames
    share = forms_case(ci, co, t, k)[4]
    print("bus forms %2d -> %2d, %2d sends per bus: tile_frames %d, saturated outputs in the model %.2f %%"
          % (ci, co, k, t, 100 * share))
    assert share < SATURATED_MAX
    run_forms(gpu, ci, co, k, False)


@pytest.mark.parametrize("ci,co", PAIRS)
def test_heavy_groups(gpu, ci, co):
    """every send (mono: every second one) starts a new int32 group: the int64 path of the fast forms"""
    cm = gpu
    t = cm.plan_bus(BUSES, ci, co, 1).tile_frames
    table, _, full, ragged, share = forms_case(ci, co, t, 5, True)
    _, _, flag, _ = cm.bus_compile(BUSES, STREAMS, ci, co, *table)
    assert flag.sum() == (15 if ci == 1 else 25)                 # five buses of five sends
    peak = max(int(np.abs(y.astype(np.int64)).max()) for y in full + ragged if y.size)
    print("bus heavy groups %2d -> %2d: largest |y| in the model %d" % (ci, co, peak))
    assert share == 0 and peak < 32767                           # the model saturates nowhere
    run_forms(cm, ci, co, 5, True)


# ---------------------------------------------------------------------------
# 2. literal values, one frame each

LITERALS = [
    # C_in, per send (x, W row), expected: what a broken version gives
    (2, [((32767, 32767), (32767, 32767))] * 2, 32767),          # an int32 sum wraps to -262140 -> -16
    (2, [((-32768, -32768), (32767, 32767))] * 2, -32768),       # the wrap gives +8
    (1, [((30000,), (16384,)), ((30000,), (16384,)), ((-30000,), (16384,))], 30000),     # per-send saturation breaks it
    (1, [((1,), (4096,))] * 2, 1),                               # rounding each send gives 0
    (1, [((-1,), (4096,)), ((-1,), (4096,)), ((-1,), (1,))], -1),
    (1, [((-1,), (4096,))] * 2, 0),
]


def test_literal_values(gpu):
    cm = gpu
    for ci, sends, want in LITERALS:
        rig = Rig(cm, len(sends), 1, ci, 1, 8, len(sends))
        rig.set([0] * len(sends), list(range(len(sends))), [[w] for _, w in sends])
        got = rig.run([np.array([x], dtype=np.int16) for x, _ in sends])
        assert got[0].tolist() == [[want]], (sends, got[0].tolist())
        rig.close()


# ---------------------------------------------------------------------------
# 3. one send per bus equals cmhip_mix_run on the same data, device against device

@pytest.mark.parametrize("ci,co", PAIRS)
def test_single_send_equals_the_mixer(gpu, ci, co):
    cm = gpu
    t = cm.plan_bus(3, ci, co, 1).tile_frames
    counts = [t + 5, t, 3]
    W = [TM.dense_matrix(ci, co, 7000 + 10 * ci + co + s) for s in range(3)]
    xs = [noise(7100 + ci + s, n, ci) for s, n in enumerate(counts)]
    rig = Rig(cm, 3, 3, ci, co, counts[0], 3)
    rig.set([2, 0, 1], [2, 0, 1], [W[2], W[0], W[1]])
    rig.fill(xs)
    mixer = cm.Mixer(3, ci, co, counts[0])
    for s in range(3):
        mixer.set_matrix(s, W[s])
    ref = cm.MappedPcm(types.SimpleNamespace(streams=3, stride=rig.out_stride))
    ref.array[:] = SENTINEL
    rig.dst.array[:] = SENTINEL
    mixer.run(rig.src.dev, rig.in_stride, counts[0], ref.dev, rig.out_stride, counts)
    mixer.sync()
    assert rig.m.run(rig.src.dev, rig.in_stride, counts[0], rig.dst.dev, rig.out_stride, counts).tolist() == counts
    rig.m.sync()
    assert np.array_equal(rig.dst.array, ref.array)
    rig.check(rig.dst.array, [TM.model_mix(x, w) for x, w in zip(xs, W)])
    if ci == co:                                                 # identity returns the input
        eye = 16384 * np.eye(ci, dtype=np.int16)
        rig.set([0, 1, 2], [0, 1, 2], [eye] * 3)
        rig.run(xs, wants=xs)
    mixer.close()
    ref.free()
    rig.close()


# ---------------------------------------------------------------------------
# 4. vector and tile edges: one short stream per count, each under one full-length send

@pytest.mark.parametrize("ci,co", sorted(FAST) + [(3, 2), (6, 2)])
def test_vector_and_tile_edges(gpu, ci, co):
    cm = gpu
    t = cm.plan_bus(1, ci, co, 1).tile_frames
    counts = list(range(0, 10)) + list(range(t - 8, t + 9))
    n = len(counts)
    full = t + 24
    W = dense_sends(ci, co, 2 * n, 2, 50 * ci + co)
    xs = [noise(3000 + 31 * ci + co + s, c, ci) for s, c in enumerate(counts)] + [noise(2999, full, ci)]
    bus = [b for b in range(n) for _ in range(2)]
    stream = [s for b in range(n) for s in (b, n)]               # the short stream first, then the long one
    rig = Rig(cm, n + 1, n, ci, co, full, 2 * n)
    rig.set(bus, stream, W)
    wants = rig.run(xs)
    assert all(w.shape[0] == full for w in wants)
    assert sum(saturated(y) for y in wants) < SATURATED_MAX * sum(y.size for y in wants)
    # the short send's zero-fill is visible: with the short sends alone the head of every bus differs
    alone = model_bus(xs, (bus[1::2], stream[1::2], W[1::2]), n, co)
    assert all(not np.array_equal(a[:c], w[:c]) for a, w, c in zip(alone, wants, counts) if c > 1)
    assert all(np.array_equal(a[c:], w[c:]) for a, w, c in zip(alone, wants, counts))
    rig.close()


# ---------------------------------------------------------------------------
# 5. sharing: mix-minus over 300 participants, one stream twice in one bus

def test_mix_minus_300(gpu):
    cm = gpu
    n = 300
    bus, stream, W = cm.bus_mix_minus(n, 1638)
    assert len(bus) == n * (n - 1) and not (bus == stream).any()
    bus, stream = bus.tolist() + [7], stream.tolist() + [5]      # stream 5 a second time in bus 7: the weights add
    W = np.concatenate([W, np.array([[[-3000]]], dtype=np.int16)])
    counts = [36 + s % 65 for s in range(n)]
    xs = [noise(5000 + s, c, 1) >> 6 for s, c in enumerate(counts)]
    # the model as one matrix product: M[b][s] the summed weight of stream s in bus b
    M = np.zeros((n, n), dtype=np.int64)
    np.add.at(M, (bus, stream), W.reshape(-1).astype(np.int64))
    X = np.zeros((n, 100), dtype=np.int64)
    for s, x in enumerate(xs):
        X[s, :counts[s]] = x.reshape(-1)
    Y = np.clip((M @ X + 8192) >> 14, -32768, 32767).astype(np.int16)
    wants = [Y[b, :max(c for s, c in enumerate(counts) if s != b), None] for b in range(n)]
    assert M[7, 5] == 1638 - 3000 and sum(saturated(y) for y in wants) == 0
    _, _, flag, _ = cm.bus_compile(n, n, 1, 1, bus, stream, W)
    assert flag.sum() > 7 * n                                    # 40 sends of 1638 to a group
    rig = Rig(cm, n, n, 1, 1, 100, len(bus))
    rig.set(bus, stream, W)
    rig.run(xs, wants=wants)
    rig.close()


# ---------------------------------------------------------------------------
# 6. set_routing is ordered with the runs by the stream alone

def test_ordering_of_set_routing(gpu):
    cm = gpu
    S, B, F = 4, 2, 3000
    xs = [noise(6000 + s, F - 7 * s, 2) for s in range(S)]
    tables = [([0, 1, 0], [0, 1, 2], dense_sends(2, 1, 3, 2, 61)), ([1, 0, 1, 1], [3, 1, 0, 2], dense_sends(2, 1, 4, 3, 62))]
    rig = Rig(cm, S, B, 2, 1, F, 8)
    counts = rig.fill(xs)
    second = cm.MappedPcm(types.SimpleNamespace(streams=B, stride=rig.out_stride))
    outs = [rig.dst, second]
    got = []
    for (bus, stream, W), dst in zip(tables, outs):
        dst.array[:] = SENTINEL
        b, s, w = np.array(bus, dtype=np.uint32), np.array(stream, dtype=np.uint32), W.copy()
        assert cm.lib.cmhip_bus_set_routing(rig.m.h, len(bus), b.ctypes.data, s.ctypes.data, w.ctypes.data) == 0
        b[:], s[:], w[:] = 0xffffffff, 0xffffffff, 32767         # the caller's arrays are free on return
        got.append(rig.m.run(rig.src.dev, rig.in_stride, F, dst.dev, rig.out_stride, counts))
    rig.m.sync()                                                 # (the only synchronisation)
    for table, dst, n in zip(tables, outs, got):
        wants = model_bus(xs, table, B, 1)
        assert n.tolist() == [w.shape[0] for w in wants]
        rig.check(dst.array, wants)
    assert not np.array_equal(outs[0].array, outs[1].array)
    second.free()
    rig.close()


# ---------------------------------------------------------------------------
# 7. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    rig = Rig(cm, 3, 2, 2, 1, 256, 4)
    rig.set([0, 1, 1], [0, 1, 2], dense_sends(2, 1, 3, 2, 71))
    m, src, dst, si, so = rig.m, rig.src.dev, rig.dst.dev, rig.in_stride, rig.out_stride
    assert (si, so) == (512, 264)
    rig.dst.array[:] = SENTINEL
    rig.src.array[:] = SENTINEL
    cases = {
        "misaligned in": (src + 2, si, 256, dst, so, None),
        "misaligned out": (src, si, 256, dst + 8, so, None),
        "in stride not a multiple of 8": (src, si + 4, 256, dst, so, None),
        "out stride not a multiple of 8": (src, si, 256, dst, so - 4, None),
        "in stride too small": (src, 504, 256, dst, so, None),
        "out stride too small": (src, si, 256, dst, 248, None),
        "frames above max_frames": (src, si, 257, dst, so, None),
        "a count above frames": (src, si, 100, dst, so, [100, 100, 101]),
        "in == out": (src, si, 256, src, so, None),
        "out inside in": (src, si, 256, src + 16, so, None),
        "out begins in the last slot of in": (src, si, 256, src + 2 * (2 * si + 256), so, None),
        "in begins inside out": (dst + 2 * so, si, 256, dst, so, None),
    }
    frames = np.full(2, 77, dtype=np.uint32)
    for name, (a, ast, n, o, ost, fps) in cases.items():
        assert m.run_rc(a, ast, n, o, ost, fps, frames) == cm.ERROR_INVAL, name
    assert cm.lib.cmhip_bus_run(m.h, None, si, 256, None, dst, so, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_bus_run(m.h, src, si, 256, None, None, so, None) == cm.ERROR_FAULT
    assert frames.tolist() == [77, 77]
    # tables: refused ones change nothing
    before = m.get_routing()
    w = dense_sends(2, 1, 5, 2, 72)
    assert m.set_routing_rc([0] * 5, [0] * 5, w) == cm.ERROR_INVAL                       # above max_sends
    assert m.set_routing_rc([0, 2], [0, 1], w[:2]) == cm.ERROR_INVAL                     # a bus out of range
    assert m.set_routing_rc([0, 1], [0, 3], w[:2]) == cm.ERROR_INVAL                     # a stream out of range
    assert m.set_routing_rc([0], [0], [[[-32768, -32768]]]) == cm.ERROR_INVAL            # a row of 65536
    assert cm.lib.cmhip_bus_set_routing(m.h, 1, None, None, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_bus_set_routing(None, 0, None, None, None) == cm.ERROR_FAULT
    after = m.get_routing()
    assert m.sends() == 3 and all(np.array_equal(x, y) for x, y in zip(before, after))
    assert cm.lib.cmhip_bus_get_routing(m.h, 2, before[0].ctypes.data, before[1].ctypes.data,
                                        before[2].ctypes.data) == cm.ERROR_INVAL
    m.sync()
    assert (rig.dst.array == SENTINEL).all() and (rig.src.array == SENTINEL).all()
    rig.run([noise(700 + s, 256 - s, 2) for s in range(3)])      # and the old routing is still in force
    rig.set([], [], np.zeros((0, 1, 2), dtype=np.int16))         # n == 0 empties it: every bus has count 0
    assert [w.size for w in rig.run([noise(710 + s, 256, 2) for s in range(3)])] == [0, 0]
    rig.close()


# ---------------------------------------------------------------------------
# 8. composition: bus -> the slots of a batch, both on the batch's stream

def test_chain_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    cm = gpu
    S, B, F = 5, 3, 3000
    fps = [F, F - 1, 1234, 7, 0]
    xs = [noise(800 + s, fps[s], 2) for s in range(S)]
    table = ([0, 0, 1, 2, 2, 2, 1], [0, 2, 3, 1, 2, 4, 4], dense_sends(2, 1, 7, 3, 81))
    want = model_bus(xs, table, B, 1)
    src_b = cm.Batch(S, 2, F, flags=cm.VU, rate=48000)           # (device memory for the sources)
    for s in range(S):
        if fps[s]:
            src_b.upload(s, xs[s])
    src_b.sync()
    b = cm.Batch(B, 1, F, flags=cm.OUT_PCM | cm.VU, rate=48000)
    assert b.set_gain(-1, 1, 1000, [1250]) == 0
    m = cm.Bus(S, B, 2, 1, F, 16, hip_stream=b.hip_stream())
    assert m.hip_stream() == b.hip_stream()
    m.set_routing(*table)
    counts = m.run(src_b.dev_in, src_b.stride, F, b.dev_in, b.stride, fps)
    assert counts.tolist() == [F, 7, F - 1] == [w.shape[0] for w in want]
    b.run(int(counts.max()), counts)                             # (no sync between the two: the order is the stream's)
    res, rcs = b.vu_results()
    _, g = oracle.gain(1, 1, 1000, [1250])
    for s, y in enumerate(want):
        pcm = oracle.gain_apply(g, y.reshape(-1), 1)
        v = oracle.vu_new(1)
        oracle.vu_accumulate(v, pcm)
        _, vr = oracle.vu_result(v)
        assert rcs[s] == 0 and oracle_ffi.vu_result_dict(vr) == res[s].as_dict(), s
        assert res[s].frames == counts[s]
        assert np.array_equal(b.download(s, int(counts[s])), pcm), s
    m.close()
    b.close()
    src_b.close()


# ---------------------------------------------------------------------------
# 9. the example

def test_batch_conference_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_conference"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_conference.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("mix-minus: 8 participants, 56 sends, w = 2340")
    assert len(out) == 9 and all(ln.startswith("participant ") for ln in out[1:])
    for ln in out[1:]:
        f = dict(kv.split("=") for kv in ln.split()[2:])
        assert int(f["frames"]) == 24000 and int(f["rate"]) == 48000 and int(f["channels"]) == 1
        # seven full-scale sines in phase at 1/7 each come out as the same sine: -3 dB
        assert -3.2 < float(f["power"]) < -2.8 and 32000 < abs(int(f["peak"])) <= 32767
