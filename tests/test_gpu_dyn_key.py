"""GPU: side-chain keys of the dynamics stage (cmhip_dyn_set_key, csrc/k_dyn.hip) against the keyed model -- the model
of tests/test_gpu_dyn.py with e taken from (the key's history, the key's input) and everything else from the stream's
own -- bit for bit, the sentinel past every count and the meter included: dense cases over five geometries and both
kernel forms with a key map of every kind, cuts queued without a synchronisation, keys in order with the runs, the
unkeyed identity, resets, literal edges, refusals that change nothing, the chain bus -> keyed dynamics -> bus ->
limiter -> batch, and the C example.  (tests/test_dyn_key_host.py takes the keyed model and the dense cases from here.)"""
import ctypes
import functools
import importlib.util
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")


def _load(name):
    spec = importlib.util.spec_from_file_location("dynkey_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _load("test_gpu_dyn")                        # the unkeyed model, the signal, the dense curve, the rig
geometry, signal, design, DENSE_CURVE, dense_seed = TG.geometry, TG.signal, TG.design, TG.DENSE_CURVE, TG.dense_seed
SETS, SENTINEL, UNITY = TG.SETS, TG.SENTINEL, TG.UNITY
MEAN, RMS = 0, 1                                  # CMHIP_DYN_DETECT_*
DIFFER_SHARE = 0.50                               # of a follower's frames whose output differs from the own detector's


# ---------------------------------------------------------------------------
# the keyed model: include/coolmic_hip.h, "dynamics", "Side-chain keys" and "RMS detector"

def _slide_max(v, n):
    """sliding maxima of n: entry i is max(v[i .. i + n - 1]) (two overlapping power-of-two windows; exact)"""
    m, p = v, 1
    while 2 * p <= n:
        m = np.maximum(m[:-p], m[p:])
        p *= 2
    return np.maximum(m[:m.size - (n - p)], m[n - p:]) if n > p else m


def isqrt(v):
    """int64 [n] in 0..2^52 -> the largest r with r * r <= v (the double root is within 1; integers decide)"""
    v = np.asarray(v, dtype=np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    assert (r * r <= v).all() and ((r + 1) * (r + 1) > v).all()
    return r


def model_dyn_keyed(x, hist, xk, histk, T, a, b, H, detector=MEAN, root=isqrt):
    """model_dyn with the detector on another stream: x, hist the stream's own input and history, xk, histk the key's
    (int16 [F][C], [HIST][C], the same F; the stream's own where it has no key) -> y int16 [F][C], s int64 [F].
    detector: MEAN or RMS ("RMS detector"); root: what takes the root of the mean square, so that a test can show what
    a wrong one would give"""
    A, B, D, W, HIST = geometry(a, b, H)
    F = x.shape[0]
    assert xk.shape[0] == F and histk.shape == hist.shape
    if F == 0:
        return x.copy(), np.zeros(0, np.int64)
    z = np.concatenate([hist, x]).astype(np.int64)
    e = np.abs(np.concatenate([histk, xk]).astype(np.int64)).max(axis=1)     # the only line that knows the key
    # ... and the only one that knows the detector
    L = root(TG._sums(e * e, A) >> a) if detector == RMS else TG._sums(e, A) >> a
    assert detector == RMS or L.max() <= UNITY
    l = _slide_max(L, W)
    g = TG.curve_at(T, np.minimum(l, UNITY))                      # (a root that is one too large may pass 32768)
    s = TG._sums(g, B) >> b
    assert s.size == F and s.max() <= UNITY and s.min() >= 0
    xd = z[HIST - D: HIST - D + F]
    y = (xd * s[:, None] + (1 << 14)) >> 15
    assert (np.abs(y) <= np.abs(xd)).all()
    return y.astype(np.int16), s


class KeyModel(TG.Model):
    """TG.Model with a detector and a key per stream; a run evaluates every stream on the histories as they were before it"""

    def __init__(self, streams, channels, a, b, H, detector=MEAN):
        super().__init__(streams, channels, a, b, H)
        self.key = list(range(streams))
        self.detector = detector

    def set_key(self, stream, key):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.key[s] = s if key < 0 else key

    def run(self, xs):
        xs = [np.asarray(x, dtype=np.int16).reshape(-1, self.C) for x in xs]
        outs = [model_dyn_keyed(x, self.hist[s], xs[self.key[s]], self.hist[self.key[s]], self.curve[s], self.a, self.b,
                                self.H, self.detector) for s, x in enumerate(xs)]
        for s, (x, (y, sg)) in enumerate(zip(xs, outs)):
            self.hist[s] = TG.next_hist(self.hist[s], x)
            if sg.size:
                self.gmin[s] = min(self.gmin[s], int(sg.min()))
                self.s[s].append(sg)
        return [y for y, _ in outs]


class KeyRig(TG.Rig):
    """TG.Rig over the keyed model"""

    def __init__(self, cm, streams, channels, a, b, H, max_frames, curve=None):
        super().__init__(cm, streams, channels, a, b, H, max_frames)
        self.model = KeyModel(streams, channels, a, b, H)
        if curve is not None:
            self.set(-1, curve)

    def set_key(self, stream, key):
        self.m.set_key(stream, key)
        self.model.set_key(stream, key)
        for s in (range(self.S) if stream < 0 else [stream]):
            assert self.m.get_key(s) == (-1 if self.model.key[s] == s else self.model.key[s])

    def set_map(self, keys):
        for s, k in enumerate(keys):
            if k != s:
                self.set_key(s, k)


# ---------------------------------------------------------------------------
# 1. dense cases: five geometries, both forms, a key map of every kind, ragged and uniform counts

CHANNELS = [1, 2, 3, 6, 16]
# a group of seven streams with one count: 0 -> 1 (the key above its follower), 1 -> 2 (a key that is itself keyed),
# 2 on its own detector, 3 -> 2 (the key below its follower), 4 <-> 5 (each other's key), 6 -> 2 (with 1 and 3: three
# streams on one key)
GROUP_KEYS = [1, 2, 2, 2, 5, 4, 2]
GROUP = len(GROUP_KEYS)


def dense_key_map(groups):
    return [GROUP * g + k for g in range(groups) for k in GROUP_KEYS]


@functools.lru_cache(maxsize=None)
def dense_key_case(a, b, H, channels, t):
    """per count of TG.dense_counts a group of GROUP streams: the full-length inputs, the counts, the key map, the curve,
    and over the ragged run followed by the uniform run on one stage: the keyed model's outputs of both, the meter, and
    the figures of the dense conditions -- computed once, never changed"""
    hist = geometry(a, b, H)[4]
    counts = [n for n in TG.dense_counts(t, hist) for _ in range(GROUP)]
    keys = dense_key_map(len(counts) // GROUP)
    xs = [signal(dense_seed(a, b, H, channels, s), counts[0], channels) for s in range(len(counts))]
    T = design(**DENSE_CURVE)
    model = KeyModel(len(counts), channels, a, b, H)
    model.set(-1, T)
    for s, k in enumerate(keys):
        model.set_key(s, k)
    ragged = model.run([x[:n] for x, n in zip(xs, counts)])
    full = model.run(xs)
    # what the own detector would give for the followers of the two long groups, from silence: a kernel that ignores
    # the key gives this
    zero = np.zeros((hist, channels), dtype=np.int16)
    differ = []
    for s in range(2 * GROUP):
        if keys[s] != s:
            own = TG.model_dyn(xs[s][:counts[s]], zero, T, a, b, H)[0]
            differ.append(float((own != ragged[s]).any(axis=1).mean()))
    followers = [s for s in range(len(counts)) if keys[s] != s]
    s_all = [sg for s in followers for sg in model.s[s]]
    change = sum(int((np.diff(sg) != 0).sum()) for sg in s_all) / sum(sg.size - 1 for sg in s_all)
    smallest = min(int(sg.min()) for sg in s_all)
    return xs, counts, keys, T, ragged, full, list(model.gmin), min(differ), change, smallest


def assert_dense_key(differ, change, smallest):
    """held on the MODEL before anything is compared: a kernel that ignores the key cannot pass, and the gain moves"""
    assert differ >= DIFFER_SHARE and change >= TG.CHANGE_SHARE and smallest < TG.MIN_S, (differ, change, smallest)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("a,b,H", SETS)
def test_dense_keyed(gpu, a, b, H, channels):
    cm = gpu
    t = cm.plan_dyn(8, channels, a, b, H, 1).tile_frames
    xs, counts, keys, T, ragged, full, gmin, differ, change, smallest = dense_key_case(a, b, H, channels, t)
    print("dyn keyed dense a %2d b %d H %4d C %2d: tile %d, differing from the own detector %.1f %%, changing %.1f %%, "
          "min s %d" % (a, b, H, channels, t, 100 * differ, 100 * change, smallest))
    assert_dense_key(differ, change, smallest)
    rig = KeyRig(cm, len(counts), channels, a, b, H, counts[0], T)
    rig.set_map(keys)
    got = rig.run([x[:n] for x, n in zip(xs, counts)])
    assert all(np.array_equal(g, w) for g, w in zip(got, ragged))
    got = rig.run(xs, uniform=True)                              # the second run continues every stream, the same map
    assert all(np.array_equal(g, w) for g, w in zip(got, full))
    assert rig.m.min_gain().tolist() == gmin
    rig.close()


# ---------------------------------------------------------------------------
# 2. cuts: one run equals the same streams in many, queued without a synchronisation

CUT_KEYS = [1, 1, 3, 2, 5, 5]                     # 0 -> 1; 2 <-> 3; 4 -> 5, the pair that gets 0 frames in alternate runs


@pytest.mark.parametrize("channels,a,b,H", [(1, 6, 6, 0), (2, 8, 5, 100), (6, 5, 9, 7), (2, 9, 9, 1024)])
def test_cuts_keyed(gpu, channels, a, b, H):
    cm = gpu
    t = cm.plan_dyn(6, channels, a, b, H, 1).tile_frames
    hist = geometry(a, b, H)[4]
    T = design(**DENSE_CURVE)
    S = len(CUT_KEYS)
    x = [signal(9000 + 10 * channels + s, 3 * t, channels) for s in range(S)]
    zero = np.zeros((hist, channels), dtype=np.int16)
    want = [model_dyn_keyed(x[s], zero, x[k], zero, T, a, b, H) for s, k in enumerate(CUT_KEYS)]
    own = [TG.model_dyn(x[s], zero, T, a, b, H)[0] for s in range(S)]
    for s, k in enumerate(CUT_KEYS):
        assert k == s or (want[s][0] != own[s]).any(axis=1).mean() >= DIFFER_SHARE, s
    cuts = [1, 7, hist - 1, hist, hist + 1, 0, t + 5]
    cuts.append(3 * t - sum(cuts))
    assert cuts[-1] > 0
    dyn = cm.Dynamics(S, channels, a, b, H, 3 * t, curve=T)
    for s, k in enumerate(CUT_KEYS):
        dyn.set_key(s, k)
    chunks, pos = [], [0] * S
    for r, n in enumerate(cuts):
        ns = [n] * 4 + [0 if r % 2 else n] * 2
        # at every cut the key's history is not silent and is not the follower's
        for s, k in enumerate(CUT_KEYS):
            if k != s and r > 0:
                hk, hs = x[k][max(pos[k] - hist, 0):pos[k]], x[s][max(pos[s] - hist, 0):pos[s]]
                assert pos[k] == pos[s] and hk.any() and not np.array_equal(hk, hs), (r, s)
        chunks.append([x[s][pos[s]:pos[s] + ns[s]] for s in range(S)])
        pos = [p + m for p, m in zip(pos, ns)]
    outs = TG.run_chunks(cm, dyn, channels, chunks)
    for s in range(S):
        got = np.concatenate([arr[s, :counts[s] * channels].reshape(-1, channels) for arr, counts in outs])
        assert got.shape[0] == pos[s] and np.array_equal(got, want[s][0][:pos[s]]), s
        for arr, counts in outs:
            assert (arr[s, counts[s] * channels:] == SENTINEL).all()
    assert pos[:4] == [3 * t] * 4 and 0 < pos[4] == pos[5] < 3 * t
    assert dyn.min_gain().tolist() == [int(want[s][1][:pos[s]].min()) for s in range(S)]
    dyn.close()


# ---------------------------------------------------------------------------
# 3. keys are ordered with the runs by the stream alone

def test_keys_in_order_with_the_runs(gpu):
    cm = gpu
    S, a, b, H = 300, 4, 3, 5
    counts = [40 + (s // 3) % 65 for s in range(S)]              # a stream and the two after it share a count
    xs = [TG.bursts(1500 + s, n, 2) for s, n in enumerate(counts)]
    T = TG.steps()                                               # every knot another gain: whatever moves the level moves the output
    rig = KeyRig(cm, S, 2, a, b, H, 104, T)
    m, model = rig.m, rig.model
    outs = [rig.dst] + [cm.MappedPcm(types.SimpleNamespace(streams=S, stride=rig.stride)) for _ in range(2)]
    rig.fill(xs)
    for o in outs:
        o.array[:] = SENTINEL
    # no synchronisation anywhere: a run, 100 sets, a run, one set for all, a run
    m.run(rig.src.dev, rig.stride, 104, outs[0].dev, rig.stride, counts)
    assert all(m.get_key(s) == -1 for s in range(S))
    for s in range(0, S, 3):
        m.set_key(s, s + 1)
        assert m.get_key(s) == s + 1 and m.get_key(s + 1) == -1 and m.get_key(s + 2) == -1
    m.run(rig.src.dev, rig.stride, 104, outs[1].dev, rig.stride, counts)
    m.set_key(-1, -1)
    assert all(m.get_key(s) == -1 for s in range(S))
    m.run(rig.src.dev, rig.stride, 104, outs[2].dev, rig.stride, counts)
    m.sync()                                                     # (the only synchronisation)
    first = model.run(xs)
    for s in range(0, S, 3):
        model.set_key(s, s + 1)
    second = model.run(xs)
    model.set_key(-1, -1)
    third = model.run(xs)
    for o, want in zip(outs, (first, second, third)):
        rig.check(o.array, want)
    assert m.min_gain().tolist() == model.gmin
    # the three runs are told apart: with the map of another run the model gives something else
    plain = TG.Model(S, 2, a, b, H)
    plain.set(-1, T)
    plain.run(xs)
    unkeyed_second = plain.run(xs)
    assert sum(not np.array_equal(u, w) for u, w in zip(unkeyed_second, second)) >= 90
    assert all(np.array_equal(u, w) for u, w in zip(plain.run(xs), third))
    for o in outs[1:]:
        o.free()
    rig.close()


# ---------------------------------------------------------------------------
# 4. an object without a key is the parent's object

def test_unkeyed_identity(gpu):
    cm = gpu
    a, b, H, ch = 6, 6, 0, 2
    t = cm.plan_dyn(4, ch, a, b, H, 1).tile_frames
    xs = [signal(1700 + s, t + 77, ch) for s in range(4)]
    T = design(**DENSE_CURVE)
    # keys that all mean "own": the plain model (TG.Rig compares with TG.Model)
    rig = TG.Rig(cm, 4, ch, a, b, H, t + 77, T)
    for s in range(4):
        rig.m.set_key(s, s)
    rig.m.set_key(-1, -1)
    assert [rig.m.get_key(s) for s in range(4)] == [-1] * 4
    rig.run(xs)
    rig.run([x[:100] for x in xs])
    rig.close()
    # keys set and cleared again before the first run, and between two runs
    rig = TG.Rig(cm, 4, ch, a, b, H, t + 77, T)
    rig.m.set_key(0, 3)
    rig.m.set_key(-1, 2)
    assert [rig.m.get_key(s) for s in range(4)] == [2, 2, -1, 2]
    rig.m.set_key(-1, -1)
    rig.run(xs)
    rig.m.set_key(1, 0)
    rig.m.set_key(1, 1)
    rig.run(xs, uniform=True)
    rig.close()


# ---------------------------------------------------------------------------
# 5. resets

def test_resets_keyed(gpu):
    cm = gpu
    a, b, H = 5, 4, 20
    T = design(**DENSE_CURVE)
    xs = [signal(1800 + s, 700, 1) for s in range(3)]
    loud = [np.full((50, 1), v, dtype=np.int16) for v in (20000, 9000, 20000)]
    rig = KeyRig(cm, 3, 1, a, b, H, 700, T)
    rig.set_key(0, 1)                                            # 0 follows 1; 1 and 2 follow themselves
    rig.run(xs)
    rig.run(loud)
    # resetting the follower keeps the key's history: the follower's first gains still come from the key's 9000s
    rig.reset(0)
    assert rig.model.hist[1].any() and not rig.model.hist[0].any()
    ys = rig.run(xs)
    zero = np.zeros((geometry(a, b, H)[4], 1), dtype=np.int16)
    assert not np.array_equal(ys[0][:40], model_dyn_keyed(xs[0], zero, xs[1], zero, T, a, b, H)[0][:40])
    rig.run(loud)
    # resetting the key changes what the follower detects
    kept = [h.copy() for h in rig.model.hist]
    rig.reset(1)
    ys = rig.run(xs)
    not_reset = model_dyn_keyed(xs[0], kept[0], xs[1], kept[1], T, a, b, H)[0]
    assert not np.array_equal(ys[0][:40], not_reset[:40])
    assert rig.m.min_gain(reset=True).tolist() == rig.model.gmin
    rig.close()


# ---------------------------------------------------------------------------
# 6. literal edges

@pytest.mark.parametrize("channels", [1, 2, 6])
def test_key_bursts_at_a_tile_edge_and_at_the_history_length(gpu, channels):
    """bursts in the key alone under a follower that is constant at full scale: one straddles a tile edge, the last frame
    of the other lies exactly HIST frames before the second run begins -- that run's first output still sees it through
    the KEY's history, the next one does not"""
    cm = gpu
    a, b, H = 6, 5, 100
    A, B, D, W, hist = geometry(a, b, H)
    t = cm.plan_dyn(2, channels, a, b, H, 1).tile_frames
    T = TG.steps()
    base = int(TG.curve_at(T, np.array([300]))[0])
    n = t + 500
    key = np.full((n, channels), 300, dtype=np.int16)
    key[t - 10:t + 10, channels - 1] = -32768
    key[n - hist - 49:n - hist + 1] = 30000                      # its last frame is frame n - hist
    full = np.full((n, channels), -32768, dtype=np.int16)
    rig = KeyRig(cm, 2, channels, a, b, H, n, T)
    rig.set_key(1, 0)
    ys = rig.run([key, full])
    s = rig.model.s[1][0]
    assert s[t - B] == base and s[t - 1] != base and s[t] != base
    assert ys[1][t - B, 0] == (-32768 * base + (1 << 14)) >> 15
    rig.run([np.full((n, channels), 300, dtype=np.int16), full])
    s2 = rig.model.s[1][1]
    assert s2[0] != base and s2[1] == base                       # frame n - hist of the key is the oldest that frame n depends on
    rig.close()


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_zero_curve_under_a_silent_key(gpu, channels):
    """a follower whose curve is unity at knot 0 and zero everywhere else, full-scale square waves in, under a key that
    is silent: the level is the key's, 0, so nothing is reduced; on its own detector the same stream is muted"""
    cm = gpu
    a, b, H = 4, 3, 3
    t = cm.plan_dyn(2, channels, a, b, H, 1).tile_frames
    n = t + 300
    D = geometry(a, b, H)[2]
    sq = np.where((np.arange(n) // 5) % 2 == 0, 32767, -32768).astype(np.int16)[:, None].repeat(channels, axis=1)
    only0 = TG.flat(0)
    only0[0] = UNITY
    rig = KeyRig(cm, 2, channels, a, b, H, n, only0)
    rig.set_key(1, 0)
    silent = np.zeros((n, channels), dtype=np.int16)
    ys = rig.run([silent, sq])
    assert np.array_equal(ys[1][D:], sq[:-D]) and not ys[1][:D].any()
    assert rig.m.min_gain().tolist() == [UNITY, UNITY]
    rig.set_key(1, -1)
    ys = rig.run([silent, sq])
    assert not ys[1][100:].any() and rig.m.min_gain().tolist() == [UNITY, 0]
    rig.close()


# ---------------------------------------------------------------------------
# 7. refusals change nothing

def test_refusals_keyed(gpu):
    cm = gpu
    lib = cm.lib
    rig = KeyRig(cm, 4, 2, 6, 6, 0, 256, design(**DENSE_CURVE))
    m, src, dst, st = rig.m, rig.src.dev, rig.dst.dev, rig.stride
    rig.set_key(0, 1)
    rig.set_key(2, 0)
    xs = [signal(1900 + s, 256, 2) for s in range(4)]
    rig.run(xs)                                                  # a history that a launch would change
    for stream, key in ((4, 0), (-2, 0), (1 << 40, 0), (0, 4), (0, -2), (-1, 4), (-1, -2), (0, 1 << 40)):
        assert m.set_key_rc(stream, key) == cm.ERROR_INVAL, (stream, key)
        assert b"dyn_set_key" in lib.cmhip_last_error()
    assert lib.cmhip_dyn_set_key(None, 0, 0) == cm.ERROR_FAULT
    k = ctypes.c_long(77)
    assert lib.cmhip_dyn_get_key(m.h, 4, ctypes.byref(k)) == cm.ERROR_INVAL and k.value == 77
    assert lib.cmhip_dyn_get_key(m.h, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_dyn_get_key(None, 0, ctypes.byref(k)) == cm.ERROR_FAULT
    assert [m.get_key(s) for s in range(4)] == [1, -1, 0, -1]    # the old map stays
    # a keyed stream and its key with different counts: refused before anything is touched
    rig.dst.array[:] = SENTINEL
    assert m.run_rc(src, st, 256, dst, st, [100, 101, 100, 7]) == cm.ERROR_INVAL
    msg = lib.cmhip_last_error().decode()
    assert "stream 0" in msg and "100" in msg and "stream 1" in msg and "101" in msg, msg
    assert m.run_rc(src, st, 256, dst, st, [100, 100, 0, 7]) == cm.ERROR_INVAL
    msg = lib.cmhip_last_error().decode()
    assert "stream 2" in msg and "stream 0" in msg and " 0 frames" in msg and "100" in msg, msg
    m.sync()
    assert (rig.dst.array == SENTINEL).all()
    rig.run([x[:n] for x, n in zip(xs, (100, 100, 100, 7))])     # the history and the parity are what the first run left
    rig.run([x[:n] for x, n in zip(xs, (0, 0, 0, 256))])         # equal counts of 0: the three keep everything
    rig.run(xs, uniform=True)
    rig.close()


# ---------------------------------------------------------------------------
# 8. composition: bus -> keyed dynamics -> second bus -> limiter -> the slots of a batch, block by block

CHAIN_BLOCKS = TG.CHAIN_BLOCKS                    # per programme: the counts of its music and its voice, block by block


def test_chain_with_ducking_into_a_batch(gpu, oracle):
    from oracle import oracle_ffi
    tb = _load("test_gpu_bus")
    TL = TG.TL
    cm = gpu
    P, F = 2, 4100                                               # programmes; first-bus outputs 2p (music), 2p + 1 (voice)
    S, B1 = 4 * P, 2 * P                                         # two sources per sum
    a, b, H, la, lh, T_lim, drive = 6, 6, 30, 6, 30, 29204, 6144
    duck = cm.dyn_design_duck(threshold_db=-36.0, depth_db=14.0, knee_db=8.0)
    comp = design(**DENSE_CURVE)
    sum_of = [s // 2 for s in range(S)]
    prog_of = [q // 2 for q in sum_of]
    total = [sum(CHAIN_BLOCKS[prog_of[s]]) for s in range(S)]
    xs = [TG.bursts(2000 + s, total[s], 1) for s in range(S)]
    for s in range(S):
        if sum_of[s] % 2:                                        # the presenters pause: the bed comes back up
            xs[s][1000:2500] = 0
    table1 = (sum_of, list(range(S)), np.full((S, 1, 1), 8192, dtype=np.int16))
    table2 = ([q // 2 for q in range(B1)], list(range(B1)), np.full((B1, 1, 1), 16384, dtype=np.int16))
    dyn_m, lim_m = KeyModel(B1, 1, a, b, H), TL.Model(P, 1, la, lh)
    for p in range(P):
        dyn_m.set(2 * p, duck)
        dyn_m.set(2 * p + 1, comp)
        dyn_m.set_key(2 * p, 2 * p + 1)
    lim_m.set(-1, T_lim, drive)
    objects, arrays = [], []
    try:
        batch = cm.Batch(P, 1, F, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, rate=48000)
        objects.append(batch)
        st = batch.hip_stream()
        bus1 = cm.Bus(S, B1, 1, 1, F, 16, hip_stream=st)
        objects.append(bus1)
        dyn = cm.Dynamics(B1, 1, a, b, H, F, hip_stream=st)
        objects.append(dyn)
        bus2 = cm.Bus(B1, P, 1, 1, F, 16, hip_stream=st)
        objects.append(bus2)
        lim = cm.Limiter(P, 1, la, lh, F, threshold=T_lim, drive=drive, hip_stream=st)
        objects.append(lim)
        bus1.set_routing(*table1)
        bus2.set_routing(*table2)
        for p in range(P):
            dyn.set_curve(2 * p, duck)
            dyn.set_curve(2 * p + 1, comp)
            dyn.set_key(2 * p, 2 * p + 1)
        stride = (F + 7) // 8 * 8 + 8
        d_sum, d_dyn = (cm.DeviceWords((B1 * stride * 2 + 7) // 8) for _ in range(2))
        d_mix, d_lim = (cm.DeviceWords((P * s_ * 2 + 7) // 8) for s_ in (stride, batch.stride))
        arrays += [d_sum, d_dyn, d_mix, d_lim]
        wants, results, pos = [], [], [0] * S
        for r in range(len(CHAIN_BLOCKS[0])):
            counts = [CHAIN_BLOCKS[prog_of[s]][r] for s in range(S)]
            ins = [xs[s][pos[s]:pos[s] + counts[s]] for s in range(S)]
            pos = [p + n for p, n in zip(pos, counts)]
            outs = lim_m.run(tb.model_bus(dyn_m.run(tb.model_bus(ins, table1, B1, 1)), table2, P, 1))
            wants.append(outs)
            feed = cm.MappedPcm(types.SimpleNamespace(streams=S, stride=stride))
            res = cm.MappedPcm(batch)
            feed.array[:] = 0x5a5a
            res.array[:] = SENTINEL
            for s, x in enumerate(ins):
                feed.array[s, :x.size] = x.reshape(-1)
            results.append(res)
            arrays += [feed, res]
            # (no wait anywhere: the order is the stream's)
            k1 = bus1.run(feed.dev, stride, max(counts), d_sum.dev, stride, counts)
            assert k1.tolist() == [CHAIN_BLOCKS[q // 2][r] for q in range(B1)]   # equal within a keyed pair
            dyn.run(d_sum.dev, stride, int(k1.max()), d_dyn.dev, stride, k1)
            k2 = bus2.run(d_dyn.dev, stride, int(k1.max()), d_mix.dev, stride, k1)
            assert k2.tolist() == [CHAIN_BLOCKS[p][r] for p in range(P)]
            lim.run(d_mix.dev, stride, int(k2.max()), d_lim.dev, batch.stride, k2)
            batch.run_slots(int(k2.max()), d_lim.dev, res.dev, k2)
        batch.sync()                                             # (the only synchronisation)
        for r, outs in enumerate(wants):
            for q in range(P):
                want = outs[q].reshape(-1)
                have = results[r].array[q, :want.size]
                bad = np.flatnonzero(have != want)
                assert bad.size == 0, ("block", r, "programme", q, "first mismatch at frame", int(bad[0]), "of", want.size)
                assert (results[r].array[q, want.size:] == SENTINEL).all(), ("block", r, "programme", q)
        assert dyn.min_gain().tolist() == dyn_m.gmin and lim.min_gain().tolist() == lim_m.gmin
        floor = int(duck[:123].min())
        for p in range(P):                                       # the bed was ducked all the way, and came back up
            assert dyn_m.gmin[2 * p] == floor < 8000 and max(int(sg.max()) for sg in dyn_m.s[2 * p]) == UNITY
        vu, rcs = batch.vu_results()
        for q in range(P):
            y = np.concatenate([outs[q].reshape(-1) for outs in wants])
            v = oracle.vu_new(1)
            oracle.vu_accumulate(v, y)
            _, vr = oracle.vu_result(v)
            assert rcs[q] == 0 and oracle_ffi.vu_result_dict(vr) == vu[q].as_dict(), q
            assert vu[q].frames == sum(CHAIN_BLOCKS[q]) and abs(vu[q].global_peak) <= T_lim
    finally:                                 # (the stages that borrow the batch's stream go before the batch, whatever the outcome)
        for o in reversed(objects):
            o.close()
        for o in arrays:
            o.free()


# ---------------------------------------------------------------------------
# 9. the example

def test_batch_ducking_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_ducking"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_ducking.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("music + voice -> bus -> dynamics (music keyed on voice): delay 63")
    f = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in out[1:]]
    assert len(out) == 4 and out[1].startswith("speech: ") and out[2].startswith("after: ")
    assert out[3].startswith("programme: ")
    assert int(f[0]["music_min_gain"]) == int(f[0]["duck_floor"]) < 12000        # ducked all the way during speech
    assert int(f[1]["music_min_gain"]) == 32768                                  # and back at unity afterwards
    assert int(f[2]["frames"]) == 48000 and int(f[2]["channels"]) == 2 and abs(int(f[2]["peak"])) <= 29204
