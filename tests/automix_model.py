"""The automixer as include/coolmic_hip.h ("automixer") states it, in numpy and Python integers: a desk of S streams walked
group by group and window by window, written from the header's text and not from the kernels.  Shared by
tests/test_gpu_automix.py (the device against it) and tests/test_automix_host.py (an emulation of the kernels' walk
against it, without a GPU); also the inputs and the cases both use."""
import collections
import math

import numpy as np

PARAM_NAMES = ("weight", "floor", "attack", "release", "initial")
BRANCHES = ("V_above", "V_below", "V_equal", "sum_zero", "floor_acts", "share", "m_full", "m_zero")


def params(**kw):
    """a parameter set as a dict: the creation defaults with `kw` over them"""
    p = dict(weight=4096, floor=0, attack=0, release=0, initial=4096)
    p.update(kw)
    assert set(p) == set(PARAM_NAMES)
    return p


def power(P, m, p, trace=None):
    """P[k] from P[k-1] and the window's m"""
    t = trace if trace is not None else collections.Counter()
    assert 0 <= m <= 2 ** 30
    V = ((m * p["weight"]) >> 12) << 8
    t["V_above" if V > P else "V_below" if V < P else "V_equal"] += 1
    t["m_full" if m == 2 ** 30 else "m_zero" if m == 0 else "m_between"] += 1
    P = P + ((V - P) >> (p["attack"] if V > P else p["release"]))          # (Python's >> floors, as an arithmetic shift)
    assert 0 <= P <= 2 ** 38
    return P


def share(P, total, floor, D_before, trace=None):
    """D[k] from P[k], the group's sum, the floor and D[k-1]"""
    t = trace if trace is not None else collections.Counter()
    if total == 0:
        t["sum_zero"] += 1
        return D_before
    q = (P << 24) // total
    assert q <= 2 ** 24 and P << 24 < 2 ** 64
    D = math.isqrt(q)
    t["floor_acts" if floor > D else "share"] += 1
    return max(floor, D)


class Stream:
    def __init__(self, p):
        self.p = dict(p)
        self.group = -1
        self.restart()

    def restart(self):
        self.n = 0
        self.sums = None
        self.a_lo = self.a_hi = self.pending = None
        self.P = 0


class Desk:
    """S streams of C channels at window 2^w: groups, parameters, runs, state"""

    def __init__(self, streams, channels, w):
        self.S, self.C, self.w, self.W = streams, channels, w, 1 << w
        self.st = [Stream(params()) for _ in range(streams)]
        self.trace = collections.Counter()
        self.squares = []                         # per group and complete window: the sum of D^2 and whether all floors are 0

    def members(self, g):
        return [s for s in range(self.S) if self.st[s].group == g]

    def set(self, stream, p):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.st[s].p = dict(p)

    def set_group(self, stream, group):
        old = self.st[stream].group
        if old >= 0:
            for s in self.members(old):
                self.st[s].restart()
        self.st[stream].group = group
        self.reset(stream)

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            g = self.st[s].group
            for j in ([s] if g < 0 else self.members(g)):
                self.st[j].restart()

    def state(self):
        """-> (gain [S], power [S], share [S]) as cmhip_automix_state reports them"""
        out = []
        for t in self.st:
            if t.group < 0:
                out.append((4096, 0, 4096))
            elif t.n == 0:
                out.append((t.p["initial"], 0, t.p["initial"]))
            else:
                out.append((t.a_hi, t.P, t.pending))
        return tuple(list(v) for v in zip(*out))

    def run(self, xs):
        """xs: per stream int16 [F_s][C], equal F_s within a group -> per stream int16 [F_s][C]"""
        xs = [np.asarray(x, dtype=np.int64).reshape(-1, self.C) for x in xs]
        ys = [None] * self.S
        for s, t in enumerate(self.st):
            if t.group < 0:
                ys[s] = xs[s].astype(np.int16)    # a copy, bit for bit
                t.n += xs[s].shape[0]
        for g in sorted({t.group for t in self.st if t.group >= 0}):
            mem = self.members(g)
            F = xs[mem[0]].shape[0]
            assert all(xs[s].shape[0] == F for s in mem) and len({self.st[s].n for s in mem}) == 1
            for s, y in zip(mem, self._run_group(mem, [xs[s] for s in mem], F)):
                ys[s] = y
        return ys

    def _run_group(self, mem, xs, F):
        ts = [self.st[s] for s in mem]
        ys = [np.zeros((F, self.C), dtype=np.int64) for _ in mem]
        f = 0
        while f < F:
            n = ts[0].n
            j = n & (self.W - 1)
            for t in ts:
                if n == 0:
                    t.a_lo = t.a_hi = t.pending = t.p["initial"]
                    t.P = 0
                    t.sums = np.zeros(self.C, dtype=np.int64)
                elif j == 0:                      # frame k W, k >= 1: A[k+1] = D[k-1]
                    t.a_lo, t.a_hi = t.a_hi, t.pending
            m = min(F - f, self.W - j)
            for t, x, y in zip(ts, xs, ys):
                seg = x[f:f + m]
                g = t.a_lo + (((t.a_hi - t.a_lo) * (j + np.arange(m, dtype=np.int64))) >> self.w)
                assert g.min() >= 0 and g.max() <= 4096
                v = (seg * g[:, None] + 2048) >> 12
                assert v.min() >= -32768 and v.max() <= 32767 and (np.abs(v) <= np.abs(seg)).all()
                y[f:f + m] = v
                t.sums += (seg * seg).sum(axis=0)
                t.n += m
            f += m
            if ts[0].n & (self.W - 1) == 0:       # the window is complete, for every member at once
                for t in ts:
                    E = int(t.sums.max())
                    t.P = power(t.P, E >> self.w, t.p, self.trace)
                    t.sums[:] = 0
                total = sum(t.P for t in ts)
                for t in ts:
                    t.pending = share(t.P, total, t.p["floor"], t.pending, self.trace)
                if total:
                    self.squares.append((sum(t.pending ** 2 for t in ts), all(t.p["floor"] == 0 for t in ts)))
        return [y.astype(np.int16) for y in ys]


# ---------------------------------------------------------------------------
# inputs and cases

def spurts(seed, frames, channels, W, quiet_first=2):
    """talk spurts: noise under an envelope that steps every 1 to 3 windows between silence -- whole windows of zeros --
    a murmur of about 40 and speech of up to 30 000; the first `quiet_first` windows are silent"""
    rng = np.random.default_rng(seed)
    x = np.zeros((frames, channels), dtype=np.int64)
    at = quiet_first * W
    while at < frames:
        n = min(int(rng.integers(1, 4)) * W, frames - at)
        amp = (0, 40, int(rng.integers(2000, 30001)))[int(rng.integers(0, 3))]
        if amp:
            x[at:at + n] = rng.integers(-amp, amp + 1, size=(n, channels))
        at += n
    return x.astype(np.int16)


CASE_STREAMS = 7
CASE_GROUPS = [0, 0, 0, 1, 1, -1, 6]              # {0, 1, 2}, {3, 4}, 5 in no group, {6} alone under group id S - 1
CASE_SHAPES = [(1, 6), (2, 6), (3, 6), (16, 6), (2, 8)]


def palette(s):
    """the parameters of stream s of the model case: together they take every branch"""
    return [
        params(),                                                        # shifts 0: P = V at once
        params(weight=2048, attack=2, release=5, initial=1000),
        params(weight=4095, floor=0, attack=8, release=8, initial=0),
        params(floor=3000),                                              # a floor above the share
        params(weight=0, floor=700, release=3, initial=2048),                      # no weight: P stays 0
        params(weight=77, floor=9, attack=1, release=1, initial=5),      # (in no group: unused)
        params(floor=100, attack=1),
    ][s]


def run_lengths(W):
    return [1, W - 1, W, W + 1, 2 * W + 3, 0, 5 * W + 3]


def case(channels, w, seed=0):
    """-> (signals, cuts): 7 streams; run k gives group number i (in no group: i = 3) length number k + 2 i of the
    list, so groups differ and members agree, and every stream meets every length"""
    W = 1 << w
    lengths = run_lengths(W)
    total = sum(lengths)
    signals = [spurts(seed + 100 * w + 10 * channels + s, total, channels, W, quiet_first=1 + s % 2)
               for s in range(CASE_STREAMS)]
    signals[4][:] = signals[3]                    # the member without weight hears what its neighbour hears
    signals[0][3 * W:5 * W] = -32768              # full scale, constant: m = 2^30
    signals[6][2 * W:4 * W] = -32768
    signals[3][5 * W:7 * W] = 0                   # group {3, 4} silent together behind speech: the sum is 0 at release 0
    signals[4][5 * W:7 * W] = 0
    signals[3][4 * W:5 * W] = 9000
    which = {0: 0, 1: 1, -1: 3, 6: 2}
    cuts = [[lengths[(k + 2 * which[g]) % len(lengths)] for g in CASE_GROUPS] for k in range(len(lengths))]
    assert all(sum(c[s] for c in cuts) == total for s in range(CASE_STREAMS))
    return signals, cuts


def walk(desk, signals, cuts):
    """the signals through a Desk as `cuts` says -> per stream the concatenated output"""
    at = [0] * desk.S
    out = [[] for _ in range(desk.S)]
    for counts in cuts:
        ys = desk.run([signals[s][at[s]:at[s] + n] for s, n in enumerate(counts)])
        for s, n in enumerate(counts):
            out[s].append(ys[s])
            at[s] += n
    return [np.concatenate(o) for o in out]


def case_desk(channels, w):
    d = Desk(CASE_STREAMS, channels, w)
    for s in range(CASE_STREAMS):
        d.set(s, palette(s))
        if CASE_GROUPS[s] >= 0:
            d.set_group(s, CASE_GROUPS[s])
    return d
