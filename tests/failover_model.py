"""The failover switch's arithmetic in Python integers, written from the text of include/coolmic_hip.h ("failover
switch") and from nothing else: the level of every candidate per window, the run counters, the decision at every window
edge, the plan of every window and the crossfade of a changeover.  tests/test_failover_host.py holds the library's step
function and an emulation of the step kernel's walk against it, tests/test_gpu_failover.py the device.

`trace` counts the branches that ran: a palette that misses one is a test bug.
"""
import numpy as np

RUN_MAX = 65535
# every branch of the decision, and the two things around it that a walk can get wrong
BRANCHES = ("return", "fail_lower", "fail_higher", "all_dead", "forced", "fade_chain", "fade_continues", "steady")
SATURATION = ("live_saturated", "dead_saturated")                 # reached by planting 65534, not by 65535 windows


def params(w, **kw):
    """the creation defaults of an object with window_log2 = w, with `kw` over them"""
    p = dict(quiet=(33, 33, 33, 33), fail_windows=1, return_windows=1, fade_log2=w, force=-1)
    p.update(kw)
    p["quiet"] = tuple(p["quiet"])
    return p


def params_ok(p, w, K):
    return (all(0 <= q <= 32767 for q in p["quiet"]) and 1 <= p["fail_windows"] <= 65535 and
            1 <= p["return_windows"] <= 65535 and w <= p["fade_log2"] <= 16 and -1 <= p["force"] < K)


def crossfade(a, b, p):
    """cmhip_delay_crossfade's formula"""
    return (a * (32768 - p) + b * p + 16384) >> 15


def count(m, quiet, live, dead, trace=None):
    """one candidate's counters moved on by a complete window of level m -> (live_run, dead_run)"""
    if m > quiet * quiet:
        if live + 1 > RUN_MAX and trace is not None:
            trace["live_saturated"] += 1
        return min(live + 1, RUN_MAX), 0
    if dead + 1 > RUN_MAX and trace is not None:
        trace["dead_saturated"] += 1
    return 0, min(dead + 1, RUN_MAX)


def step(K, p, cur, live, dead, trace=None):
    """rule 2: the candidate wanted at an edge outside a fade"""
    def took(name):
        if trace is not None:
            trace[name] += 1

    if p["force"] >= 0:
        took("forced")
        return p["force"]
    b = next((i for i in range(K) if live[i] >= p["return_windows"]), None)
    if b is not None and b < cur:
        took("return")
        return b
    if dead[cur] >= p["fail_windows"]:
        for i in range(K):
            if i != cur and live[i] >= 1:
                took("fail_lower" if i > cur else "fail_higher")
                return i
        took("all_dead")
    return cur


def new_trace():
    return {b: 0 for b in BRANCHES + SATURATION}


class Output:
    """one output: its list, its parameters and everything it carries from frame to frame"""

    def __init__(self, channels, w, source, trace):
        self.C, self.w, self.W, self.trace = channels, w, 1 << w, trace
        self.src = [source]
        self.p = params(w)
        self.switches = 0
        self.reset()

    K = property(lambda self: len(self.src))

    def reset(self):
        self.n = 0
        self.live, self.dead, self.level = [0] * 4, [0] * 4, [0] * 4
        self.acc = [[0] * self.C for _ in range(4)]
        self.plan = None                              # (from, to, phi', q) of the window the last frame lies in

    def set_sources(self, streams):
        self.src = list(streams)
        self.p = dict(self.p, force=-1)
        self.reset()

    def c0(self):
        return self.p["force"] if self.p["force"] >= 0 else 0

    def edge(self):
        """frame n = k W is about to be processed"""
        if self.n == 0:
            self.plan = (self.c0(), self.c0(), 0, 0)
            return
        for i in range(self.K):
            self.live[i], self.dead[i] = count(self.level[i], self.p["quiet"][i], self.live[i], self.dead[i], self.trace)
        fr, to, phi, q = self.plan
        fading = fr != to
        if fading and q + 1 < (1 << (phi - self.w)):
            self.trace["fade_continues"] += 1
            self.plan = (fr, to, phi, q + 1)
            return
        want = step(self.K, self.p, to, self.live, self.dead, self.trace)
        if want != to:
            if fading:
                self.trace["fade_chain"] += 1
            self.switches += 1
            self.plan = (to, want, self.p["fade_log2"], 0)
        else:
            self.trace["steady"] += 1
            self.plan = (to, to, 0, 0)

    def run(self, xs):
        """xs: per candidate int16 [F][C] -> int16 [F][C]"""
        F = xs[0].shape[0]
        y = np.empty((F, self.C), dtype=np.int16)
        f = 0
        while f < F:
            j = self.n & (self.W - 1)
            if j == 0:
                self.edge()
            seg = min(F - f, self.W - j)
            fr, to, phi, q = self.plan
            if fr == to:
                y[f:f + seg] = xs[to][f:f + seg]
            else:
                d = q * self.W + j + np.arange(seg, dtype=np.int64)
                p = ((d << 15) >> phi)[:, None]
                a, b = xs[fr][f:f + seg].astype(np.int64), xs[to][f:f + seg].astype(np.int64)
                v = (a * (32768 - p) + b * p + 16384) >> 15
                assert v.min() >= -32768 and v.max() <= 32767
                y[f:f + seg] = v
            for i in range(self.K):
                sq = (xs[i][f:f + seg].astype(np.int64) ** 2).sum(axis=0)
                for c in range(self.C):
                    self.acc[i][c] += int(sq[c])
            self.n += seg
            f += seg
            if self.n & (self.W - 1) == 0:
                for i in range(self.K):
                    self.level[i] = max(self.acc[i]) >> self.w
                    self.acc[i] = [0] * self.C
        return y

    def state(self):
        fr, to, _, q = self.plan if self.n else (self.c0(), self.c0(), 0, 0)
        return dict(fr=fr, to=to, fade_window=q, switches=self.switches, live_run=list(self.live),
                    dead_run=list(self.dead), level=list(self.level))


class Switch:
    """S input slots, O outputs"""

    def __init__(self, streams, outputs, channels, w):
        self.S, self.O, self.C, self.w = streams, outputs, channels, w
        self.trace = new_trace()
        self.out = [Output(channels, w, min(o, streams - 1), self.trace) for o in range(outputs)]

    def _outs(self, output):
        return range(self.O) if output < 0 else [output]

    def set(self, output, p):
        assert all(params_ok(p, self.w, self.out[o].K) for o in self._outs(output))
        for o in self._outs(output):
            self.out[o].p = dict(p, quiet=tuple(p["quiet"]))

    def set_sources(self, output, streams):
        assert 1 <= len(streams) <= 4 and len(set(streams)) == len(streams) and all(0 <= s < self.S for s in streams)
        self.out[output].set_sources(streams)

    def reset(self, output=-1):
        for o in self._outs(output):
            self.out[o].reset()

    def run(self, slots, counts):
        """slots: per input slot int16 [frames][C]; counts: per output -> per output int16 [count][C]"""
        ys = []
        for o, n in enumerate(counts):
            t = self.out[o]
            ys.append(t.run([np.asarray(slots[s])[:n] for s in t.src]) if n else np.empty((0, self.C), dtype=np.int16))
        return ys

    def state(self):
        st = [t.state() for t in self.out]
        return {k: [s[k] for s in st] for k in st[0]}


# ---------------------------------------------------------------------------
# the case the device tests and the host emulation share: S = 6 inputs, O = 5 outputs; input 5 is the backup of three
# outputs, input 4 is read by nobody

CASE_STREAMS, CASE_OUTPUTS = 6, 5
CASE_SOURCES = ([0, 5], [1, 5, 2, 3], [2, 5], [3], [3, 0, 1, 2])
CASE_SHAPES = [(1, 6), (2, 6), (3, 6), (6, 6), (16, 6), (2, 7)]


def case_params(w, o):
    """per output: a palette that differs in every field; output 0 fades over four windows"""
    return (params(w, quiet=(40, 40, 40, 40), fail_windows=2, return_windows=3, fade_log2=w + 2),
            params(w, quiet=(1, 300, 1, 0), fail_windows=1, return_windows=2, fade_log2=w),
            params(w, quiet=(33, 2000, 33, 33), fail_windows=3, return_windows=1, fade_log2=w + 1),
            params(w),
            params(w, quiet=(0, 1, 1, 500), fail_windows=1, return_windows=1, fade_log2=w))[o]


def spurts(seed, frames, channels, W, amp=9000):
    """noise in spurts with silent stretches of whole windows between them"""
    rng = np.random.default_rng(seed)
    x = np.zeros((frames, channels), dtype=np.int16)
    at, on = 0, bool(seed & 1)
    while at < frames:
        n = int(rng.integers(1, 7)) * W + int(rng.integers(0, W))
        if on:
            x[at:at + n] = rng.integers(-amp, amp + 1, size=(min(n, frames - at), channels))
        on = not on
        at += n
    return x


def threshold_signal(frames, channels, W):
    """stretches whose windows have m of exactly 0, 1 and 2: silence but for one sample of 1 per window (m = 0), every
    sample 1 or -1 (m = 1), every other frame 2 (m = 2), and full scale (m = 2^30)"""
    x = np.zeros((frames, channels), dtype=np.int16)
    n = np.arange(frames)
    kind = (n // (3 * W)) % 5
    x[kind == 0] = 1
    x[(kind == 1) & (n % 2 == 0)] = 2
    x[(kind == 2) & (n % W == 5)] = 1
    x[kind == 3] = -32768
    x[(kind == 1)] *= np.where(np.arange(channels) % 2 == 0, 1, -1).astype(np.int16)
    return x


def case_signals(channels, w, frames):
    W = 1 << w
    sig = [spurts(11 + s, frames, channels, W) for s in range(CASE_STREAMS)]
    sig[1] = threshold_signal(frames, channels, W)
    sig[2] = np.roll(threshold_signal(frames, channels, W), 4 * W, axis=0)
    sig[3][5 * W:9 * W] = 32767                      # full scale, every channel
    sig[3][9 * W:12 * W] = -32768
    return sig


def case_cuts(w, rounds=4):
    """run lengths 1, W-1, W, W+1, 2W+3, 0 and 5W+3, rotated per output -> [run][output]"""
    W = 1 << w
    lens = [1, W - 1, W, W + 1, 2 * W + 3, 0, 5 * W + 3]
    return [[lens[(r + o) % len(lens)] for o in range(CASE_OUTPUTS)] for r in range(rounds * len(lens))]


def case_script(channels, w):
    """-> the case as a list of ("run", slots, counts), ("set", o, p), ("sources", o, list) and ("reset", o).  Where
    fade_log2 is set inside a fade is found by walking a model along: the first two times a run leaves output 0 in a
    fade of four windows with at least two still to come, phi is set to w there, and put back two runs later."""
    cuts = case_cuts(w)
    total = sum(max(c) for c in cuts)
    sig = case_signals(channels, w, total)
    ops = [("sources", o, CASE_SOURCES[o]) for o in range(CASE_OUTPUTS)]
    ops += [("set", o, case_params(w, o)) for o in range(CASE_OUTPUTS)]
    shadow = Switch(CASE_STREAMS, CASE_OUTPUTS, channels, w)
    play_model(shadow, ops)
    at, mid_fade_sets, restore = 0, 0, -1
    for r, counts in enumerate(cuts):
        n = max(counts)
        ops.append(("run", [x[at:at + n] for x in sig], counts))
        shadow.run(ops[-1][1], counts)
        at += n
        more = []
        t = shadow.out[0]
        if r == restore:
            more.append(("set", 0, case_params(w, 0)))
        elif mid_fade_sets < 2 and r > restore and t.n and t.plan[0] != t.plan[1] and t.plan[2] == w + 2 and t.plan[3] < 2:
            more.append(("set", 0, dict(case_params(w, 0), fade_log2=w)))   # a fade under way keeps its length
            mid_fade_sets += 1
            restore = r + 2
        if r == 6:
            more.append(("set", 1, dict(case_params(w, 1), force=2)))       # forced, and forced back below
        if r == 10:
            more.append(("set", 1, case_params(w, 1)))
        if r == 13:
            more.append(("reset", 2))
        if r == 16:
            more.append(("sources", 4, [0, 3, 2]))
            more.append(("set", 4, dict(case_params(w, 4), force=1)))
        if r == 19:
            more.append(("set", 4, case_params(w, 4)))
        ops += more
        play_model(shadow, more)
    assert mid_fade_sets == 2
    return ops


def play_model(model, ops):
    """a script's operations on the model alone -> per output the whole output"""
    outs = [[] for _ in range(model.O)]
    for op in ops:
        if op[0] == "run":
            for o, y in enumerate(model.run(op[1], op[2])):
                outs[o].append(y)
        elif op[0] == "set":
            model.set(op[1], op[2])
        elif op[0] == "sources":
            model.set_sources(op[1], op[2])
        else:
            model.reset(op[1])
    return [np.concatenate(o) if o else np.empty((0, model.C), dtype=np.int16) for o in outs]
