"""CPU: the planted-pattern table of tests/test_gpu_truepeak_edges.py -- the model, the cases and the conditions the
cases rely on, on the model alone.

The true-peak meter (csrc/k_tpeak.hip) reports a maximum per channel and window, and a maximum hides local errors: an
output lost at a tile edge, at the end of a ragged count or at the start of a run leaves the peak of a noise signal
where it was.  Every case here is one silent stream with the 12-frame worst-case pattern planted on one input channel,
so that the window's peak sits at ONE known output -- the pattern's last frame -- and that frame is put at every
boundary the kernels have: tiles, the inner units of a tile, the end of the count, the cut between two runs (where only
the 11-frame history carries it), window closes and 0-frame runs.  Gains, channel map and the planted channel rotate
with the case index.

The model is the integer model of tests/test_gpu_truepeak.py (`tp`, `Model`): 11 frames of history per channel, kept
over a window close, over the transformed stream orc.gain_apply(g, orc.chmap(map, raw, C), C), with the table of
cm.tp_coefficients() -- never a run of the device code.  It takes a `fault=` switch per way a kernel could be subtly
wrong; test_every_fault_changes_some_case asserts that each of them changes what at least 3 cases expect, which makes
"the device test would fail on such a kernel" something the CPU checks.  Run with -s to see the counts."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle_ffi as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]     # phase 1 of the filter
WORST = 542986257                                  # the largest value the filter can produce ...
WORST_PATTERN = np.array([32767 if P1[11 - j] >= 0 else -32768 for j in range(12)], dtype=np.int16)  # ... and its input
HIST = 11

CHANNELS = [1, 2, 3, 4, 5, 6, 8, 12, 16]           # the device test's channel counts
SWEEP = [3, 6, 16, 1, 2]                           # the fault sweep: the any kernel, then the fast kernel
GAIN_KINDS = ("none", "below", "saturating")
MAP_KINDS = ("identity", "permutation", "duplicate")
KINDS = ("pos", "count", "decoy", "split", "dribble")
SCALE = 1000

FAULTS = (
    "halo_tile",       # halo lost at tiles k >= 1
    "halo_inner",      # halo lost at every inner edge (the 16-frame run; the lane's 128 bytes)
    "last_frame",      # last frame of the count not counted
    "last_unit",       # last partial inner unit not counted (the 16-frame run; the 16-byte vector)
    "past_count",      # outputs counted up to the end of the inner unit past the count
    "hist_raw",        # history stored raw
    "hist_nomap",      # history stored without the channel map
    "hist_noshift",    # history not shifted when a run has fewer than 11 frames
    "hist_zero_run",   # history cleared by a 0-frame run
    "hist_take",       # history cleared by a window close
    "hist_tile0",      # history taken from the end of tile 0 instead of the last tile
)


def geometry(C):
    """the kernel's boundaries in frames.  tile: what a workgroup takes; inner: the edges inside a tile; halo: the
    unit whose first outputs need frames of the unit before (a thread's run, a lane's 128 bytes); unit: the unit the
    end of a count falls into (a thread's run with its `break`, the 16-byte vector that nvec counts)"""
    if C >= 3:                                     # k_tpeak_any
        return dict(tile=1024, inner=(16,), halo=16, unit=16)
    return dict(tile=4096 // C, inner=(64 // C, 8 // C), halo=64 // C, unit=8 // C)      # k_tpeak_fast<C>


def max_frames(C):
    return 2 * geometry(C)["tile"] + 155


# ---------------------------------------------------------------------------
# the model


def _peak(H, z, lo, hi):
    """max |y_p[f]| over the four phases and the frames lo <= f < hi; z: 11 values of history, then the frames"""
    if hi <= lo:
        return 0
    seg = z[lo:hi + HIST]
    if not seg.any():                              # (the filter of silence is silence)
        return 0
    return max(int(np.abs(np.convolve(seg, H[p], "valid")).max()) for p in range(4))


def _peak_without_halo(H, z, n, step):
    """the fault of a kernel that starts every `step` frames from zeros instead of the frames before"""
    pk = _peak(H, z, 0, min(n, step))
    for e in range(step, n, step):
        seg = z[HIST + e:HIST + min(n, e + step)]
        if seg.any():
            pk = max(pk, _peak(H, np.concatenate([np.zeros(HIST, dtype=np.int64), seg]), 0, seg.size))
    return pk


def response(H, x):
    """per frame, max over the phases of |y_p[f]| from zero history (the conditions on the table)"""
    z = np.concatenate([np.zeros(HIST, dtype=np.int64), np.asarray(x, dtype=np.int64)])
    return np.max([np.abs(np.convolve(z, H[p], "valid")) for p in range(4)], axis=0)


class EdgeModel:
    """one stream: history per channel (kept over window closes), the open window's maxima and frame count.
    fault: None, or one of FAULTS -- the same stream as a kernel with that fault would meter it"""

    def __init__(self, H, C, fault=None):
        assert fault is None or fault in FAULTS
        self.H, self.C, self.fault, self.geo = np.asarray(H, dtype=np.int64), C, fault, geometry(C)
        self.hist = [np.zeros(HIST, dtype=np.int64) for _ in range(C)]
        self.peak = [0] * C
        self.frames = 0

    def run(self, y, n, raw=None, unmapped=None):
        """y: the transformed samples of what the slot holds, n frames of them the stream's; raw: the same before map
        and gain; unmapped: with the gain and without the map (the history faults)"""
        C, fault, geo = self.C, self.fault, self.geo
        y = np.asarray(y, dtype=np.int64)
        for c in range(C):
            held = y[c::C]
            x = held[:n]
            z = np.concatenate([self.hist[c], held])
            if fault == "halo_tile":
                pk = _peak_without_halo(self.H, z, n, geo["tile"]) if z.any() else 0
            elif fault == "halo_inner":
                pk = _peak_without_halo(self.H, z, n, geo["halo"]) if z.any() else 0
            elif fault == "last_frame":
                pk = _peak(self.H, z, 0, n - 1)
            elif fault == "last_unit":
                pk = _peak(self.H, z, 0, n - n % geo["unit"])
            elif fault == "past_count":
                pk = _peak(self.H, z, 0, min(-(-n // geo["unit"]) * geo["unit"], held.size))
            else:
                pk = _peak(self.H, z, 0, n)
            self.peak[c] = max(self.peak[c], pk)
            new = x
            if fault == "hist_raw":
                new = np.asarray(raw, dtype=np.int64)[c::C][:n]
            elif fault == "hist_nomap":
                new = np.asarray(unmapped, dtype=np.int64)[c::C][:n]
            elif fault == "hist_tile0":
                new = x[:geo["tile"]]
            if fault == "hist_noshift" and 0 < n < HIST:
                self.hist[c] = np.concatenate([self.hist[c][:HIST - n], new])
            elif fault == "hist_zero_run" and n == 0:
                self.hist[c] = np.zeros(HIST, dtype=np.int64)
            else:
                self.hist[c] = np.concatenate([self.hist[c], new])[-HIST:]
        self.frames += n

    def take(self):
        out = (list(self.peak), self.frames)
        self.peak = [0] * self.C
        self.frames = 0
        if self.fault == "hist_take":
            self.hist = [np.zeros(HIST, dtype=np.int64) for _ in range(self.C)]
        return out


# ---------------------------------------------------------------------------
# the case table


def _plant(total, C, ch, at):
    x = np.zeros(total * C, dtype=np.int16)
    x[at * C + ch:(at + 12) * C:C] = WORST_PATTERN
    return x


def _rotation(i, C):
    """planted input channel, gains and channel map of case i"""
    ch = i % C
    gain_kind = GAIN_KINDS[(i // C + i % C) % 3]                       # (every channel meets every kind of gain)
    map_kind = MAP_KINDS[(i // 3) % 3] if C > 1 else "identity"        # (mono has no map but the identity)
    if gain_kind == "none":
        gains = None
    elif gain_kind == "below":
        gains = [250 + 41 * ((i + 3 * c) % 18) for c in range(C)]      # 250 .. 947: all below the scale
    else:
        gains = [1500 + 100 * ((i + c) % 10) for c in range(C)]        # +-full scale stays +-full scale
    cmap = None
    if map_kind != "identity":
        r = 1 + i % (C - 1)
        cmap = [(c + r) % C for c in range(C)]                         # output c takes input cmap[c]
        if map_kind == "duplicate":
            cmap[(cmap.index(ch) + 1) % C] = ch
    return ch, gain_kind, gains, map_kind, cmap


def _case(cases, C, kind, at, pieces, what):
    """pieces: "take", or (n, past) -- a run that takes the stream's next n frames, with `past` more frames of the
    stream uploaded behind them, inside the slot and beyond the count"""
    i = len(cases)
    ch, gain_kind, gains, map_kind, cmap = _rotation(i, C)
    counted = sum(p[0] for p in pieces if p != "take")
    held = counted + sum(p[1] for p in pieces if p != "take")
    raw = _plant(max(held, at + 12), C, ch, at)
    steps, pos = [], 0
    for p in pieces:
        if p == "take":
            steps.append(("take",))
        else:
            n, past = p
            steps.append(("run", raw[pos * C:(pos + n + past) * C].copy(), n))
            pos += n
    assert all(st[0] == "take" or st[1].size // C <= max_frames(C) for st in steps), what
    cases.append(dict(index=i, C=C, kind=kind, what=what, ch=ch, at=at, frames=counted,
                      inside=max(0, min(12, counted - at)), gain_kind=gain_kind, gains=gains, map_kind=map_kind,
                      cmap=cmap, steps=steps,
                      planted=[c for c in range(C) if (cmap[c] if cmap else c) == ch]))


_TABLES = {}


def table(C):
    """the cases of channel count C (built once)"""
    if C in _TABLES:
        return _TABLES[C]
    geo = geometry(C)
    tile = geo["tile"]
    cases = []
    # pos: one run, the pattern at every start in a band around each edge and through the end of the run
    total = max_frames(C)
    starts = set(range(total - 12 - 44, total - 12 + 1))
    for edge in [0, tile, 2 * tile] + [k * e for e in geo["inner"] for k in (1, 2)]:
        starts |= set(range(edge - 30, edge + 20))
    for at in sorted(a for a in starts if 0 <= a and a + 12 <= total):
        _case(cases, C, "pos", at, [(total, 0), "take"], ("pos", at))
    # count: the pattern's last frame is the last frame of the count
    for n in (12, 13, 15, 16, 17, 31, 32, 33, tile - 1, tile, tile + 1, tile + 15, tile + 16, tile + 17,
              2 * tile - 1, 2 * tile, 2 * tile + 1):
        _case(cases, C, "count", n - 12, [(n, 0), "take"], ("count", n))
    # decoy: the first k frames of the pattern are the stream's, the rest lies past the count inside the slot
    for n in (1, 5, 13, 17, 31, 33, tile - 1, tile + 1, tile + 15, tile + 17, 2 * tile - 1, 2 * tile + 1):
        for k in (0, 1, 6, 11):
            if k <= n:
                _case(cases, C, "decoy", n - k, [(n, 12 - k), "take"], ("decoy", n, k))
    # split: the first `cut` frames of the pattern end one run, the rest start the next
    for lead in (0, 1, 10, 11, 12, tile - 5, tile, tile + 3):
        for cut in range(1, 12):
            first, second = (lead + cut, 0), (12 - cut, 0)
            _case(cases, C, "split", lead, [first, second, "take"], ("split", lead, cut))
            if cut % 3 == 1:
                _case(cases, C, "split", lead, [first, (0, 0), second, "take"], ("split, 0-frame run", lead, cut))
                _case(cases, C, "split", lead, [first, "take", second, "take"], ("split, take", lead, cut))
    # dribble: the pattern in pieces shorter than the history, from zero history and after a run of 20 frames
    for parts in ([1] * 12, [5, 5, 2], [3, 1, 8], [10, 1, 1], [2, 10]):
        for before in (0, 20):
            pieces = ([(before, 0)] if before else []) + [(k, 0) for k in parts] + ["take"]
            _case(cases, C, "dribble", before, pieces, ("dribble", tuple(parts), before))
    _TABLES[C] = cases
    return cases


# ---------------------------------------------------------------------------
# expected values


def oracle_gain(orc, C, gains):
    if gains is None:
        return of.Gain()
    rc, g = orc.gain(C, C, SCALE, gains)
    assert rc == 0
    return g


def transform(orc, raw, C, g, cmap):
    x = np.asarray(raw, dtype=np.int16)
    if x.size == 0:
        return x
    if cmap is not None:
        x = orc.chmap(cmap, x, C)
    return orc.gain_apply(g, x, C)


_SIGNALS = {}


def signals(orc, C):
    """per case and run step (transformed, raw, gain without map) of what the slot holds; kept for one channel
    count at a time"""
    if C not in _SIGNALS:
        out = []
        for case in table(C):
            g = oracle_gain(orc, C, case["gains"])
            steps = []
            for st in case["steps"]:
                if st[0] == "take":
                    steps.append(None)
                    continue
                y = transform(orc, st[1], C, g, case["cmap"])
                steps.append((y, st[1], y if case["cmap"] is None else transform(orc, st[1], C, g, None)))
            out.append(steps)
        _SIGNALS.clear()
        _SIGNALS[C] = out
    return _SIGNALS[C]


_EXPECTED = {}


def expected(cm, orc, C, fault=None):
    """per case the list of its takes, (peaks per channel, frames): the model's, left unchanged by the callers"""
    if (C, fault) not in _EXPECTED:
        H = cm.tp_coefficients().astype(np.int64)
        out = []
        for case, sig in zip(table(C), signals(orc, C)):
            m = EdgeModel(H, C, fault)
            takes = []
            for st, tr in zip(case["steps"], sig):
                if st[0] == "take":
                    takes.append(m.take())
                else:
                    m.run(tr[0], st[2], tr[1], tr[2])
            out.append(takes)
        _EXPECTED[(C, fault)] = out
    return _EXPECTED[(C, fault)]


# ---------------------------------------------------------------------------
# the tests


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_truepeak_edges",
                                                  os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pattern_and_geometry(cm):
    H = cm.tp_coefficients().astype(np.int64)
    assert H[1].tolist() == P1
    r = response(H, WORST_PATTERN)
    assert int(r.max()) == WORST == int(np.abs(H).sum(axis=1).max()) * 32768 - int(H[1][H[1] > 0].sum())
    assert np.flatnonzero(r == WORST).tolist() == [11]                     # at the pattern's last frame, only there
    # the constants of csrc/k_tpeak.hip that the table is built around
    src = open(os.path.join(ROOT, "libcoolmic-dsp_amd", "csrc", "k_tpeak.hip")).read()
    for text in ("TP_ANY_FRAMES = 1024;", "TP_ANY_RUN = 16;", "TP_U = 8;", "TP_TILE_VEC = 64 * TP_U;"):
        assert text in src, text
    assert geometry(3) == geometry(16) == dict(tile=1024, inner=(16,), halo=16, unit=16)
    assert geometry(1) == dict(tile=4096, inner=(64, 8), halo=64, unit=8)  # 8 KiB, 128 bytes, 16 bytes of mono
    assert geometry(2) == dict(tile=2048, inner=(32, 4), halo=32, unit=4)
    for C in CHANNELS:
        p = cm.plan_tpeak(1, C, max_frames(C))
        assert p.chunks == 3 and p.fast == (1 if C <= 2 else 0)            # two whole tiles and a ragged third


@pytest.mark.parametrize("C", CHANNELS)
def test_table_covers_every_edge_with_every_rotation(C):
    cases = table(C)
    geo = geometry(C)
    tile, total = geo["tile"], max_frames(C)
    by_kind = {k: [c for c in cases if c["kind"] == k] for k in KINDS}
    print(f"C={C:2d}: {len(cases)} cases, " + ", ".join(f"{k} {len(v)}" for k, v in by_kind.items()))
    assert 380 <= len(cases) <= 520
    assert max(len(c["steps"]) for c in cases) == 14
    # pos: the pattern's last frame on both sides of every edge, and on the run's last frame
    lasts = {c["at"] + 11 for c in by_kind["pos"]}
    for edge in (tile, 2 * tile) + tuple(k * e for e in geo["inner"] for k in (1, 2)):
        assert set(range(max(11, edge - 12), edge + 12)) <= lasts, edge
    assert {11, total - 1} <= lasts and all(c["frames"] == total for c in by_kind["pos"])
    # count, decoy: ends in every residue class the inner unit makes a difference for
    ends = {c["frames"] for c in by_kind["count"]}
    assert {n % geo["unit"] for n in ends} >= {0, 1, geo["unit"] - 1} and {n // tile for n in ends} == {0, 1, 2}
    assert all(c["inside"] == 12 and c["at"] + 12 == c["frames"] for c in by_kind["count"])
    assert all(c["frames"] % geo["unit"] for c in by_kind["decoy"])    # none ends a unit: room to overcount
    assert {c["inside"] for c in by_kind["decoy"]} == {0, 1, 6, 11}
    for c in by_kind["decoy"]:
        run = c["steps"][0]
        assert run[2] == c["frames"] and run[1].size // C == c["frames"] + 12 - c["inside"] <= total
    # split, dribble: the whole pattern inside the counts, runs of fewer than 11 frames among them
    assert all(c["inside"] == 12 for k in ("pos", "split", "dribble") for c in by_kind[k])
    assert sum(any(st[0] == "run" and st[2] == 0 for st in c["steps"]) for c in by_kind["split"]) == 32
    assert sum(len([st for st in c["steps"] if st[0] == "take"]) == 2 for c in by_kind["split"]) == 32
    assert any(st[0] == "run" and st[2] > tile for c in by_kind["split"] for st in c["steps"])
    # the rotation: every channel, every kind of gain and every kind of map meet every kind of case
    for kind, lst in by_kind.items():
        assert len({c["ch"] for c in lst}) >= min(C, len(lst)), kind
        assert {c["gain_kind"] for c in lst} == set(GAIN_KINDS), kind
        assert {c["map_kind"] for c in lst} == (set(MAP_KINDS) if C > 1 else {"identity"}), kind
        if C > 1 and len(lst) >= 40:
            pairs = {(c["gain_kind"], c["map_kind"]) for c in lst}
            assert pairs == {(g, m) for g in GAIN_KINDS for m in MAP_KINDS}, kind
    for c in cases:
        if c["map_kind"] == "identity":
            assert c["cmap"] is None and c["planted"] == [c["ch"]]
        elif c["map_kind"] == "permutation":
            assert sorted(c["cmap"]) == list(range(C)) and c["cmap"] != list(range(C)) and len(c["planted"]) == 1
        else:
            assert len(c["planted"]) == 2 and len(set(c["cmap"])) == C - 1
        if c["gain_kind"] == "below":
            assert all(0 < g < SCALE for g in c["gains"])
        elif c["gain_kind"] == "saturating":
            assert all(SCALE < g <= 65535 for g in c["gains"])


@pytest.mark.parametrize("C", CHANNELS)
def test_every_take_pins_one_output(cm, oracle, C):
    """a non-zero peak on the planted output channels and exactly 0 elsewhere; with the whole pattern inside the count
    and no gain or a saturating one the literal 542986257, which the model attains at exactly one frame"""
    H = cm.tp_coefficients().astype(np.int64)
    literal = 0
    for case, takes, sig in zip(table(C), expected(cm, oracle, C), signals(oracle, C)):
        assert len(takes) == sum(st[0] == "take" for st in case["steps"]) >= 1
        assert sum(fr for _, fr in takes) == case["frames"] and all(fr > 0 for _, fr in takes), case["what"]
        for peaks, _ in takes:
            for c in range(C):
                if c not in case["planted"]:
                    assert peaks[c] == 0, (case["what"], c)
                elif case["inside"]:
                    assert peaks[c] > 0, (case["what"], c)
                else:                              # a decoy with all 12 frames past the count: silence
                    assert case["kind"] == "decoy" and peaks[c] == 0, (case["what"], c)
        if case["inside"] == 12 and case["gain_kind"] != "below":
            y = np.concatenate([tr[0][:st[2] * C] for st, tr in zip(case["steps"], sig) if st[0] == "run"])
            for c in case["planted"]:
                assert max(p[c] for p, _ in takes) == WORST and takes[-1][0][c] == WORST, case["what"]
                assert np.flatnonzero(response(H, y[c::C]) == WORST).tolist() == [case["at"] + 11], case["what"]
            literal += 1
        elif case["inside"] == 12:
            assert all(0 < takes[-1][0][c] < WORST for c in case["planted"]), case["what"]
    assert literal >= len(table(C)) // 2


@pytest.mark.parametrize("C", [1, 2, 3, 6])
def test_model_is_the_model_of_the_random_tests(cm, oracle, C):
    """without a fault, EdgeModel is `Model` of tests/test_gpu_truepeak.py on the same transformed samples"""
    TG = _load("test_gpu_truepeak")
    assert TG.WORST == WORST and np.array_equal(TG.WORST_PATTERN, WORST_PATTERN)
    assert np.array_equal(TG.H, cm.tp_coefficients())
    want = expected(cm, oracle, C)
    for case, sig in list(zip(table(C), signals(oracle, C)))[::5]:
        m = TG.Model(C)
        takes = []
        for st, tr in zip(case["steps"], sig):
            if st[0] == "take":
                takes.append(m.take())
            else:
                m.run(tr[0][:st[2] * C])
        assert takes == want[case["index"]], case["what"]


@pytest.mark.parametrize("C", SWEEP)
def test_every_fault_changes_some_case(cm, oracle, C):
    """each fault a kernel could have changes the expected result of at least 3 cases: the device test, which
    compares every case exactly, would fail on it"""
    base = expected(cm, oracle, C)
    kernel = "k_tpeak_any" if C >= 3 else "k_tpeak_fast"
    for fault in FAULTS:
        got = expected(cm, oracle, C, fault)
        caught = [case for case, a, b in zip(table(C), base, got) if a != b]
        kinds = {k: sum(c["kind"] == k for c in caught) for k in KINDS}
        print(f"C={C:2d} {kernel:12s} {fault:14s} caught by {len(caught):3d} of {len(base)} cases "
              + " ".join(f"{k}={v}" for k, v in kinds.items() if v))
        if C == 1 and fault == "hist_nomap":       # mono has no map but the identity: there is no such kernel
            assert not caught
        else:
            assert len(caught) >= 3, (C, fault)
        del _EXPECTED[(C, fault)]                  # (only the fault-free values are shared)
