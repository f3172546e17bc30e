"""GPU: sample-rate conversion (cmhip_src_*, csrc/k_src.hip) through the C ABI and the Python mirror.

Bar: bit-exact against the numpy model below of the arithmetic include/coolmic_hip.h specifies -- int64, per-stream
history and r -- never another run of the device code.  Tables are taken from the library (cmhip_src_design), or are
the test's own where the test is about a table: the designed tables are windowed sincs whose outer taps are next to
nothing (at 48000 -> 8000 the first and last six are zero), so whatever a kernel does wrong at the ends of the filter
-- the oldest history frames, the oldest frames of a tile's halo, the last tap pair -- adds nothing to their sums.
dense_table() gives every tap weight; CASES lists the geometries that reach each staging path of the kernel, with
the property that makes a case reach its path asserted from plan_src and host arithmetic (tests/test_src_host.py
runs the same list through its emulation of the kernel, without a GPU).
"""
import os
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
SENTINEL = -21555                                 # what the output slots hold before a run


class Model:
    """one stream: y[m] = sat16((sum_k H[p][k] x[n-k] + 8192) >> 14), n = floor(m M / L), p = m M mod L"""

    def __init__(self, L, M, H, channels):
        self.L, self.M, self.H, self.C = L, M, np.asarray(H, dtype=np.int64), channels
        self.T = self.H.shape[1]
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.T - 1, self.C), dtype=np.int64)
        self.r = 0

    def run(self, x):
        """x: int16 [F][C] (or flat interleaved) -> int16 [K][C]"""
        L, M, T = self.L, self.M, self.T
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.C)
        F = x.shape[0]
        z = np.concatenate([self.hist, x])
        m = np.arange(-(-self.r * L // M), -(-(self.r + F) * L // M), dtype=np.int64)
        n = m * M // L - self.r                                  # the run's frame that output m reads
        p = (m * M) % L
        assert m.size == 0 or (n.min() >= 0 and n.max() < F)
        y = np.zeros((m.size, self.C), dtype=np.int64)
        for lo in range(0, m.size, 2048):                        # (in pieces: [K][T][C] gets large)
            sl = slice(lo, lo + 2048)
            idx = (T - 1) + n[sl, None] - np.arange(T)[None, :]
            acc = np.einsum("kt,ktc->kc", self.H[p[sl]], z[idx])
            assert np.abs(acc + 8192).max() < 2 ** 31
            y[sl] = np.clip((acc + 8192) >> 14, -32768, 32767)
        self.hist = z[z.shape[0] - (T - 1):]
        self.r = (self.r + F) % M
        return y.astype(np.int16)


def lcg(seed, n):
    """the engine's noise: st = st * 1664525 + 1013904223, sample = st >> 16 as int16"""
    out = np.empty(n, dtype=np.int16)
    st = seed & 0xFFFFFFFF
    for i in range(n):
        st = (st * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = ((st >> 16) ^ 0x8000) - 0x8000
    return out


def noise(seed, frames, channels):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(frames, channels)).astype(np.int16)
    x[rng.integers(0, max(frames, 1), size=frames // 16)] = 32767           # full-scale frames here and there
    x[rng.integers(0, max(frames, 1), size=frames // 16)] = -32768
    return x


_tables = {}


def table(cm, rate_in, rate_out):
    if (rate_in, rate_out) not in _tables:
        _tables[(rate_in, rate_out)] = cm.src_design(rate_in, rate_out)
    return _tables[(rate_in, rate_out)]


class Rig:
    """a resampler between two arrays of pinned, device-mapped host memory, and one model per stream"""

    def __init__(self, cm, streams, channels, L, M, H, max_in, rates=(44100, 48000)):
        self.cm, self.S, self.C, self.L, self.M = cm, streams, channels, L, M
        self.H = np.asarray(H, dtype=np.int16)
        self.r = cm.Resampler(streams, channels, rates[0], rates[1], max_in, table=(L, M, self.H))
        assert self.r.geometry() == (L, M, self.H.shape[1])
        self.max_out = self.r.max_out_frames()
        assert self.max_out == max_in * L // M + 1
        self.in_stride = (max_in * channels + 7) // 8 * 8
        self.out_stride = (self.max_out * channels + 7) // 8 * 8 + 8
        self.src = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.in_stride))
        self.dst = cm.MappedPcm(types.SimpleNamespace(streams=streams, stride=self.out_stride))
        self.models = [Model(L, M, H, channels) for _ in range(streams)]
        self.samples = self.saturated = 0                        # of the models' outputs so far

    def saturated_share(self):
        return self.saturated / max(self.samples, 1)

    def close(self):
        self.r.close()
        self.src.free()
        self.dst.free()

    def run(self, xs, frames=None, uniform=False):
        """xs: per stream int16 [F_s][C]; runs device and models, compares counts, outputs and the untouched rest"""
        counts = [np.asarray(x).reshape(-1, self.C).shape[0] for x in xs]
        frames = max(counts) if frames is None else frames
        self.src.array[:] = 0x5a5a
        for s, x in enumerate(xs):
            self.src.array[s, :counts[s] * self.C] = np.asarray(x, dtype=np.int16).reshape(-1)
        self.dst.array[:] = SENTINEL
        got = self.r.run(self.src.dev, self.in_stride, frames, self.dst.dev, self.out_stride,
                         None if uniform else counts)
        self.r.sync()
        outs = []
        for s, x in enumerate(xs):
            want = self.models[s].run(x)
            assert got[s] == want.shape[0], (s, got[s], want.shape[0])
            n = want.size
            self.samples += n
            self.saturated += int(((want == 32767) | (want == -32768)).sum())
            have = self.dst.array[s, :n].reshape(-1, self.C)
            bad = np.argwhere(have != want)
            assert bad.size == 0, ("stream", s, "first mismatch (frame, channel)", bad[0].tolist(),
                                   "got", int(have[tuple(bad[0])]), "want", int(want[tuple(bad[0])]))
            assert (self.dst.array[s, n:] == SENTINEL).all(), ("stream", s, "written past its count")
            outs.append(have.copy())
        return outs

    def reset(self, stream=-1):
        self.r.reset(stream)
        for s in (range(self.S) if stream < 0 else [stream]):
            self.models[s].reset()


# ---------------------------------------------------------------------------
# dense tables, and the cases that reach every staging path

SATURATED_MAX = 0.10              # of a dense case's outputs in the MODEL: a saturated output hides a wrong sum


def dense_table(L, T, seed):
    """int16 [L][T] with weight at every tap: |h| in [3B/4, B], B = min(65535 // T, 4096), random signs, no two phases
    alike.  sum |h| <= 65535 per phase (what the library asks of a table); the phases do not sum to 16384."""
    B = min(65535 // T, 4096)
    rng = np.random.default_rng(seed)
    while True:
        H = rng.integers(-(-3 * B // 4), B + 1, size=(L, T)) * rng.choice([-1, 1], size=(L, T))
        if len({row.tobytes() for row in H}) == L:
            break
    assert int(np.abs(H).min()) >= 3 * B / 4 and int(np.abs(H).sum(axis=1).max()) <= 65535
    return H.astype(np.int16)


def ragged(F, T):
    """per-stream counts of one run: a full stream, one with nothing, one frame, T - 2 frames, F - 1 frames"""
    return [F, 0, 1, T - 2, F - 1]


def _case(name, geometry, channels, runs, table="dense", rates=None, plan=None, reach=()):
    """runs: per run the streams' frame counts.  plan: the SrcPlan fields the case relies on, for its longest run.
    reach: what tile_facts() must find (REACH)."""
    L, M, T = geometry
    return types.SimpleNamespace(name=name, L=L, M=M, T=T, C=channels, runs=runs, table=table, rates=rates,
                                 plan=dict(plan or {}), reach=tuple(reach))


def _twice(counts):
    return [counts, counts[::-1]]


def _rotated(counts):
    """two streams: the list, and the list rotated by one run -- different r and fill of the history per run"""
    return [list(c) for c in zip(counts, counts[1:] + counts[:1])]


CASES = []
# 1. 11025 -> 48000 as designed: 640 x 40 x 2 = 51200 bytes of table, read from global memory; 8708 outputs in three
# tiles
for _c in (1, 2, 3, 16):
    CASES.append(_case("global-designed-c%d" % _c, (640, 147, 32), _c, _twice(ragged(2000, 32)), "designed",
                       (11025, 48000), dict(table_lds=0, tile_out=4096, chunks=3),
                       ("lds60000",) if _c == 16 else ()))
# 2. 44100 -> 32000: the padded table is exactly the 46080 bytes a table in LDS may have
for _t in ("designed", "dense"):
    CASES.append(_case("bound-%s-c2" % _t, (320, 441, 64), 2, _twice(ragged(3000, 64)), _t, (44100, 32000),
                       dict(table_lds=1, tile_out=1024, lds_bytes=57888, chunks=3)))
    CASES.append(_case("bound-%s-c16" % _t, (320, 441, 64), 16, _twice(ragged(600, 64)), _t, (44100, 32000),
                       dict(table_lds=1, tile_out=128, lds_bytes=61568, chunks=4), ("lds60000",)))
# 3. the halo reaches behind the previous tile: a tile of 4096 outputs covers 6.4 (25.6, 17.9) input frames
for _c, _T in ((1, 192), (2, 192), (16, 192), (3, 190)):
    CASES.append(_case("halo-640x%d-c%d" % (_T, _c), (640, 1, _T), _c, _rotated([14, 1, 0, 14, 40]),
                       plan=dict(table_lds=0, tile_out=4096), reach=("halo",)))
CASES.append(_case("halo-160x32-c2", (160, 1, 32), 2, _rotated([60, 1, 0, 60]), plan=dict(table_lds=1, tile_out=4096),
                   reach=("halo", "mix", "clear")))
CASES.append(_case("halo-229x30-c1", (229, 1, 30), 1, _rotated([60, 1, 0, 60]), plan=dict(table_lds=1, tile_out=4096),
                   reach=("halo", "mix")))
# 4. the reciprocal's range (t = p0 + q M up to 2.6e6, inv = 2^31, inv = 0) and the small ends (T = 2, tiles of 2 and 8)
# (five channels beside the table of 639 phases leave room for tiles of 1024 only: t goes up to 1023 * 640 there)
for _c, _g, _tile in ((2, (640, 639, 6), 4096), (1, (639, 640, 10), 4096), (5, (639, 640, 10), 1024)):
    CASES.append(_case("divmod-%dx%d-c%d" % (_g[0], _g[1], _c), _g, _c, [[5] * 5] + _twice(ragged(9000, _g[2])),
                       plan=dict(table_lds=1, tile_out=_tile), reach=("t21" if _tile == 4096 else "tfull",)))
CASES.append(_case("divmod-2x3-c2", (2, 3, 2), 2, _twice(ragged(13000, 2)), plan=dict(table_lds=1, tile_out=4096)))
for _c, _tile in ((2, 8), (16, 2)):
    CASES.append(_case("divmod-1x640-c%d" % _c, (1, 640, 192), _c, _twice(ragged(12800, 192)),
                       plan=dict(table_lds=1, tile_out=_tile), reach=("tile8",)))


def case_table(cm, case):
    if case.table == "designed":
        L, M, T, H = table(cm, *case.rates)
        assert (L, M, T) == (case.L, case.M, case.T)
        return H
    return dense_table(case.L, case.T, 1000 + case.L + case.T)


def tile_facts(cm, case):
    """-> (the plan of the longest run, one record per run, stream and tile: j_lo, the first frame the tile stages as
    the kernel computes it, t_hi, the largest t = p0 + q M it hands to src_divmod, and whether the tile is the
    stream's first in its run) from plan_src and host arithmetic alone"""
    L, M, T, Tp = case.L, case.M, case.T, (case.T + 7) // 8 * 8
    S = len(case.runs[0])
    r, recs, longest = [0] * S, [], None
    for i, counts in enumerate(case.runs):
        K = [cm.src_out_frames(L, M, r[s], counts[s]) for s in range(S)]
        plan = cm.plan_src(S, case.C, L, M, T, max(K) or 1)      # (cmhip_src_run: at least one workgroup per stream)
        assert plan.err == 0 and plan.grid == S * plan.chunks
        if longest is None or plan.chunks > longest.chunks:
            longest = plan
        for s in range(S):
            kb = -(-r[s] * L // M)
            for q0 in range(0, K[s], plan.tile_out):
                nq = min(plan.tile_out, K[s] - q0)
                n0, p0 = divmod((kb + q0) * M, L)
                recs.append(types.SimpleNamespace(run=i, stream=s, first=q0 == 0, j_lo=n0 - r[s] - (Tp - 1),
                                                  t_hi=p0 + (nq - 1) * M))
            r[s] = (r[s] + counts[s]) % M
    return longest, recs


REACH = {
    "lds60000": lambda case, plan, recs: plan.lds_bytes > 60000,
    # a tile after the stream's first stages frames from before the run
    "halo": lambda case, plan, recs: any(not t.first and t.j_lo < 0 for t in recs),
    # ... and it stages history frames AND frames of the run
    "mix": lambda case, plan, recs: any(not t.first and -(case.T - 1) < t.j_lo < 0 for t in recs),
    # ... and another one stages no history at all
    "clear": lambda case, plan, recs: any(not t.first and t.j_lo >= 0 for t in recs),
    "t21": lambda case, plan, recs: max(t.t_hi for t in recs) >= 1 << 21,
    # the largest t the plan's tile can give: a whole tile
    "tfull": lambda case, plan, recs: max(t.t_hi for t in recs) >= (plan.tile_out - 1) * case.M,
    "tile8": lambda case, plan, recs: plan.tile_out <= 8 and plan.chunks >= 3,
}


def assert_reaches(cm, case):
    """the case reaches what it is there for, or fails loudly (a planner that changed, say)"""
    plan, recs = tile_facts(cm, case)
    assert max(t.t_hi for t in recs) < 1 << 22                   # (what src_divmod is exact for)
    assert plan.lds_bytes <= 65536
    assert plan.fast == (1 if case.C <= 2 else 0)
    for field, want in case.plan.items():
        assert getattr(plan, field) == want, (case.name, field, getattr(plan, field), want)
    for what in case.reach:
        assert REACH[what](case, plan, recs), (case.name, what)
    return plan, recs


def run_case(cm, case):
    assert_reaches(cm, case)
    H = case_table(cm, case)
    S = len(case.runs[0])
    rig = Rig(cm, S, case.C, case.L, case.M, H, max(max(c) for c in case.runs))
    for i, counts in enumerate(case.runs):
        xs = [noise(1000 * i + 10 * case.C + s, n, case.C) for s, n in enumerate(counts)]
        rig.run(xs, frames=max(max(counts), 1))
    share = rig.saturated_share()
    print("src case", case.name, "outputs", rig.samples, "saturated in the model %.4f" % share)
    if case.table == "dense":
        assert share < SATURATED_MAX
    rig.close()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_staging_paths(gpu, case):
    run_case(gpu, case)


def test_many_streams_and_uniform_counts(gpu):
    """300 stereo streams: the indexing of history, r, slots and grid by the stream, and nframes == NULL with S > 1"""
    S, F = 300, 64
    rig = Rig(gpu, S, 2, 3, 2, dense_table(3, 8, 5), F)
    rig.run([noise(3000 + s, F, 2) for s in range(S)], uniform=True)
    counts = [s % 65 for s in range(S)]
    assert max(counts) == F and min(counts) == 0
    rig.run([noise(4000 + s, n, 2) for s, n in enumerate(counts)], frames=F)
    assert len({m.r for m in rig.models}) == 2 and rig.saturated_share() < SATURATED_MAX
    rig.close()


# ---------------------------------------------------------------------------
# 1. an adversarial table: saturation both ways, the largest |acc|, rounding of negative sums

ADV = np.array([[32767, -32767, 1, 0], [-32767, 1, 32767, 0], [16384, 16383, -16384, -16384]], dtype=np.int16)


def test_adversarial_table(gpu):
    assert int(np.abs(ADV.astype(np.int64)).sum(axis=1).max()) == 65535
    rig = Rig(gpu, 1, 1, 3, 2, ADV, 4096)
    alt = np.where(np.arange(4096) % 2 == 0, 32767, -32768).astype(np.int16)
    ramp = (np.arange(4096) * 16 - 32768).astype(np.int16)
    small = ((np.arange(4096) * 7) % 23 - 11).astype(np.int16)              # sums around zero, both signs
    lowest, highest = 0, 0
    for name, x in (("alternating", alt), ("inverted", (-1 - alt.astype(np.int32)).astype(np.int16)), ("ramp", ramp),
                    ("small", small), ("noise", lcg(12345, 4096))):
        rig.reset()
        # what this input exercises, from the specification's sums
        z = np.concatenate([np.zeros(3, dtype=np.int64), x.astype(np.int64)])
        mm = np.arange(0, -(-4096 * 3 // 2))
        acc = (ADV.astype(np.int64)[(mm * 2) % 3] * z[3 + (mm * 2 // 3)[:, None] - np.arange(4)[None, :]]).sum(axis=1)
        y = rig.run([x.reshape(-1, 1)])[0]
        print("src adversarial", name, "max |acc|", int(np.abs(acc).max()), "min", int(y.min()), "max", int(y.max()),
              "negative unrounded sums", int(((acc + 8192 < 0) & ((acc + 8192) % 16384 != 0)).sum()))
        if name == "alternating":
            assert int(np.abs(acc).max()) >= 65534 * 32767       # the largest |acc| the bound allows, within a step
        lowest, highest = min(lowest, int(y.min())), max(highest, int(y.max()))
        if name in ("small", "noise", "ramp"):
            assert ((acc + 8192 < 0) & ((acc + 8192) % 16384 != 0)).any()
    assert (lowest, highest) == (-32768, 32767)                  # saturated both ways
    rig.close()


# ---------------------------------------------------------------------------
# 2. the designed tables, every channel form, ragged per-stream counts in one run

@pytest.mark.parametrize("channels", [1, 2, 3, 6, 16])
@pytest.mark.parametrize("rates", [(44100, 48000), (48000, 44100), (8000, 48000), (48000, 8000)])
def test_designed_tables(gpu, rates, channels):
    L, M, T, H = table(gpu, *rates)
    assert (L, M, T) == {(44100, 48000): (160, 147, 32), (48000, 44100): (147, 160, 64), (8000, 48000): (6, 1, 32),
                         (48000, 8000): (1, 6, 192)}[rates]
    F = 1500
    rig = Rig(gpu, 5, channels, L, M, H, F, rates)
    counts = [F, 0, 1, T - 2, F - 1]
    rig.run([noise(100 * channels + s, n, channels) for s, n in enumerate(counts)], frames=F)
    # and once more on top of that history, from five different r
    rig.run([noise(200 * channels + s, n, channels) for s, n in enumerate(counts[::-1])], frames=F)
    rig.close()


# ---------------------------------------------------------------------------
# 3. the output does not depend on how the stream was cut into runs

def _table_of(cm, rates, dense):
    """the designed table of a pair of rates, or a dense one of the same (L, M, T)"""
    L, M, T, H = table(cm, *rates)
    return L, M, T, dense_table(L, T, L + T) if dense else H


CUTTING = [((44100, 48000), 1), ((48000, 44100), 2), ((48000, 8000), 3)]


def _cutting(gpu, rates, channels, dense):
    L, M, T, H = _table_of(gpu, rates, dense)
    plan = gpu.plan_src(1, channels, L, M, T, 1 << 20)
    total = 3 * M + 5 + 2 * plan.tile_in
    rig = Rig(gpu, 1, channels, L, M, H, total, rates)
    x = noise(7, total, channels)
    whole = rig.run([x], uniform=True)[0]
    rig.reset()
    cuts, pos, pieces, wraps = [1, 7, T - 2, 0, T - 1, T], 0, [], 0
    for n in cuts + [total - sum(cuts)]:
        before = rig.models[0].r
        pieces.append(rig.run([x[pos:pos + n]], frames=max(n, 1))[0])      # (n == 0: a run that hands the stream nothing)
        wraps += (before + n) // M
        pos += n
    assert pos == total and wraps >= 3
    assert np.array_equal(np.concatenate(pieces), whole)
    assert not dense or rig.saturated_share() < SATURATED_MAX
    rig.close()


@pytest.mark.parametrize("rates,channels", CUTTING)
def test_cutting(gpu, rates, channels):
    _cutting(gpu, rates, channels, False)


@pytest.mark.parametrize("rates,channels", CUTTING)
def test_cutting_dense(gpu, rates, channels):
    _cutting(gpu, rates, channels, True)


# ---------------------------------------------------------------------------
# 4. tile edges: exactly tile_out - 1, tile_out, tile_out + 1 and 2 tile_out + 1 output frames

def _reach(cm, L, M, want):
    """(r, F): a stream at position r that gets F frames produces exactly `want` output frames"""
    for r in ((want * 7 + 1 + i) % M for i in range(M)):         # (any r will do: a different one per count)
        F = want * M // L
        for f in range(max(F - 2, 0), F + 3):
            if cm.src_out_frames(L, M, r, f) == want:
                return r, f
    raise AssertionError((L, M, want))


TILE_EDGES = [((44100, 48000), 1), ((48000, 44100), 2), ((44100, 48000), 2), ((48000, 8000), 3)]


def _tile_edges(gpu, rates, channels, dense):
    L, M, T, H = _table_of(gpu, rates, dense)
    plan = gpu.plan_src(1, channels, L, M, T, 1 << 20)
    assert plan.fast == (1 if channels <= 2 else 0)
    tile = plan.tile_out
    wants = [tile - 1, tile, tile + 1, 2 * tile + 1]
    reach = [_reach(gpu, L, M, w) for w in wants]
    rig = Rig(gpu, len(wants), channels, L, M, H, max(max(f for _, f in reach), M), rates)
    rig.run([noise(40 + s, r, channels) for s, (r, _) in enumerate(reach)], frames=M)       # puts every stream at its r
    assert [m.r for m in rig.models] == [r for r, _ in reach]
    outs = rig.run([noise(50 + s, f, channels) for s, (_, f) in enumerate(reach)])
    assert [o.shape[0] for o in outs] == wants
    assert not dense or rig.saturated_share() < SATURATED_MAX
    rig.close()


@pytest.mark.parametrize("rates,channels", TILE_EDGES)
def test_tile_edges(gpu, rates, channels):
    _tile_edges(gpu, rates, channels, False)


@pytest.mark.parametrize("rates,channels", TILE_EDGES)
def test_tile_edges_dense(gpu, rates, channels):
    _tile_edges(gpu, rates, channels, True)


# ---------------------------------------------------------------------------
# 5. reset

def _reset(gpu, dense):
    L, M, T, H = _table_of(gpu, (44100, 48000), dense)
    rig = Rig(gpu, 3, 2, L, M, H, 500)
    xs = [noise(60 + s, 333 + s, 2) for s in range(3)]
    first = rig.run(xs)
    rig.reset(1)                                                 # stream 1 alone: its neighbours go on
    again = rig.run(xs)
    assert np.array_equal(again[1], first[1])
    assert not np.array_equal(again[0][:T], first[0][:T])        # (history kept: the filter's start differs)
    rig.reset(-1)
    third = rig.run(xs)
    for s in range(3):
        assert np.array_equal(third[s], first[s])
    assert not dense or rig.saturated_share() < SATURATED_MAX
    rig.close()


def test_reset(gpu):
    _reset(gpu, False)


def test_reset_dense(gpu):
    _reset(gpu, True)


# ---------------------------------------------------------------------------
# 6. a constant comes out as the same constant once the history is full

def test_dc(gpu):
    L, M, T, H = table(gpu, 44100, 48000)
    rig = Rig(gpu, 1, 2, L, M, H, 2000)
    y = rig.run([np.full((2000, 2), 12345, dtype=np.int16)])[0]
    settled = -(-T * L // M) + 1
    assert (y[settled:] == 12345).all() and y.shape[0] > 2000
    assert (y[0] != 12345).all()
    rig.close()


# ---------------------------------------------------------------------------
# 7. composition: straight into a 48 kHz batch's slots, on the batch's stream

def _check_batch(cm, oracle, b, models_out, counts):
    from oracle import oracle_ffi
    res, rcs = b.vu_results()
    _, g = oracle.gain(2, 2, 1000, [750, 1250])
    for s, y in enumerate(models_out):
        want = oracle.gain_apply(g, oracle.chmap([1, 0], y.reshape(-1), 2), 2)
        v = oracle.vu_new(2)
        oracle.vu_accumulate(v, want)
        _, r = oracle.vu_result(v)
        assert rcs[s] == 0 and oracle_ffi.vu_result_dict(r) == res[s].as_dict(), s
        assert res[s].frames == counts[s] and res[s].rate == 48000
        yield s, want


def test_composition_into_a_batch(gpu, oracle):
    cm = gpu
    L, M, T, H = table(cm, 44100, 48000)
    S, F = 4, 3000
    fps = [F, F - 1, 1234, 7]
    xs = [noise(70 + s, fps[s], 2) for s in range(S)]
    models = [Model(L, M, H, 2) for _ in range(S)]
    want = [m.run(x) for m, x in zip(models, xs)]
    src_b = cm.Batch(S, 2, F, flags=cm.VU, rate=44100)           # (device memory for the 44.1 kHz sources)
    for s in range(S):
        src_b.upload(s, xs[s])
    src_b.sync()
    max_out = F * L // M + 1
    # a batch with slots of its own
    b = cm.Batch(S, 2, max_out, flags=cm.OUT_PCM | cm.VU, rate=48000)
    assert b.set_gain(-1, 2, 1000, [750, 1250]) == 0 and b.set_chmap(-1, [1, 0]) == 0
    r = cm.Resampler(S, 2, 44100, 48000, F, hip_stream=b.hip_stream())
    assert r.hip_stream() == b.hip_stream() and r.max_out_frames() == max_out
    counts = r.run(src_b.dev_in, src_b.stride, F, b.dev_in, b.stride, fps)
    assert counts.tolist() == [w.shape[0] for w in want]
    b.run(int(counts.max()), counts)                             # (no sync between: the order is the stream's)
    for s, pcm in _check_batch(cm, oracle, b, want, counts):
        assert np.array_equal(b.download(s, int(counts[s])), pcm), s
    # the same through run_slots on a batch without slots
    e = cm.Batch(S, 2, max_out, flags=cm.OUT_PCM | cm.VU | cm.EXTSLOTS, rate=48000, hip_stream=b.hip_stream())
    assert e.set_gain(-1, 2, 1000, [750, 1250]) == 0 and e.set_chmap(-1, [1, 0]) == 0
    assert e.stride == b.stride
    slots_in, slots_out = cm.MappedPcm(e), cm.MappedPcm(e)
    r.reset()
    counts2 = r.run(src_b.dev_in, src_b.stride, F, slots_in.dev, e.stride, fps)
    assert counts2.tolist() == counts.tolist()
    e.run_slots(int(counts2.max()), slots_in.dev, slots_out.dev, counts2.tolist())
    e.sync()
    for s, pcm in _check_batch(cm, oracle, e, want, counts):
        assert np.array_equal(slots_out.array[s, :pcm.size], pcm), s
    r.close()
    for o in (b, e, src_b):
        o.close()
    slots_in.free()
    slots_out.free()


# ---------------------------------------------------------------------------
# 8. refusals launch nothing

def test_refusals(gpu):
    cm = gpu
    L, M, T, H = table(cm, 44100, 48000)
    rig = Rig(cm, 2, 2, L, M, H, 256)
    x = [noise(80 + s, 256, 2) for s in range(2)]
    rig.run(x)                                                   # some history and r to lose
    r, src, dst, si, so = rig.r, rig.src.dev, rig.dst.dev, rig.in_stride, rig.out_stride
    rig.dst.array[:] = SENTINEL
    cases = {
        "misaligned in": (src + 2, si, 256, dst, so, None),
        "misaligned out": (src, si, 256, dst + 8, so, None),
        "in stride not a multiple of 8": (src, si + 4, 256, dst, so, None),
        "out stride not a multiple of 8": (src, si, 256, dst, so - 4, None),
        "in stride too small": (src, 504, 256, dst, so, None),
        "out stride too small": (src, si, 256, dst, 8, None),
        "frames above max_in_frames": (src, si, 257, dst, so, None),
        "a count above frames": (src, si, 100, dst, so, [100, 101]),
        "in == out": (src, si, 256, src, so, None),
    }
    for name, (a, ast, n, o, ost, fps) in cases.items():
        rc, _ = r.run_rc(a, ast, n, o, ost, fps)
        assert rc == cm.ERROR_INVAL, name
    assert cm.lib.cmhip_src_run(r.h, None, si, 256, None, dst, so, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_src_run(r.h, src, si, 256, None, None, so, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_src_reset(r.h, 2) == cm.ERROR_INVAL
    r.sync()
    assert (rig.dst.array == SENTINEL).all()
    rig.run(x)                                                   # history and r are where the model's are
    rig.close()


# ---------------------------------------------------------------------------
# 9. the example

def test_batch_resample_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_resample"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_resample.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[0].startswith("44100 -> 48000: L 160 M 147 T 32")
    assert len(out) >= 3 and all(ln.startswith("stream ") for ln in out[1:])
    for ln in out[1:]:
        f = dict(kv.split("=") for kv in ln.split()[2:])
        assert int(f["frames"]) == 4800                          # 4410 frames at 44.1 kHz are 4800 at 48 kHz
        assert -3.2 < float(f["power"]) < -2.8 and -0.5 < float(f["dbtp"]) < 0.5     # a full-scale sine
