"""GPU: the signal watch (dead air, clipping, DC offset) through the batch ABI, the group, the Python mirror and the C
example.

Bar: equality.  Every integer of a result EQUALS the model's and every dc is bit-equal to the host formula evaluated
here.  The model is tests/watch_model.py -- the online definition in numpy on the transformed stream,
orc.gain_apply(g, orc.chmap(map, raw, C), C) -- never another run of the device code.

Geometry the sizes below sit on.  k_watch_fast gives one wave a tile of 512 16-byte vectors: 2048 stereo or 4096 mono
frames.  A lane loads the vectors lane, lane + 64, ... (a vector is 4 stereo / 8 mono frames, a row of 64 vectors 256 /
512 frames), the tile goes through LDS and comes back as words of 64 consecutive frames (mono: two words per dword, 128
frames), whose predicate masks are read run by run; a stream's tiles are folded in order by k_watch_fold.  The edges
are therefore the vector (4 / 8), the word (64; 128), the row (256 / 512) and the tile (2048 / 4096).  k_watch_any
gives a workgroup 1024 frames, a thread the frames t, t + 256, ..., a wave's ballot 64 of them.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle_ffi as of
from watch_model import KEYS, Watch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")
WORD, ANY_TILE = 64, 1024
GEOM = {1: dict(vec=8, row=512, tile=4096), 2: dict(vec=4, row=256, tile=2048)}


def _bits(x):
    return struct.pack("<d", x)


def _check(r, want, what=""):
    """a WatchResult against the model's window (a dict): integers equal, dc bit-equal, the rest of the arrays zero"""
    got = r.as_dict()
    print("watch", what, "got", {k: v for k, v in got.items() if k != "dc"})
    assert want is not None, what
    for k in want:
        if k != "dc":
            assert got[k] == want[k], (what, k, got[k], want[k])
    assert [_bits(v) for v in got["dc"]] == [_bits(v) for v in want["dc"]], (what, got["dc"], want["dc"])
    for k in KEYS:
        assert all(v == 0 for v in list(getattr(r, k))[r.channels:]), (what, k)


def _transform(orc, raw, Cn, g, cmap):
    x = np.asarray(raw, dtype=np.int16)
    if cmap is not None:
        x = orc.chmap(cmap, x, Cn)
    return orc.gain_apply(g, x, Cn)


def _set(orc, b, s, Cn, gains, cmap):
    """gain (None: disabled) and map (None: identity) of stream s (-1: all) -> the oracle's gain"""
    if gains is None:
        assert b.set_gain(s, 0, 0, None) == 0
        g = of.Gain()
    else:
        assert b.set_gain(s, Cn, 1000, gains) == 0
        rc, g = orc.gain(Cn, Cn, 1000, gains)
        assert rc == 0
    assert b.set_chmap(s, cmap) == 0
    return g


def _busy(rng, frames, Cn, lo=100, hi=30000):
    """a signal that is never quiet (32) and never at the rail"""
    mag = rng.integers(lo, hi, size=frames * Cn, dtype=np.int64)
    return (mag * rng.choice([-1, 1], size=frames * Cn)).astype(np.int16)


def _pattern(rng, frames, Cn, mean=40):
    """busy, with runs planted per channel: quiet ones (0, +-32, small), ones at the rail (32767, -32768, -32767) and
    stretches where every channel is quiet; run lengths 1 .. 4 * mean, mostly short"""
    x = _busy(rng, frames, Cn).reshape(frames, Cn)
    at = 0
    while at < frames:
        n = int(min(frames - at, 1 + rng.geometric(1.0 / mean)))
        kind = int(rng.integers(0, 6))
        ch = range(Cn) if kind == 0 else [int(rng.integers(0, Cn))]
        for c in ch:
            if kind <= 2:                            # 0: dead air, 1 and 2: one channel quiet
                x[at:at + n, c] = rng.choice([0, 0, 32, -32, 1, -7], size=n)
            elif kind == 3:
                x[at:at + n, c] = rng.choice([32767, -32768, -32767], size=n)
        at += n
    return x.reshape(-1)


def _batch(cm, Cn, streams=1, max_frames=6300, flags=None, **conf):
    b = cm.Batch(streams, Cn, max_frames, flags=cm.VU if flags is None else flags)
    assert b.get_watch() == 0
    if conf:
        assert b.watch_configure(**conf) == 0
    assert b.set_watch(1) == 0
    assert b.get_watch() == 1
    return b


def _one(b, stream=0):
    rc, r = b.watch_result(stream)
    assert rc == 0
    return r


# ---------------------------------------------------------------------------
# 1. planted runs in a busy signal


def _plant(x, Cn, kind, start, n):
    f = x.reshape(-1, Cn)
    alt = np.where(np.arange(n) % 2 == 0, 1, -1)
    if kind == "D":
        for c in range(Cn):
            f[start:start + n, c] = 32 * alt
    elif kind == "Q":
        f[start:start + n, Cn - 1] = -32 * alt
    else:
        f[start:start + n, Cn - 1] = np.where(alt > 0, 32767, -32768)


@pytest.mark.parametrize("kind", ["D", "Q", "R"])
@pytest.mark.parametrize("Cn", [1, 2])
def test_planted_runs(gpu, oracle, Cn, kind):
    """three tiles and a ragged tail; one run per stream: inside one vector, across a vector's edge, a word's, a row's,
    a tile's, covering the whole second tile between two partial ones (pre == len through the fold), covering the
    whole run"""
    cm, orc = gpu, oracle
    vec, row, tile = GEOM[Cn]["vec"], GEOM[Cn]["row"], GEOM[Cn]["tile"]
    n = 3 * tile + 71
    runs = [(5 * vec + 1, 2), (7 * vec - 1, 3), (3 * WORD - 2, 5), (row - 3, 7), (tile - 5, 11),
            (tile - 9, tile + 9 + 13), (2 * tile - 1, tile + 1 + 71), (0, n)]
    rng = np.random.default_rng(21 + Cn)
    b = _batch(cm, Cn, streams=len(runs), max_frames=n)
    g = _set(orc, b, -1, Cn, None, None)
    models = []
    for s, (start, k) in enumerate(runs):
        x = _busy(rng, n, Cn)
        _plant(x, Cn, kind, start, k)
        b.upload(s, x)
        m = Watch(Cn)
        m.feed(_transform(orc, x, Cn, g, None))
        models.append(m)
    b.run(n)
    out, rc = b.watch_results()
    for s, (start, k) in enumerate(runs):
        assert rc[s] == 0
        want = models[s].result()
        key = {"D": "dead_longest", "Q": "quiet_longest", "R": "clip_longest"}[kind]
        longest = want[key] if kind == "D" else want[key][Cn - 1]
        assert longest == k, (start, k)              # the model saw the planted run and nothing longer
        _check(out[s], want, what=(Cn, kind, start, k))
        if kind == "R":
            assert out[s].clip_events[Cn - 1] == (1 if k >= 3 else 0)
        if start + k == n:                           # the run is still going at the window's end
            cur = {"D": out[s].dead_current, "Q": out[s].quiet_current[Cn - 1], "R": k}[kind]
            assert cur == k
    b.close()


# ---------------------------------------------------------------------------
# 2. events


@pytest.mark.parametrize("K", [1, 3, 16])
def test_events(gpu, oracle, K):
    cm, orc = gpu, oracle
    Cn, tile = 2, GEOM[2]["tile"]
    n = 2 * tile + 37
    # (start, length, events): the K-th rail sample on a tile's last frame; on the next tile's first; K - 1 at a
    # tile's end, then off the rail; 2K: one event; a run of K inside a tile; K + 1 across the ragged tile's edge
    cases = [(tile - K, K, 1), (tile - K + 1, K, 1), (tile - (K - 1), K - 1, 0), (tile - K, 2 * K, 1),
             (100, K, 1), (2 * tile - 1, K + 1, 1), (n - K, K, 1)]
    rng = np.random.default_rng(31)
    b = _batch(cm, Cn, streams=len(cases), max_frames=n, clip_run=K)
    g = _set(orc, b, -1, Cn, None, None)
    models = []
    for s, (start, k, _) in enumerate(cases):
        x = _busy(rng, n, Cn)
        _plant(x, Cn, "R", start, k)
        x.reshape(-1, Cn)[start + k:start + k + 1, 1] = 5          # (off the rail behind it, whatever the noise drew)
        b.upload(s, x)
        m = Watch(Cn, clip_run=K)
        m.feed(_transform(orc, x, Cn, g, None))
        models.append(m)
    b.run(n)
    out, rc = b.watch_results()
    for s, (start, k, ev) in enumerate(cases):
        _check(out[s], models[s].result(), what=("events", K, start, k))
        assert (out[s].clip_events[0], out[s].clip_events[1]) == (0, ev), (K, start, k)
        assert out[s].clip_samples[1] == k and out[s].clip_longest[1] == k
    b.close()


@pytest.mark.parametrize("K", [1, 3, 16])
def test_event_counted_once_in_the_run_and_window_where_it_reaches_k(gpu, K):
    """a run at the rail reaches K in the first run of frames and goes on in the second: counted once, in the first --
    with a result between the two (two windows) and without (one window)"""
    cm = gpu
    Cn, first, second = 2, 300, 200
    x = np.full((first + second, Cn), 1000, dtype=np.int16)
    x[first - K - 2:first + 5, 0] = -32768           # reaches K two frames before the cut, 5 more behind it
    x = x.reshape(-1)
    for between in (True, False):
        b = _batch(cm, Cn, max_frames=first + second, clip_run=K)
        b.upload(0, x[:first * Cn])
        b.run(first)
        if between:
            r = _one(b)
            assert (r.clip_events[0], r.clip_longest[0], r.clip_samples[0]) == (1, K + 2, K + 2)
        b.upload(0, x[first * Cn:])
        b.run(second)
        r = _one(b)
        if between:                                  # the run continues into this window: its full length, no event
            assert (r.clip_events[0], r.clip_longest[0], r.clip_samples[0]) == (0, K + 7, 5)
        else:
            assert (r.clip_events[0], r.clip_longest[0], r.clip_samples[0]) == (1, K + 7, K + 7)
        assert r.clip_events[1] == 0 and r.frames == (second if between else first + second)
        b.close()


# ---------------------------------------------------------------------------
# 3. ragged counts


@pytest.mark.parametrize("fill", [0, 32767])
@pytest.mark.parametrize("Cn", [1, 2])
def test_ragged_counts(gpu, oracle, Cn, fill):
    """counts 0, 1, vector - 1, tile + 1 and the maximum; what lies behind a stream's count -- zeros in one case, 32767
    in the other -- is not counted, extends no run and makes no tile `all quiet`: every stream ends on a run of the
    predicate the fill would continue"""
    cm, orc = gpu, oracle
    vec, tile = GEOM[Cn]["vec"], GEOM[Cn]["tile"]
    T = tile + 2 * WORD + 9
    counts = [0, 1, vec - 1, WORD, tile, tile + 1, T]
    rng = np.random.default_rng(41 + Cn)
    b = _batch(cm, Cn, streams=len(counts), max_frames=T)
    g = _set(orc, b, -1, Cn, None, None)
    models = [Watch(Cn) for _ in counts]
    # a first run gives every stream a window, so that the stream with count 0 has one to keep
    for s in range(len(counts)):
        x = _pattern(rng, 10, Cn, mean=3)
        b.upload(s, x)
        models[s].feed(_transform(orc, x, Cn, g, None))
    b.run(10)
    for s, n in enumerate(counts):
        x = np.full(T * Cn, fill, dtype=np.int16)
        y = _pattern(rng, n, Cn)
        y[max(0, n - 3) * Cn:] = 0 if fill == 0 else -32768          # the stream ends dead / at the rail
        x[:n * Cn] = y
        b.upload(s, x)
        models[s].feed(_transform(orc, y, Cn, g, None))
    b.run(T, counts)
    out, rc = b.watch_results()
    for s, n in enumerate(counts):
        assert rc[s] == 0
        want = models[s].result()
        assert want["frames"] == 10 + n
        if 0 < n < T:
            tail = want["dead_current"] if fill == 0 else models[s].state[-1]
            assert tail > 0                          # a run is open at the count: the fill would have extended it
        _check(out[s], want, what=("ragged", Cn, fill, n))
    b.close()


# ---------------------------------------------------------------------------
# 4. cut invariance, and what keeps and what clears the state


@pytest.mark.parametrize("Cn", [1, 2])
def test_cut_invariance(gpu, oracle, Cn):
    cm, orc = gpu, oracle
    tile = GEOM[Cn]["tile"]
    n = 3 * tile + 71
    rng = np.random.default_rng(51 + Cn)
    x = _pattern(rng, n, Cn, mean=60)
    f = x.reshape(-1, Cn)
    f[tile - 40:tile + 90, :] = 0                    # dead air across the first tile's edge ...
    f[2 * tile - 30:2 * tile + 20, Cn - 1] = 32767   # ... and a clipped stretch across the second's
    b = _batch(cm, Cn, max_frames=n)
    g = _set(orc, b, 0, Cn, [1000] * Cn, None)
    y = _transform(orc, x, Cn, g, None)
    whole = Watch(Cn)
    whole.feed(y)
    want_whole = whole.result()
    b.upload(0, x)
    b.run(n)
    one = _one(b)
    _check(one, want_whole, what="one run")

    # the same samples in ragged runs, 0-frame and 1-frame runs among them, results taken mid-way (inside the dead
    # air and inside the clipped stretch)
    b.watch_reset(0)
    cuts = [1, 0, tile - 41, 1, 60, 0, 2 * tile - 30 + 5 - (tile + 21), 1, 0, 700]
    cuts.append(n - sum(cuts))
    take_after = {4, 6, 8}
    m = Watch(Cn)
    pos, windows = 0, []
    cut_in = set()
    for i, k in enumerate(cuts):
        b.upload(0, x[pos * Cn:(pos + k) * Cn] if k else x[:Cn])
        b.run(max(k, 1), [k])
        m.feed(y[pos * Cn:(pos + k) * Cn])
        pos += k
        if i in take_after:
            for name, st in (("D", m.state[0]), ("Q", m.state[Cn]), ("R", m.state[2 * Cn])):
                if st:
                    cut_in.add(name)
            want = m.result()
            r = _one(b)
            _check(r, want, what=("window closed after cut", i))
            windows.append(r.as_dict())
    assert pos == n and 0 in cuts and 1 in cuts
    assert cut_in == {"D", "Q", "R"}                 # a window closed inside a run of each kind
    r = _one(b)
    _check(r, m.result(), what="last window")
    windows.append(r.as_dict())
    full = one.as_dict()
    assert sum(w["frames"] for w in windows) == n
    assert sum(w["dead_frames"] for w in windows) == full["dead_frames"]
    assert max(w["dead_longest"] for w in windows) == full["dead_longest"]
    assert windows[-1]["dead_current"] == full["dead_current"]
    for c in range(Cn):
        for k in ("quiet_frames", "clip_samples", "clip_events", "sum"):
            assert sum(w[k][c] for w in windows) == full[k][c], (k, c)
        for k in ("quiet_longest", "clip_longest"):
            assert max(w[k][c] for w in windows) == full[k][c], (k, c)
        assert windows[-1]["quiet_current"][c] == full["quiet_current"][c]
    b.close()


def test_result_keeps_the_state_reset_and_configure_clear_it(gpu):
    cm = gpu
    b = _batch(cm, 2, streams=2, max_frames=64)
    z = np.zeros(128, dtype=np.int16)
    b.upload(0, z)
    b.upload(1, z)
    b.run(50)
    assert _one(b, 0).dead_longest == 50
    b.run(10)
    r = _one(b, 0)                                   # the result kept the state: sixty frames of dead air by now
    assert (r.frames, r.dead_frames, r.dead_longest, r.dead_current) == (10, 10, 60, 60)
    b.watch_reset(0)                                 # stream 0 starts over, stream 1 goes on
    b.run(7)
    out, rc = b.watch_results()
    assert rc == [0, 0]
    assert (out[0].frames, out[0].dead_longest, out[0].dead_current) == (7, 7, 7)
    assert (out[1].frames, out[1].dead_longest, out[1].quiet_current[1]) == (67, 67, 67)
    assert b.watch_configure(32, 32767, 3) == 0      # every window is empty: allowed, and it clears the state
    b.run(5)
    out, rc = b.watch_results()
    assert [(o.frames, o.dead_longest, o.dead_current) for o in out] == [(5, 5, 5)] * 2
    assert b.set_watch(0) == 0 and b.set_watch(1) == 0           # off and on again: both discarded
    b.run(3)
    assert _one(b, 1).dead_longest == 3
    b.close()


# ---------------------------------------------------------------------------
# 5. the transform


def test_transform(gpu, oracle):
    cm, orc = gpu, oracle
    rng = np.random.default_rng(61)
    n, Cn = 2500, 2
    x = _busy(rng, n, Cn, lo=300, hi=20000)          # never near the rail
    x.reshape(-1, Cn)[700:760, 0] = 5                # channel 0 quiet for 60 frames, channel 1 busy
    x.reshape(-1, Cn)[1200:1230, 1] = 19000          # thirty frames that a gain of 2 drives into the rail
    b = _batch(cm, Cn, max_frames=n)

    def measure(gains, cmap):
        g = _set(orc, b, 0, Cn, gains, cmap)
        b.watch_reset(0)
        b.upload(0, x)
        b.run(n)
        r = _one(b)
        m = Watch(Cn)
        m.feed(_transform(orc, x, Cn, g, cmap))
        _check(r, m.result(), what=(gains, cmap))
        return r.as_dict()

    plain = measure([1000, 1000], None)
    assert plain["clip_samples"] == [0, 0] and plain["quiet_longest"] == [60, 0] and plain["dead_frames"] == 0
    assert measure(None, None) == plain              # gain disabled
    hot = measure([2000, 2000], None)                # saturation: events from a signal that never touched the rail
    assert hot["clip_events"][1] >= 1 and hot["clip_longest"][1] >= 30 and hot["clip_samples"][0] > 0
    faint = measure([1, 1], None)                    # 20000 / 1000 = 20: below quiet, all of it dead air
    assert (faint["dead_frames"], faint["dead_longest"], faint["dead_current"]) == (n, n, n)
    swapped = measure([1000, 1000], [1, 0])          # a swap moves the per-channel numbers
    for k in KEYS:
        assert swapped[k] == plain[k][::-1], k
    measure([700, 3000], [0, 0])                     # both channels read channel 0, one gain below and one above
    b.close()


@pytest.mark.parametrize("form", ["in_place", "out_pcm", "run_slots"])
def test_batch_forms(gpu, oracle, form):
    """the pass reads the run's input slots ahead of the block kernel: an in-place batch (whose block kernel overwrites
    them), a batch that writes PCM elsewhere, and slots named per run"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(71)
    S, Cn, n = 3, 2, 2048 + 300
    flags = {"in_place": cm.OUT_PCM | cm.VU | cm.INPLACE, "out_pcm": cm.OUT_PCM | cm.VU,
             "run_slots": cm.OUT_PCM | cm.VU | cm.EXTSLOTS}[form]
    b = _batch(cm, Cn, streams=S, max_frames=n, flags=flags)
    g = _set(orc, b, -1, Cn, [1700, 650], [1, 0])
    xs = [_pattern(rng, n, Cn) for _ in range(S)]
    counts = [n, 0, 2049]
    models = [Watch(Cn) for _ in range(S)]
    if form == "run_slots":
        i, o = cm.MappedPcm(b), cm.MappedPcm(b)
        for s in range(S):
            i.array[s, :n * Cn] = xs[s]
    for fps in (None, counts):
        if form == "run_slots":
            b.run_slots(n, i.dev, o.dev, frames_per_stream=fps)
        else:
            for s in range(S):
                b.upload(s, xs[s])
            b.run(n, fps)
        b.sync()
        for s in range(S):
            k = n if fps is None else fps[s]
            y = _transform(orc, xs[s][:k * Cn], Cn, g, [1, 0])
            models[s].feed(y)
            if k:
                pcm = o.array[s, :k * Cn] if form == "run_slots" else b.download(s, k)
                assert np.array_equal(pcm, y), (form, s)
    out, rc = b.watch_results()
    for s in range(S):
        assert rc[s] == 0
        _check(out[s], models[s].result(), what=(form, s))
    if form == "run_slots":
        i.free()
        o.free()
    b.close()


# ---------------------------------------------------------------------------
# 6. widths and scale


@pytest.mark.parametrize("Cn", [3, 5, 6, 16])
def test_any_kernel(gpu, oracle, Cn):
    """k_watch_any: runs of 1, 1023, 1024, 1025 and 2051 frames (the workgroup's 1024 and its neighbours, a ragged third
    tile) with ragged counts, maps and gains of every kind; the state runs on from run to run, a window per run"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(100 + Cn)
    S, T = 5, 2051
    b = _batch(cm, Cn, streams=S, max_frames=T)
    params, models = [], [Watch(Cn) for _ in range(S)]
    for s in range(S):
        gains = [None, [int(v) for v in rng.integers(900, 1100, Cn)], [1000] * Cn][s % 3]
        cmap = [int(v) for v in rng.permutation(Cn)] if s != 2 else None
        params.append((_set(orc, b, s, Cn, gains, cmap), cmap))
    almost_dead = dead_over_edge = 0
    for frames in (1, ANY_TILE - 1, ANY_TILE, ANY_TILE + 1, T):
        counts = [frames, frames // 2, 0, 1, frames - 1]
        for s in range(S):
            x = np.full(T * Cn, 32767, dtype=np.int16)
            y = _pattern(rng, counts[s], Cn, mean=25)
            if counts[s] > ANY_TILE + 10:
                y.reshape(-1, Cn)[ANY_TILE - 20:ANY_TILE + 9, :] = 0             # dead air over the tile's edge ...
                y.reshape(-1, Cn)[ANY_TILE - 3:ANY_TILE + 3, Cn - 1] = 999       # ... but for one channel
                y.reshape(-1, Cn)[300:340, :] = 0
                dead_over_edge += 1
            x[:counts[s] * Cn] = y
            b.upload(s, x)
            t = _transform(orc, y, Cn, *params[s])
            _, preds = models[s].predicates(t)
            q = np.stack(preds[1:1 + Cn])
            almost_dead += int(((q.sum(axis=0) == Cn - 1)).sum())
            models[s].feed(t)
        b.run(frames, counts)
        out, rc = b.watch_results()
        for s in range(S):
            assert rc[s] == (0 if counts[s] else cm.ERROR_INVAL), (frames, s)
            if counts[s]:
                _check(out[s], models[s].result(), what=(Cn, frames, s))
    assert almost_dead > 0 and dead_over_edge > 0    # frames with every channel quiet but one: D is false there
    b.close()


def test_300_streams(gpu, oracle):
    """distinct ragged counts and distinct patterns per stream, two runs and one round trip"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(81)
    S, Cn, T = 300, 2, 2048 + 300
    b = _batch(cm, Cn, streams=S, max_frames=T)
    g = _set(orc, b, -1, Cn, [1100, 900], None)
    counts = [(s * 37) % (T + 1) for s in range(S)]
    counts[7], counts[11] = 0, T
    assert len(set(counts)) > 280
    models = [Watch(Cn) for _ in range(S)]
    for fps in (counts, None):
        for s in range(S):
            k = T if fps is None else fps[s]
            x = np.full(T * Cn, -32768 if s % 2 else 0, dtype=np.int16)
            x[:k * Cn] = _pattern(rng, k, Cn, mean=30 + s % 50)
            b.upload(s, x)
            models[s].feed(_transform(orc, x[:k * Cn], Cn, g, None))
        b.run(T, fps)
    out, rc = b.watch_results()
    assert rc == [0] * S
    for s in range(S):
        _check(out[s], models[s].result(), what=("of 300", s))
    b.close()


def test_beside_the_other_meters(gpu, oracle):
    """the watch beside true peak, correlation and the VU in one batch: each equal to what it gives alone"""
    cm, orc = gpu, oracle
    rng = np.random.default_rng(91)
    S, T = 3, 2500
    xs = [_pattern(rng, T, 2) for _ in range(S)]
    counts = [T, 0, 2049]

    def run(tp, co, wa):
        b = cm.Batch(S, 2, T, flags=cm.OUT_PCM | cm.VU)
        g = _set(orc, b, -1, 2, [800, 1300], [1, 0])
        assert b.set_true_peak(tp) == 0 and b.set_correlation(co) == 0 and b.set_watch(wa) == 0
        n0 = cm.lib.cmhip_debug_watch_count()
        for k, fps in enumerate((None, counts)):
            for s in range(S):
                b.upload(s, xs[s])
            b.run(T, fps)
            assert cm.lib.cmhip_debug_watch_count() == n0 + (k + 1 if wa else 0)
        res = {}
        if tp:
            out, rc = b.tp_results()
            res["tp"] = [(rc[s], out[s].as_dict()) for s in range(S)]
        if co:
            out, rc = b.corr_results()
            res["corr"] = [(rc[s], bytes(out[s])) for s in range(S)]
        if wa:
            out, rc = b.watch_results()
            res["watch"] = [(rc[s], bytes(out[s])) for s in range(S)]
            for s in range(S):
                y = _transform(orc, xs[s], 2, g, [1, 0])
                m = Watch(2)
                m.feed(y)
                m.feed(y[:counts[s] * 2])
                _check(out[s], m.result(), what=("beside", s))
        vu, rc = b.vu_results()
        res["vu"] = [(rc[s], vu[s].as_dict()) for s in range(S)]
        res["pcm"] = [b.download(s, T).tobytes() for s in range(S)]
        b.close()
        return res

    together = run(1, 1, 1)
    for alone in (run(1, 0, 0), run(0, 1, 0), run(0, 0, 1), run(0, 0, 0)):
        for key, val in alone.items():
            assert together[key] == val, key


# ---------------------------------------------------------------------------
# 7. the calls


def test_api(gpu):
    cm = gpu
    b = cm.Batch(3, 2, 64, flags=cm.VU)
    sentinel = cm.WatchResult()
    C.memset(C.byref(sentinel), 0x5a, C.sizeof(sentinel))
    before = bytes(sentinel)
    # a batch without the watch
    assert b.watch_result(0, out=sentinel)[0] == cm.ERROR_INVAL and bytes(sentinel) == before
    assert cm.lib.cmhip_batch_watch_results(b.h, (cm.WatchResult * 3)(), None) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_watch_reset(b.h, -1) == cm.ERROR_INVAL
    # configure: allowed while off; out of range changes nothing
    assert b.watch_configure(100, 30000, 2) == 0
    for bad in ((32768, 32767, 3), (32, 0, 3), (32, 32768, 3), (32, 32767, 0), (32, 32767, 17)):
        assert b.watch_configure(*bad) == cm.ERROR_INVAL, bad
    assert b.set_watch(1) == 0 and b.set_watch(1) == 0
    x = np.tile(np.array([100, 30000], dtype=np.int16), 64)
    for s in range(3):
        b.upload(s, x)
    # an empty window: INVAL, `out` unchanged
    assert b.watch_result(1, out=sentinel)[0] == cm.ERROR_INVAL and bytes(sentinel) == before
    assert cm.lib.cmhip_batch_watch_result(b.h, 3, C.byref(sentinel)) == cm.ERROR_INVAL
    assert cm.lib.cmhip_batch_watch_result(b.h, 0, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_batch_watch_results(b.h, None, None) == cm.ERROR_FAULT
    assert b.watch_configure(100, 30000, 2) == 0     # on, every window empty: allowed
    b.run(8, [0, 8, 3])
    assert b.watch_configure(32, 32767, 3) == cm.ERROR_BUSY          # streams 1 and 2 hold frames
    assert b.watch_configure(32, 0, 3) == cm.ERROR_INVAL
    out = (cm.WatchResult * 3)()
    C.memset(out, 0x5a, C.sizeof(out))
    out, rc = b.watch_results(out)
    assert rc == [cm.ERROR_INVAL, 0, 0] and bytes(out[0]) == before
    r = out[1]                                       # the refused calls changed nothing: 100 is quiet, 30000 at the rail
    assert (r.quiet, r.rail, r.clip_run, r.frames, r.rate, r.channels) == (100, 30000, 2, 8, 48000, 2)
    assert r.quiet_frames[0] == 8 and r.clip_samples[1] == 8 and r.clip_events[1] == 1 and r.dead_frames == 0
    assert r.sum[0] == 800 and r.sum[1] == 240000 and _bits(r.dc[1]) == _bits(240000.0 / 8.0 / 32768.0)
    assert out[2].frames == 3 and out[2].clip_longest[1] == 3
    b.run(3)
    assert cm.lib.cmhip_batch_watch_results(b.h, out, None) == 0     # rc may be NULL
    assert out[0].frames == 3 and out[1].clip_longest[1] == 11 and out[1].clip_events[1] == 0
    assert cm.lib.cmhip_batch_watch_reset(b.h, 3) == cm.ERROR_INVAL
    # off: no pass, the results refuse; on again: the parameters kept
    assert b.set_watch(0) == 0 and b.get_watch() == 0
    n0 = cm.lib.cmhip_debug_watch_count()
    b.run(8)
    assert cm.lib.cmhip_debug_watch_count() == n0
    assert b.watch_result(0)[0] == cm.ERROR_INVAL
    assert b.set_watch(1) == 0
    assert b.watch_results()[1] == [cm.ERROR_INVAL] * 3
    b.run(4)
    assert cm.lib.cmhip_debug_watch_count() == n0 + 1
    r = _one(b, 0)
    assert (r.quiet, r.rail, r.clip_run, r.clip_longest[1], r.clip_events[1]) == (100, 30000, 2, 4, 1)
    b.close()
    mono = _batch(cm, 1, max_frames=64)              # a mono batch is allowed
    mono.upload(0, np.zeros(64, dtype=np.int16))
    mono.run(64)
    r = _one(mono)
    assert (r.channels, r.dead_frames, r.quiet_frames[0], r.dead_longest, r.quiet_current[0]) == (1, 64, 64, 64, 64)
    mono.close()


def test_watch_and_equaliser_exclude_each_other(gpu):
    cm = gpu
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    e = cm.Batch(2, 2, 256, flags=cm.OUT_PCM | cm.VU | cm.EQ)
    assert e.set_watch(1) == 0
    assert e.set_eq(-1, coef) == cm.ERROR_INVAL      # sections while the watch is on
    assert e.set_eq(-1, []) == 0                     # (no sections stays allowed)
    assert e.set_watch(0) == 0
    assert e.set_eq(-1, coef) == 0
    assert e.set_watch(1) == cm.ERROR_INVAL and e.get_watch() == 0
    assert e.set_eq(-1, []) == 0
    assert e.set_watch(1) == 0
    e.upload(0, np.tile(np.array([3, -32768], dtype=np.int16), 21))
    e.upload(1, np.zeros(42, dtype=np.int16))
    e.run(21)
    r = _one(e, 0)
    assert (r.quiet_frames[0], r.clip_samples[1], r.clip_events[1], r.sum[1]) == (21, 21, 1, -21 * 32768)
    e.close()


# ---------------------------------------------------------------------------
# 8. a group


def test_group(gpu, oracle):
    """three table sources in a group that is not full, pumped block by block: every window equals the model on the
    concatenated blocks, the run lengths going on from block to block and from window to window"""
    cm, orc = gpu, oracle
    Cn, block, blocks = 2, 1000, 8
    rng = np.random.default_rng(95)
    grp = cm.Group(Cn, 5, block, queue_blocks=8)
    assert grp.watch_configure(40, 32000, 4) == 0
    assert grp.watch_configure(40, 32000, 17) == cm.ERROR_INVAL
    assert grp.set_watch(1) == 0
    assert cm.lib.coolmic_group_watch(grp.ptr, 3, C.byref(cm.WatchResult())) == cm.ERROR_INVAL
    setup = [([1000, 500], None), ([2500, 900], [1, 0]), (None, None)]
    N = len(setup)
    raws, models, gs = [], [], []
    for i, (gains, cmap) in enumerate(setup):
        x = _pattern(rng, blocks * block, Cn, mean=300)
        x.reshape(-1, Cn)[block - 100:2 * block + 50, :] = 0         # dead air over two block edges
        h = cm.IoHandle.from_bytes(x.tobytes(), chunk=(0, 7, 1024)[i])
        assert grp.add_stream(h) == i
        h.unref()
        if gains is None:
            assert grp.set_master_gain(i, 0, 0, None) == 0
            g = of.Gain()
        else:
            assert grp.set_master_gain(i, Cn, 1000, gains) == 0
            _, g = orc.gain(Cn, Cn, 1000, gains)
        assert grp.set_channel_map(i, cmap) == 0
        raws.append(x)
        gs.append(g)
        models.append(Watch(Cn, 40, 32000, 4))
    coef = np.zeros(5, dtype=np.float32)
    cm.lib.cmhip_design_biquad(1, 48000., 1000., 3., 1., coef.ctypes.data)
    assert grp.set_eq(-1, coef) == cm.ERROR_INVAL    # the engine's INVAL, passed through
    pos = [0] * N

    def feed(k):
        """the frames the last k pumps took, by the VU windows closed at the same point"""
        vu, rc_vu = grp.vumeter_results()
        assert rc_vu == [0] * N
        for i in range(N):
            n = vu[i].frames
            assert n == k * block
            models[i].feed(_transform(orc, raws[i][pos[i] * Cn:(pos[i] + n) * Cn], Cn, gs[i], setup[i][1]))
            pos[i] += n

    for _ in range(2):                               # two pumps, then every window at once: the block in flight counts
        assert grp.pump() == N
    out, rc = grp.watches()
    feed(2)
    assert len(rc) == N and rc == [0] * N
    for i in range(N):
        assert models[i].state[0] > block            # the windows close inside the dead air
        _check(out[i], models[i].result(), what=("group", i))
    keep = bytes(out[2])                             # empty windows: every rc INVAL, results left alone
    out, rc = grp.watches(out)
    assert rc == [cm.ERROR_INVAL] * N and bytes(out[2]) == keep
    assert grp.watch_configure(40, 32000, 4) == 0    # every window empty: allowed; clears the state
    for m in models:
        m.configure(40, 32000, 4)
    assert grp.pump() == N
    rc1, r1 = grp.watch(1)                           # a single-slot call closes only that slot's window
    assert rc1 == 0
    feed(1)
    _check(r1, models[1].result(), what="group, slot 1 alone")
    assert grp.watch(1)[0] == cm.ERROR_INVAL
    assert grp.watch_configure(40, 32000, 4) == cm.ERROR_BUSY
    assert grp.pump() == N
    out, rc = grp.watches()
    feed(1)
    assert rc == [0] * N
    for i in range(N):
        _check(out[i], models[i].result(), what=("group, after the single slot", i))
    assert grp.pump() == N                           # reset: one slot, all
    assert grp.watch_reset(0) == 0
    assert grp.watch_reset(3) == cm.ERROR_INVAL
    out, rc = grp.watches()
    feed(1)
    assert rc == [cm.ERROR_INVAL, 0, 0]
    models[0].reset()
    for i in (1, 2):
        _check(out[i], models[i].result(), what=("group, after reset(0)", i))
    assert grp.pump() == N
    assert grp.watch_reset(-1) == 0
    assert grp.watches()[1] == [cm.ERROR_INVAL] * N
    assert grp.set_watch(0) == 0
    grp.unref()


# ---------------------------------------------------------------------------
# 9. the example


def test_batch_watch_in_c(gpu, tmp_path):
    exe = tmp_path / "batch_watch"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "batch_watch.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-lm", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert len(out) == 4
    assert out[0].startswith("programme: ") and "longest dead air 0.000 s" in out[0] and "clip events 0" in out[0]
    assert out[1].startswith("programme with a gap: ") and "longest dead air 2.000 s" in out[1]
    assert out[2].startswith("sine 6 dB over: ") and "clip events 0" not in out[2]
    assert out[3].startswith("sine on DC: ") and "DC +0.0305" in out[3]
