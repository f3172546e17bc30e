"""CPU: the host side of the signal watch -- the result struct's layout, the level helper, the refusals that need no
device, the launcher's plan at the 2^31 limit, and the model (tests/watch_model.py) against sequences worked by hand.
No device is touched.

Bar: equality.
"""
import ctypes as C
import math

import numpy as np
import pytest

from watch_model import Watch, online, run_lengths


def test_result_struct_layout(cm):
    """coolmic_watch_result_t on LP64: 1080 bytes, the fields where include/coolmic-dsp/vumeter.h puts them"""
    R = cm.WatchResult
    assert C.sizeof(R) == 1080
    want = {"rate": 0, "channels": 4, "frames": 8, "quiet": 16, "rail": 20, "clip_run": 24,
            "dead_frames": 32, "dead_longest": 40, "dead_current": 48,
            "quiet_frames": 56, "quiet_longest": 184, "quiet_current": 312,
            "clip_samples": 440, "clip_events": 568, "clip_longest": 696, "sum": 824, "dc": 952}
    assert {n: getattr(R, n).offset for n, _ in R._fields_} == want
    assert R.dc.size == 128 and R.sum.size == 128 and R.frames.size == 8


def test_watch_level(cm):
    assert cm.watch_level(-60.0) == 33
    assert cm.watch_level(0.0) == 32767
    assert cm.watch_level(-math.inf) == 0
    assert cm.watch_level(6.0) == 32767
    assert cm.watch_level(-60.2) == 32                      # the default `quiet`
    assert cm.watch_level(-6.0) == round(32768 * 10 ** (-6.0 / 20))
    assert cm.watch_level(-200.0) == 0
    assert cm.watch_level(math.nan) == 0
    for db in np.linspace(-96, 0, 97):
        assert cm.watch_level(float(db)) == min(32767, math.floor(32768 * 10 ** (db / 20) + 0.5))


def test_null_arguments_are_refused_without_a_device(cm):
    lib = cm.lib
    r = cm.WatchResult()
    assert lib.cmhip_batch_set_watch(None, 1) == cm.ERROR_FAULT
    assert lib.cmhip_batch_get_watch(None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_watch_configure(None, 32, 32767, 3) == cm.ERROR_FAULT
    assert lib.cmhip_batch_watch_result(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert lib.cmhip_batch_watch_results(None, C.byref(r), None) == cm.ERROR_FAULT
    assert lib.cmhip_batch_watch_reset(None, -1) == cm.ERROR_FAULT
    assert lib.coolmic_group_set_watch(None, 1) == cm.ERROR_FAULT
    assert lib.coolmic_group_watch_configure(None, 32, 32767, 3) == cm.ERROR_FAULT
    assert lib.coolmic_group_watch(None, 0, C.byref(r)) == cm.ERROR_FAULT
    assert lib.coolmic_group_watches(None, C.byref(r), None) == cm.ERROR_FAULT
    assert lib.coolmic_group_watch_reset(None, -1) == cm.ERROR_FAULT
    assert bytes(r) == bytes(1080)
    n0 = lib.cmhip_debug_watch_count()
    assert lib.cmhip_batch_watch_reset(None, -1) == cm.ERROR_FAULT and lib.cmhip_debug_watch_count() == n0


def test_plan(cm):
    """tiles of 4096 / C frames (mono, stereo) or 1024 (the rest), one summary per stream, tile and predicate, and the
    refusal where streams x tiles reaches 2^31"""
    p = cm.plan_watch(4096, 2, 65536)
    assert (p.refused, p.fast, p.tile_frames, p.chunks, p.grid, p.block) == (0, 1, 2048, 32, 4096 * 32, 64)
    assert (p.fold_grid, p.fold_block, p.scratch) == ((4096 * 5 + 255) // 256, 256, 4096 * 32 * 5)
    p = cm.plan_watch(8192, 1, 65536)
    assert (p.fast, p.tile_frames, p.chunks, p.grid, p.scratch) == (1, 4096, 16, 8192 * 16, 8192 * 16 * 3)
    p = cm.plan_watch(5, 6, 1025)
    assert (p.fast, p.tile_frames, p.chunks, p.grid, p.block, p.scratch) == (0, 1024, 2, 10, 256, 10 * 13)
    for frames, chunks in ((1, 1), (2048, 1), (2049, 2), (4096, 2), (4097, 3)):
        assert cm.plan_watch(3, 2, frames).chunks == chunks
    for args in ((0, 2, 100), (4, 2, 0), (4, 0, 100), (4, 17, 100)):
        p = cm.plan_watch(*args)
        assert (p.refused, p.grid) == (0, 0), args
    # on the limit and just under it, for each kernel's tile
    for C_, tile in ((2, 2048), (1, 4096), (6, 1024)):
        streams = 1 << 20
        tiles = (1 << 31) // streams
        p = cm.plan_watch(streams, C_, tiles * tile)
        assert (p.refused, p.grid, p.scratch) == (1, 0, 0), C_
        p = cm.plan_watch(streams, C_, tiles * tile - tile + 1)     # still `tiles` tiles, the last one ragged
        assert p.refused == 1, C_
        p = cm.plan_watch(streams, C_, (tiles - 1) * tile)
        assert (p.refused, p.chunks, p.grid) == (0, tiles - 1, streams * (tiles - 1)), C_
        assert p.scratch == p.grid * (2 * C_ + 1)
        p = cm.plan_watch(streams - 1, C_, tiles * tile)
        assert (p.refused, p.grid) == (0, (streams - 1) * tiles), C_


# ---------------------------------------------------------------------------
# the model


def test_model_by_hand():
    #          frame  0  1  2  3  4  5  6  7  8  9
    P = np.array([1, 1, 0, 1, 1, 1, 1, 0, 0, 1], dtype=bool)
    #   l from l0=0:  1  2  0  1  2  3  4  0  0  1
    assert run_lengths(P, 0).tolist() == [1, 2, 0, 1, 2, 3, 4, 0, 0, 1]
    assert online(P, 0, 3) == (7, 4, 1, 1)
    assert online(P, 0, 2) == (7, 4, 2, 1)
    assert online(P, 0, 1) == (7, 4, 3, 1)
    assert online(P, 0, 5) == (7, 4, 0, 1)
    #   l from l0=5:  6  7  0  1  2  3  4  0  0  1      the run from before continues into the window: longest 7
    assert run_lengths(P, 5).tolist() == [6, 7, 0, 1, 2, 3, 4, 0, 0, 1]
    assert online(P, 5, 3) == (7, 7, 1, 1)           # the first run passed 3 before the window: no event for it
    assert online(P, 5, 7) == (7, 7, 1, 1)           # ... and reaches 7 inside it
    assert online(P, 1, 3) == (7, 4, 2, 1)           # l = 2, 3: the run reaches K in this window
    # a window whose first frame is not P takes nothing from the state
    Z = np.array([0, 1, 1], dtype=bool)
    assert run_lengths(Z, 1000).tolist() == [0, 1, 2]
    assert online(Z, 1000, 3) == (2, 2, 0, 2)
    # all P: the state grows, an event only where l passes K
    A = np.ones(4, dtype=bool)
    assert online(A, 0, 3) == (4, 4, 1, 4) and online(A, 3, 3) == (4, 7, 0, 7) and online(A, 2, 3) == (4, 6, 1, 6)
    assert online(A, 2**32 - 2, 3) == (4, 2**32 + 2, 0, 2**32 + 2)
    assert run_lengths(A, 2**32 - 2).tolist() == [2**32 - 1, 2**32, 2**32 + 1, 2**32 + 2]
    assert run_lengths(np.zeros(0, dtype=bool), 7).size == 0


def test_model_stream_by_hand():
    """stereo, quiet 2, rail 100, K = 2; frames (L, R)"""
    w = Watch(2, quiet=2, rail=100, clip_run=2)
    x = [(0, 0), (2, -2), (3, 0), (100, -100), (101, -32768), (-100, 5), (1, 1)]
    w.feed(np.array(x, dtype=np.int16).reshape(-1))
    d = w.result()
    assert d["frames"] == 7 and (d["quiet"], d["rail"], d["clip_run"]) == (2, 100, 2)
    assert (d["dead_frames"], d["dead_longest"], d["dead_current"]) == (3, 2, 1)
    assert d["quiet_frames"] == [3, 4] and d["quiet_longest"] == [2, 3] and d["quiet_current"] == [1, 1]
    assert d["clip_samples"] == [3, 2] and d["clip_longest"] == [3, 2] and d["clip_events"] == [1, 1]
    assert d["sum"] == [0 + 2 + 3 + 100 + 101 - 100 + 1, 0 - 2 + 0 - 100 - 32768 + 5 + 1]
    assert d["dc"] == [107 / 7 / 32768.0, -32864 / 7 / 32768.0]
    # the next window: the state stays (one dead frame behind us), the window starts empty
    assert w.peek() is None
    w.feed(np.array([(0, 0), (0, 0), (9, 0)], dtype=np.int16).reshape(-1))
    d = w.result()
    assert (d["dead_frames"], d["dead_longest"], d["dead_current"]) == (2, 3, 0)
    assert d["quiet_longest"] == [3, 4] and d["quiet_current"] == [0, 4]
    w.reset()
    w.feed(np.array([(0, 0)], dtype=np.int16).reshape(-1))
    assert w.result()["quiet_longest"] == [1, 1]


def test_model_numpy_form_is_the_online_definition():
    rng = np.random.default_rng(5)
    for i in range(300):
        n = int(rng.integers(1, 200))
        P = rng.random(n) < (0.03, 0.5, 0.97, 1.0)[i % 4]
        l0 = int(rng.choice([0, 1, 2, 15, 16, 2**32 - 2]))
        K = 1 + i % 16
        l = run_lengths(P, l0)
        assert (int(P.sum()), int(l.max()), int((l == K).sum()), int(l[-1])) == online(P, l0, K)
        # cut anywhere: the same
        cut = int(rng.integers(0, n + 1))
        a = online(P[:cut], l0, K)
        b = online(P[cut:], a[3], K)
        whole = online(P, l0, K)
        assert (a[0] + b[0], a[2] + b[2], b[3]) == (whole[0], whole[2], whole[3])
