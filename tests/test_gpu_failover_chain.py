"""GPU: the failover switch where it belongs -- switch -> leveller -> limiter -> the slots of a batch with the signal
watch on, all on the batch's stream with no synchronisation in between, over five ragged blocks (counted from 0).  Output
0 has the list (main, backup) and every block's full count: its main source goes silent inside block 2, for far longer
than fail_windows, and returns inside block 4.  Output 1 has three candidates and counts of its own.  Bar: the batch's
PCM equals the composed numpy models (the leveller's and the limiter's from their own test files, the switch's from
tests/failover_model.py, the watch's from tests/watch_model.py) bit for bit, block by block, with every stage's state
carried across the blocks."""
import importlib.util
import os
import types

import numpy as np
import pytest

import failover_model as FM
import watch_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -21555
POISON = 0x5a5a
INPUTS, OUTPUTS, MAXF, W_LOG2 = 3, 2, 2000, 6
BLOCKS = [[1200, 700], [1, 0], [2000, 1999], [1234, 0], [1501, 5]]       # per block: the counts of the two outputs
SILENT_FROM, SILENT_TO = 1201 + 300, 1201 + 2000 + 1234 + 200            # of input 0: inside block 2 .. inside block 4
LOOKAHEAD_LOG2, HOLD, THRESHOLD, DRIVE = 6, 30, 20000, 4096


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_failover_chain", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TL = _load("test_gpu_lim")             # model_lim, next_hist, geometry
TA = _load("test_gpu_agc")             # Model, params, enveloped


@pytest.mark.parametrize("channels", [1, 2])
def test_switch_leveller_limiter_batch(gpu, channels):
    cm = gpu
    W = 1 << W_LOG2
    stride = (MAXF * channels + 7) // 8 * 8 + 8
    b = cm.Batch(OUTPUTS, channels, MAXF, flags=cm.OUT_PCM | cm.VU, rate=48000)
    assert b.set_watch(True) == 0
    sw = cm.Failover(INPUTS, OUTPUTS, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    agc = cm.Leveller(OUTPUTS, channels, W_LOG2, MAXF, hip_stream=b.hip_stream())
    lim = cm.Limiter(OUTPUTS, channels, LOOKAHEAD_LOG2, HOLD, MAXF, threshold=THRESHOLD, drive=DRIVE,
                     hip_stream=b.hip_stream())
    assert sw.hip_stream() == agc.hip_stream() == lim.hip_stream() == b.hip_stream()
    model = FM.Switch(INPUTS, OUTPUTS, channels, W_LOG2)
    lists = ([0, 1], [2, 1, 0])
    plist = [FM.params(W_LOG2, quiet=(33, 33, 33, 33), fail_windows=3, return_windows=4, fade_log2=W_LOG2 + 1),
             FM.params(W_LOG2, quiet=(2000, 33, 33, 33), fail_windows=1, return_windows=2)]
    for o in range(OUTPUTS):
        sw.set_sources(o, lists[o])
        model.set_sources(o, lists[o])
        sw.set(o, cm.failover_params(W_LOG2, **plist[o]))
        model.set(o, plist[o])
    aplist = [TA.params(target=6000, gate=0, gain_min=1, gain_max=8192, rise=30000, fall=30000),
              TA.params(target=20000, gate=10, gain_min=1, gain_max=65535, rise=65535, fall=65535, initial=16384)]
    for s, p in enumerate(aplist):
        agc.set(s, cm.AgcParams(**p))
    levellers = [TA.Model(channels, W_LOG2, p) for p in aplist]
    hist = [np.zeros((TL.geometry(LOOKAHEAD_LOG2, HOLD)[3], channels), dtype=np.int16) for _ in range(OUTPUTS)]
    watches = [WM.Watch(channels) for _ in range(OUTPUTS)]
    src = cm.MappedPcm(types.SimpleNamespace(streams=INPUTS, stride=stride))
    picked, level = (cm.MappedPcm(types.SimpleNamespace(streams=OUTPUTS, stride=stride)) for _ in range(2))
    total = sum(max(blk) for blk in BLOCKS)
    signals = [(TA.enveloped(500 + s, total, channels, W) // 2).astype(np.int16) for s in range(INPUTS)]
    signals[0] = np.clip(signals[0].astype(np.int64) + 900, -32768, 32767).astype(np.int16)   # never quiet by itself
    signals[0][SILENT_FROM:SILENT_TO] = 0
    signals[1] = FM.spurts(77, total, channels, 64 * W, amp=7000)         # the backup: one long spurt
    signals[1][signals[1] == 0] = 1234
    try:
        at = 0
        seen = []
        for k, counts in enumerate(BLOCKS):
            frames = max(counts)
            slots = [x[at:at + frames] for x in signals]
            at += frames
            src.array[:] = POISON
            for s, x in enumerate(slots):
                src.array[s, :x.size] = x.reshape(-1)
            picked.array[:] = SENTINEL
            level.array[:] = SENTINEL
            sw.run(src.dev, stride, frames, picked.dev, stride, counts)
            agc.run(picked.dev, stride, frames, level.dev, stride, counts)
            lim.run(level.dev, stride, frames, b.dev_in, b.stride, counts)
            b.run(frames, np.array(counts, dtype=np.uint32))       # (no sync between the four: the order is the stream's)
            res, rcs = b.vu_results()
            want_picked = model.run(slots, counts)
            for o in range(OUTPUTS):
                n = counts[o]
                want_level = levellers[o].run(want_picked[o])
                want, _ = TL.model_lim(want_level, hist[o], THRESHOLD, DRIVE, LOOKAHEAD_LOG2, HOLD)
                hist[o] = TL.next_hist(hist[o], want_level)
                assert np.array_equal(picked.array[o, :n * channels].reshape(-1, channels), want_picked[o]), ("switch", k, o)
                assert (picked.array[o, n * channels:] == SENTINEL).all(), ("switch wrote past its count", k, o)
                assert np.array_equal(level.array[o, :n * channels].reshape(-1, channels), want_level), ("leveller", k, o)
                if n:
                    have = b.download(o, n).reshape(-1, channels)
                    assert np.array_equal(have, want), ("limiter", k, o)
                    assert rcs[o] == 0 and res[o].frames == n
                    watches[o].feed(want)
            have, want_state = sw.state(), model.state()
            for key, name in (("from", "fr"), ("to", "to"), ("fade_window", "fade_window"), ("switches", "switches"),
                              ("live_run", "live_run"), ("dead_run", "dead_run"), ("level", "level")):
                assert have[key].tolist() == want_state[name], (k, key)
            gain, lv, clips = agc.state()
            assert [(int(gain[s]), int(lv[s]), int(clips[s])) for s in range(OUTPUTS)] == [m.state() for m in levellers]
            seen.append(want_state["to"][0])
        # output 0 left its main source in block 2 and had it back by the end of block 4
        assert at == total and seen == [0, 0, 1, 1, 0] and model.state()["switches"][0] == 2
        wres, wrc = b.watch_results()
        for o in range(OUTPUTS):
            want = watches[o].peek()
            got = wres[o].as_dict()
            assert wrc[o] == 0 and all(got[key] == want[key] for key in want if key != "dc"), (o, got, want)
        # the listener's dead air is what the switch let through: far less than the source's
        assert wres[0].dead_longest < (3 + 2) * W + W and SILENT_TO - SILENT_FROM > 40 * W
    finally:
        for o in (lim, agc, sw, b):
            o.close()
        for a in (src, picked, level):
            a.free()
