"""CPU: the model of the programme chain (tests/test_gpu_programme_chain.py: resampler -> mixer with ramps -> bus ->
limiter, the composition of the per-object tests' numpy models) held to its own properties, so that the device test
compares against something that means what it says: (a) the model run block by block over the chain's ragged cuts equals
the model run once over every stream's whole signal, the ramp calls placed at the same frame positions; (b) the chain's
inputs are dense -- the limiter works (neither idle nor pinned), the ceiling is reached, and the mixer's and the bus's
outputs are mostly not saturated, for a saturated output hides a wrong sum.  These are conditions on the inputs, not
tolerances.  Nothing here needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_programme_chain_model",
                                                  os.path.join(ROOT, "tests", "test_gpu_programme_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # the chain's shape, inputs and model
UNITY_SHARE, CHANGE_SHARE = TG.TL.UNITY_SHARE, TG.TL.CHANGE_SHARE
SATURATED_MAX = TG.TS.SATURATED_MAX
VARIANTS = ["fast", "any"]


def test_the_cuts_are_what_the_chain_test_says():
    a, b = TG.CUTS
    assert len(a) == len(b) == 14 and (sum(a), sum(b)) == (40564, 40755) and max(a + b) == TG.MAX_IN
    hist = TG.TL.geometry(TG.LOOKAHEAD_LOG2, TG.HOLD)[3]
    assert hist == 226
    for cuts in (a, b):
        # blocks of 0, 1 and 7 frames with a long one at most two blocks before; counts on both sides of the limiter's tile
        for short in (0, 1, 7):
            assert short in cuts
            assert any(n == short and max(c[max(i - 2, 0):i], default=0) > 4000 for c in (a, b) for i, n in enumerate(c))
        assert any(n > 4096 for n in cuts) and any(hist < n <= 4096 for n in cuts)
    # every run is ragged; one stream gets 0 frames in a run where another gets thousands
    assert all(x != y for x, y in zip(a, b))
    assert any(x == 0 and y > 1000 for x, y in zip(a, b)) and any(y == 0 and x > 1000 for x, y in zip(a, b))


@pytest.mark.parametrize("variant", VARIANTS)
def test_ramps_meet_block_edges(cm, variant):
    """block edges strictly inside a ramp, a block wholly inside one, a retarget mid-ramp, blocks after a ramp's end"""
    case = TG.chain_case(cm, variant)
    seen = set()
    for s in (0, TG.STREAMS - 1):                                # a stream of either bus
        m = TG.TR.RampModel(TG.matrices(variant, 0)[s])
        for r, blk in enumerate(case.blocks):
            if r in TG.RAMPS:
                if m.ramping() and 0 < m.done:
                    seen.add("retarget mid-ramp")
                m.ramp(TG.matrices(variant, 1 if r == 2 else 2)[s], TG.RAMPS[r])
            before, n = m.done, blk.src_counts[s]
            was = m.ramping()
            m.done = min(m.R, m.done + n) if was else m.done
            if was and n and 0 < before and m.done < m.R:
                seen.add("a block wholly inside")
            if was and 0 < m.done < m.R:
                seen.add("an edge inside")
            if not was and n and r > max(TG.RAMPS):
                seen.add("a block after the end")
    assert seen == {"retarget mid-ramp", "a block wholly inside", "an edge inside", "a block after the end"}, seen


@pytest.mark.parametrize("variant", VARIANTS)
def test_block_by_block_equals_the_whole_signal(cm, variant):
    case = TG.chain_case(cm, variant)
    v, co = case.v, case.v["co"]
    L, M, T, H = case.table
    # where the ramp calls fall, in each stream's resampled frames
    at = {r: [sum(blk.src_counts[s] for blk in case.blocks[:r]) for s in range(TG.STREAMS)] for r in TG.RAMPS}
    mixed = []
    for s, x in enumerate(case.xs):
        y = TG.TS.Model(L, M, H, v["ci"]).run(x)
        assert y.shape[0] == sum(blk.src_counts[s] for blk in case.blocks)
        m = TG.TR.RampModel(TG.matrices(variant, 0)[s])
        parts, lo = [], 0
        for r in sorted(TG.RAMPS):
            parts.append(m.run(y[lo:at[r][s]]))
            lo = at[r][s]
            m.ramp(TG.matrices(variant, 1 if r == 2 else 2)[s], TG.RAMPS[r])
        parts.append(m.run(y[lo:]))
        mixed.append(np.concatenate(parts))
        assert m.state()[:2] == case.model.ramp[s].state()[:2]
    sums = TG.TB.model_bus(mixed, TG.routing(co), TG.BUSES, co)
    zero = np.zeros((TG.TL.geometry(TG.LOOKAHEAD_LOG2, TG.HOLD)[3], co), dtype=np.int16)
    for b in range(TG.BUSES):
        whole, s = TG.TL.model_lim(sums[b], zero, v["threshold"], v["drive"], TG.LOOKAHEAD_LOG2, TG.HOLD)
        blocks = TG.programme(case, b)
        assert blocks.shape == whole.shape and np.array_equal(blocks, whole), b
        assert case.model.lim.gmin[b] == int(s.min())
        assert np.array_equal(np.concatenate(case.model.lim.s[b]), s)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_chain_is_dense(cm, variant):
    case = TG.chain_case(cm, variant)
    T = case.v["threshold"]
    for b in range(TG.BUSES):
        s = np.concatenate(case.model.lim.s[b])
        unity, change = float((s == TG.UNITY).mean()), float((np.diff(s) != 0).mean())
        peak = int(np.abs(TG.programme(case, b).astype(np.int64)).max())
        print("chain %s bus %d: %d frames, limiter at unity %.1f %%, changing %.1f %%, peak %d (threshold %d), min gain %d"
              % (variant, b, s.size, 100 * unity, 100 * change, peak, T, case.model.lim.gmin[b]))
        assert UNITY_SHARE[0] <= unity <= UNITY_SHARE[1] and change >= CHANGE_SHARE
        assert peak == T                                         # the ceiling is reached, never passed
    for name, outs in (("mixer", case.model.mixed), ("bus", case.model.summed)):
        share = sum(TG.TB.saturated(y) for y in outs) / sum(y.size for y in outs)
        print("chain %s: saturated %s outputs %.2f %%" % (variant, name, 100 * share))
        assert share <= SATURATED_MAX
