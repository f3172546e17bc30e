"""CPU: the cases of tests/test_gpu_eq_forms.py, held against the conditions they rely on -- on the oracle alone.

A device test only bites where its case does: a list of counts that never ends a stream at some residue, an idle
launch whose streams hold no state, streams whose coefficients differ but whose results do not, or a conversion sweep
without ties would pass a wrong kernel.  Nothing here needs a GPU; run with -s to see the figures."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_eq_forms_cases",
                                                  os.path.join(ROOT, "tests", "test_gpu_eq_forms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # the signals, counts and cases of the GPU tests


def _any_state(states):
    return any(st.any() for st in states)


def test_counts_end_streams_at_every_residue():
    """a stream's end n * C (mod 8 samples, one 16-byte vector) decides between whole-vector stores and the
    sample-by-sample tails: every residue a channel count can make occurs among the streams of its case"""
    assert TG.COUNTS[:16] == [TG.T, 0, 1, 63, 64, 65, 127, 128, 129, TG.T - 1, 3, 4, 5, 7, 8, 9]
    assert all(0 <= n <= TG.T for n in TG.COUNTS)
    assert {(n + 63) // 64 for n in TG.COUNTS} == {0, 1, 2, 3, 4}              # streams end in every block, or never start
    for C in TG.CHANS:
        S = TG.streams_of(C)
        assert 64 < S * C <= 96 and (S * C % 32 != 0) == (C != 16)            # three workgroups, idle rows
        assert any((s * C) % 32 + C > 32 for s in range(S)) == (32 % C != 0)   # streams straddle workgroup borders
        ends = set()
        for k in (0, 2):
            ends |= {(n * C) % 8 for n in TG.counts(S, k) if n}
        possible = {(n * C) % 8 for n in range(8)}
        print(f"C={C:2d} S={S:2d}: ends n*C mod 8 = {sorted(ends)} of {sorted(possible)}")
        assert ends == possible, C
        one = TG.counts(S, 1)
        assert all(one[s] == (0 if s % 2 else TG.T) for s in range(S))


@pytest.mark.parametrize("nsec", TG.NSECS)
def test_matrix_cases_carry_state_into_the_idle_launch(cm, oracle, nsec):
    for C in TG.CHANS:
        case = TG.matrix_case(cm, oracle, nsec, C)
        S, lens = case["S"], case["lens"]
        for s in range(1, S, 2):                 # idle in launch 1, with the history launch 0 left
            assert lens[1][s] == 0
            if lens[0][s]:
                assert _any_state(case["state0"][s]), (nsec, C, s)
        carried = 0
        for s in range(S):
            if lens[2][s] and (lens[0][s] or lens[1][s]):
                carried += 1
                planes, zero = case["want"][2][s][1], case["zero2"][s][1]
                assert any(not TG._same_bits(planes[c], zero[c]) for c in range(C)), (nsec, C, s)
        assert carried >= S // 2
        assert any(g is None for g in case["gains"]) and any(g is not None for g in case["gains"])
        assert sum(g is None for g in case["gains"]) == S // 2
    case = TG.short_case(cm, oracle)
    assert [set(l) for l in case["lens"]] == [{1}, {64}, {65}] and case["S"] * case["C"] == 96


@pytest.mark.parametrize("variant", TG.VARIANTS)
def test_streams_with_coefficients_of_their_own_differ_at_once(cm, oracle, variant):
    """the int16 results of any two streams differ within the first 64 frames: a lane with a neighbour's coefficients
    cannot produce its own stream's expected block"""
    for C in TG.COEF_CHANS:
        for nsec in TG.COEF_NSECS:
            case = TG.coef_case(cm, oracle, C, nsec, variant)
            S = case["S"]
            for k in range(2):
                heads = {case["want"][k][s][0][:64 * C].tobytes() for s in range(S)}
                assert len(heads) == S, (variant, C, nsec, k)
            # one group of coefficients differs, everything else is shared
            ref = TG.shared_coef(cm, nsec)
            lo, hi = {"a_last": (5 * nsec - 2, 5 * nsec), "b_first": (0, 3), "b_last": (5 * nsec - 5, 5 * nsec - 2)}[variant]
            for s in range(S):
                same = np.ones(5 * nsec, dtype=bool)
                same[lo:hi] = False
                assert np.array_equal(case["coef1"][s][same], ref[same]) and np.array_equal(case["coef2"][s][same], ref[same])
                assert (case["coef2"][s] != case["coef1"][s]).any() == (s in case["changed"])
            assert len({c[lo:hi].tobytes() for c in case["coef1"]}) == S
            r = case["reset"]
            assert r not in case["changed"] and not {r - 1, r + 1} & set(case["changed"])
            assert np.array_equal(case["want"][1][r][0], case["zero2"][r][0])
            for s in (r - 1, r + 1):
                assert not np.array_equal(case["want"][1][s][0], case["zero2"][s][0]), (variant, C, nsec, s)
            print(f"{variant} C={C} nsec={nsec}: {S} streams pairwise distinct in the first 64 frames, both launches")


def test_tail_cases(cm, oracle):
    for C, nsec, mode in TG.TAIL_FORMS:
        case = TG.tail_case(cm, oracle, C, nsec, mode == "inplace_maps")
        if mode == "inplace_maps":
            assert any(m is not None and m != list(range(C)) for m in case["maps"]), (C, nsec)
        else:
            assert all(m is None for m in case["maps"])
        assert any(0 < n < TG.T for n in case["lens"][0]) and 0 in case["lens"][0] and TG.T in case["lens"][0]
    assert TG.SENTINEL == np.int16(TG.SENTINEL)


@pytest.mark.parametrize("name", list(TG.CONV_FILTERS))
def test_oracle_conversion_equals_the_closed_form(oracle, name):
    coef, b0 = TG.CONV_FILTERS[name]
    x = np.arange(-32768, 32768, dtype=np.int64)
    exact = b0 * x.astype(np.float64)
    ties = np.abs(exact - np.trunc(exact)) == 0.5
    closed = TG.closed_form(x, b0).astype(np.int64)
    sat = (exact > 32767) | (exact < -32768)
    print(f"b0 = {name}: ties {ties.mean():.4f}, saturated {sat.mean():.4f}")
    for C in TG.CONV_CHANS:
        case = TG.conv_case(oracle, name, C)
        xs = np.concatenate(case["x"])
        assert xs.shape == (65536, C)
        for c in range(C):
            assert np.array_equal(np.sort(xs[:, c]), x)                       # every value, in every channel
        assert np.array_equal(np.concatenate([w[0] for w in case["want"]]), np.concatenate(case["closed"])), (name, C)
    if name == "0.5":
        assert np.array_equal(ties, x % 2 == 1)
    if name == "1.5":
        assert np.array_equal(ties, x % 2 == 1) and sat.any()
    if name == "2.0":
        assert np.array_equal(closed != 2 * x, np.abs(x) > 16383 + (x < 0)) and (sat == (np.abs(x) > 16383 + (x < 0))).all()
    if name == "-1.0":
        assert closed[0] == 32767 and np.array_equal(closed[1:], -x[1:]) and sat.sum() == 1
    if b0 == 1.0:
        assert np.array_equal(closed, x) and not ties.any() and not sat.any()
    # round half to even, both signs
    assert TG.closed_form(np.array([1, 3, -1, -3]), 0.5).tolist() == [0, 2, 0, -2]


def test_oracle_window_of_the_largest_magnitude(oracle):
    for C in TG.CONV_CHANS:
        case = TG.window_case(oracle, C)
        rc, r = case["vu"]
        assert rc == 0 and (case["pcm"] == -32768).all()
        assert r["global_peak"] == -32768 and r["global_power"] == 0.0 and r["frames"] == TG.WINDOW_T
    assert 3 * 32768 ** 2 < 2 ** 32 <= 4 * 32768 ** 2       # three squares to a u32, and not a fourth
