"""CPU: the host side of the phase-correlation meter -- the finish in double, the result struct's layout and the
launcher's plan.  No device is touched.

Bar: bit-exact.  cmhip_corr_value and cmhip_corr_balance_db are compared as bit patterns with the formulas of
include/coolmic_hip.h evaluated here: int -> double conversions by float(), math.sqrt (correctly rounded), IEEE
products and quotients, and libm's log10 through ctypes -- the function the library itself calls.
"""
import ctypes as C
import math
import struct

import pytest

_libm = C.CDLL("libm.so.6")
_libm.log10.restype = C.c_double
_libm.log10.argtypes = [C.c_double]

# A window whose unclamped quotient is 0x1.0000000000001p+0: cross = isqrt(ea * eb), so the three sums respect
# Cauchy-Schwarz, yet the product's and the root's roundings leave the divisor one unit below the dividend.  Found by a
# random search over sums in [2^61, 2^63) (about one draw in 10^5 does it); none exists among ea, eb < 3000.
OVER = (9160161135367988464, 6924904945536772599, 7964499051931861534)


def _bits(x):
    return struct.pack("<d", x)


def _unclamped(ea, eb, x):
    return float(x) / math.sqrt(float(ea) * float(eb))


def corr(ea, eb, x):
    if ea == 0 or eb == 0:
        return 0.0
    return min(1.0, max(-1.0, _unclamped(ea, eb, x)))


def balance(ea, eb):
    if ea == 0 and eb == 0:
        return 0.0
    if eb == 0:
        return math.inf
    return 10.0 * _libm.log10(float(ea) / float(eb)) if ea else -math.inf


CASES = [
    (0, 0, 0), (0, 5, 0), (5, 0, 0), (0, 2**63, 0), (2**63, 0, 0),
    (1, 1, 1), (9, 25, -15), (9, 25, 15), (7, 7, 7), (7, 7, -7),
    (4103 * 2**30, 4103 * 2**30, 4103 * 2**30),
    (4103 * 2**30, 4103 * 32767**2, -4103 * 32768 * 32767),
    (12345678901, 12345678901, -12345678901),
    # near 2^62 the conversions to double round (odd values have no double)
    (2**62 + 1, 2**62 + 1, 2**62 + 1), (2**62 + 1, 2**62 + 1, -(2**62 + 1)),
    (2**62 + 513, 2**62 - 511, 2**62 - 1023), (2**62 - 1, 2**62 + 3, -(2**62 - 5)),
    (2**63 - 1, 2**63 - 1, 2**63 - 1), (2**64 - 1, 2**64 - 1, -2**63), (2**64 - 1, 1, 2**31),
    (3, 5, 1), (1000001, 999999, 12345), (2**40 + 7, 2**50 + 9, -(2**44 + 3)),
    OVER, (OVER[0], OVER[1], -OVER[2]),
]


@pytest.mark.parametrize("ea,eb,x", CASES)
def test_finish_is_bit_equal_to_the_formula(cm, ea, eb, x):
    got_c, got_b = cm.corr_value(ea, eb, x), cm.corr_balance_db(ea, eb)
    print("corr", ea, eb, x, "->", got_c.hex(), "want", corr(ea, eb, x).hex(), "| balance", got_b, "want", balance(ea, eb))
    assert _bits(got_c) == _bits(corr(ea, eb, x))
    assert _bits(got_b) == _bits(balance(ea, eb))


def test_literal_values(cm):
    assert _bits(cm.corr_value(0, 0, 0)) == _bits(0.0) and _bits(cm.corr_balance_db(0, 0)) == _bits(0.0)
    assert _bits(cm.corr_value(0, 9, 0)) == _bits(0.0) and _bits(cm.corr_value(9, 0, 0)) == _bits(0.0)
    assert cm.corr_balance_db(0, 9) == -math.inf and cm.corr_balance_db(9, 0) == math.inf
    for e in (1, 25, 4103 * 2**30, 2**62 + 1, 2**63 - 1):
        assert _bits(cm.corr_value(e, e, e)) == _bits(1.0), e
        assert _bits(cm.corr_value(e, e, -e)) == _bits(-1.0), e
        assert _bits(cm.corr_balance_db(e, e)) == _bits(0.0), e
    assert _bits(cm.corr_value(9, 25, -15)) == _bits(-1.0)
    assert cm.corr_balance_db(100, 1) == 20.0 and cm.corr_balance_db(1, 100) == -20.0


def test_the_clamp_is_needed(cm):
    """OVER: without the clamp the quotient is one unit in the last place above 1"""
    ea, eb, x = OVER
    assert x * x <= ea * eb and x < 2**63
    assert _unclamped(ea, eb, x).hex() == "0x1.0000000000001p+0"
    assert _bits(cm.corr_value(ea, eb, x)) == _bits(1.0)
    assert _bits(cm.corr_value(ea, eb, -x)) == _bits(-1.0)


def test_result_struct_layout(cm):
    R = cm.CorrResult
    assert C.sizeof(R) == 360
    offs = {n: getattr(R, n).offset for n, _ in R._fields_}
    assert offs == {"rate": 0, "channels": 4, "frames": 8, "pairs": 16, "a": 20, "b": 28, "energy_a": 40,
                    "energy_b": 104, "cross": 168, "correlation": 232, "balance_db": 296}
    assert cm.CORR_MAX_PAIRS == 8


def test_struct_layout_in_c(tmp_path):
    """the same figures from the header itself"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include <coolmic_hip.h>
#define O(f) (unsigned)offsetof(coolmic_correlation_result_t, f)
int main(void)
{
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %d\\n", (unsigned)sizeof(coolmic_correlation_result_t), O(rate),
           O(channels), O(frames), O(pairs), O(a), O(b), O(energy_a), O(energy_b), O(cross), O(correlation),
           O(balance_db), CMHIP_CORR_MAX_PAIRS);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [360, 0, 4, 8, 16, 20, 28, 40, 104, 168, 232, 296, 8]


def _plan(cm, streams, channels, frames, npairs=1):
    p = cm.plan_corr(streams, channels, frames, npairs)
    return p.err, p.fast, p.grid, p.block, p.chunks


def test_plan(cm):
    """the fast kernel: one wave per 2048 stereo frames; the other: one workgroup of 256 threads per 1024 frames"""
    ok = 0
    # mono has no pair: nothing to launch
    assert _plan(cm, 4, 1, 4096) == (ok, 0, 0, 0, 0)
    # stereo, one pair: k_corr_fast
    assert _plan(cm, 1, 2, 1) == (ok, 1, 1, 64, 1)
    assert _plan(cm, 1, 2, 2048) == (ok, 1, 1, 64, 1)
    assert _plan(cm, 1, 2, 2049) == (ok, 1, 2, 64, 2)
    assert _plan(cm, 7, 2, 4103) == (ok, 1, 21, 64, 3)
    assert _plan(cm, 4096, 2, 65536) == (ok, 1, 4096 * 32, 64, 32)
    # stereo with several pairs, and every other channel count: k_corr_any
    assert _plan(cm, 3, 2, 2051, 2) == (ok, 0, 9, 256, 3)
    for ch in (3, 6, 16):
        for npairs in (1, 3, 8):
            assert _plan(cm, 1, ch, 1, npairs) == (ok, 0, 1, 256, 1)
            assert _plan(cm, 1, ch, 1024, npairs) == (ok, 0, 1, 256, 1)
            assert _plan(cm, 5, ch, 1025, npairs) == (ok, 0, 10, 256, 2)
    # nothing to launch
    assert _plan(cm, 0, 2, 100) == (ok, 0, 0, 0, 0)
    assert _plan(cm, 3, 2, 0) == (ok, 0, 0, 0, 0)
    assert _plan(cm, 3, 17, 100) == (ok, 0, 0, 0, 0)
    assert _plan(cm, 3, 6, 100, 0) == (ok, 0, 0, 0, 0) and _plan(cm, 3, 6, 100, 9) == (ok, 0, 0, 0, 0)
    # a grid of 2^31 workgroups is refused, one below is not
    invalid = 1                                      # hipErrorInvalidValue
    assert _plan(cm, 2**20, 2, 2048 * 2048) == (invalid, 0, 0, 0, 0)
    assert _plan(cm, 2**20, 2, 2048 * 2047) == (ok, 1, 2**20 * 2047, 64, 2047)
    assert _plan(cm, 2**21, 6, 1024 * 1024) == (invalid, 0, 0, 0, 0)
    assert _plan(cm, 2**21, 6, 1024 * 1023) == (ok, 0, 2**21 * 1023, 256, 1023)


def test_debug_count_exists(cm):
    n = cm.lib.cmhip_debug_corr_count()              # (passes launched by this process so far)
    assert isinstance(n, int) and n >= 0
