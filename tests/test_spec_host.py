"""CPU: the host side of the spectrum meter -- the tables, the plain reference of the transform against a numpy int64
model (tests/spec_model.py), the band design, the finish in double, the result struct's layout and the launcher's
plan.  No device is touched.

Bar: bit-exact wherever integers or IEEE operations decide; the tables are held to numpy's values within +-1 (another
libm may round another way) and to their exact entries and symmetries exactly.  The band design and the dB finish are
restated here with libm's pow and log10 through ctypes -- the functions the library itself calls.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from spec_model import Model, octaves

_libm = C.CDLL("libm.so.6")
for _f, _n in ((_libm.log10, 1), (_libm.pow, 2)):
    _f.restype = C.c_double
    _f.argtypes = [C.c_double] * _n

SIZES = (8, 10, 12)
EVERY = (8, 9, 10, 11, 12)


def _bits(x):
    return struct.pack("<d", x)


@pytest.fixture(scope="module")
def models(cm):
    return {n: Model(cm, n) for n in SIZES}


# ---------------------------------------------------------------------------
# tables


@pytest.mark.parametrize("n", EVERY)
def test_window(cm, n):
    N = 1 << n
    w = cm.spec_window(n).astype(np.int64)
    i = np.arange(N)
    want = np.minimum(32767, np.rint(32768 * 0.5 * (1 - np.cos(2 * np.pi * i / N)))).astype(np.int64)
    assert np.abs(w - want).max() <= 1
    assert w[0] == 0 and w[N // 2] == 32767 and w[N // 4] == 16384 and w.min() == 0 and w.max() == 32767
    assert np.array_equal(w[1:], w[1:][::-1])        # win[i] = win[N - i]
    assert abs(int(w.sum()) - 16384 * N) <= N        # mean 1/2


@pytest.mark.parametrize("n", EVERY)
def test_twiddles(cm, n):
    N, Q = 1 << n, 1 << (n - 2)
    wr, wi = (a.astype(np.int64) for a in cm.spec_twiddles(n))
    k = np.arange(N // 2)
    assert np.abs(wr - np.rint(2**30 * np.cos(2 * np.pi * k / N)).astype(np.int64)).max() <= 1
    assert np.abs(wi - np.rint(-2**30 * np.sin(2 * np.pi * k / N)).astype(np.int64)).max() <= 1
    # the exact entries
    assert (wr[0], wi[0]) == (2**30, 0) and (wr[Q], wi[Q]) == (0, -2**30)
    assert wr[Q // 2] == -wi[Q // 2] == wr[3 * Q // 2] * -1 == 759250125      # llround(2^30 / sqrt 2)
    # the symmetries, exactly: the mirror inside the first quarter, and the quarter turn W[k + N/4] = -i W[k]
    q = np.arange(Q + 1)
    assert np.array_equal(wr[Q - q], -wi[q])
    assert np.array_equal(wr[Q:], wi[:Q]) and np.array_equal(wi[Q:], -wr[:Q])


def test_tables_refuse(cm):
    buf = np.zeros(8192, dtype=np.int32)
    for n in (0, 7, 13):
        assert cm.lib.cmhip_spec_window(n, buf.ctypes.data) == cm.ERROR_INVAL
        assert cm.lib.cmhip_spec_twiddles(n, buf.ctypes.data, buf.ctypes.data) == cm.ERROR_INVAL
    assert cm.lib.cmhip_spec_window(8, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_spec_twiddles(8, None, buf.ctypes.data) == cm.ERROR_FAULT
    assert cm.lib.cmhip_spec_twiddles(8, buf.ctypes.data, None) == cm.ERROR_FAULT
    assert not buf.any()


# ---------------------------------------------------------------------------
# the reference block against the model


def _signals(n, rng):
    N = 1 << n
    i = np.arange(N)
    return {
        "noise": rng.integers(-32768, 32768, size=N),
        "dc -32768": np.full(N, -32768),
        "dc 32767": np.full(N, 32767),
        "nyquist": np.where(i & 1, 32767, -32768),
        "nyquist inverted": np.where(i & 1, -32768, 32767),
        "square 16": np.where((i // 8) & 1, -32768, 32767),
        "square 3.5": np.where(((i * 7) // N) & 1, -32768, 32767),
        "silence": np.zeros(N, dtype=np.int64),
    }


@pytest.mark.parametrize("n", SIZES)
def test_block_equals_the_model(cm, models, n):
    m = models[n]
    for name, x in _signals(n, np.random.default_rng(100 + n)).items():
        got = cm.spec_block(n, x)
        want = m.powers(x)
        print("spec block n", n, name, "total", int(want.sum()), "max bin", int(want.max()))
        assert np.array_equal(got, want), (n, name)
        assert int(want.sum()) <= 2**42.4, (n, name)


def test_an_impulse_at_every_position(cm, models):
    m = models[8]
    x = np.zeros((512, 256), dtype=np.int64)
    x[np.arange(256), np.arange(256)] = -32768
    x[256 + np.arange(256), np.arange(256)] = 32767
    want = m.powers(x)
    for r in range(512):
        assert np.array_equal(cm.spec_block(8, x[r]), want[r]), r
    # (the window is 0 at position 0: that impulse is silent)
    assert not want[0].any() and want[128].all()


@pytest.mark.parametrize("n", SIZES)
def test_components_stay_small(cm, n):
    """every component of every stage in the model, over the extreme inputs, stays below 2^30 + 12 (int32 storage
    leaves 2^31)"""
    m = Model(cm, n)
    for x in _signals(n, np.random.default_rng(7)).values():
        m.powers(x)
    print("spec n", n, "largest component", m.max_component, "= 2^%.3f" % math.log2(m.max_component))
    assert m.max_component < 2**30 + 12


@pytest.mark.parametrize("n", SIZES)
def test_a_full_scale_sine_reads_zero_db(cm, models, n):
    N = 1 << n
    for k0 in (N // 16, N // 4 + 3, N // 2 - 2):
        x = np.rint(32767 * np.sin(2 * np.pi * k0 * np.arange(N) / N)).astype(np.int64)
        p = cm.spec_block(n, x)
        assert np.array_equal(p, models[n].powers(x))
        db = cm.spec_db(int(p[k0 - 1:k0 + 2].sum()), 1)
        print("spec n", n, "bin", k0, "reads", db, "dB")
        assert abs(db) < 0.001
        rest = int(p.sum()) - int(p[k0 - 1:k0 + 2].sum())
        assert cm.spec_db(rest, 1) < -80.0           # (the rounding noise of everything else)


# ---------------------------------------------------------------------------
# band design, finish


def design(rate, n, per_octave):
    """the rule of include/coolmic_hip.h, restated"""
    N = 1 << n
    top = N // 2 + 1
    edges = []
    for i in range(-100, 101):
        f = 1000.0 * _libm.pow(2.0, float(2 * i - 1) / (2.0 * float(per_octave)))
        e = min(top, max(1, math.ceil(f * float(N) / float(rate))))
        if not edges or e != edges[-1]:
            edges.append(e)
    return edges


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_band_design(cm, rate):
    for n in EVERY:
        for per in (1, 2, 3):
            want = design(rate, n, per)
            got = cm.spec_design_bands(rate, n, per)
            print("spec design", rate, n, per, "->", got if isinstance(got, int) else len(got) - 1, "bands")
            assert want == sorted(set(want)) and want[0] == 1 and want[-1] == (1 << (n - 1)) + 1
            if len(want) - 1 > 32:
                assert got == cm.ERROR_INVAL, (rate, n, per)
            else:
                assert got == want, (rate, n, per)


def test_band_design_literal(cm):
    # octaves around 1 kHz at 48 kHz, N = 1024 (46.875 Hz per bin): 707.1 Hz -> bin 16, 1414.2 Hz -> bin 31
    e = cm.spec_design_bands(48000, 10, 1)
    assert e[0] == 1 and e[-1] == 513 and 16 in e and 31 in e and e[e.index(16) + 1] == 31
    # a third-octave table that fits: the example's
    assert len(cm.spec_design_bands(48000, 12, 3)) - 1 <= 32


def test_band_design_refuses(cm):
    e = np.full(33, 7, dtype=np.uint16)
    for args in ((0, 10, 3), (48000, 7, 3), (48000, 13, 3), (48000, 10, 0), (48000, 10, 4)):
        assert cm.lib.cmhip_spec_design_bands(*args, e.ctypes.data) == cm.ERROR_INVAL, args
    assert cm.lib.cmhip_spec_design_bands(48000, 10, 3, None) == cm.ERROR_FAULT
    assert (e == 7).all()


def db(power, blocks):
    if blocks == 0:
        return 0.0
    return 10.0 * _libm.log10(float(power) / (float(blocks) * 1649267441664.0))


DB_CASES = [(0, 0), (5, 0), (0, 1), (0, 2**21), (1, 1), (1649267441664, 1), (1649267441664 * 3, 3), (2**42, 1),
            (2**63, 2**21), (2**64 - 1, 1), (2**62 + 1, 4097), (123456789012345, 77), (3, 2**40), (2**53 + 1, 3)]


@pytest.mark.parametrize("power,blocks", DB_CASES)
def test_db_is_bit_equal_to_the_formula(cm, power, blocks):
    got = cm.spec_db(power, blocks)
    print("spec db", power, blocks, "->", got, "want", db(power, blocks))
    assert _bits(got) == _bits(db(power, blocks))


def test_db_literal(cm):
    assert _bits(cm.spec_db(0, 0)) == _bits(0.0) and _bits(cm.spec_db(99, 0)) == _bits(0.0)
    assert cm.spec_db(0, 1) == -math.inf and cm.spec_db(0, 2**30) == -math.inf
    assert _bits(cm.spec_db(1649267441664, 1)) == _bits(0.0) and _bits(cm.spec_db(1649267441664 * 5, 5)) == _bits(0.0)
    assert cm.spec_db(16492674416640, 1) == 10.0
    assert cm.SPEC_DB_REF == 1.5 * 2**40


# ---------------------------------------------------------------------------
# layout, plan


def test_result_struct_layout(cm):
    R = cm.SpecResult
    assert C.sizeof(R) == 4208
    offs = {n: getattr(R, n).offset for n, _ in R._fields_}
    assert offs == {"rate": 0, "channels": 4, "frames": 8, "blocks": 16, "fft_log2": 24, "bands": 28, "selected": 32,
                    "edges": 36, "channel": 102, "power": 112, "db": 2160}
    assert (cm.SPEC_MAX_CHANNELS, cm.SPEC_MAX_BANDS) == (8, 32)


def test_struct_layout_in_c(tmp_path):
    """the same figures from the header itself"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include <coolmic_hip.h>
#include <coolmic-dsp/group.h>
#define O(f) (unsigned)offsetof(coolmic_spectrum_result_t, f)
int main(void)
{
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %d %d\\n", (unsigned)sizeof(coolmic_spectrum_result_t), O(rate),
           O(channels), O(frames), O(blocks), O(fft_log2), O(bands), O(selected), O(edges), O(channel), O(power),
           O(db), CMHIP_SPEC_MAX_CHANNELS, CMHIP_SPEC_MAX_BANDS);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [4208, 0, 4, 8, 16, 24, 28, 32, 36, 102, 112, 2160, 8, 32]


def _plan(cm, streams, channels, frames, n=10, nch=1, nb=10, max_blocks=0):
    p = cm.plan_spec(streams, channels, frames, n, nch, nb, max_blocks)
    return p.err, p.grid, p.block, p.chunks


def test_plan(cm):
    """one workgroup of 256 threads per stream, selected channel and block of the run's largest count, and one more
    per stream and channel for the state"""
    ok = 0
    assert _plan(cm, 1, 1, 1) == (ok, 1, 256, 1)                     # no block completes: the state alone
    assert _plan(cm, 3, 2, 4103, 8, 2, 8, 31) == (ok, 3 * 2 * 32, 256, 32)
    assert _plan(cm, 5, 16, 100, 12, 8, 32, 0) == (ok, 40, 256, 1)
    assert _plan(cm, 4096, 2, 65536, 8, 2, 8, 511) == (ok, 4096 * 2 * 512, 256, 512)
    # nothing to launch
    for bad in ((0, 2, 100), (3, 2, 0), (3, 0, 100), (3, 17, 100), (3, 2, 100, 7), (3, 2, 100, 13),
                (3, 2, 100, 10, 0), (3, 2, 100, 10, 9), (3, 2, 100, 10, 1, 0), (3, 2, 100, 10, 1, 33)):
        assert _plan(cm, *bad) == (ok, 0, 0, 0), bad
    # a grid of 2^31 workgroups is refused, one below is not
    invalid = 1                                      # hipErrorInvalidValue
    assert _plan(cm, 2**20, 2, 100, 10, 2, 10, 1023) == (invalid, 0, 0, 0)
    assert _plan(cm, 2**20, 2, 100, 10, 2, 10, 1022) == (ok, 2**21 * 1023, 256, 1023)


def test_kernel_assembly_has_no_scratch_and_no_register_offset_scalar_load():
    """build/k_spec.s: every size's kernel keeps its registers (a spilled one means a private segment per wave), and no
    scalar load takes a register and an immediate offset together (the form tests/test_abi.py documents)"""
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libcoolmic-dsp_amd")
    subprocess.run(["make", "-s", "-C", pkg, "build/k_spec.s"], check=True)
    text = open(os.path.join(pkg, "build", "k_spec.s")).read()
    assert text.count(".amdhsa_kernel") == 5 and "v_mad_i64_i32" in text
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(pkg, "build", "k_spec.usage.txt")).read()
    spills = {m.group(1): int(m.group(2))
              for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(spills) == 5 and all("k_spec" in n for n in spills) and not any(spills.values()), spills


def test_default_table(cm):
    assert octaves(10) == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 513]


def test_debug_count_exists(cm):
    n = cm.lib.cmhip_debug_spec_count()              # (passes launched by this process so far)
    assert isinstance(n, int) and n >= 0
