"""CPU: the drift stage's host side (cmhip_drift_design, _out_frames, _ppm, the servo, the refusals and the mirror
through an object without a device, csrc/drift_plan.h) and an emulation of k_drift.hip's walk -- planes in two copies,
history in the first tile, table rows p and p + 1 in the kernel's form -- held against tests/drift_model.py at the
plan's own tile sizes, and shown to notice three planted mistakes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import drift_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "drift_plan_test.cpp")
ONE, DMAX = DM.ONE, DM.DELTA_MAX
INVAL, FAULT = 0, 0                       # (set from the package below)


@pytest.fixture(scope="module", autouse=True)
def _errors(cm):
    global INVAL, FAULT
    INVAL, FAULT = cm.ERROR_INVAL, cm.ERROR_FAULT


# ---------------------------------------------------------------------------
# host helpers and the design

def test_out_frames_against_the_model(cm):
    rng = np.random.default_rng(1)
    for _ in range(3000):
        delta = int(rng.choice([0, 1, -1, DMAX, -DMAX, int(rng.integers(-DMAX, DMAX + 1))]))
        F = int(rng.choice([0, 1, 2, int(rng.integers(0, 5000))]))
        pos = int(rng.choice([0, 1, ONE - 1, ONE, F * ONE, max(F * ONE - 1, 0), int(rng.integers(0, ONE + delta))]))
        assert cm.drift_out_frames(pos, delta, F) == DM.out_frames(pos, delta, F), (pos, delta, F)
    assert cm.drift_out_frames(0, -DMAX, 255) == 256 and cm.drift_out_frames(ONE - 1 - DMAX, DMAX, 1) == 1
    assert cm.drift_out_frames(ONE, DMAX, 1) == 0
    assert cm.drift_out_frames(0, DMAX + 1, 10) == 0


def test_ppm_both_ways(cm):
    assert cm.drift_ppm(0.0) == 0 and cm.drift_ppm(float("nan")) == 0
    assert cm.drift_ppm(1000.0) == round(1000.0 * ONE / 1e6) == 4294967
    assert cm.drift_ppm(1e9) == DMAX and cm.drift_ppm(-1e9) == -DMAX
    assert cm.drift_ppm(-3000.0) == -12884902
    for d in (0, 1, -1, 858993, DMAX, -DMAX):
        assert cm.drift_to_ppm(d) == d * 1e6 / ONE
        assert cm.drift_ppm(cm.drift_to_ppm(d)) == d


@pytest.mark.parametrize("phi", [5, 6, 7, 8])
@pytest.mark.parametrize("T", [4, 16, 32, 48, 64])
def test_design_properties(cm, phi, T):
    H = cm.drift_design(phi, T)
    assert H.shape == (1 << phi, T) and DM.table_valid(H)
    H1 = DM.with_row_p(H)
    assert (H1.sum(axis=1) == 16384).all()                       # row P too
    assert H[0, 0] == 0 and int(np.abs(H1).sum(axis=1).max()) <= 65535
    if 16 <= T <= 48:
        assert int(np.abs(H1).sum(axis=1).max()) <= 36168        # what the issue's prototype found for T 16..48
    # a constant comes out as the constant at every mu: num = c * 16384 * 32768 whatever mu is
    for c in (-32768, -1, 1, 12345, 32767):
        for p in (0, 1, (1 << phi) - 1):
            a0, a1 = c * int(H1[p].sum()), c * int(H1[p + 1].sum())
            for mu in (0, 1, 16384, 32767):
                assert (a0 * (32768 - mu) + a1 * mu + (1 << 28)) >> 29 == c


def test_design_refusals(cm):
    for phi, T in ((4, 32), (9, 32), (7, 2), (7, 66), (7, 31)):
        rc, h = cm.drift_design_rc(phi, T, cap=1 << 16)
        assert rc == INVAL and not h.any()
    rc, h = cm.drift_design_rc(7, 32, cap=7 * 32)
    assert rc == INVAL and not h.any()
    assert cm.lib.cmhip_drift_design(7, 32, None, 1 << 16) == FAULT


def _sine_snr(y, t, f, fs):
    """SNR in dB of y against the ideal half-scale sine at the instants t (in input frames)"""
    skip = 200
    ideal = 16384.0 * np.sin(2.0 * np.pi * f * t / fs)
    err = y.astype(np.float64) - ideal
    return 10.0 * math.log10(float((ideal[skip:] ** 2).sum()) / float((err[skip:] ** 2).sum()))


def _snr_drift(H, f, ppm_delta, frames=24000, fs=48000.0):
    phi, T = H.shape[0].bit_length() - 1, H.shape[1]
    x = np.rint(16384.0 * np.sin(2.0 * np.pi * f * np.arange(frames) / fs)).astype(np.int64)
    m = DM.DriftModel(1, 1, H)
    m.set(0, ppm_delta)
    y = m.run_stream(0, x.reshape(-1, 1))[:, 0]
    t = np.arange(len(y), dtype=np.float64) * ((ONE + ppm_delta) / ONE) - T / 2.0
    return _sine_snr(y, t, f, fs)


def _snr_src(L, M, H, f, frames=24000, fs=48000.0):
    """cmhip_src's arithmetic (include/coolmic_hip.h, "sample-rate conversion") on the same sine: the same samples, so
    the same frequency as a fraction of the input rate"""
    T = H.shape[1]
    H = H.astype(np.int64)
    x = np.rint(16384.0 * np.sin(2.0 * np.pi * f * np.arange(frames) / fs)).astype(np.int64)
    z = np.concatenate([np.zeros(T - 1, dtype=np.int64), x])
    m = np.arange(-(-frames * L // M), dtype=np.int64)
    n, p = m * M // L, (m * M) % L
    acc = (H[p] * z[(T - 1) + n[:, None] - np.arange(T)[None, :]]).sum(axis=1)
    y = np.clip((acc + 8192) >> 14, -32768, 32767)
    t = m.astype(np.float64) * M / L - (L * T - 1) / 2.0 / L
    return _sine_snr(y, t, f, fs)


def test_quality_of_the_default_against_the_resamplers_table(cm, capsys):
    """Measured here, both on the same samples: the resampler's designed 44100 -> 48000 table gives 78.1 dB at 1 kHz
    and 75.7 dB at 15 kHz; the drift default (phi 7, T 32) 78.4 and 76.0 dB at +200 ppm, 78.4 and 75.9 dB at -3000 ppm.  3 dB is the margin for
    the 15-bit linear interpolation between rows."""
    L, M, T, Hs = cm.src_design(44100, 48000)
    Hd = cm.drift_design()
    for f in (1000.0, 15000.0):
        ref = _snr_src(L, M, Hs, f)
        for ppm in (200.0, -3000.0):
            got = _snr_drift(Hd, f, cm.drift_ppm(ppm))
            with capsys.disabled():
                print("drift quality: %5.0f Hz %+6.0f ppm: %.2f dB, resampler %.2f dB" % (f, ppm, got, ref))
            assert got >= ref - 3.0, (f, ppm, got, ref)


# ---------------------------------------------------------------------------
# the ABI through an object without a device

def _dry(cm, S=3, Cn=2, max_in=4096, table=None):
    return cm.test_drift_without_device(S, Cn, max_in, table=table)


def test_creation_and_its_refusals(cm):
    m = _dry(cm)
    assert m.geometry() == (7, 32) and m.max_out_frames() == DM.out_frames(0, -DMAX, 4096)
    assert m.get(1) == (0, 0, 0, 0)
    m.close()
    H = DM.dense_table(np.random.default_rng(2), 5, 8)
    m = _dry(cm, table=H)
    assert m.geometry() == (5, 8)
    m.close()
    for S, Cn, F in ((0, 2, 16), (1, 0, 16), (1, 17, 16), (1, 2, 0), (1, 16, (1 << 27) + 1)):
        with pytest.raises(cm.CoolmicError):
            _dry(cm, S, Cn, F)
    bad = H.copy()
    bad[0, 0] = 1
    with pytest.raises(cm.CoolmicError):
        _dry(cm, table=bad)
    bad = H.copy().astype(np.int16)
    bad[3, :] = 0
    bad[3, :2] = -32768
    with pytest.raises(cm.CoolmicError):
        _dry(cm, table=bad)
    d = cm.DriftDesc(0, 1, 1, 16, None)
    for phi, T in ((4, 8), (9, 8), (5, 2), (5, 66), (5, 7)):
        assert not cm.lib.cmhip_test_drift_new_dry(C.byref(d), phi, T, np.zeros(512 * 66, dtype=np.int16).ctypes.data)
    assert not cm.lib.cmhip_drift_new(None) and not cm.lib.cmhip_drift_new_table(C.byref(d), 5, 8, None)


def test_every_refusal_changes_nothing(cm):
    m = _dry(cm, 3, 2, 1024)
    m.set(0, 1234)
    m.seek(1, 99)
    m.advance_rc(100, [100, 7, 0])
    before = [m.get(s) for s in range(3)]
    assert m.set_rc(0, DMAX + 1) == INVAL and m.set_rc(0, -DMAX - 1) == INVAL and m.set_rc(3, 0) == INVAL
    assert m.set_rc(-2, 0) == INVAL and m.seek_rc(0, ONE) == INVAL and m.seek_rc(5, 0) == INVAL
    assert cm.lib.cmhip_drift_set(None, 0, 0) == FAULT and cm.lib.cmhip_drift_seek(None, 0, 0) == FAULT
    assert cm.lib.cmhip_drift_reset(None, 0) == FAULT and cm.lib.cmhip_drift_reset(m.h, 3) == INVAL
    assert cm.lib.cmhip_drift_get(m.h, 3, None, None, None, None) == INVAL
    assert cm.lib.cmhip_drift_get(None, 0, None, None, None, None) == FAULT
    assert cm.lib.cmhip_drift_get(m.h, 0, None, None, None, None) == 0
    assert m.advance_rc(2000)[0] == INVAL and m.advance_rc(10, [10, 11, 0])[0] == INVAL
    # the run's own refusals, through stage_run_begin (pointers are never dereferenced)
    a, b, stride = 0x10000, 0x80000, 2048
    run = lambda **k: m.run_rc(k.get("src", a), k.get("ist", stride), k.get("frames", 100), k.get("dst", b),
                               k.get("ost", stride + 8), k.get("fps"))[0]
    assert run(src=None) == FAULT and run(dst=None) == FAULT
    assert run(src=a + 2) == INVAL and run(ist=stride + 4) == INVAL and run(frames=1025) == INVAL
    assert run(fps=[100, 101, 0]) == INVAL and run(ist=192) == INVAL and run(dst=a) == INVAL
    assert run(ost=192) == INVAL                                 # below the run's largest output count
    assert run() == INVAL                                        # no device behind a dry object: refused as well
    assert "no device" in cm.last_error()
    assert cm.lib.cmhip_drift_run(None, a, stride, 1, None, b, stride, None) == FAULT
    assert [m.get(s) for s in range(3)] == before
    assert run(frames=0) == 0 and [m.get(s) for s in range(3)] == before
    assert m.sync() is None and m.hip_stream() == 0
    m.close()


def test_mirror_against_the_model_over_random_cuts(cm):
    rng = np.random.default_rng(3)
    S = 4
    H = DM.dense_table(rng, 5, 4)
    m = _dry(cm, S, 1, 4096, table=H)
    model = DM.DriftModel(S, 1, H)
    for step in range(400):
        op = rng.integers(0, 10)
        s = int(rng.integers(-1, S))
        if op == 0:
            d = int(rng.choice([0, DMAX, -DMAX, int(rng.integers(-DMAX, DMAX + 1))]))
            m.set(s, d)
            model.set(s, d)
        elif op == 1:
            f = int(rng.choice([0, 1, ONE - 1, int(rng.integers(0, ONE))]))
            m.seek(s, f)
            model.seek(s, f)
        elif op == 2:
            m.reset(s)
            model.reset(s)
        else:
            frames = int(rng.integers(0, 600))
            counts = [int(rng.choice([frames, 0, min(1, frames), int(rng.integers(0, frames + 1))])) for _ in range(S)]
            uniform = rng.integers(0, 4) == 0
            rc, got = m.advance_rc(frames, None if uniform else counts)
            assert rc == 0
            for i in range(S):
                F = frames if uniform else counts[i]
                want = DM.out_frames(model.pos[i], model.delta[i], F)
                model.pos[i] = DM.next_pos(model.pos[i], model.delta[i], F)
                model.in_total[i] += F
                model.out_total[i] += want
                assert got[i] == want and 0 <= model.pos[i] < max(ONE + model.delta[i], ONE + DMAX)
        for i in range(S):
            assert m.get(i) == model.get(i), (step, i)
    m.close()


# ---------------------------------------------------------------------------
# the servo

def test_servo_against_the_model(cm):
    rng = np.random.default_rng(4)
    with pytest.raises(cm.CoolmicError):
        cm.Servo(1 << 31, 1, 1)
    for bad in ((1, 25, 1, 1), (1, 1, 25, 1), (1, 1, 1, 0), (1, 1, 1, DMAX + 1)):
        with pytest.raises(cm.CoolmicError):
            cm.Servo(*bad)
    assert cm.lib.cmhip_drift_servo_init(None, 1, 1, 1, 1) == FAULT and cm.lib.cmhip_drift_servo_step(None, 5) == 0
    for _ in range(50):
        args = (int(rng.integers(0, 5000)), int(rng.integers(0, 25)), int(rng.integers(0, 25)), int(rng.integers(1, DMAX + 1)))
        sv, mo = cm.Servo(*args), DM.ServoModel(*args)
        for _ in range(300):
            fill = int(rng.choice([int(rng.integers(0, 10000)), -1, 1 << 31, 0]))
            assert sv.step(fill) == mo.step(fill)
            assert (sv.s.integ, sv.s.delta, sv.s.clamped) == (mo.integ, mo.delta, mo.clamped)
        sv.reset()
        assert (sv.s.integ, sv.s.delta, sv.s.clamped, sv.s.target) == (0, 0, 0, args[0])


SERVO = dict(target=1024, kp_log2=15, ki_log2=6)
SERVO_BLOCK, SERVO_JITTER = 512, 8
# The settled delta's distance from the source's true offset, in ppm, as simulate_servo measures it over the last 2000
# of 12000 blocks and every offset below: the largest single value 73.9 ppm (the jitter of +-8 frames through the
# proportional path alone is +-61 ppm), the mean 2.78 ppm.  Both are asserted with a margin of two.
SERVO_RESIDUAL_PPM, SERVO_MEAN_PPM = 2 * 73.9, 2 * 2.78


def simulate_servo(cm, ppm, blocks=12000, seed=5):
    """A source whose clock runs `ppm` fast delivers about 512 frames per block, with jitter, into an elastic buffer of
    twice the target; the stage takes from it what 512 outputs at the servo's delta need.  -> (fill per block, delta per
    block)"""
    rng = np.random.default_rng(seed)
    sv = cm.Servo(SERVO["target"], SERVO["kp_log2"], SERVO["ki_log2"])
    fill, pos, owed = SERVO["target"], 0, 0.0
    fills, deltas = [], []
    for _ in range(blocks):
        owed += SERVO_BLOCK * (1.0 + ppm * 1e-6)
        arrive = int(owed) + int(rng.integers(-SERVO_JITTER, SERVO_JITTER + 1))
        arrive = max(arrive, 0)
        owed -= arrive
        fill += arrive
        hi = fill                                                              # the most the buffer holds in this block
        delta = sv.step(fill)
        need = ((pos + (SERVO_BLOCK - 1) * (ONE + delta)) >> 32) + 1          # frames that 512 outputs read
        k = DM.out_frames(pos, delta, need)
        assert SERVO_BLOCK <= k <= SERVO_BLOCK + 1
        pos = DM.next_pos(pos, delta, need)
        fill -= need                                                           # (below 0: an underrun)
        fills.append((fill, hi))
        deltas.append(delta)
    return np.array(fills), np.array(deltas)


@pytest.mark.parametrize("ppm", [100, -100, 1000, -1000, 3000, -3000])
def test_servo_holds_the_buffer(cm, ppm, capsys):
    fills, deltas = simulate_servo(cm, ppm)
    assert fills[:, 0].min() >= 0, "underrun"
    assert fills[:, 1].max() <= 2 * SERVO["target"], "past the buffer's capacity"
    settled = np.array([cm.drift_to_ppm(int(d)) for d in deltas[-2000:]])
    residual = float(np.abs(settled - ppm).max())
    with capsys.disabled():
        print("servo %+5d ppm: fill %d..%d, settled residual %.1f ppm (mean %.2f)" %
              (ppm, fills.min(), fills.max(), residual, float(settled.mean() - ppm)))
    assert residual <= SERVO_RESIDUAL_PPM
    assert abs(float(settled.mean()) - ppm) <= SERVO_MEAN_PPM    # the integrator leaves no offset


# ---------------------------------------------------------------------------
# an emulation of the kernel's walk at the plan's own tile sizes

def compile_table(H):
    """drift_compile in numpy: dword [P + 1][T/2 + 1], older | newer << 16"""
    H1 = DM.with_row_p(H)
    T = H1.shape[1]
    w = np.zeros((H1.shape[0], T // 2 + 1), dtype=np.int64)
    w[:, :T // 2] = (H1[:, 1::2] & 0xffff) | ((H1[:, 0::2] & 0xffff) << 16)
    return w


def _s16(v):
    return ((v & 0xffff) ^ 0x8000) - 0x8000


def emulate_run(cm, H, Cn, hist, x, pos, delta, bug=None):
    """One stream's run as k_drift.hip walks it: per tile the planes (copy A, copy B one sample later) with a mask of
    what was written, the history in front, the table's dwords.  Every plane element read must have been written and
    lie inside its plane.  -> (y int16 [K][C], facts)"""
    phi, T = H.shape[0].bit_length() - 1, H.shape[1]
    tab = compile_table(H)
    x = np.asarray(x, dtype=np.int64).reshape(-1, Cn)
    F = x.shape[0]
    K = DM.out_frames(pos, delta, F)
    step = ONE + delta
    facts = dict(tiles=0, table_lds=None, hist_tiles=0, later_hist=0)
    y = np.zeros((K, Cn), dtype=np.int64)
    if K == 0:
        return y.astype(np.int16), facts
    plan = cm.plan_drift(1, Cn, phi, T, K)
    assert plan.grid == plan.chunks and not plan.err
    row, HT = plan.row, T - 1
    facts.update(tiles=plan.chunks, table_lds=plan.table_lds, tile_out=plan.tile_out)
    for k in range(plan.chunks):
        q0 = k * plan.tile_out
        nq = min(plan.tile_out, K - q0)
        tb = pos + q0 * step
        jf, jh = tb >> 32, (tb + (nq - 1) * step) >> 32
        j_lo = jf - (T - 1)
        staged = jh - j_lo + 1
        assert staged <= plan.tile_in and staged + 1 <= row and jh < F
        planes = np.zeros((2 * Cn, row), dtype=np.int64)
        written = np.zeros((2 * Cn, row), dtype=bool)
        npre = min(staged, -j_lo) if j_lo < 0 else 0
        if npre:
            facts["hist_tiles"] += 1
            facts["later_hist"] += k > 0
        for i in range(npre):
            at = HT + j_lo + i
            if bug == "oldest_hist" and at == 0:
                at = 1
            planes[:Cn, i], planes[Cn:, i + 1] = hist[at], hist[at]
            written[:Cn, i] = written[Cn:, i + 1] = True
        jb = max(j_lo, 0)
        if staged > npre:
            seg = x[jb:jh + 1].T
            planes[:Cn, jb - j_lo:jh - j_lo + 1] = seg
            planes[Cn:, jb - j_lo + 1:jh - j_lo + 2] = seg
            written[:Cn, jb - j_lo:jh - j_lo + 1] = written[Cn:, jb - j_lo + 1:jh - j_lo + 2] = True
        q = np.arange(nq)
        t = (tb & (ONE - 1)) + q * step
        a0, f = (t >> 32) + T - 1, t & (ONE - 1)
        p, mu = f >> (32 - phi), (f >> (17 - phi)) & 32767
        sel = np.where(a0 & 1, 0, Cn)
        for c in range(Cn):
            acc0 = np.zeros(nq, dtype=np.int64)
            acc1 = np.zeros(nq, dtype=np.int64)
            for kk in range(T // 2 - (1 if bug == "drop_last_pair" else 0)):
                d = (a0 >> 1) - kk
                lo, hi = 2 * d, 2 * d + 1
                assert lo.min() >= 0 and hi.max() < row, "a read outside the plane"
                assert written[sel + c, lo].all() and written[sel + c, hi].all(), "a read of what was never staged"
                older, newer = planes[sel + c, lo], planes[sel + c, hi]
                k0 = tab[p, kk]
                k1 = tab[p if bug == "row_p1_as_p" else p + 1, kk]
                acc0 += _s16(k0) * older + _s16(k0 >> 16) * newer
                acc1 += _s16(k1) * older + _s16(k1 >> 16) * newer
            num = acc0 * (32768 - mu) + acc1 * mu
            y[q0:q0 + nq, c] = np.clip((num + (1 << 28)) >> 29, -32768, 32767)
    return y.astype(np.int16), facts


def full_scale_noise(rng, frames, channels):
    x = rng.integers(-32768, 32768, size=(frames, channels))
    if frames >= 16:
        x[rng.integers(0, frames, size=frames // 16)] = 32767
        x[rng.integers(0, frames, size=frames // 16)] = -32768
    return x.astype(np.int64)


# (phi, T, channels, delta, seek, runs of frames): what the GPU test runs on the device as well
EMU_CASES = [
    (7, 32, 2, 858993, 0, [2500, 100, 0, 37]),                  # +200 ppm, two tiles in the first run, table in LDS
    (7, 32, 1, -DMAX, 1, [2200, 1, 30]),                         # the largest ratio, mono pairs
    (5, 64, 2, DMAX, ONE - 1, [14, 1, 0, 14, 40, 50]),           # T = 64 over a history that fills up only in the last run
    (8, 64, 16, -12884902, 123456789, [14, 1, 0, 14, 40, 300]),  # the any-channel form, short runs read the table globally
    (6, 4, 3, 1, (1 << 26) - 1, [70, 5]),                        # the shortest filter
    (5, 8, 5, 0, (1 << 27) + (1 << 20), [33, 300]),              # delta 0: one row pair and one mu for every output
]


def emulate_case(cm, case, bug=None, seed=6):
    """-> (whether every output equals the model's, the facts of the walk, the model's saturated share)"""
    phi, T, Cn, delta, seek, runs = case
    rng = np.random.default_rng(seed)
    H = DM.dense_table(rng, phi, T)
    model = DM.DriftModel(1, Cn, H)
    model.set(0, delta)
    model.seek(0, seek)
    same, facts = True, []
    for F in runs:
        x = full_scale_noise(rng, F, Cn)
        hist, pos = model.hist[0].copy(), model.pos[0]
        want = model.run_stream(0, x)
        got, fa = emulate_run(cm, H, Cn, hist, x, pos, delta, bug=bug)
        facts.append(fa)
        same = same and got.shape == want.shape and bool((got == want).all())
    return same, facts, model.saturated / max(model.outputs, 1)


@pytest.mark.parametrize("case", EMU_CASES, ids=lambda c: "phi%d-T%d-c%d" % c[:3])
def test_the_walk_equals_the_model(cm, case):
    same, facts, sat = emulate_case(cm, case)
    assert same
    assert sat < 0.10, sat                                       # a saturated output hides a wrong sum
    assert any(f["hist_tiles"] for f in facts)


def test_the_cases_reach_their_paths(cm):
    facts = {c[:3]: emulate_case(cm, c)[1] for c in EMU_CASES}
    assert facts[(7, 32, 2)][0]["tiles"] == 2 and facts[(7, 32, 2)][0]["table_lds"] == 1
    assert facts[(7, 32, 1)][0]["tiles"] == 2
    assert all(f["table_lds"] == 0 for f in facts[(8, 64, 16)][:5] if f["tiles"])
    assert facts[(8, 64, 16)][5]["table_lds"] == 1 and facts[(8, 64, 16)][5]["tiles"] == 2
    assert {f["table_lds"] for f in facts[(5, 64, 2)] if f["tiles"]} == {0, 1}
    # With |delta| <= 2^24 and T <= 64 a tile of the plan's smallest size, 256 outputs, spans at least 255 input frames:
    # only a stream's FIRST tile can begin inside the history, whatever the case.
    # (Should the plan ever allow tiles below 64 outputs, a case whose second tile starts inside the history must be added.)
    assert not any(f["later_hist"] for fs in facts.values() for f in fs)
    for phi in range(5, 9):
        for T in range(4, 65, 2):
            for Cn in range(1, 17):
                p = cm.plan_drift(1, Cn, phi, T, 100000)
                assert (p.tile_out * (ONE - DMAX)) >> 32 >= T - 1 and p.tile_out >= 256


@pytest.mark.parametrize("bug", ["row_p1_as_p", "drop_last_pair", "oldest_hist"])
def test_the_dense_cases_notice_mistakes(cm, bug):
    """a mistake made on purpose in the emulation is caught by the dense tables"""
    noticed = [not emulate_case(cm, c, bug=bug)[0] for c in EMU_CASES]
    assert all(noticed), noticed


def test_saturation_estimate_of_the_dense_tables(cm):
    """the dense tables are tables the library takes, and under 10 % of the outputs of full-scale noise through one
    saturate (about 0.5 % by estimate); the counts of that run are the mirror's"""
    rng = np.random.default_rng(7)
    for T in (8, 16, 32, 64):
        H = DM.dense_table(rng, 5, T)
        d = _dry(cm, 1, 2, 4000, table=H)
        assert d.geometry() == (5, T)
        d.set(0, 4321)
        m = DM.DriftModel(1, 2, H)
        m.set(0, 4321)
        y = m.run_stream(0, full_scale_noise(rng, 4000, 2))
        rc, got = d.advance_rc(4000)
        assert rc == 0 and got[0] == y.shape[0] and d.get(0) == m.get(0)
        d.close()
        assert m.saturated / m.outputs < 0.10, (T, m.saturated / m.outputs)


# ---------------------------------------------------------------------------
# the stand-alone plan program, the header, the exports, the assembly

def _build_plan_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        PLAN_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_plan_program(tmp_path):
    exe, r = _build_plan_test(tmp_path, "drift_plan_test", [])                # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "drift plan ok:" in out.stdout, out.stdout + out.stderr


def test_plan_program_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_plan_test(tmp_path, "drift_plan_san",
                              ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "drift plan ok:" in out.stdout, out.stdout + out.stderr[-2000:]


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_drift_desc_t d; cmhip_drift_servo_t v; int16_t h[4]; uint32_t k; int32_t dl; uint64_t a;\n"
           "unsigned n;\n"
           "d.device = 0; d.streams = d.channels = 1; d.max_in_frames = 1; d.hip_stream = 0;\n"
           "return (cmhip_drift_new(&d) != 0) + (cmhip_drift_new_table(&d, 5, 4, h) != 0) + cmhip_drift_geometry(0, &n, &n)"
           " + (int)cmhip_drift_max_out_frames(0) + cmhip_drift_set(0, -1, 0) + cmhip_drift_seek(0, -1, 0)"
           " + cmhip_drift_reset(0, -1) + cmhip_drift_get(0, 0, &dl, &a, &a, &a) + cmhip_drift_run(0, 0, 0, 0, 0, 0, 0, &k)"
           " + cmhip_drift_sync(0) + (cmhip_drift_hip_stream(0) != 0) + cmhip_drift_design(5, 4, h, 4)"
           " + (int)cmhip_drift_out_frames(0, 0, 1) + cmhip_drift_ppm(1.0) + (int)cmhip_drift_to_ppm(1)"
           " + cmhip_drift_servo_init(&v, 1, 1, 1, CMHIP_DRIFT_DELTA_MAX) + cmhip_drift_servo_step(&v, 1)"
           " + (cmhip_drift_servo_reset(&v), 0) + (cmhip_drift_free(0), 0) + (int)sizeof(d);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_every_entry_point_is_exported(cm):
    for name in ("new", "new_table", "free", "geometry", "max_out_frames", "set", "seek", "reset", "get", "run", "sync",
                 "hip_stream", "design", "out_frames", "ppm", "to_ppm", "servo_init", "servo_step", "servo_reset"):
        assert hasattr(cm.lib, "cmhip_drift_" + name) and "cmhip_drift_" + name in cm.SIGNATURES, name
    for name in ("drift_new_dry", "drift_advance", "plan_drift"):
        assert hasattr(cm.lib, "cmhip_test_" + name), name
    assert C.sizeof(cm.DriftServo) == 40 and C.sizeof(cm.DriftPlan) == 44


def test_kernel_assembly_names_and_resources():
    """make asm produces build/k_drift.s: it holds the three kernels by name, each issues the 16-bit dot instruction, and
    the resource usage beside it shows that none of them keeps a register in scratch memory"""
    subprocess.run(["make", "-s", "-C", PKG, "build/k_drift.s"], check=True)
    text = open(os.path.join(PKG, "build", "k_drift.s")).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(names) == 3 and sum("k_drift_fast" in n for n in names) == 2 and sum("k_drift_any" in n for n in names) == 1
    assert "v_dot2c_i32_i16" in text or "v_dot2_i32_i16" in text
    usage = open(os.path.join(PKG, "build", "k_drift.usage.txt")).read()
    scratch = {m.group(1): int(m.group(2))
               for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S)}
    assert len(scratch) == 3 and not [n for n in scratch if scratch[n]], scratch
