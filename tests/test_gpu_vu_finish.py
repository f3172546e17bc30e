"""GPU: the opt-in device-side dB finish of VU windows (CMHIP_VU_FINISH_DEVICE, k_vu_finish) and the group-wide
results (coolmic_group_vumeter_results).

The reference for every dB value is the HOST finish -- oracle_power_db / the host-mode batch, glibc's log10 -- never
another run of the device code.  Integers (peaks, frames, rate, channels, every rc) and the two special values
(-inf for a silent window, 0.0 at full scale) must be exactly equal; the finite dB doubles within ULP_BOUND."""
import ctypes as Ct
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libcoolmic-dsp_amd", "lib")

# Distance, in units of the last place, allowed between a dB double finished on the device and the same value
# finished on the host: the measured maximum over the fixed set of test_device_finish_against_the_host_finish
# plus ONE.  The set is deterministic, so the maximum is a property of the build and the host's libm, not of the
# run; the margin of one is for a host whose log10 differs in a last bit from the one measured on (glibc's log10 is
# not correctly rounded: even a correctly rounded device logarithm ends up to 2 ULP from it after the * 20).
# Above 3 ULP would not be a last-bit effect of log10: then the stage is to be found (out_log of the hook), not
# the bound widened.
# Measured on an MI355X (gfx950, ROCm 7.2 device library) against glibc 2.35 over the 608 183 pairs of ulp_pairs():
# equal 481 515, 1 ULP 98 862, 2 ULP 19 800, none further (profiles/vu_finish_ulp_histogram.txt); -inf
# and 0.0 exact.  The log10 stage alone is 0 / 1 / 2 ULP from glibc's in 152 725 / 47 249 / 89 of the count-1 pairs.
MEASURED_MAX_ULP = 2
ULP_BOUND = None if MEASURED_MAX_ULP is None else MEASURED_MAX_ULP + 1


def _ordered(a):
    """float64 array -> int64 keys whose differences are distances in units of the last place"""
    i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i, i)


def _ulp(a, b):
    """distances between two float64 arrays; where either is not finite: 0 if the bits are equal, else 2^62"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    d = np.abs(_ordered(a) - _ordered(b))
    odd = ~(np.isfinite(a) & np.isfinite(b))
    return np.where(odd, np.where(a.view(np.int64) == b.view(np.int64), 0, np.int64(1) << 62), d)


def ulp_pairs():
    """The fixed, seeded set of (sum, count) pairs.  The 200 061 means p: 1 .. 20 000, the 20 000 up to 2^30, 2^k and
    2^k + 1, 160 000 random below 2^30.  Each mean with count 1; as sum = p * count + r with small counts and with
    counts up to 2^32, 0 <= r < count (the integer division must drop r); sum = 0; means of exactly 2^30."""
    rng = np.random.default_rng(20240607)
    p = np.concatenate([np.arange(1, 20001), np.arange(2 ** 30 - 19999, 2 ** 30 + 1),
                        2 ** np.arange(0, 31), 2 ** np.arange(0, 30) + 1,
                        rng.integers(1, 2 ** 30, 160000)]).astype(np.uint64)
    assert p.size == 200061
    sums, counts = [p], [np.ones_like(p)]
    for hi in (4097, 2 ** 32 + 1):
        c = rng.integers(2, hi, p.size).astype(np.uint64)
        r = (rng.random(p.size) * c).astype(np.uint64)
        r = np.minimum(r, c - np.uint64(1))
        r[::7] = c[::7] - np.uint64(1)                     # the largest remainder there is
        r[3::7] = 0
        sums.append(p * c + r)
        counts.append(c)
    c0 = np.concatenate([np.arange(1, 1001), rng.integers(1, 2 ** 32 + 1, 1000)]).astype(np.uint64)
    sums += [np.zeros_like(c0), c0 - np.uint64(1), np.uint64(2 ** 30) * c0, np.uint64(2 ** 30) * c0 + c0 - np.uint64(1)]
    counts += [c0, c0, c0, c0]                             # (sum = count - 1: a mean below one is a mean of zero)
    return np.concatenate(sums), np.concatenate(counts)


def measure_ulp(cm, oracle, report=print):
    """the ULP test's measurement; reports the histogram of the distances before anything is asserted"""
    sums, counts = ulp_pairs()
    assert int(sums.max()) < 2 ** 63
    db, lg = cm.power_db_device(sums, counts, want_log=True)
    fn = oracle.lib.oracle_power_db
    host = np.array([fn(int(s), int(c)) for s, c in zip(sums.tolist(), counts.tolist())], dtype=np.float64)
    mean = sums // counts
    zero, full = mean == 0, mean == 2 ** 30
    dist = _ulp(db, host)
    hist = np.bincount(np.minimum(dist[~zero & ~full], 64).astype(np.int64))
    report("pairs %d (zero mean %d, full-scale mean %d); %s" % (sums.size, zero.sum(), full.sum(),
                                                                os.confstr("CS_GNU_LIBC_VERSION")))
    report("dB distance device vs host finish, ULP: " + ", ".join("%d: %d" % (k, n) for k, n in enumerate(hist) if n))
    # the stage before the * 20, against the host's libm through CPython's math (diagnosis only, asserts nothing)
    pick = np.flatnonzero((counts == 1) & ~zero)
    hl = np.array([math.log10(math.sqrt(float(m)) / 32768.0) for m in mean[pick].tolist()])
    lh = np.bincount(np.minimum(_ulp(lg[pick], hl), 64).astype(np.int64))
    report("log10 stage (count = 1 pairs) device vs host libm, ULP: " +
           ", ".join("%d: %d" % (k, n) for k, n in enumerate(lh) if n))
    return db, host, zero, full, dist


def test_device_finish_against_the_host_finish(gpu, oracle):
    """vu_power_db on the device (cmhip_test_power_db_device) against oracle_power_db on the host over the fixed set:
    -inf and 0.0 exact, everything else within ULP_BOUND"""
    db, host, zero, full, dist = measure_ulp(gpu, oracle)
    assert zero.sum() > 2000 and full.sum() > 2000
    assert np.all(np.isneginf(host[zero])) and np.all(np.isneginf(db[zero]))
    assert np.all(host[full] == 0.0) and np.all(db[full].view(np.int64) == 0)          # +0.0, bit for bit
    rest = ~zero & ~full
    assert np.all(np.isfinite(db[rest])) and np.all(db[rest] <= 0.0)
    worst = int(dist[rest].max())
    print("measured maximum %d ULP, bound %s" % (worst, ULP_BOUND))
    assert ULP_BOUND is not None and ULP_BOUND <= 4
    assert worst <= ULP_BOUND


def _poisoned(cm, S):
    out, rc = (cm.VuResult * S)(), (Ct.c_int * S)()
    Ct.memset(out, 0xA5, Ct.sizeof(out))
    return out, rc


def _same_but_for_last_bits(cm, host, rc_h, dev, rc_d, S, what):
    """results of a host-mode and a device-mode collect: rc equal, an INVAL result untouched (both arrays were
    poisoned), integers and special values equal, dB within the bound, every other byte equal"""
    assert list(rc_h) == list(rc_d), what
    for s in range(S):
        if rc_h[s] != 0:
            assert rc_h[s] == cm.ERROR_INVAL and bytes(dev[s]) == b"\xa5" * 192 == bytes(host[s]), (what, s)
            continue
        h, d = host[s], cm.VuResult.from_buffer_copy(dev[s])
        ch = h.channels
        hp = np.array([h.global_power] + [h.channel_power[c] for c in range(ch)])
        dp = np.array([d.global_power] + [d.channel_power[c] for c in range(ch)])
        special = np.isneginf(hp) | (hp == 0.0)
        assert np.array_equal(hp[special].view(np.int64), dp[special].view(np.int64)), (what, s, hp, dp)
        assert int(_ulp(hp, dp).max()) <= ULP_BOUND, (what, s, hp, dp, _ulp(hp, dp))
        d.global_power = h.global_power                    # ... and with the doubles set aside, all 192 bytes
        for c in range(ch):
            d.channel_power[c] = h.channel_power[c]
        assert bytes(d) == bytes(h), (what, s, h.as_dict(), dev[s].as_dict())


@pytest.mark.parametrize("C", [1, 2, 6, 16])
def test_twin_batches_one_in_each_mode(gpu, C):
    """the same generated input through a host-finish and a device-finish batch: noise, sine and silence; ragged
    frame counts with streams that get no frame; gains that saturate"""
    cm = gpu
    assert ULP_BOUND is not None
    S, T = 150, 1100
    rng = np.random.default_rng(77 + C)
    twins = [cm.Batch(S, C, T, flags=cm.VU | cm.OUT_PCM) for _ in range(2)]
    assert twins[1].vu_set_finish(cm.VU_FINISH_DEVICE) == 0
    assert [b.vu_get_finish() for b in twins] == [cm.VU_FINISH_HOST, cm.VU_FINISH_DEVICE]
    silent_seen = 0
    for mode, seed in ((cm.GEN_NOISE, 31), (cm.GEN_SINE, 0), (cm.GEN_NULL, 0), (cm.GEN_NOISE, 32)):
        fps = rng.integers(0, T + 1, S).astype(np.uint32)
        fps[[0, 64, S - 1]] = 0                            # streams without a frame
        fps[[1, 65]] = T
        gains = [int(v) for v in rng.integers(200, 4000, C)]       # above the scale: saturates on noise
        got = []
        for b in twins:
            assert b.set_gain(-1, C, 1000, gains) == 0
            if mode == cm.GEN_NOISE and seed == 32:
                assert b.set_gain(-1, C, 1, [60000] * C) == 0       # everything but zeros hits the rails: near 0 dB
            b.generate(mode, seed, T)
            b.run(T, fps)
            b.vu_snapshot()
            out, rc = _poisoned(cm, S)
            b.vu_collect(out, rc)
            got.append((out, rc))
        (host, rc_h), (dev, rc_d) = got
        assert [r == 0 for r in rc_h] == [int(f) > 0 for f in fps]
        _same_but_for_last_bits(cm, host, rc_h, dev, rc_d, S, (C, mode, seed))
        if mode == cm.GEN_NULL:
            for s in range(S):
                if rc_d[s] == 0:
                    silent_seen += 1
                    assert np.isneginf(dev[s].global_power) and np.isneginf(host[s].global_power)
                    assert all(np.isneginf(dev[s].channel_power[c]) for c in range(C))
    assert silent_seen > S // 2
    for b in twins:
        b.close()


def _window_per_block(cm, b, S, blocks, T, seed0):
    """the small-block loop of the bench line: a window per block, up to three snapshots pending, the collect in
    two halves"""
    outs = [_poisoned(cm, S) for _ in range(blocks)]
    collecting = False
    for k in range(blocks):
        b.generate(cm.GEN_NOISE, seed0 + k, T)
        b.run(T)
        b.vu_snapshot()
        if k >= 2:
            assert cm.lib.cmhip_batch_vu_snapshot(b.h) == cm.ERROR_BUSY          # three are pending
            assert b.vu_set_finish(b.vu_get_finish()) == cm.ERROR_BUSY
        if collecting:
            b.vu_collect_end()
            collecting = False
        if k >= 1:
            b.vu_collect_begin(*outs[k - 1])
            assert b.vu_set_finish(b.vu_get_finish()) == cm.ERROR_BUSY
            collecting = True
    b.vu_collect_end()
    b.vu_collect(*outs[blocks - 1])
    return outs


@pytest.mark.parametrize("S,C", [(700, 2), (1500, 1), (520, 6)])
def test_window_per_block_three_pending_collect_in_halves(gpu, S, C):
    """device mode against the same sequence in host mode (S >= 512: the helper pool unpacks)"""
    cm = gpu
    assert ULP_BOUND is not None
    T, blocks = 480, 8
    seqs = []
    for where in (cm.VU_FINISH_HOST, cm.VU_FINISH_DEVICE):
        b = cm.Batch(S, C, T, flags=cm.VU | cm.OUT_PCM)
        assert b.set_gain(-1, C, 1000, [750, 1250, 900, 1000, 300, 2000][:C]) == 0
        assert b.vu_set_finish(where) == 0
        seqs.append(_window_per_block(cm, b, S, blocks, T, 6000))
        out, rc = b.vu_results()                           # a window nobody filled
        assert all(r == cm.ERROR_INVAL for r in rc)
        b.close()
    for k in range(blocks):
        (host, rc_h), (dev, rc_d) = seqs[0][k], seqs[1][k]
        assert all(r == 0 for r in rc_h)
        _same_but_for_last_bits(cm, host, rc_h, dev, rc_d, S, (S, C, k))


def test_setter_rules_and_a_batch_switched_there_and_back(gpu):
    cm = gpu
    assert ULP_BOUND is not None
    S, C, T = 600, 2, 700
    plain = cm.Batch(S, C, T, flags=cm.OUT_PCM)
    assert plain.vu_set_finish(cm.VU_FINISH_DEVICE) == cm.ERROR_INVAL       # no CMHIP_VU
    assert plain.vu_get_finish() == cm.ERROR_INVAL
    plain.close()
    never, switched = (cm.Batch(S, C, T, flags=cm.VU | cm.OUT_PCM) for _ in range(2))
    assert never.vu_get_finish() == cm.VU_FINISH_HOST == switched.vu_get_finish()    # how a batch starts
    assert switched.vu_set_finish(2) == cm.ERROR_INVAL and switched.vu_set_finish(-1) == cm.ERROR_INVAL
    assert switched.vu_get_finish() == cm.VU_FINISH_HOST

    def block(b, seed):
        b.generate(cm.GEN_NOISE, seed, T)
        b.run(T)

    for b in (never, switched):
        assert b.set_gain(-1, C, 1000, [750, 1250]) == 0
    block(switched, 1)
    switched.vu_snapshot()
    assert switched.vu_set_finish(cm.VU_FINISH_DEVICE) == cm.ERROR_BUSY     # a snapshot is pending
    assert switched.vu_get_finish() == cm.VU_FINISH_HOST
    out, rc = _poisoned(cm, S)
    switched.vu_collect_begin(out, rc)
    assert switched.vu_set_finish(cm.VU_FINISH_DEVICE) == cm.ERROR_BUSY     # a collect is under way
    switched.vu_collect_end()
    block(never, 1)
    first = never.vu_results()
    assert bytes(first[0]) == bytes(out) and list(first[1]) == list(rc)
    assert switched.vu_set_finish(cm.VU_FINISH_DEVICE) == 0
    for seed in (2, 3):                                    # two windows finished on the device
        block(switched, seed)
        block(never, seed)
        d, rc_d = _poisoned(cm, S)
        switched.vu_snapshot()
        switched.vu_collect(d, rc_d)
        h, rc_h = _poisoned(cm, S)
        never.vu_snapshot()
        never.vu_collect(h, rc_h)
        _same_but_for_last_bits(cm, h, rc_h, d, rc_d, S, seed)
    assert switched.vu_set_finish(cm.VU_FINISH_HOST) == 0
    for seed in (4, 5):                                    # and back: bit-equal to the batch never switched
        block(switched, seed)
        block(never, seed)
        a, b = switched.vu_results(), never.vu_results()
        assert bytes(a[0]) == bytes(b[0]) and list(a[1]) == list(b[1]) == [0] * S
    # the per-stream call is out of the mode's reach: host-finished, bit-equal, in device mode too
    assert switched.vu_set_finish(cm.VU_FINISH_DEVICE) == 0
    block(switched, 6)
    block(never, 6)
    for s in (0, 1, 300, S - 1):
        (ra, a), (rb, b) = switched.vu_result(s), never.vu_result(s)
        assert ra == rb == 0 and bytes(a) == bytes(b), s
    never.close()
    switched.close()


def test_mono_host_finish_reuses_channel_0_bit_for_bit(gpu, oracle):
    """C = 1: the host finish takes the global power from channel 0 (same arguments) -- against
    oracle_vumeter_result, which computes it a second time, bit for bit; through the collect and the per-stream call"""
    cm = gpu
    S, T = 40, 3000
    b = cm.Batch(S, 1, T, flags=cm.VU | cm.OUT_PCM)
    assert b.set_gain(-1, 1, 1000, [900]) == 0
    _, g = oracle.gain(1, 1, 1000, [900])
    for k in range(2):
        b.generate(cm.GEN_NOISE, 810 + k, T)
        b.run(T)
        if k == 0:
            res, rcs = b.vu_results()
            got = [(rcs[s], res[s]) for s in range(S)]
        else:
            got = [b.vu_result(s) for s in range(S)]
        for s in range(S):
            v = oracle.vu_new(1)
            oracle.vu_accumulate(v, oracle.gain_apply(g, oracle.lcg(810 + k + s, T), 1))
            rc_o, ro = oracle.vu_result(v)
            r_s, r = got[s]
            assert r_s == rc_o == 0
            assert r.as_dict() == of.vu_result_dict(ro), (k, s)
            assert np.float64(r.global_power).view(np.int64) == np.float64(ro.global_power).view(np.int64)
            assert np.float64(r.global_power).view(np.int64) == np.float64(r.channel_power[0]).view(np.int64)
    b.close()


@pytest.mark.parametrize("full", [False, True])
def test_group_results_for_every_slot_in_one_call(gpu, oracle, full):
    """twin groups on the same sources: coolmic_group_vumeter_result per slot on one, coolmic_group_vumeter_results
    on the other -- host mode: all 192 bytes and every rc equal, slots that never got a frame included; device mode:
    within the bound; a second call right after: INVAL for every slot.  (full: the group has as many streams as its
    engine, the results go straight into the caller's array.)"""
    cm = gpu
    assert ULP_BOUND is not None
    C, block, N = 2, 500, 9
    rng = np.random.default_rng(4)
    frames = [int(v) for v in rng.integers(1, 2400, N)]
    frames[2] = frames[N - 1] = 0                          # sources that never deliver a frame
    frames[3] = 4 * block
    groups = []
    for _ in range(2):
        g = cm.Group(C, N if full else N + 5, block, queue_blocks=100)
        for i in range(N):
            src = cm.IoHandle.from_bytes(oracle.lcg(7000 + i, frames[i] * C).tobytes(), chunk=[0, 7, 1024][i % 3])
            assert g.add_stream(src) == i
            src.unref()
            assert g.set_master_gain(i, C, 1000, [700 + 100 * i, 1300]) == 0
        groups.append(g)
    one, all_ = groups
    for g in groups:                                       # two blocks, the second still in flight
        g.pump()
        g.pump()
    out, _ = _poisoned(cm, N)
    out, rc = all_.vumeter_results(out)
    for i in range(N):
        r_i, r = one.vumeter_result(i)
        assert rc[i] == r_i == (0 if frames[i] else cm.ERROR_INVAL), i
        if r_i == 0:
            assert bytes(out[i]) == bytes(r), i
        else:
            assert bytes(out[i]) == b"\xa5" * 192, i
    assert out[3].frames == 2 * block                      # the block in flight counts
    assert all_.set_vu_finish(7) == cm.ERROR_INVAL
    assert all_.set_vu_finish(cm.VU_FINISH_DEVICE) == 0
    for g in groups:
        g.pump()
        g.pump()
    dev, _ = _poisoned(cm, N)
    dev, rc_d = all_.vumeter_results(dev)
    host, rc_h = _poisoned(cm, N)
    for i in range(N):
        r_i, r = one.vumeter_result(i)
        rc_h[i] = r_i
        if r_i == 0:
            Ct.memmove(Ct.byref(host[i]), Ct.byref(r), 192)
    assert sum(1 for r in rc_h if r == 0) >= 3
    _same_but_for_last_bits(cm, host, list(rc_h), dev, rc_d, N, ("group", full))
    dev, _ = _poisoned(cm, N)
    dev, rc_d = all_.vumeter_results(dev)                  # the windows were closed
    assert rc_d == [cm.ERROR_INVAL] * N and bytes(dev) == b"\xa5" * (192 * N)
    assert cm.lib.coolmic_group_vumeter_results(all_.ptr, dev, None) == 0      # rc may be NULL
    for g in groups:
        g.unref()


def test_group_meters_in_c(gpu, oracle, tmp_path):
    """examples/group_meters.c: a plain C server loop on a group that takes every stream's meter every block, with the
    finish on the host and on the device.  Every stream is the 48 kHz sine at unity gain; the meter of the last
    block is the oracle's over those frames -- bit for bit on the host, within the bound on the device."""
    assert ULP_BOUND is not None
    exe = tmp_path / "group_meters"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "group_meters.c"), "-L", LIBDIR, "-lcoolmic-dsp-hip", "-lpthread",
                    "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    streams, block, rounds = 600, 512, 30
    rc_s, sine = oracle.sine_table(48000)
    assert rc_s == 0 and len(sine) == 48
    x = np.tile(np.asarray(sine, dtype=np.int16), rounds * block // 48 + 2)[(rounds - 1) * block: rounds * block]
    v = oracle.vu_new(1)
    oracle.vu_accumulate(v, x)
    _, want = oracle.vu_result(v)
    for where in ("host", "device"):
        out = subprocess.run([str(exe), str(streams), str(block), str(rounds), where], check=True,
                             capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
        assert out[0].startswith("streams %d block %d rounds %d finish %s:" % (streams, block, rounds, where)), out
        assert out[0].endswith("meters %d" % (streams * rounds)), out
        assert len(out) == 3
        for line, s in zip(out[1:], (0, streams - 1)):
            f = line.split()
            assert f[:2] == ["stream", "%d:" % s] and f[2::2] == ["frames", "peak", "power"], line
            assert int(f[3]) == block and int(f[5]) == want.global_peak
            got = float(f[7])
            if where == "host":
                assert got == want.global_power, line
            else:
                assert int(_ulp(np.array([got]), np.array([want.global_power]))[0]) <= ULP_BOUND, line
