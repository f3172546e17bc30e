"""CPU: the host side of the opt-in device-side dB finish (CMHIP_VU_FINISH_DEVICE).  In that mode the collect of a
snapshot only unpacks the record k_vu_finish wrote (csrc/k_misc.hip) -- [word][stream] over S streams:

    [0]              samples accounted (frames * C)
    [1, 1 + C)       channel_power[c], the double's bits
    [1 + C]          global_power, C > 1 only (mono: channel 0's arguments, hence channel 0's bits)
    then ceil((C + 1) / 4) words of int16 peaks, four to a word from bit 0 up: channel 0 .. C - 1, the global peak

cmhip_test_unpack_finished runs that unpack on records made up here; no GPU is involved."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _record(rng, S, Cn, empty=()):
    """a made-up record for S streams of Cn channels -> (uint64 [words][S], what every stream's result must be)"""
    P = 1 if Cn == 1 else Cn + 1
    words = np.zeros((1 + P + (Cn + 1 + 3) // 4, S), dtype=np.uint64)
    assert words.shape[0] <= 1 + 2 * Cn                   # never longer than the raw record of k_vu_pack
    want = []
    for s in range(S):
        frames = 0 if s in empty else int(rng.integers(1, 1 << 40))
        power = [-float(rng.uniform(0.0, 96.0)) for _ in range(Cn + 1)]
        power[int(rng.integers(0, Cn + 1))] = float("-inf") if s % 3 == 0 else 0.0
        if Cn == 1:
            power[1] = power[0]
        peak = [int(v) for v in rng.integers(-32768, 32768, Cn + 1)]
        peak[int(rng.integers(0, Cn + 1))] = -32768 if s % 2 else 32767
        words[0, s] = frames * Cn
        for c in range(Cn):
            words[1 + c, s] = _bits(power[c])
        if Cn > 1:
            words[1 + Cn, s] = _bits(power[Cn])
        for i in range(Cn + 1):
            words[1 + P + i // 4, s] |= np.uint64((peak[i] & 0xFFFF) << (16 * (i % 4)))
        want.append(None if frames == 0 else
                    {"frames": frames, "channel_power": power[:Cn], "global_power": power[Cn],
                     "channel_peak": peak[:Cn], "global_peak": peak[Cn]})
    return words, want


@pytest.mark.parametrize("Cn", [1, 2, 6, 16])
def test_unpack_of_a_finished_record(cm, Cn):
    rng = np.random.default_rng(1000 + Cn)
    S, rate = 37, 44100
    empty = {0, 5, S - 1}
    words, want = _record(rng, S, Cn, empty)
    out = (cm.VuResult * S)()
    C.memset(out, 0xA5, C.sizeof(out))                     # poison: INVAL must leave a result alone
    out, rc = cm.unpack_finished(words, S, Cn, rate, out=out)
    for s in range(S):
        raw = bytes(out[s])
        if want[s] is None:
            assert rc[s] == cm.ERROR_INVAL, s
            assert raw == b"\xa5" * 192, s
            continue
        assert rc[s] == cm.ERROR_NONE, s
        exp = cm.VuResult()                                # every byte the record does not name is zero
        exp.rate, exp.channels, exp.frames = rate, Cn, want[s]["frames"]
        exp.global_peak, exp.global_power = want[s]["global_peak"], want[s]["global_power"]
        for c in range(Cn):
            exp.channel_peak[c] = want[s]["channel_peak"][c]
            exp.channel_power[c] = want[s]["channel_power"][c]
        assert raw == bytes(exp), (Cn, s, out[s].as_dict(), want[s])


def test_mono_record_has_no_global_word(cm):
    """mono: samples, ONE power word, one word of peaks -- three words as the raw record; the global power is
    channel 0's"""
    S = 5
    words = np.zeros((3, S), dtype=np.uint64)
    for s in range(S):
        words[0, s] = 100 + s
        words[1, s] = _bits(-3.25 - s)
        words[2, s] = ((-7 - s) & 0xFFFF) | (((9 + s) & 0xFFFF) << 16)
    out, rc = cm.unpack_finished(words, S, 1)
    assert rc == [0] * S
    for s in range(S):
        r = out[s]
        assert (r.frames, r.channels, r.rate) == (100 + s, 1, 48000)
        assert r.channel_power[0] == -3.25 - s and r.global_power == r.channel_power[0]
        assert (r.channel_peak[0], r.global_peak) == (-7 - s, 9 + s)


def test_a_partial_frame_is_no_frame(cm):
    """the host divides the sample count by C, as the host finish does: fewer samples than a frame -> INVAL"""
    words = np.zeros((5, 2), dtype=np.uint64)
    words[0, 0], words[0, 1] = 1, 2
    out, rc = cm.unpack_finished(words, 2, 2)
    assert rc == [cm.ERROR_INVAL, cm.ERROR_NONE] and out[1].frames == 1
    assert cm.lib.cmhip_test_unpack_finished(None, 1, 1, 48000, out, None) == cm.ERROR_FAULT
    assert cm.lib.cmhip_test_unpack_finished(words.ctypes.data, 1, 17, 48000, out, None) == cm.ERROR_INVAL


def test_new_names_and_macros(cm):
    for name in ("cmhip_batch_vu_set_finish", "cmhip_batch_vu_get_finish", "coolmic_group_vumeter_results",
                 "coolmic_group_set_vu_finish"):
        assert name in cm.SIGNATURES and hasattr(cm.lib, name), name
    for hook in ("cmhip_test_unpack_finished", "cmhip_test_power_db_device"):
        assert hasattr(cm.lib, hook), hook
    header = open(os.path.join(ROOT, "include", "coolmic_hip.h")).read()
    macros = dict(re.findall(r"^#define\s+(CMHIP_VU_FINISH_\w+)\s+(\d+)\s*$", header, flags=re.M))
    assert macros == {"CMHIP_VU_FINISH_HOST": "0", "CMHIP_VU_FINISH_DEVICE": "1"}
    assert (cm.VU_FINISH_HOST, cm.VU_FINISH_DEVICE) == (0, 1)
    # the hooks are not part of the public ABI
    for h in ("include/coolmic_hip.h", "include/coolmic-dsp/group.h"):
        assert "cmhip_test_" not in open(os.path.join(ROOT, h)).read()
    assert cm.lib.cmhip_batch_vu_set_finish(None, 1) == cm.ERROR_FAULT
    assert cm.lib.coolmic_group_set_vu_finish(None, 1) == cm.ERROR_FAULT
    assert cm.lib.coolmic_group_vumeter_results(None, None, None) == cm.ERROR_FAULT
