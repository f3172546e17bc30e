"""GPU: the planted-pattern table of tests/test_truepeak_edges_host.py on the device -- k_tpeak_any (3..16 channels) and
k_tpeak_fast (mono, stereo) with the worst-case pattern's last frame at every tile edge, inner edge, end of a count and
cut between runs, under gains and channel maps, through the batch and through the group.

Bar: bit-exact, no tolerance anywhere.  Peaks are integers and equal the model's; every dBTP double is bit-equal to the
host formula; the frames are counted (`_check_result` of tests/test_gpu_truepeak.py).  Model, cases and the conditions
that make a case bite are the host file's, which checks them on the CPU; the expected values of a channel count are
computed once and shared by the forms."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_gpu_truepeak_edges",
                                                  os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TH = _load("test_truepeak_edges_host")   # the model, the case table, the expected values
TG = _load("test_gpu_truepeak")          # _check_result

# in place the block kernel overwrites what the true-peak pass and its history read
FORMS = ["VU", "OUT_PCM|VU|INPLACE"]


def _flags(cm, form):
    f = 0
    for name in form.split("|"):
        f |= getattr(cm, name)
    return f


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Cn", TH.CHANNELS)
def test_planted_pattern_at_every_edge(gpu, oracle, Cn, form):
    """one batch, every case of the channel count a stream of it, the scripts in lockstep: step k of every case goes
    into run k (cases with fewer steps, and those whose step k closes the window, get 0 frames), a `take` is tp_result
    on that stream alone"""
    cm, orc = gpu, oracle
    cases = TH.table(Cn)
    want = TH.expected(cm, orc, Cn)
    S, T = len(cases), TH.max_frames(Cn)
    b = cm.Batch(S, Cn, T, flags=_flags(cm, form))
    assert b.set_true_peak(1) == 0
    for s, case in enumerate(cases):
        if case["gains"] is None:
            assert b.set_gain(s, 0, 0, None) == 0
        else:
            assert b.set_gain(s, Cn, TH.SCALE, case["gains"]) == 0
        assert b.set_chmap(s, case["cmap"]) == 0
    taken = [0] * S
    for k in range(max(len(case["steps"]) for case in cases)):
        fps = [0] * S
        for s, case in enumerate(cases):
            st = case["steps"][k] if k < len(case["steps"]) else None
            if st is not None and st[0] == "run":
                fps[s] = st[2]
                if st[1].size:
                    b.upload(s, st[1])           # (with what lies past the count: a decoy's rest of the pattern)
        if max(fps):
            b.run(max(fps), fps)
        for s, case in enumerate(cases):
            if k < len(case["steps"]) and case["steps"][k][0] == "take":
                peaks, frames = want[s][taken[s]]
                taken[s] += 1
                rc, r = b.tp_result(s)
                assert rc == 0, (Cn, form, case["what"])
                TG._check_result(r, peaks, frames, Cn, (Cn, form, case["index"], case["what"], case["gain_kind"],
                                                        case["map_kind"], case["ch"]))
    assert taken == [len(w) for w in want]
    b.close()


GROUP_BLOCK = 5                          # frames per pull (coolmic_iohandle_read fills a block whatever the chunks are)
PUMPS_PER_WINDOW = 3                     # windows close every 15 frames, some of them inside the pattern


@pytest.mark.parametrize("Cn", [2, 6])
def test_group_cuts_the_split_cases_into_short_pulls(gpu, oracle, Cn):
    """coolmic_group_true_peaks over sources that deliver 3 or 7 bytes per read and a group block of 5 frames: the
    engine itself cuts every stream into runs of 5 frames, the planted pattern included, and only the history carries
    the filter over them.  What a window holds is counted by the VU window taken with it, as test_group_true_peaks
    does; the readers take the blocks that have come home after every window, so no stream waits for room in its
    queue"""
    cm, orc = gpu, oracle
    H = cm.tp_coefficients().astype(np.int64)
    cases = [case for case in TH.table(Cn) if case["kind"] == "split"]
    N = len(cases)
    raws = [np.concatenate([st[1][:st[2] * Cn] for st in case["steps"] if st[0] == "run"]) for case in cases]
    total = [x.size // Cn for x in raws]
    grp = cm.Group(Cn, N, GROUP_BLOCK, queue_blocks=2 * PUMPS_PER_WINDOW + 2)
    assert grp.set_true_peak(1) == 0
    wants, chunks, handles = [], [], []
    for i, case in enumerate(cases):
        chunks.append((3, 7)[i % 2])
        src = cm.IoHandle.from_bytes(raws[i].tobytes(), chunk=chunks[i])
        slot = grp.add_stream(src)
        src.unref()
        assert slot == i
        if case["gains"] is not None:
            assert grp.set_master_gain(slot, Cn, TH.SCALE, case["gains"]) == 0
        assert grp.set_channel_map(slot, case["cmap"]) == 0
        wants.append(TH.transform(orc, raws[i], Cn, TH.oracle_gain(orc, Cn, case["gains"]), case["cmap"]))
        handles.append(grp.get_iohandle(slot))
    models = [TH.EdgeModel(H, Cn) for _ in range(N)]
    pos, most, windows, got = [0] * N, [[0] * Cn for _ in range(N)], 0, [b"" for _ in range(N)]

    def read(i, frames):
        """exactly `frames` frames of slot i's PCM, which wait there (a read that finds nothing pumps the group)"""
        k, data = handles[i].read(frames * Cn * 2)
        assert k == frames * Cn * 2, (i, k)
        got[i] += data

    pumps = 0
    while pos != total:
        for _ in range(PUMPS_PER_WINDOW):
            assert grp.pump() >= 0
        pumps += PUMPS_PER_WINDOW
        assert pumps * GROUP_BLOCK < max(total) + PUMPS_PER_WINDOW * GROUP_BLOCK
        out, rc = grp.true_peaks()
        vu, rc_vu = grp.vumeter_results()
        for i in range(N):
            n = vu[i].frames if rc_vu[i] == 0 else 0
            if n == 0:
                assert rc[i] == cm.ERROR_INVAL and pos[i] == total[i], i
                continue
            assert rc[i] == 0 and n == min(GROUP_BLOCK * PUMPS_PER_WINDOW, total[i] - pos[i]), i
            models[i].run(wants[i][pos[i] * Cn:(pos[i] + n) * Cn], n)
            pos[i] += n
            peaks, frames = models[i].take()
            TG._check_result(out[i], peaks, frames, Cn, ("group", Cn, cases[i]["what"], chunks[i], pos[i]))
            most[i] = [max(a, v) for a, v in zip(most[i], peaks)]
            windows += 1
        for i in range(N):                       # the readers: every block but the one on its way
            home = min(total[i], (pumps - 1) * GROUP_BLOCK) - len(got[i]) // (Cn * 2)
            if home:
                read(i, home)
    assert windows == sum(-(-t // (GROUP_BLOCK * PUMPS_PER_WINDOW)) for t in total) > 20 * N
    for i, case in enumerate(cases):             # one of a stream's windows held the pattern's last frame
        if len(got[i]) < wants[i].size * 2:
            read(i, total[i] - len(got[i]) // (Cn * 2))
        assert handles[i].eof() == 1
        assert np.array_equal(np.frombuffer(got[i], np.int16), wants[i]), case["what"]
        if case["gain_kind"] != "below":
            assert [most[i][c] for c in case["planted"]] == [TH.WORST] * len(case["planted"]), case["what"]
        assert all(most[i][c] == 0 for c in range(Cn) if c not in case["planted"]), case["what"]
    for h in handles:
        h.unref()
    grp.unref()
