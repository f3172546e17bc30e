"""GPU: every form of the pipelined EQ kernel (k_eq_pipe<NSEC, G, CH>, csrc/k_eq.hip) against the oracle, bit for bit.

1. the instantiation matrix: 1..4 sections x 12 channel counts (mono, stereo and the any-count form with odd counts,
   even counts that divide 32 and even counts that share streams with the neighbouring workgroup), three output sets,
   three launches with deterministic ragged counts -- among them a launch in which every other stream idles with
   filter state while its neighbours run whole blocks;
2. per-stream coefficients, one role at a time (R lanes, T-in lanes, T-ff lanes), with a coefficient change and a
   cmhip_batch_eq_reset between two launches;
3. nothing is written past a stream's count or into a neighbour (sentinels, in place: the uploaded samples, float
   planes: the launch before);
4. the float -> int16 conversion on all 65 536 inputs through filters whose arithmetic is exact: ties and both
   saturation edges by construction, against a closed form in numpy integers as well as the oracle.

Expected values are oracle.eq_run_mono, once per channel, computed once per case and shared by the output sets and by
tests/test_eq_forms_host.py, which checks on the CPU that the oracle alone meets the conditions the cases rely on."""
import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu

T = 200                                  # three whole 64-frame blocks and one of 8
NSECS = (1, 2, 3, 4)
CHANS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 16)
# A stream's count in launch 0 is entry s mod len, in launch 2 the same of the reversed list.  The first sixteen make
# ends at and beside every block border; the last six add the ends n = 2 .. 6 (mod 8) that the sixteen lack, at the
# end of the list so that the few streams of the wide cases (six at 15 and 16 channels) meet them in launch 2.
COUNTS = [T, 0, 1, 63, 64, 65, 127, 128, 129, T - 1, 3, 4, 5, 7, 8, 9, 2, 6, 66, 67, 68, 69]
SENTINEL = 0x5a5a


def streams_of(C):
    return 70 // C + 2                   # 72-96 rows: three workgroups of 32, the last with idle rows except at C = 16


def counts(S, launch):
    if launch == 1:                      # every other stream idles a whole launch beside neighbours running whole blocks
        return [T if s % 2 == 0 else 0 for s in range(S)]
    lst = COUNTS if launch == 0 else COUNTS[::-1]
    return [lst[s % len(lst)] for s in range(S)]


def shared_coef(cm, nsec):
    return np.concatenate([cm.eq3(48000.0), cm.design_biquad(1, 48000.0, 3000.0, 4.0, 2.0)])[: 5 * nsec].copy()


def _biquads(coef, nsec):
    q = (of.Biquad * max(nsec, 1))()
    for i in range(nsec):
        q[i].b0, q[i].b1, q[i].b2, q[i].a1, q[i].a2 = [float(v) for v in coef[5 * i:5 * i + 5]]
    return q


class Rows:
    """the oracle's run of one stream: one mono filter per channel, state carried from block to block"""

    def __init__(self, oracle, coef, nsec, C, gain=None, cmap=None):
        self.oracle, self.nsec, self.C, self.cmap = oracle, nsec, C, cmap
        self.set_coef(coef)
        self.g = []
        for c in range(C):
            g = None
            if gain is not None:
                rc, g = oracle.gain(1, 1, gain[0], [gain[1][c]])
                assert rc == 0
            self.g.append(g)
        self.state = [np.zeros(4 * max(nsec, 1), dtype=np.float32) for _ in range(C)]

    def set_coef(self, coef):
        self.q = _biquads(coef, self.nsec)

    def reset(self):
        for st in self.state:
            st[:] = 0

    def run(self, x, state=None):
        """x int16 [n][C] -> (interleaved int16 [n * C], [C] float planes)"""
        n = x.shape[0]
        pcm = np.empty((n, self.C), dtype=np.int16)
        planes = []
        for c in range(self.C):
            src = c if self.cmap is None else self.cmap[c]
            wf, wi = self.oracle.eq_run_mono(self.g[c], self.q, self.nsec, (state or self.state)[c], x[:, src].copy())
            pcm[:, c] = wi
            planes.append(wf)
        return pcm.reshape(-1), planes

    def zeros(self):
        return [np.zeros_like(st) for st in self.state]


def _vu_of(oracle, C, blocks):
    v = oracle.vu_new(C)
    for blk in blocks:
        oracle.vu_accumulate(v, blk)
    rc, r = oracle.vu_result(v)
    return rc, (of.vu_result_dict(r) if rc == 0 else None)


def _check_vu(b, want, what):
    for s, (rc_o, r_o) in enumerate(want):
        rc_g, r_g = b.vu_result(s)
        assert rc_g == rc_o, (what, s)
        if rc_o == 0:
            assert r_g.as_dict() == r_o, (what, s)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------
# 1. The instantiation matrix

def matrix_case(cm, oracle, nsec, C, lens=None):
    """inputs, parameters and the oracle's results of one case (lens: the three launches' counts, else counts())"""
    def make():
        S = streams_of(C)
        rng = np.random.default_rng(1000 * nsec + C + (500 if lens else 0))
        coef = shared_coef(cm, nsec)
        gains, maps = [], []
        for s in range(S):
            g = None if s < S // 2 else (int(rng.integers(1, 3000)), [int(v) for v in rng.integers(0, 4000, C)])
            m = None if s % 3 == 0 else [int(v) for v in rng.integers(0, C, C)]
            gains.append(g)
            maps.append(m)
        ls = lens if lens else [counts(S, k) for k in range(3)]
        x = [[rng.integers(-32768, 32768, (T, C)).astype(np.int16) for _ in range(S)] for _ in range(3)]  # whole slots
        want = [[None] * S for _ in range(3)]
        state0, zero2, vu = [], [], []
        for s in range(S):
            rows = Rows(oracle, coef, nsec, C, gains[s], maps[s])
            for k in range(3):
                if k == 2:
                    zero2.append(rows.run(x[k][s][:ls[k][s]], state=rows.zeros()))
                want[k][s] = rows.run(x[k][s][:ls[k][s]])
                if k == 0:
                    state0.append([st.copy() for st in rows.state])
            vu.append(_vu_of(oracle, C, [want[k][s][0] for k in range(3)]))
        return dict(S=S, C=C, nsec=nsec, coef=coef, gains=gains, maps=maps, lens=ls, x=x, want=want, state0=state0,
                    zero2=zero2, vu=vu)
    return _cached(("matrix", nsec, C, str(lens)), make)


def output_sets(cm):
    return (cm.EQ | cm.OUT_F32 | cm.OUT_PCM | cm.VU, cm.EQ | cm.OUT_PCM | cm.VU | cm.INPLACE, cm.EQ | cm.OUT_F32)


def _run_matrix(cm, case, flags, frames=None):
    S, C = case["S"], case["C"]
    what = (case["nsec"], C, hex(flags))
    b = cm.Batch(S, C, T, flags=flags)
    assert b.set_eq(-1, case["coef"]) == 0
    for s in range(S):
        if case["gains"][s]:
            assert b.set_gain(s, C, case["gains"][s][0], case["gains"][s][1]) == 0
        if case["maps"][s]:
            assert b.set_chmap(s, case["maps"][s]) == 0
    for k in range(3):
        lens = case["lens"][k]
        for s in range(S):
            b.upload(s, case["x"][k][s])
        if frames:
            b.run(frames[k])
        else:
            b.run(T, frames_per_stream=lens)
        for s in range(S):
            n = lens[s]
            w_pcm, w_planes = case["want"][k][s]
            if flags & cm.OUT_PCM:
                got = b.download(s, T)
                assert np.array_equal(got[:n * C], w_pcm), what + (k, s)
                if flags & cm.INPLACE:           # the input slot past the stream's count: what was uploaded
                    assert np.array_equal(got[n * C:], case["x"][k][s].reshape(-1)[n * C:]), what + (k, s)
            if flags & cm.OUT_F32:
                for c in range(C):
                    assert _same_bits(b.download_f32(s, c, n), w_planes[c]), what + (k, s, c)
    if flags & cm.VU:
        _check_vu(b, case["vu"], what)
    b.close()


@pytest.mark.parametrize("C", CHANS)
@pytest.mark.parametrize("nsec", NSECS)
def test_every_instantiation_and_channel_count(gpu, oracle, nsec, C):
    """float planes, the interleaved int16 result and the VU results of three ragged launches, on each of three output
    sets; in place the slot past a stream's count keeps the uploaded samples"""
    cm = gpu
    case = matrix_case(cm, oracle, nsec, C)
    if C > 1:      # in place with a non-identity map keeps a stream's rows in one workgroup (whole_streams)
        assert any(m is not None and m != list(range(C)) for m in case["maps"])
    for flags in output_sets(cm):
        _run_matrix(cm, case, flags)


SHORT_FRAMES = (1, 64, 65)               # one and two blocks: shorter than the pipeline's 2 * NSEC + 1 steps


def short_case(cm, oracle):
    S = streams_of(16)
    return matrix_case(cm, oracle, 4, 16, lens=[[n] * S for n in SHORT_FRAMES])


def test_four_sections_sixteen_channels_in_launches_shorter_than_the_pipeline(gpu, oracle):
    """<4, 32, 0> at 16 channels uses the LDS to its last byte and keeps the rows' counts in tile padding; frames
    arguments of 1, 64 and 65 without per-stream counts, on a batch of 200 frames"""
    cm = gpu
    case = short_case(cm, oracle)
    for flags in output_sets(cm):
        _run_matrix(cm, case, flags, frames=SHORT_FRAMES)


# ---------------------------------------------------------------------------
# 2. Per-stream coefficients, one role at a time

COEF_CHANS = (1, 2, 6)
COEF_NSECS = (2, 4)
VARIANTS = ("a_last", "b_first", "b_last")   # which coefficients differ from stream to stream, and which lanes read them:
                                             # R lanes (lane % G), T-in lanes (8 tw + lane / 8), T-ff lanes (f_r[p])


SECTION_HZ = (200.0, 1000.0, 6000.0, 3000.0)      # where the shared sections sit (shared_coef)


def stream_filter(cm, s, hz, again=False):
    """a stable RBJ peaking design of stream s's own, around hz (again: the one it changes to between the launches).
    Its poles or zeros replace those of the shared section at hz: near that section's own, stream by stream 1 % apart,
    the spliced filter stays a moderate one -- poles at 200 Hz under zeros at 3 kHz have a gain of thousands, and
    full-range noise through them is a row of saturated samples that looks the same for every stream."""
    return cm.design_biquad(1, 48000.0, hz * 1.01 ** (s - 36) * (1.03 if again else 1.0),
                            -6.0 + 12.0 * (s % 7) / 6.0 + (1.5 if again else 0.0), 1.0 + (s % 3))


def spliced(cm, nsec, variant, s, again=False):
    coef = shared_coef(cm, nsec)
    k = 0 if variant == "b_first" else nsec - 1
    p = stream_filter(cm, s, SECTION_HZ[k], again)
    if variant == "a_last":
        coef[5 * k + 3:5 * k + 5] = p[3:5]
    else:
        coef[5 * k:5 * k + 3] = p[0:3]
    return coef


def coef_case(cm, oracle, C, nsec, variant):
    def make():
        S = streams_of(C)
        rng = np.random.default_rng(77 + C)
        x = [rng.integers(-32768, 32768, (T, C)).astype(np.int16) for _ in range(2)]     # the SAME for every stream
        changed, reset = (1, S - 2), S // 2
        coef1 = [spliced(cm, nsec, variant, s) for s in range(S)]
        coef2 = [spliced(cm, nsec, variant, s, again=True) if s in changed else coef1[s] for s in range(S)]
        want, zero2, vu = [[], []], {}, []
        for s in range(S):
            rows = Rows(oracle, coef1[s], nsec, C)
            want[0].append(rows.run(x[0]))
            rows.set_coef(coef2[s])                  # the history stays
            if s == reset:
                rows.reset()
            if abs(s - reset) <= 1:
                zero2[s] = rows.run(x[1], state=rows.zeros())
            want[1].append(rows.run(x[1]))
            vu.append(_vu_of(oracle, C, [want[0][s][0], want[1][s][0]]))
        return dict(S=S, C=C, nsec=nsec, x=x, coef1=coef1, coef2=coef2, changed=changed, reset=reset, want=want,
                    zero2=zero2, vu=vu)
    return _cached(("coef", C, nsec, variant), make)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nsec", COEF_NSECS)
@pytest.mark.parametrize("C", COEF_CHANS)
def test_coefficients_of_a_streams_own(gpu, oracle, C, nsec, variant):
    """every stream the same input, coefficients that differ in one group only: a lane that took another stream's
    would produce that stream's expected output.  Between the launches two streams change theirs and keep their
    history, one is reset (cmhip_batch_eq_reset) and starts from zeros, all others go on undisturbed."""
    cm = gpu
    case = coef_case(cm, oracle, C, nsec, variant)
    S, what = case["S"], (C, nsec, variant)
    b = cm.Batch(S, C, T, flags=cm.EQ | cm.OUT_F32 | cm.OUT_PCM | cm.VU)
    assert b.set_eq(-1, shared_coef(cm, nsec)) == 0
    for s in range(S):
        assert b.set_eq(s, case["coef1"][s]) == 0
    got2 = {}
    for k in range(2):
        if k == 1:
            for s in case["changed"]:
                assert b.set_eq(s, case["coef2"][s]) == 0
            b.eq_reset(case["reset"])
        for s in range(S):
            b.upload(s, case["x"][k])
        b.run(T)
        for s in range(S):
            w_pcm, w_planes = case["want"][k][s]
            pcm = b.download(s, T)
            assert np.array_equal(pcm, w_pcm), what + (k, s)
            for c in range(C):
                assert _same_bits(b.download_f32(s, c, T), w_planes[c]), what + (k, s, c)
            got2[s] = pcm
    r = case["reset"]
    assert np.array_equal(got2[r], case["zero2"][r][0]), what            # the reset stream: as from zero state
    for s in (r - 1, r + 1):                                             # its neighbours kept theirs
        assert not np.array_equal(got2[s], case["zero2"][s][0]), what + (s,)
    _check_vu(b, case["vu"], what)
    b.close()


# ---------------------------------------------------------------------------
# 3. Nothing is written past a stream's end or into a neighbour

TAIL_CHANS = (1, 2, 3, 5, 6, 12, 16)
TAIL_NSECS = (1, 3)
TAIL_LAUNCHES = (0, 2)
# ext: output array apart (CMHIP_EXTSLOTS); inplace: slots_out == slots_in; inplace_maps: the same with channel maps,
# which keeps a stream's rows in one workgroup (mono has no map but the identity)
TAIL_FORMS = [(C, nsec, mode) for C in TAIL_CHANS for nsec in TAIL_NSECS for mode in ("ext", "inplace", "inplace_maps")
              if not (C == 1 and mode == "inplace_maps")]


def tail_case(cm, oracle, C, nsec, mapped):
    def make():
        S = streams_of(C)
        rng = np.random.default_rng(9000 + 10 * C + nsec)
        coef = shared_coef(cm, nsec)
        maps = [[int(v) for v in rng.integers(0, C, C)] if (mapped and s % 3) else None for s in range(S)]
        lens = [counts(S, k) for k in TAIL_LAUNCHES]
        x = [[rng.integers(-32768, 32768, (T, C)).astype(np.int16) for _ in range(S)] for _ in TAIL_LAUNCHES]
        full, want = [], [[] for _ in TAIL_LAUNCHES]
        vu = []
        for s in range(S):
            if not mapped:                           # the float-plane batch: launch one whole, launch two ragged
                rows = Rows(oracle, coef, nsec, C)
                full.append((rows.run(x[0][s]), rows.run(x[1][s][:lens[0][s]])))
            rows = Rows(oracle, coef, nsec, C, None, maps[s])
            for k in range(len(TAIL_LAUNCHES)):
                want[k].append(rows.run(x[k][s][:lens[k][s]]))
            vu.append(_vu_of(oracle, C, [want[k][s][0] for k in range(len(TAIL_LAUNCHES))]))
        return dict(S=S, coef=coef, maps=maps, lens=lens, x=x, want=want, full=full, vu=vu)
    return _cached(("tail", C, nsec, mapped), make)


@pytest.mark.parametrize("C,nsec,mode", TAIL_FORMS)
def test_int16_result_stops_at_the_streams_count(gpu, oracle, C, nsec, mode):
    """run_slots on mapped arrays, the output filled with a sentinel before every run: below n * C the oracle's
    samples, from n * C to the end of the slot the sentinel -- in place, the uploaded samples"""
    cm = gpu
    case = tail_case(cm, oracle, C, nsec, mode == "inplace_maps")
    S, what = case["S"], (C, nsec, mode)
    inplace = mode != "ext"
    b = cm.Batch(S, C, T, flags=cm.EQ | cm.OUT_PCM | cm.VU | cm.EXTSLOTS | (cm.INPLACE if inplace else 0))
    assert b.stride == T * C
    assert b.set_eq(-1, case["coef"]) == 0
    for s in range(S):
        if case["maps"][s]:
            assert b.set_chmap(s, case["maps"][s]) == 0
    i = cm.MappedPcm(b)
    o = i if inplace else cm.MappedPcm(b)
    try:
        for k in range(len(TAIL_LAUNCHES)):
            lens = case["lens"][k]
            up = np.stack([case["x"][k][s].reshape(-1) for s in range(S)])
            if not inplace:
                o.array[:] = np.int16(SENTINEL)
            i.array[:] = up
            b.run_slots(T, i.dev, o.dev, frames_per_stream=lens)
            b.sync()
            res = o.array.copy()
            for s in range(S):
                n = lens[s] * C
                assert np.array_equal(res[s, :n], case["want"][k][s][0]), what + (k, s)
                rest = up[s, n:] if inplace else np.full(T * C - n, SENTINEL, dtype=np.int16)
                assert np.array_equal(res[s, n:], rest), what + (k, s, "past the count")
            if not inplace:
                assert np.array_equal(i.array, up), what + (k, "the input")
        _check_vu(b, case["vu"], what)
    finally:
        i.free()
        if o is not i:
            o.free()
        b.close()


@pytest.mark.parametrize("nsec", TAIL_NSECS)
@pytest.mark.parametrize("C", TAIL_CHANS)
def test_float_planes_stop_at_the_streams_count(gpu, oracle, C, nsec):
    """launch one runs every stream whole, launch two ragged: frames n .. T - 1 of every plane keep launch one's bits"""
    cm = gpu
    case = tail_case(cm, oracle, C, nsec, False)
    S, what = case["S"], (C, nsec)
    b = cm.Batch(S, C, T, flags=cm.EQ | cm.OUT_F32)
    assert b.set_eq(-1, case["coef"]) == 0
    lens = case["lens"][0]
    for s in range(S):
        b.upload(s, case["x"][0][s])
    b.run(T)
    first = [[b.download_f32(s, c, T) for c in range(C)] for s in range(S)]
    for s in range(S):
        b.upload(s, case["x"][1][s])
    b.run(T, frames_per_stream=lens)
    for s in range(S):
        (_, w1), (_, w2) = case["full"][s]
        n = lens[s]
        for c in range(C):
            assert _same_bits(first[s][c], w1[c]), what + (s, c)
            got = b.download_f32(s, c, T)
            assert _same_bits(got[:n], w2[c]), what + (s, c)
            assert _same_bits(got[n:], first[s][c][n:]), what + (s, c, "past the count")
    b.close()


# ---------------------------------------------------------------------------
# 4. Conversion edges by construction

CONV_CHANS = (1, 2, 3, 6)                # mono, stereo, odd scatter, even swap: staged and direct
CONV_S, CONV_T = 32, 2048                # all 65 536 int16 values, dealt over 32 streams


def _b0_sections(values):
    coef = np.zeros(5 * len(values), dtype=np.float32)
    coef[0::5] = values
    return coef


# name -> (coefficients, the gain of the whole chain): every product and sum is exact in float
CONV_FILTERS = {
    "1.0": (_b0_sections([1.0]), 1.0), "0.5": (_b0_sections([0.5]), 0.5), "1.5": (_b0_sections([1.5]), 1.5),
    "2.0": (_b0_sections([2.0]), 2.0), "-1.0": (_b0_sections([-1.0]), -1.0),
    "2.0*0.5*-1.0*-1.0": (_b0_sections([2.0, 0.5, -1.0, -1.0]), 1.0),
}


def closed_form(x, b0):
    """clip(rne(b0 * x)): b0 * x is an exactly representable double, np.rint rounds halves to even"""
    return np.clip(np.rint(b0 * x.astype(np.float64)), -32768, 32767).astype(np.int16)


def conv_input(C):
    """[CONV_S] arrays int16 [CONV_T][C]: channel c holds the 65 536 values rotated by c"""
    base = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    chans = np.stack([np.roll(base, c) for c in range(C)], axis=1)
    return [chans[s * CONV_T:(s + 1) * CONV_T].copy() for s in range(CONV_S)]


def conv_case(oracle, name, C):
    def make():
        coef, b0 = CONV_FILTERS[name]
        x = conv_input(C)
        want = [Rows(oracle, coef, coef.size // 5, C).run(x[s]) for s in range(CONV_S)]
        vu = [_vu_of(oracle, C, [want[s][0]]) for s in range(CONV_S)]
        return dict(x=x, want=want, vu=vu, closed=[closed_form(x[s], b0).reshape(-1) for s in range(CONV_S)])
    return _cached(("conv", name, C), make)


@pytest.mark.parametrize("name", list(CONV_FILTERS))
@pytest.mark.parametrize("C", CONV_CHANS)
def test_conversion_of_every_int16_value(gpu, oracle, C, name):
    cm = gpu
    coef, _ = CONV_FILTERS[name]
    case = conv_case(oracle, name, C)
    b = cm.Batch(CONV_S, C, CONV_T, flags=cm.EQ | cm.OUT_F32 | cm.OUT_PCM | cm.VU)
    assert b.set_eq(-1, coef) == 0
    for s in range(CONV_S):
        b.upload(s, case["x"][s])
    b.run(CONV_T)
    for s in range(CONV_S):
        got = b.download(s, CONV_T)
        assert np.array_equal(got, case["closed"][s]), (C, name, s, "closed form")
        assert np.array_equal(got, case["want"][s][0]), (C, name, s, "oracle")
        for c in range(C):
            assert _same_bits(b.download_f32(s, c, CONV_T), case["want"][s][1][c]), (C, name, s, c)
    _check_vu(b, case["vu"], (C, name))
    b.close()


WINDOW_T = 4096


def window_case(oracle, C):
    def make():
        x = np.full((WINDOW_T, C), -32768, dtype=np.int16)
        pcm, _ = Rows(oracle, CONV_FILTERS["2.0"][0], 1, C).run(x)
        return dict(x=x, pcm=pcm, vu=_vu_of(oracle, C, [pcm]))
    return _cached(("window", C), make)


@pytest.mark.parametrize("C", CONV_CHANS)
def test_window_of_nothing_but_the_largest_magnitude(gpu, oracle, C):
    """4096 frames of -32768 through b0 = 2.0: every result -32768, the largest sum the packed squares (three to a
    u32) can meet; the peak is -32768, the first of equals, and the power is capped at 0 dB"""
    cm = gpu
    case = window_case(oracle, C)
    b = cm.Batch(1, C, WINDOW_T, flags=cm.EQ | cm.OUT_F32 | cm.OUT_PCM | cm.VU)
    assert b.set_eq(-1, CONV_FILTERS["2.0"][0]) == 0
    b.upload(0, case["x"])
    b.run(WINDOW_T)
    got = b.download(0, WINDOW_T)
    assert (got == -32768).all() and np.array_equal(got, case["pcm"])
    rc_o, r_o = case["vu"]
    rc_g, r_g = b.vu_result(0)
    assert rc_g == rc_o == 0
    r_g = r_g.as_dict()
    assert r_g == r_o
    assert r_g["global_peak"] == -32768 and r_g["channel_peak"] == [-32768] * C
    assert r_g["global_power"] == 0.0 and r_g["channel_power"] == [0.0] * C and r_g["frames"] == WINDOW_T
    b.close()
