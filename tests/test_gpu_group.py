"""coolmic_group_t on the GPU: many per-stream pipelines, one launch per block, each stream
still wired through coolmic_iohandle_t on both sides.  Checked against one oracle chain
per stream (PCM read from the group's handles + VU windows)."""
import numpy as np
import pytest

from oracle import oracle_ffi as of

pytestmark = pytest.mark.gpu


def _expect(oracle, x, C, gains, cmap):
    y = oracle.chmap(cmap, x, C) if cmap else x
    _, g = oracle.gain(C, C, 1000, gains)
    return oracle.gain_apply(g, y, C)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_group_pull_driven(gpu, oracle, C):
    cm = gpu
    rng = np.random.default_rng(40 + C)
    N, block = 9, 1000
    grp = cm.Group(C, 16, block, queue_blocks=2)
    xs, params, handles = [], [], []
    for i in range(N):
        frames = int(rng.integers(0, 5000))
        x = oracle.lcg(900 + i, frames * C)
        chunk = int(rng.choice([0, 3, 7, 512, 1024]))          # upstream delivers in odd pieces
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=chunk)
        slot = grp.add_stream(src)
        src.unref()
        assert slot == i
        gains = [int(v) for v in rng.integers(100, 2500, C)]
        cmap = [int(v) for v in rng.integers(0, C, C)] if i % 2 else None
        assert grp.set_master_gain(slot, C, 1000, gains) == 0
        assert grp.set_channel_map(slot, cmap) == 0
        xs.append(x)
        params.append((gains, cmap))
        handles.append(grp.get_iohandle(slot))
    assert grp.streams() == N
    assert grp.set_master_gain(N, C, 1000, [1] * C) == cm.ERROR_INVAL
    # readers pull at different paces; empty queues pump the whole group
    got = [b"" for _ in range(N)]
    active = set(range(N))
    sizes = [64, 1000, 4096, 7 * 2 * C, 100000, 2 * C, 333 * 2 * C, 8192, 2 * C + 1]
    guard = 0
    while active and guard < 100000:
        guard += 1
        for i in list(active):
            n, data = handles[i].read(sizes[i])
            assert n >= 0 and n % (2 * C) == 0
            got[i] += data
            if n == 0 and handles[i].eof() == 1:
                active.discard(i)
    assert not active
    for i in range(N):
        want = _expect(oracle, xs[i], C, *params[i])
        assert np.array_equal(np.frombuffer(got[i], np.int16), want), (C, i)
        rc, r = grp.vumeter_result(i)
        v = oracle.vu_new(C)
        oracle.vu_accumulate(v, want)
        rc_o, r_o = oracle.vu_result(v)
        assert rc == rc_o, (C, i)
        if rc_o == 0:
            assert r.as_dict() == of.vu_result_dict(r_o), (C, i)
    for h in handles:
        h.unref()
    grp.unref()


def test_group_pump_driven_sine_sources(gpu, oracle, golden):
    """64 sine pipelines pumped explicitly: every stream reproduces golden G1"""
    cm = gpu
    N, block = 64, 512
    grp = cm.Group(1, N, block, queue_blocks=100)
    for i in range(N):
        dev = cm.Snddev("sine", 48000, 1)
        h = dev.get_iohandle()
        assert grp.add_stream(h) == i
        h.unref(); dev.unref()
        assert grp.set_master_gain(i, 1, 1000, [1000]) == 0
    for _ in range(94):
        assert grp.pump() == N
    exp = golden["cases"]["G1"]["vu"]
    for i in range(N):
        rc, r = grp.vumeter_result(i)
        assert rc == 0 and r.frames == exp["frames"] and r.global_peak == exp["global_peak"]
        assert r.global_power == exp["global_power"]
    # queues are full now (100 blocks allowed, 94 used): a few more pumps still fit, then stop
    for _ in range(6):
        assert grp.pump() == N
    assert grp.pump() == 0
    grp.unref()


def test_group_equaliser(gpu, oracle):
    """coolmic_group_set_eq(): every stream of a group through the equaliser, block by block
    (state carried between pumps), per-stream coefficients, VU of the filtered PCM"""
    cm = gpu
    C, N, block = 2, 5, 700
    rng = np.random.default_rng(5)
    grp = cm.Group(C, 8, block, queue_blocks=2)
    xs, coefs, handles = [], [], []
    base = cm.eq3(48000.0)
    for i in range(N):
        x = oracle.lcg(300 + i, int(rng.integers(1, 4000)) * C)
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=int(rng.choice([0, 5, 1024])))
        slot = grp.add_stream(src)
        src.unref()
        xs.append(x)
        handles.append(grp.get_iohandle(slot))
    assert grp.set_eq(-1, base) == 0
    assert grp.set_eq(0, base[:10]) == cm.ERROR_INVAL          # a slot cannot change the section count
    for i in range(N):
        c = base.copy()
        c[0] *= np.float32(1.0 - 0.01 * i)                     # per-stream coefficients
        assert grp.set_eq(i, c) == 0
        coefs.append(c)
    got = [b"" for _ in range(N)]
    active = set(range(N))
    while active:
        for i in list(active):
            n, data = handles[i].read(4096)
            got[i] += data
            if n == 0 and handles[i].eof() == 1:
                active.discard(i)
    for i in range(N):
        q = (of.Biquad * 3)()
        for k in range(3):
            q[k].b0, q[k].b1, q[k].b2, q[k].a1, q[k].a2 = [float(v) for v in coefs[i][5 * k:5 * k + 5]]
        frames = xs[i].size // C
        want = np.empty((frames, C), dtype=np.int16)
        for c in range(C):
            st = np.zeros(12, dtype=np.float32)
            _, oi = oracle.eq_run_mono(None, q, 3, st, xs[i].reshape(-1, C)[:, c].copy())
            want[:, c] = oi
        want = want.reshape(-1)
        assert np.array_equal(np.frombuffer(got[i], np.int16), want), i
        rc, r = grp.vumeter_result(i)
        v = oracle.vu_new(C)
        oracle.vu_accumulate(v, want)
        rc_o, r_o = oracle.vu_result(v)
        assert rc == rc_o == 0 and r.as_dict() == of.vu_result_dict(r_o), i
    for h in handles:
        h.unref()
    grp.unref()


def test_group_slow_readers_and_small_blocks(gpu, oracle):
    """The processed PCM stays in the pinned set the kernel wrote until a reader takes it; sets are
    reused in ring order.  Readers of very different pace, sources that deliver a few bytes per pull
    (many small segments), a queue of one block: every byte still arrives once and in order, and the
    VU windows are those of the whole streams."""
    cm = gpu
    C, N, block = 2, 6, 256
    grp = cm.Group(C, 8, block, queue_blocks=1)
    xs, handles = [], []
    for i in range(N):
        x = oracle.lcg(7100 + i, (3000 + 517 * i) * C)
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=[0, 5, 64, 0, 1000, 3][i])
        slot = grp.add_stream(src)
        src.unref()
        assert grp.set_master_gain(slot, C, 1000, [900, 1100]) == 0
        xs.append(x)
        handles.append(grp.get_iohandle(slot))
    got = [b"" for _ in range(N)]
    active = set(range(N))
    rounds = 0
    while active and rounds < 200000:
        rounds += 1
        for i in list(active):
            if i >= 3 and rounds % (7 * i) != 0:       # the last three readers come rarely ...
                if rounds % 3 == 0:
                    grp.pump()                          # ... while the host keeps pumping
                continue
            n, data = handles[i].read([4096, 4, 100000, 8, 512, 2048][i])
            assert n >= 0 and n % (2 * C) == 0
            got[i] += data
            if n == 0 and handles[i].eof() == 1:
                active.discard(i)
    assert not active
    for i in range(N):
        want = _expect(oracle, xs[i], C, [900, 1100], None)
        assert np.array_equal(np.frombuffer(got[i], np.int16), want), i
        rc, r = grp.vumeter_result(i)
        v = oracle.vu_new(C)
        oracle.vu_accumulate(v, want)
        _, r_o = oracle.vu_result(v)
        assert rc == 0 and r.as_dict() == of.vu_result_dict(r_o), i
    for h in handles:
        h.unref()
    grp.unref()


@pytest.mark.parametrize("threads", [1, 5])
def test_group_pull_spread_over_threads(gpu, oracle, threads):
    """coolmic_group_set_pull_threads: the reads of a pump's upstream handles on several threads -- native
    sources (the library's own sine device) and callbacks of the host (here Python's) side by side, ragged
    lengths, pieces of odd sizes.  Every stream's PCM and window as with one thread, i.e. as the oracle's chain."""
    cm = gpu
    C, N, block = 1, 40, 700
    grp = cm.Group(C, N, block, queue_blocks=2)
    assert grp.set_pull_threads(65) == cm.ERROR_INVAL
    assert grp.set_pull_threads(threads) == 0
    rng = np.random.default_rng(55)
    xs, gains, handles = [], [], []
    for i in range(N):
        frames = int(rng.integers(0, 6000))
        if i % 4 == 0:                                   # a native source: one period of the sine device, repeated
            dev = cm.Snddev("sine", 48000, 1)
            src = dev.get_iohandle()
            dev.unref()
            rc, period = cm.sine_period(48000)
            assert rc == 0
            x = np.tile(period, frames // period.size + 1)[:frames]
            frames_limit = frames
        else:
            x = oracle.lcg(300 + i, frames * C)
            src = cm.IoHandle.from_bytes(x.tobytes(), chunk=int(rng.choice([0, 3, 64, 1001])))
            frames_limit = None
        slot = grp.add_stream(src)
        src.unref()
        g = [int(rng.integers(100, 2500))]
        assert grp.set_master_gain(slot, C, 1000, g) == 0
        xs.append((x, frames_limit))
        gains.append(g)
        handles.append(grp.get_iohandle(slot))
    got = [b"" for _ in range(N)]
    active = set(range(N))
    guard = 0
    while active and guard < 100000:
        guard += 1
        for i in list(active):
            x, limit = xs[i]
            want_bytes = 2 * C * x.size
            if limit is not None:                        # the endless source: read what the test compares, no more
                left = want_bytes - len(got[i])
                if left == 0:
                    active.discard(i)
                    continue
                n, data = handles[i].read(min(left, 1400))
            else:
                n, data = handles[i].read(4096)
            assert n >= 0 and n % (2 * C) == 0
            got[i] += data
            if limit is None and n == 0 and handles[i].eof() == 1:
                active.discard(i)
    assert not active
    for i in range(N):
        x, limit = xs[i]
        want = _expect(oracle, x, C, gains[i], None)
        assert np.array_equal(np.frombuffer(got[i], np.int16), want), (threads, i)
    for h in handles:
        h.unref()
    grp.unref()


def _run_group_on(cm, oracle, device, seed):
    """one group made through coolmic_group_new_on(device): 7 stereo streams, PCM and windows against the oracle"""
    rng = np.random.default_rng(seed)
    C, N, block = 2, 7, 900
    grp = cm.Group(C, 8, block, queue_blocks=2, device=device)
    assert grp.device == device and grp.engine()
    xs, params, handles = [], [], []
    for i in range(N):
        x = oracle.lcg(seed * 100 + i, int(rng.integers(1, 4000)) * C)
        src = cm.IoHandle.from_bytes(x.tobytes(), chunk=int(rng.choice([0, 5, 1024])))
        assert grp.add_stream(src) == i
        src.unref()
        gains = [int(v) for v in rng.integers(100, 2500, C)]
        cmap = [1, 0] if i % 2 else None
        assert grp.set_master_gain(i, C, 1000, gains) == 0 and grp.set_channel_map(i, cmap) == 0
        xs.append(x)
        params.append((gains, cmap))
        handles.append(grp.get_iohandle(i))
    for i in range(N):
        got = b""
        while True:
            n, data = handles[i].read(4096)
            got += data
            if n == 0 and handles[i].eof() == 1:
                break
        want = _expect(oracle, xs[i], C, *params[i])
        assert np.array_equal(np.frombuffer(got, np.int16), want), (device, i)
        rc, r = grp.vumeter_result(i)
        v = oracle.vu_new(C)
        oracle.vu_accumulate(v, want)
        rc_o, r_o = oracle.vu_result(v)
        assert rc == rc_o == 0 and r.as_dict() == of.vu_result_dict(r_o), (device, i)
    for h in handles:
        h.unref()
    grp.unref()


def test_groups_on_a_device_of_the_callers_choice(gpu, oracle):
    """coolmic_group_new_on(): the GPU is the caller's choice, not the process-wide $COOLMIC_HIP_DEVICE -- a C host
    with one pipeline per capture stream (ref: src/simple.c:198-200) places stream s on GPU s % N from ONE process.
    Two groups through the call on device 0, bit-exact against the oracle (device 1: the next test)."""
    cm = gpu
    assert not cm.lib.coolmic_group_new_on(cm.device_count(), None, None, 48000, 2, 4, 64, 2)     # no such GPU
    assert not cm.lib.coolmic_group_new_on(-1, None, None, 48000, 2, 4, 64, 2)
    _run_group_on(cm, oracle, 0, 11)
    _run_group_on(cm, oracle, 0, 12)


def test_groups_on_a_second_device_of_the_process(gpu, oracle):
    """the same on device 1, beside a group that stays alive on device 0 (skipped on a one-GPU box: N > 1
    placement in one process is unmeasured on hardware until a box has two)"""
    cm = gpu
    if cm.device_count() < 2:
        pytest.skip("one GPU here: needs a second one")
    keep = cm.Group(2, 4, 256, device=0)
    _run_group_on(cm, oracle, 1, 13)
    _run_group_on(cm, oracle, 1, 14)
    _run_group_on(cm, oracle, 0, 15)
    keep.unref()


def test_stage_device_setters(gpu, oracle):
    """coolmic_transform_set_device / coolmic_vumeter_set_device: valid before the stage has device state of its
    own, BUSY after, INVAL for a GPU the process does not see; the chain's results are the oracle's"""
    cm = gpu
    x = oracle.lcg(77, 2000)
    tr = cm.Transform(48000, 1)
    assert tr.set_device(cm.device_count()) == cm.ERROR_INVAL and tr.set_device(-1) == cm.ERROR_INVAL
    assert cm.lib.coolmic_transform_set_device(None, 0) == cm.ERROR_FAULT
    assert tr.set_device(0) == 0
    src = cm.IoHandle.from_bytes(x.tobytes())
    tr.attach(src); src.unref()
    assert tr.set_master_gain(1, 1000, [1500]) == 0
    h = tr.get_iohandle()
    n, data = h.read(2 * 1000)
    assert n == 2000
    assert tr.set_device(0) == cm.ERROR_BUSY                     # the batch exists now
    _, g = oracle.gain(1, 1, 1000, [1500])
    assert np.array_equal(np.frombuffer(data, np.int16), oracle.gain_apply(g, x[:1000], 1))
    vu = cm.Vumeter(48000, 1)
    assert vu.set_device(cm.device_count()) == cm.ERROR_INVAL and vu.set_device(0) == 0
    src2 = cm.IoHandle.from_bytes(x.tobytes())                   # a meter on a plain source: a launch of its own
    vu.attach(src2); src2.unref()
    assert vu.read(-1) == 1024
    assert vu.set_device(0) == cm.ERROR_BUSY
    rc, r = vu.result()
    v = oracle.vu_new(1)
    oracle.vu_accumulate(v, x[:512])
    _, r_o = oracle.vu_result(v)
    assert rc == 0 and r.as_dict() == of.vu_result_dict(r_o)
    h.unref(); tr.unref(); vu.unref()


def test_streams_that_share_a_source_stay_on_the_pumping_thread(gpu, oracle):
    """coolmic_group_set_pull_threads(4): streams with a source of their own are pulled on four threads; two
    streams that were given the SAME handle, and two with different handles of one sound device (two
    get_iohandle() of it), are recognised at add_stream and read by the pumping thread alone, in slot order -- so
    what each of them gets is what a single-threaded pump gives: alternating blocks of the shared source.  The
    witness here is the data, and a device or one handle is all it covers; the readers of a tee, whose handles
    share neither address nor userdata, and the thread that reads them:
    test_streams_behind_one_tee_stay_on_the_pumping_thread."""
    cm = gpu
    C, N, block, blocks = 1, 20, 256, 6
    grp = cm.Group(C, N, block, queue_blocks=blocks + 2)
    assert grp.set_pull_threads(4) == 0
    shared = oracle.lcg(4242, block * blocks * 2)
    sh = cm.IoHandle.from_bytes(shared.tobytes())
    dev = cm.Snddev("sine", 48000, 1)
    xs, handles = {}, []
    for i in range(N):
        if i in (3, 11):
            src = sh                                                   # one handle, twice
        elif i in (5, 17):
            src = dev.get_iohandle()                                   # two handles, one sine phase behind them
        else:
            xs[i] = oracle.lcg(7000 + i, block * blocks)
            src = cm.IoHandle.from_bytes(xs[i].tobytes())
        assert grp.add_stream(src) == i
        if src is not sh:
            src.unref()
        assert grp.set_master_gain(i, 1, 1000, [1300]) == 0
        handles.append(grp.get_iohandle(i))
    sh.unref(); dev.unref()
    for _ in range(blocks):
        assert grp.pump() == N
    _, g = oracle.gain(1, 1, 1000, [1300])
    rc_s, table = oracle.sine_table(48000)
    sine = np.tile(np.asarray(table, dtype=np.int16), block * blocks * 2 // 48 + 2)
    for i in range(N):
        n, data = handles[i].read(block * blocks * 2)
        got = np.frombuffer(data, np.int16)
        assert n == block * blocks * 2
        if i in (3, 11):                                               # blocks 0, 2, 4 .. / 1, 3, 5 .. of the shared source
            first = 0 if i == 3 else 1
            want = np.concatenate([shared[(2 * k + first) * block:(2 * k + first + 1) * block] for k in range(blocks)])
        elif i in (5, 17):
            first = 0 if i == 5 else 1
            want = np.concatenate([sine[(2 * k + first) * block:(2 * k + first + 1) * block] for k in range(blocks)])
        else:
            want = xs[i]
        assert np.array_equal(got, oracle.gain_apply(g, want, 1)), i
    for h in handles:
        h.unref()
    grp.unref()


# ---- which thread reads a shared source -----------------------------------------------------------------------
# The data cannot tell: two threads inside one tee may well deliver the right bytes, or crash once a week.  The
# witness is the identity of the thread each upstream read came from.

PT_N, PT_BLOCK, PT_PUMPS, PT_THREADS = 48, 256, 12, 4
# The pool hands out chunks of 8 slots and the pumping thread takes chunk 0 while the helpers wake: the sources
# of slots 0..7 sleep this long in every read, which keeps it there (about 8 ms a pump) while the helpers go
# through chunks 1..5 -- where the streams that share a source sit.  (A helper still spinning from the pump
# before may take chunk 0 instead; then two helpers and the pumping thread share the rest.)  1 ms is what the
# MI355X host needed: over two runs of the five cases, between 215 and 456 of the 432 to 456 reads of slots
# 8..47 came from a helper where a tee is in the group, 312 and 480 of 480 where none is.  The set-up assertion
# below checks it in every run; if it ever fails, lengthen this, never relax that.
PT_CONTROL_SLEEP_S = 0.001


class _RecordedSource:
    """a callback source: consecutive bytes of `pcm`, and for every read the thread it came from and what it got"""

    def __init__(self, cm, pcm, sleep=0.0):
        import threading
        import time
        self.pcm = pcm
        self.data = pcm.tobytes()
        self.pos = 0
        self.reads = []

        def read(n):
            if sleep:
                time.sleep(sleep)
            k = min(n, len(self.data) - self.pos)
            self.reads.append((threading.get_ident(), k))
            out = self.data[self.pos:self.pos + k]
            self.pos += k
            return out

        self.handle = cm.IoHandle.from_callbacks(read, eof=lambda: 1 if self.pos >= len(self.data) else 0)


# case -> (readers of the tee, slot of each reader's stream, a transform between reader and group, slot added late)
PT_CASES = {
    "two-readers": (2, (19, 43), False, None),
    "four-readers": (4, (11, 19, 35, 43), False, None),
    "two-transforms": (2, (19, 43), True, None),
    "second-reader-added-late": (2, (19, 47), False, 47),
    "no-shared-source": (0, (), False, None),
}


@pytest.mark.parametrize("case", list(PT_CASES))
def test_streams_behind_one_tee_stay_on_the_pumping_thread(gpu, oracle, case):
    """coolmic_group_set_pull_threads(4) over 48 streams whose sources are callbacks that note the calling thread.
    The readers of one coolmic_tee_t are different handles with different userdata over one buffer without a
    lock: the group has to find the tee behind them (and behind transforms attached to them) when they are added,
    mark the streams (cmhip_test_group_shared_source: 1 for exactly those slots), and read them on the pumping
    thread.  Asserted per case: every read of the tee's upstream came from the pumping thread -- in the late case
    from the moment the second reader is added, which also marks the first --, the upstream was read front to
    back once, in whole blocks; every reader got ALL of it (a tee, not one handle given twice), and every
    stream's PCM is the oracle's gain over its own source.  The run only counts if the helpers did read: at least
    one source of slots 8..47 must have been read from another thread (set-up assertion).  The case without a
    tee is the control: no slot marked, everything else the same."""
    import threading
    cm = gpu
    readers, slots, through_transform, late = PT_CASES[case]
    N, block, pumps = PT_N, PT_BLOCK, PT_PUMPS
    nbytes = 2 * block
    me = threading.get_ident()
    grp = cm.Group(1, N, block, queue_blocks=4)
    assert grp.set_pull_threads(PT_THREADS) == 0

    up = _RecordedSource(cm, oracle.lcg(4242, block * pumps))
    tee, shared, transforms = None, {}, []                  # shared: slot -> (handle to add, gain before the group)
    if readers:
        tee = cm.Tee(readers)
        assert tee.attach(up.handle) == 0
        for k, slot in enumerate(slots):
            h, pre = tee.get_iohandle(k), None
            if through_transform:
                tr = cm.Transform(48000, 1)
                pre = [1500, 700][k]
                assert tr.attach(h) == 0 and tr.set_master_gain(1, 1000, [pre]) == 0
                h.unref()
                h = tr.get_iohandle()
                transforms.append(tr)
            shared[slot] = (h, pre)
    controls, handles, gains = {}, {}, {}

    def add(slot):
        if slot in shared:
            src = shared[slot][0]
        else:
            controls[slot] = _RecordedSource(cm, oracle.lcg(7000 + slot, block * pumps),
                                             sleep=PT_CONTROL_SLEEP_S if slot < 8 else 0.0)
            src = controls[slot].handle
        assert grp.add_stream(src) == slot
        gains[slot] = [700 + 37 * slot]                      # every stream its own, the sharing ones too
        assert grp.set_master_gain(slot, 1, 1000, gains[slot]) == 0
        handles[slot] = grp.get_iohandle(slot)

    for slot in range(N):
        if slot != late:
            add(slot)
    got = {slot: b"" for slot in range(N)}
    late_mark = 0
    for p in range(pumps):
        if late is not None and p == pumps // 2:
            assert [grp.shared_source(s) for s in range(N - 1)] == [0] * (N - 1)
            late_mark = len(up.reads)
            add(late)
            assert grp.shared_source(slots[0]) == 1 and grp.shared_source(late) == 1    # the older stream too
        assert grp.pump() == grp.streams()
        for slot in range(grp.streams()):                    # (the block just pumped: no read here pumps again)
            n, data = handles[slot].read(nbytes)
            assert n == nbytes, (p, slot, n)
            got[slot] += data
        if late is not None and p < pumps // 2:              # a tee's reader that is not read stalls the others:
            n, data = shared[late][0].read(nbytes)           # until it joins the group the test reads it, between pumps
            assert data == up.data[p * nbytes:(p + 1) * nbytes]

    # the marks: deterministic
    assert [grp.shared_source(s) for s in range(N)] == [1 if s in shared else 0 for s in range(N)]
    assert grp.shared_source(N) == cm.ERROR_INVAL
    # the set-up: the helpers did pull
    far = [t for s, c in controls.items() if s >= 8 for t, _ in c.reads]
    off = sum(1 for t in far if t != me)
    print("pull threads, %s: %d of %d reads of the control sources in slots 8..47 came from a helper thread "
          "(the sources of slots 0..7 sleep %.1f ms a read)" % (case, off, len(far), 1e3 * PT_CONTROL_SLEEP_S))
    assert off > 0, "set-up failure: every source was read by the pumping thread, the helpers never pulled"
    # the controls: one read of a block per pump, the oracle's chain (as test_group_pull_spread_over_threads)
    for slot, c in controls.items():
        assert [k for _, k in c.reads] == [nbytes] * pumps, slot
        assert np.array_equal(np.frombuffer(got[slot], np.int16), _expect(oracle, c.pcm, 1, gains[slot], None)), slot
    if readers:
        # the tee's upstream: only the pumping thread, front to back, once, never past the data
        assert [t for t, _ in up.reads[late_mark:]] == [me] * (len(up.reads) - late_mark), up.reads
        assert [k for _, k in up.reads] == [nbytes] * pumps and up.pos == len(up.data)
        for slot, (_, pre) in shared.items():
            first = pumps // 2 * block if slot == late else 0                # (the late reader's first half: above)
            assert len(got[slot]) == len(up.data) - 2 * first, slot
            x = up.pcm[first:]
            if pre is not None:
                _, g = oracle.gain(1, 1, 1000, [pre])
                x = oracle.gain_apply(g, x, 1)
            assert np.array_equal(np.frombuffer(got[slot], np.int16), _expect(oracle, x, 1, gains[slot], None)), slot
    else:
        assert up.reads == []

    for h in handles.values():
        h.unref()
    for h, _ in shared.values():
        h.unref()
    for c in controls.values():
        c.handle.unref()
    for tr in transforms:
        tr.unref()
    if tee:
        tee.unref()
    up.handle.unref()
    grp.unref()
