"""CPU: the host side of the mix bus (cmhip_bus_*): the header, the table check, the mix-minus table, NULL and
descriptor refusals, the routing compiler (csrc/bus_route.h) against a Python restatement of its greedy rule and, as a
stand-alone C++ program, over random tables plainly and under AddressSanitizer + UBSan, the launcher's plan for every
pair of channel counts, an emulation of k_bus_any's decomposition (per send: 16-byte vectors staged into pair planes as
far as the send's stream reaches, one thread per frame adding into int64, one rounding, the staged output tile) and of
k_bus_fast's (a lane's units, int32 inside a group, int64 across groups) against the model of tests/test_gpu_bus.py at
the plan's own tile_frames, and the generated assembly of k_bus.hip.  Nothing here
needs a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
ROUTE_SRC = os.path.join(ROOT, "tests", "cpp", "bus_route_test.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_bus", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RH = _load("test_bus_ramp_host")   # the emulations of both kernels' decomposition: every send at rest, they are k_bus.hip's
TG = RH.TG.TB                      # tests/test_gpu_bus.py: the model and the tables of the GPU tests
UNWRITTEN = RH.UNWRITTEN


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){cmhip_bus_desc_t d; uint32_t b[2], s[2], n[1]; int16_t w[2]; (void)sizeof(d);\n"
           "d.streams = d.buses = d.channels_in = d.channels_out = 1; d.max_frames = d.max_sends = 1; d.hip_stream = 0;\n"
           "if (cmhip_bus_mix_minus(2, 16384, b, s, w, 2, 1)) return 1;\n"
           "return cmhip_bus_check(2, 2, 1, 1, 2, b, s, w) + (cmhip_bus_new(0) != 0) + cmhip_bus_sync(0)"
           " + (cmhip_bus_hip_stream(0) != 0) + cmhip_bus_run(0, 0, 0, 0, 0, 0, 0, n) + cmhip_bus_set_routing(0, 2, b, s, w)"
           " + cmhip_bus_get_routing(0, 2, b, s, w) + (int)cmhip_bus_sends(0) + (cmhip_bus_free(0), 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_check(cm):
    ok = cm.bus_check
    assert ok(2, 3, 2, 1, [0, 1], [2, 0], [[[-32768, 32767]], [[1, 2]]]) == 0            # a row at 65535
    assert ok(2, 3, 2, 1, [0, 1], [2, 0], [[[1, 2]], [[-32768, -32768]]]) == cm.ERROR_INVAL          # 65536
    assert b"send 1" in cm.lib.cmhip_last_error()
    assert ok(1, 1, 3, 2, [0], [0], [[[1, 2, 3], [32767, 32767, 1]]]) == 0
    assert ok(1, 1, 3, 2, [0], [0], [[[1, 2, 3], [32767, 32767, 2]]]) == cm.ERROR_INVAL
    w16 = np.full((1, 16, 16), 4095, dtype=np.int16)
    assert ok(1, 1, 16, 16, [0], [0], w16) == 0
    w16[0, 15, 15] = -4111                                                    # 15 * 4095 + 4111 = 65536
    assert ok(1, 1, 16, 16, [0], [0], w16) == cm.ERROR_INVAL
    one = [[[1]]]
    assert ok(2, 3, 1, 1, [1], [2], one) == 0
    assert ok(2, 3, 1, 1, [2], [2], one) == cm.ERROR_INVAL                    # a bus index out of range
    assert ok(2, 3, 1, 1, [1], [3], one) == cm.ERROR_INVAL                    # a stream index out of range
    assert ok(2, 3, 1, 1, [0xffffffff], [0], one) == cm.ERROR_INVAL
    wide = np.ones((1, 17, 17), dtype=np.int16)
    for buses, streams, ci, co in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 17, 1), (1, 1, 1, 17)):
        assert ok(buses, streams, ci, co, [0], [0], wide) == cm.ERROR_INVAL, (buses, streams, ci, co)
    # n above what a table can hold (2^31 entries of packed matrix): judged before an array is read
    assert ok(1, 1, 1, 1, None, None, None, n=1 << 31) == cm.ERROR_INVAL
    assert ok(1, 1, 16, 16, None, None, None, n=1 << 24) == cm.ERROR_INVAL
    assert ok(1, 1, 16, 16, None, None, None, n=(1 << 24) - 1) == cm.ERROR_FAULT         # fits: the arrays are missing
    assert ok(1, 1, 1, 1, None, None, None, n=0) == 0                                    # the empty table
    assert b"bus_check" in cm.lib.cmhip_last_error()


def test_mix_minus(cm):
    for n in (1, 2, 5):
        for channels in (1, 2):
            bus, stream, W = cm.bus_mix_minus(n, 1638, channels)
            assert len(bus) == len(stream) == len(W) == n * (n - 1)
            assert not (bus == stream).any()                                  # no bus names itself
            assert sorted(zip(bus.tolist(), stream.tolist())) == [(b, s) for b in range(n) for s in range(n) if s != b]
            assert all(np.array_equal(w, 1638 * np.eye(channels, dtype=np.int16)) for w in W)
            assert cm.bus_check(n, n, channels, channels, bus, stream, W, n=len(bus)) == 0
    # cap_sends too small: INVAL with nothing written
    b, s, w = np.full(20, 77, dtype=np.uint32), np.full(20, 77, dtype=np.uint32), np.full(20, 77, dtype=np.int16)
    assert cm.lib.cmhip_bus_mix_minus(5, 1638, b.ctypes.data, s.ctypes.data, w.ctypes.data, 19, 1) == cm.ERROR_INVAL
    assert (b == 77).all() and (s == 77).all() and (w == 77).all()
    assert cm.lib.cmhip_bus_mix_minus(5, 1638, b.ctypes.data, s.ctypes.data, w.ctypes.data, 20, 1) == 0
    assert (w == 1638).all() and b.tolist() == [i // 4 for i in range(20)]
    assert cm.lib.cmhip_bus_mix_minus(0, 1, b.ctypes.data, s.ctypes.data, w.ctypes.data, 20, 1) == cm.ERROR_INVAL
    assert cm.lib.cmhip_bus_mix_minus(2, 1, b.ctypes.data, s.ctypes.data, w.ctypes.data, 20, 17) == cm.ERROR_INVAL
    assert cm.lib.cmhip_bus_mix_minus(2, 1, None, s.ctypes.data, w.ctypes.data, 20, 1) == cm.ERROR_FAULT
    with pytest.raises(cm.CoolmicError):
        cm.bus_mix_minus(5, 1638, 1, cap_sends=19)


def test_null_arguments_and_descriptor_refusals(cm):
    lib = cm.lib
    assert lib.cmhip_bus_new(None) is None
    assert lib.cmhip_bus_run(None, None, 0, 0, None, None, 0, None) == cm.ERROR_FAULT
    assert lib.cmhip_bus_set_routing(None, 0, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_bus_get_routing(None, 0, None, None, None) == cm.ERROR_FAULT
    assert lib.cmhip_bus_sends(None) == 0
    assert lib.cmhip_bus_sync(None) == cm.ERROR_FAULT
    assert lib.cmhip_bus_hip_stream(None) is None
    lib.cmhip_bus_free(None)
    # descriptors are refused before any device is touched
    for streams, buses, ci, co, frames, sends in ((0, 1, 2, 1, 1024, 4), (1, 0, 2, 1, 1024, 4), (1, 1, 0, 1, 1024, 4),
                                                  (1, 1, 2, 0, 1024, 4), (1, 1, 17, 1, 1024, 4), (1, 1, 2, 17, 1024, 4),
                                                  (1, 1, 2, 1, 0, 4), (1, 1, 2, 1, 1024, 0), (1, 1, 2, 1, 1 << 30, 4),
                                                  (1, 1, 1, 16, 1 << 27, 4), (1, 1, 1, 1, 1024, 1 << 31),
                                                  (1 << 31, 1, 1, 1, 1024, 4)):
        d = cm.BusDesc(0, streams, buses, ci, co, frames, sends, None)
        assert lib.cmhip_bus_new(C.byref(d)) is None, (streams, buses, ci, co, frames, sends)
        assert b"bus_new" in lib.cmhip_last_error()
        with pytest.raises(cm.CoolmicError):
            cm.Bus(streams, buses, ci, co, frames, sends)


# ---------------------------------------------------------------------------
# The routing compiler against the rule restated in Python

def _compile_py(buses, ci, co, bus, stream, W):
    """the header's rule: a stable sort by bus; inside a bus, in table order, a send joins the running group iff every
    row's running sum of sum |w| stays <= 65535, else it starts a group (flag); the mixer's packed matrices"""
    W = np.asarray(W, dtype=np.int64).reshape(len(bus), co, ci)
    order = sorted(range(len(bus)), key=lambda j: bus[j])                     # (sorted is stable)
    first = [0] * (buses + 1)
    for b in bus:
        first[b + 1] += 1
    first = np.cumsum(first).tolist()
    flags, run = [], None
    for p, j in enumerate(order):
        rows = np.abs(W[j]).sum(axis=1)
        if p == first[bus[j]] or (run + rows > 65535).any():
            flags.append(1)
            run = rows
        else:
            flags.append(0)
            run = run + rows
    cp = (ci + 1) // 2
    wk = np.zeros((len(bus), co, 2 * cp), dtype=np.int64)
    wk[:, :, :ci] = W[order] if len(bus) else 0
    wk = (wk[:, :, 0::2] & 0xffff) | ((wk[:, :, 1::2] & 0xffff) << 16)
    return first, [stream[j] for j in order], flags, wk


def _compare(cm, buses, streams, ci, co, bus, stream, W):
    first, so, flag, wk = cm.bus_compile(buses, streams, ci, co, bus, stream, W)
    want = _compile_py(buses, ci, co, bus, stream, W)
    assert first.tolist() == want[0] and so.tolist() == want[1] and flag.tolist() == want[2]
    assert np.array_equal(wk.astype(np.int64), want[3])
    return first.tolist(), so.tolist(), flag.tolist()


def test_routing_compiler(cm):
    rng = np.random.default_rng(5)
    # sends given in shuffled order, a bus with no sends (2), a stream used twice in one bus (stream 1 in bus 3)
    bus, stream = [3, 0, 1, 3, 0, 4, 3, 1, 0], [1, 2, 0, 4, 3, 2, 1, 1, 0]
    for ci, co in ((1, 1), (2, 1), (2, 2), (3, 2), (6, 2), (16, 16)):
        W = TG.dense_sends(ci, co, len(bus), 3, 40 + ci + co)
        first, so, flag = _compare(cm, 5, 5, ci, co, bus, stream, W)
        assert first == [0, 3, 5, 5, 8, 9] and so == [2, 3, 0, 0, 1, 1, 4, 1, 2]
        perm = rng.permutation(len(bus))
        _compare(cm, 5, 5, ci, co, [bus[i] for i in perm], [stream[i] for i in perm], W[perm])
    # (a) three unity sends: one group
    assert _compare(cm, 1, 3, 1, 1, [0] * 3, [0, 1, 2], [[[16384]]] * 3)[2] == [1, 0, 0]
    assert _compare(cm, 1, 3, 2, 2, [0] * 3, [0, 1, 2], [16384 * np.eye(2, dtype=np.int16)] * 3)[2] == [1, 0, 0]
    # (b) mono sends of |w| = 32767: groups of two
    w = [[[32767]], [[-32767]], [[32767]], [[32767]], [[-32767]]]
    assert _compare(cm, 1, 5, 1, 1, [0] * 5, list(range(5)), w)[2] == [1, 0, 1, 0, 1]
    # (c) every row of every send above 32768: every send its own group
    for ci, co in ((2, 1), (2, 2), (6, 2), (16, 16)):
        W = TG.heavy_sends(ci, co, 6, 50 + ci)
        assert _compare(cm, 2, 6, ci, co, [0, 1, 0, 1, 0, 0], list(range(6)), W)[2] == [1] * 6
    # one heavy row is enough to end a group, and a light send after it may join again
    W = np.array([[[100, 100], [100, 100]], [[100, 100], [32768 - 150, 32767]], [[1, 1], [1, 1]]], dtype=np.int16)
    assert _compare(cm, 1, 1, 2, 2, [0] * 3, [0] * 3, W)[2] == [1, 1, 0]
    # the empty table
    first, so, flag, wk = cm.bus_compile(3, 2, 2, 2, [], [], np.zeros((0, 2, 2), dtype=np.int16))
    assert first.tolist() == [0, 0, 0, 0] and so.size == flag.size == wk.size == 0
    # the tables of the GPU tests
    for k in TG.KS:
        b, s = TG.forms_table(k)
        _compare(cm, TG.BUSES, TG.STREAMS, 2, 1, b, s, TG.dense_sends(2, 1, len(b), k, k))


def _build_route_test(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        ROUTE_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


def test_routing_compiler_over_random_tables(tmp_path):
    exe, r = _build_route_test(tmp_path, "bus_route_test", [])               # g++ alone: the header includes no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "routes ok: 3000 tables" in out.stdout, out.stdout + out.stderr


def test_routing_compiler_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build_route_test(tmp_path, "bus_route_san",
                               ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                "-fno-omit-frame-pointer"])
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "routes ok: 3000 tables" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# The launcher's plan

def _lds_bytes(ci, co, tile):
    cp = (ci + 1) // 2
    return 8 * co * tile + 4 * cp * tile + 4 * ((co * cp + 3) // 4 * 4) + 2 * co * tile


def test_plan(cm):
    for ci in range(1, 17):
        for co in range(1, 17):
            fast = ci <= 2 and co <= 2
            p = cm.plan_bus(5, ci, co, 1)                         # a one-frame run: one workgroup per bus
            assert (p.err, p.grid, p.chunks) == (0, 5, 1), (ci, co)
            assert p.fast == (1 if fast else 0) and p.block == (64 if fast else 256)
            t = p.tile_frames
            assert t % 8 == 0 and t >= 8
            assert p.lds_bytes <= 65536                          # what a workgroup may use without a raised limit
            if fast:
                assert p.lds_bytes == 0 and t == (2048 if (ci, co) == (1, 1) else 1024)
                assert t == cm.plan_mix(5, ci, co, 1).tile_frames                        # MixFast's geometry
            else:
                assert p.lds_bytes == _lds_bytes(ci, co, t)
                assert t == 1024 or _lds_bytes(ci, co, 2 * t) > 65536        # the largest power of two that fits
            for frames in (1, t - 1, t, t + 1, 100000):
                q = cm.plan_bus(3, ci, co, frames)
                assert (q.err, q.chunks, q.grid, q.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
    assert cm.plan_bus(5, 16, 16, 1).tile_frames == 256 and cm.plan_bus(5, 3, 2, 1).tile_frames == 1024
    # no grid of 2^31 workgroups
    p = cm.plan_bus(1 << 20, 2, 1, 1 << 21)                      # 2^20 buses x 2^11 tiles
    assert p.err != 0 and p.grid == 0
    p = cm.plan_bus(1 << 20, 2, 1, (1 << 21) - 1024)
    assert p.err == 0 and p.grid == (1 << 20) * ((1 << 11) - 1)
    p = cm.plan_bus(1 << 21, 16, 16, 1 << 18)                    # 2^21 buses x 2^10 tiles of 256
    assert p.err != 0 and p.grid == 0
    assert cm.plan_bus(0, 2, 1, 100).grid == 0 and cm.plan_bus(4, 2, 1, 0).grid == 0
    assert cm.plan_bus(0, 2, 1, 100).err == 0
    for ci, co in ((0, 1), (17, 1), (1, 0), (1, 17)):
        assert cm.plan_bus(4, ci, co, 100).grid == 0


# ---------------------------------------------------------------------------
# The decomposition of k_bus_any (csrc/k_bus.hip), step by step in Python: per bus tile the int64 accumulators; per
# send, skipped when its stream ends at or before the tile, the tile's 16-byte vectors as far as the SEND's stream
# reaches (its ragged last one zero padded, none past it), the scatter into CP planes (even C_in: by dwords, odd: by
# halves, the unused half never written), one thread per frame of the send adding its int32 sums; then one rounding, the
# interleaved output tile and its whole vectors / ragged end by the BUS's count.  It holds the index arithmetic (every
# plane element read was written, nothing past a count is read or written) where no GPU is.

# The steps are tests/test_bus_ramp_host.py's emulation of k_busr_any with every send at rest: the kernels share them.

def _at_rest(table, buses, ci, co):
    """the table as a model whose sends all rest on their matrices; what the emulation compiles of it is the routing
    compiler's table"""
    bus, stream, W = table
    model = RH.TG.BusRampModel(buses, ci, co)
    model.set(bus, stream, W)
    first, order, flags = RH._compile_two_ended(model)
    assert (first, [stream[j] for j in order], flags) == _compile_py(buses, ci, co, bus, stream, W)[:3]
    return model


def _emulate_any(xs, table, buses, ci, co, tile, max_frames):
    """-> per bus the output slot as the kernel leaves it (UNWRITTEN where it stored nothing)"""
    outs, paths = RH._emulate_any(xs, _at_rest(table, buses, ci, co), tile, max_frames)
    assert paths <= {False}                                      # the plain path alone
    return outs


@pytest.mark.parametrize("ci,co", [(3, 2), (6, 2), (5, 3), (16, 16), (1, 16)])
def test_emulated_decomposition_equals_the_model(cm, ci, co):
    p = cm.plan_bus(TG.BUSES, ci, co, 1)
    assert p.fast == 0
    t = p.tile_frames
    counts = TG.forms_counts(t)
    for k in (1, 3, 17):
        bus, stream = TG.forms_table(k)
        table = (bus, stream, TG.dense_sends(ci, co, len(bus), k, 9000 + 10 * ci + co + k))
        xs = [TG.noise(9100 + s, n, ci) for s, n in enumerate(counts)]
        want = TG.model_bus(xs, table, TG.BUSES, co)
        got = _emulate_any(xs, table, TG.BUSES, ci, co, t, counts[0])
        for b, (g, w) in enumerate(zip(got, want)):
            w = w.astype(np.int64).reshape(-1)
            assert np.array_equal(g[:w.size], w), (ci, co, k, b)
            assert (g[w.size:] == UNWRITTEN).all(), (ci, co, k, b)            # nothing past the bus's count


def _emulate_fast(xs, table, buses, ci, co, max_frames):
    """k_bus_fast<CI, CO> (csrc/k_bus.h, bus_fast_tile without the ramp): one wave per (bus, tile) walks the bus's sends
    -- a send whose stream ends at or before the tile is skipped, its flag still closes the group; a lane's units and
    vectors zero-filled past the SEND's count; one dot per output sample and send on the input dword that holds the
    frame, chained in int32 inside a group (held below 2^31 here) and added into the int64 at a flag; one rounding;
    whole vectors and the ragged end by the BUS's count -> per bus the slot, and the tile"""
    outs, tile, paths = RH._emulate_fast(xs, _at_rest(table, buses, ci, co), max_frames)
    assert not [p for p in paths if p[0]]                        # (ramp, wide): the plain path alone
    return outs, tile


@pytest.mark.parametrize("ci,co", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_emulated_fast_forms_equal_the_model(cm, ci, co):
    t = cm.plan_bus(TG.BUSES, ci, co, 1).tile_frames
    counts = TG.forms_counts(t)
    xs = [TG.noise(9600 + s, n, ci) for s, n in enumerate(counts)]
    for k, heavy in ((1, False), (3, False), (17, False), (5, True)):
        bus, stream = TG.forms_table(k)
        W = TG.heavy_sends(ci, co, len(bus), 9500 + k) if heavy else TG.dense_sends(ci, co, len(bus), k, 9500 + k)
        table = (bus, stream, W)
        ins = [x >> 4 for x in xs] if heavy else xs
        want = TG.model_bus(ins, table, TG.BUSES, co)
        got, tile = _emulate_fast(ins, table, TG.BUSES, ci, co, counts[0])
        assert tile == t
        for b, (g, w) in enumerate(zip(got, want)):
            w = w.astype(np.int64).reshape(-1)
            assert np.array_equal(g[:w.size], w), (ci, co, k, b)
            assert (g[w.size:] == UNWRITTEN).all(), (ci, co, k, b)


def test_kernel_assembly_house_rules():
    """make asm produces build/k_bus.s: it holds kernels and the dot instruction, no scalar load has a register AND an
    immediate offset (tests/test_abi.py tells why; every wave indexes the routing table with its bus and its sends), and
    the mono / stereo kernels keep every register out of scratch memory."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_bus.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_dot2\w*_i32_i16", text, flags=re.M)
    assert re.search(r"^\s*s_load_dword", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    usage = open(os.path.join(PKG, "build", "k_bus.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_bus_fast" in k}
    forms = {re.search(r"k_bus_fastILi(\d)ELi(\d)E", k).groups() for k in fast}
    assert forms == {("1", "1"), ("1", "2"), ("2", "1"), ("2", "2")} and any("k_bus_any" in k for k in scratch), sorted(scratch)
    assert all(v == 0 for v in fast.values()), fast
    src = "".join(open(os.path.join(PKG, "csrc", f)).read() for f in ("k_bus.hip", "k_bus.h", "k_mix.h"))
    assert "getenv" not in src
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_(?!K_(?:BUS|MIX)_H\b)\w+", m.group(1)), m.group(0)   # (but the include guards)
