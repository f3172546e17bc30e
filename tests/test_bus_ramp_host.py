"""CPU: the host side of the mix bus's send ramps (cmhip_bus_ramp_*): the header, the exported symbols, NULL refusals
without a device, the mirror (csrc/bus_ramp.h) replayed by a stand-alone C++ program against a plain-Python model, the
two-ended group split over random tables and independent ramps by the same program plainly and under sanitizers, the
ramp launcher's plan for every pair of channel counts, an emulation of both ramp kernels' decomposition at the plan's
own tile against the model of tests/test_gpu_bus_ramp.py -- the GPU cases rehearsed on the CPU -- and the generated
assembly of k_busramp.hip.  Nothing here needs a GPU."""
import copy
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "libcoolmic-dsp_amd")
RAMP_SRC = os.path.join(ROOT, "tests", "cpp", "bus_ramp_test.cpp")


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_bus_ramp_model",
                                                  os.path.join(ROOT, "tests", "test_gpu_bus_ramp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TG = _gpu_test_module()            # the model of the GPU tests (and, through it, the bus's and the mixer's helpers)


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = ("#include <coolmic_hip.h>\n"
           "int main(void){int16_t w[4] = {0, 0, 0, 0}; uint32_t done, of;\n"
           "return cmhip_bus_ramp_sends(0, 0, 1, w, 480) + cmhip_bus_ramp_state(0, 0, &done, &of, w)"
           " + cmhip_bus_ramp_state(0, 0, &done, &of, 0);}\n")
    for comp, ext, std in (("gcc", "c", "-std=gnu11"), ("g++", "cpp", "-std=c++17")):
        f = tmp_path / ("t." + ext)
        f.write_text(src)
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(f)], check=True)


def test_symbols_and_refusals_without_a_device(cm):
    lib = cm.lib
    for name in ("cmhip_bus_ramp_sends", "cmhip_bus_ramp_state"):
        assert name in cm.SIGNATURES and hasattr(lib, name) and name not in cm.MISSING
    w = np.zeros(4, dtype=np.int16)
    a, b = C.c_uint32(77), C.c_uint32(77)
    assert lib.cmhip_bus_ramp_sends(None, 0, 1, w.ctypes.data, 480) == cm.ERROR_FAULT
    assert lib.cmhip_bus_ramp_sends(None, 0, 0, None, 480) == cm.ERROR_FAULT
    assert b"bus_ramp_sends" in lib.cmhip_last_error()
    assert lib.cmhip_bus_ramp_state(None, 0, C.byref(a), C.byref(b), w.ctypes.data) == cm.ERROR_FAULT
    assert (a.value, b.value) == (77, 77) and b"bus_ramp_state" in lib.cmhip_last_error()
    header = open(os.path.join(ROOT, "include", "coolmic_hip.h")).read()
    section = header[header.index("---- send ramps"):header.index("---- peak limiter")]
    assert header.index("---- mix bus") < header.index("---- send ramps")
    assert "zero-matrix send adds nothing to the sum but does count" in section and "OUTPUT frames of its bus" in section
    # no second copy of the formulas is exported
    assert not [n for n in cm.SIGNATURES if n.startswith("cmhip_bus_ramp_") and n.endswith(("position", "weight"))]


# ---------------------------------------------------------------------------
# the mirror: csrc/bus_ramp.h under a stand-alone program

def _build(tmp_path, name, extra):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        RAMP_SRC, "-o", str(exe)] + extra, capture_output=True, text=True)
    return exe, r


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _py_position(n, R):
    """the header's p(n), in plain Python integers"""
    n = min(n, R)
    return min(32768, (n * -(-(1 << 32) // R)) >> 17)


def _py_weight(w0, w1, p):
    N = w0 * (32768 - p) + w1 * p
    return (abs(N) >> 15) * (1 if N >= 0 else -1)


class PySend:
    """(W0, W1, R, done) of one send, lists of Python integers"""

    def __init__(self, w):
        self.w0, self.w1, self.R, self.done = list(w), list(w), 0, 0

    def ramping(self):
        return self.done < self.R

    def now(self):
        if not self.ramping():
            return list(self.w1)
        p = _py_position(self.done, self.R)
        return [_py_weight(a, b, p) for a, b in zip(self.w0, self.w1)]

    def start(self, w, R):
        self.w0, self.w1, self.R, self.done = self.now(), list(w), R, 0

    def step(self, w):
        self.w0, self.w1, self.R, self.done = list(w), list(w), 0, 0

    def advance(self, count):
        if self.ramping():
            self.done = min(self.R, self.done + count)

    def line(self):
        on = self.ramping()
        return [self.done if on else 0, self.R if on else 0, int(on)] + self.now()


def _mirror_script(R, seed):
    """start, retarget mid-ramp, step, advance with 0 and with more than the remainder, now -- three sends on two buses"""
    rng = np.random.default_rng(seed)
    co, ci, sends, bus = 2, 3, 3, [1, 0, 1]
    mat = lambda: [int(v) for v in rng.integers(-10000, 10001, size=co * ci)]
    W = [mat() for _ in range(sends)]
    model = [PySend(w) for w in W]
    ops = ["init %d %d %d 2  %s  %s" % (sends, co, ci, " ".join(map(str, bus)), " ".join(str(v) for w in W for v in w))]
    want = [[m.line() for m in model]]

    def op(text, fn):
        ops.append(text)
        fn()
        want.append([m.line() for m in model])

    def start(j, R):
        w = mat()
        op("start %d %d %s" % (j, R, " ".join(map(str, w))), lambda: model[j].start(w, R))

    def step(j):
        w = mat()
        op("step %d %s" % (j, " ".join(map(str, w))), lambda: model[j].step(w))

    def adv(c0, c1):
        op("adv %d %d" % (c0, c1), lambda: [m.advance((c0, c1)[b]) for m, b in zip(model, bus)])

    start(0, R)
    start(1, R)
    adv(0, 0)                                        # a run of no frames: positions kept
    adv(1, 0)                                        # bus 0 alone moves: send 1
    assert [m.done for m in model] == [0, 1, 0]
    adv(R // 3, R // 2)
    start(0, max(2, R // 2))                         # a retarget mid-ramp: from the matrix in force, n restarts
    start(2, 2)
    adv(0, 1)
    step(1)                                          # a step ends a ramp
    adv(1, 1)
    adv(5, R + 7)                                    # more than the remainder: capped at R, the ramp is over
    assert not model[0].ramping() and not model[2].ramping()
    start(2, R)
    adv(3, R - 1)                                    # one frame before the end
    assert model[2].ramping() or R == 2
    adv(0, 0xffffffff)
    assert not any(m.ramping() for m in model)
    return "\n".join(ops) + "\n", want


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizers"])
def test_mirror_against_a_plain_python_model(tmp_path, san):
    exe, r = _build(tmp_path, "bus_ramp_replay", SAN if san else [])
    if san and r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    for i, R in enumerate((2, 3, 7, 1000, 1 << 20)):
        script, want = _mirror_script(R, 300 + i)
        f = tmp_path / ("script%d.txt" % R)
        f.write_text(script)
        out = subprocess.run([str(exe), "replay", str(f)], capture_output=True, text=True, timeout=120,
                             env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
        assert out.returncode == 0, out.stderr[-2000:]
        got = [[int(v) for v in ln.split()] for ln in out.stdout.splitlines()]
        assert got == [line for block in want for line in block], R


def test_two_ended_split_over_random_tables_and_ramps(tmp_path):
    exe, r = _build(tmp_path, "bus_ramp_test", [])                           # g++ alone: the headers include no HIP
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "send ramps ok: 1500 sequences" in out.stdout, out.stdout + out.stderr
    moved = int(re.search(r"(\d+) splits moved by a ramp's other end", out.stdout).group(1))
    assert moved > 1000                                                      # the case a one-ended compile gets wrong


def test_two_ended_split_under_address_and_ub_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "bus_ramp_san", SAN)
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan in this toolchain: " + r.stderr[-200:])
    out = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and "send ramps ok: 1500 sequences" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------------------
# the ramp launcher's plan

def _lds_bytes(ci, co, tile):
    cp = (ci + 1) // 2
    return 8 * co * tile + 4 * cp * tile + 12 * ((co * cp + 3) // 4 * 4) + 2 * co * tile


def test_plan_busramp(cm):
    for ci in range(1, 17):
        for co in range(1, 17):
            fast = ci <= 2 and co <= 2
            p, q = cm.plan_busramp(5, ci, co, 1), cm.plan_bus(5, ci, co, 1)
            assert (p.err, p.grid, p.chunks, p.fast, p.block) == (0, 5, 1, q.fast, q.block), (ci, co)
            t = p.tile_frames
            assert t % 8 == 0 and t >= 8 and p.lds_bytes <= 65536 and t <= q.tile_frames
            if fast:
                assert p.lds_bytes == 0 and t == q.tile_frames
            else:
                assert p.lds_bytes == _lds_bytes(ci, co, t)                  # W0 and W1 counted
                assert t == 1024 or _lds_bytes(ci, co, 2 * t) > 65536        # the largest power of two that fits
            for frames in (1, t - 1, t, t + 1, 100000):
                r = cm.plan_busramp(3, ci, co, frames)
                assert (r.err, r.chunks, r.grid, r.tile_frames) == (0, -(-frames // t), 3 * -(-frames // t), t)
    p = cm.plan_busramp(1 << 21, 16, 16, 1 << 18)                # no grid of 2^31 workgroups
    assert p.err != 0 and p.grid == 0
    assert cm.plan_busramp(0, 2, 1, 100).grid == 0 and cm.plan_busramp(4, 2, 1, 0).grid == 0


# ---------------------------------------------------------------------------
# The decomposition of the two ramp kernels (csrc/k_busramp.hip), step by step in Python with the device's own integer
# steps (the position from n clamped to R, a 64-bit product and a shift; an entry by two products and the
# add-32767-to-negatives arithmetic shift) on the host's own records: sends in compiled order, the group flags from
# BOTH ends of every running ramp, per (tile, send) the uniform choice between the ramp path and the plain one with the
# target.  k_busr_fast: a lane's units, int32 inside a group (held below 2^31 here), int64 across groups.  k_busr_any:
# vectors staged into pair planes as far as the SEND's stream reaches, one thread per frame.  Positions are read, not
# advanced.  The rehearsal before GPU time.  With every send at rest these are the decompositions of k_bus.hip's two
# kernels: tests/test_bus_host.py calls them so.

UNWRITTEN = 1 << 40


def _dev_pos(n, R, inc):
    q = np.minimum(n, R) * inc
    assert (q < (1 << 32) + R).all()
    return np.minimum(q >> 17, 32768)


def _dev_w(w0, w1, p):
    N = w0 * (32768 - p) + w1 * p
    assert (np.abs(N) <= 1 << 30).all()
    return (N + ((N >> 31) & 32767)) >> 15


def _compile_two_ended(model):
    """csrc/bus_ramp.h + bus_route_compile_bounds restated: a stable sort by bus; a send's bound per row is the larger
    of its two ends' sums while it ramps, its matrix's own otherwise; greedy groups on the bounds"""
    order = sorted(range(len(model.bus)), key=lambda j: model.bus[j])
    first = [0] * (model.B + 1)
    for b in model.bus:
        first[b + 1] += 1
    first = np.cumsum(first).tolist()
    flags, run = [], None
    for p, j in enumerate(order):
        s = model.sends[j]
        rows = np.abs(s.w1).sum(axis=1)
        if s.ramping():
            rows = np.maximum(rows, np.abs(s.w0).sum(axis=1))
        if p == first[model.bus[j]] or (run + rows > 65535).any():
            flags.append(1)
            run = rows
        else:
            flags.append(0)
            run = run + rows
    return first, order, flags


def _slots(xs, ci, max_frames):
    counts = [np.asarray(x).reshape(-1, ci).shape[0] for x in xs]
    slots = []
    for x, c in zip(xs, counts):                                 # the input slots: poison past the count
        slot = np.full(max_frames * ci + 8, UNWRITTEN, dtype=np.int64)
        slot[:c * ci] = np.asarray(x, dtype=np.int64).reshape(-1)
        slots.append(slot)
    return counts, slots


def _vector(ins, ns_in, v, ragged_ok, past_ok):
    vec = np.zeros(8, dtype=np.int64)                            # load_vec: whole, the ragged end zero padded, or zeros
    if v < ns_in // 8:
        vec[:] = ins[v * 8:v * 8 + 8]
    elif v == ns_in // 8 and ns_in % 8:
        assert ragged_ok
        vec[:ns_in % 8] = ins[v * 8:v * 8 + ns_in % 8]
    else:
        assert past_ok                                           # zeros: nothing past the send's count is read
    assert (vec != UNWRITTEN).all()
    return vec


def _emulate_fast(xs, model, max_frames):
    ci, co = model.CI, model.CO
    first, order, flags = _compile_two_ended(model)
    uf = 8 // min(ci, co)
    vi, vo = uf * ci // 8, uf * co // 8
    nu = 4 // max(vi, vo)
    tile = 64 * nu * uf
    counts, slots = _slots(xs, ci, max_frames)
    lane = np.arange(64)
    outs, paths = [], set()
    for b in range(model.B):
        out = np.full(max_frames * co + 16, UNWRITTEN, dtype=np.int64)
        outs.append(out)
        j0, j1 = first[b], first[b + 1]
        if j0 == j1:
            continue
        F = max(counts[model.stream[order[j]]] for j in range(j0, j1))
        wide = sum(flags[j0:j1]) > 1
        ns_out = F * co
        for k in range(-(-F // tile)):                           # one wave each
            f0 = k * tile
            acc = np.full((64, nu, vo * 8), 0 if wide else 8192, dtype=np.int64)
            tot = np.zeros((64, nu, vo * 8), dtype=np.int64)
            for j in range(j0, j1):
                if wide and flags[j]:
                    tot += acc
                    acc[:] = 0
                send, s = model.sends[order[j]], model.stream[order[j]]
                c, ins = counts[s], slots[s]
                if c <= f0:
                    continue
                ramp = send.done + f0 < send.R                   # (uniform)
                paths.add((ramp, wide))
                ns_in = c * ci
                lo = np.zeros((64, nu, vi * 4), dtype=np.int64)
                hi = np.zeros((64, nu, vi * 4), dtype=np.int64)
                for u in range(nu):
                    for i in range(vi):
                        for ln in lane:
                            vec = _vector(ins, ns_in, ((k * 64 * nu) + 64 * u + ln) * vi + i, f0 + tile > c, f0 + tile > c)
                            lo[ln, u, i * 4:i * 4 + 4], hi[ln, u, i * 4:i * 4 + 4] = vec[0::2], vec[1::2]
                if ramp:                                         # [lane][unit][frame of the unit] -> per entry
                    inc = -(-(1 << 32) // send.R)
                    n = send.done + f0 + (64 * np.arange(nu)[None, :, None] + lane[:, None, None]) * uf + 1 + \
                        np.arange(uf)[None, None, :]
                    p = _dev_pos(n, send.R, inc)
                    w = [[_dev_w(int(send.w0[oc, cc]), int(send.w1[oc, cc]), p) for cc in range(ci)] for oc in range(co)]
                else:
                    w = [[int(send.w1[oc, cc]) * np.ones((64, nu, uf), dtype=np.int64) for cc in range(ci)]
                         for oc in range(co)]
                for e in range(vo * 8):                          # output sample of the unit
                    f, oc = divmod(e, co)
                    dw = (f * ci) >> 1
                    if ci == 2:
                        wl, wh = w[oc][0][:, :, f], w[oc][1][:, :, f]
                    else:
                        wl, wh = (0, w[oc][0][:, :, f]) if f & 1 else (w[oc][0][:, :, f], 0)
                    acc[:, :, e] += lo[:, :, dw] * wl + hi[:, :, dw] * wh
                assert np.abs(acc).max() < 2 ** 31               # the int32 chain of a group never wraps
            y = np.clip((tot + acc + (8192 if wide else 0)) >> 14, -32768, 32767)
            for u in range(nu):
                for i in range(vo):
                    for ln in lane:
                        v = ((k * 64 * nu) + 64 * u + ln) * vo + i
                        o8 = y[ln, u, i * 8:i * 8 + 8]
                        if v < ns_out // 8:
                            out[v * 8:v * 8 + 8] = o8
                        elif v == ns_out // 8 and ns_out % 8:
                            out[v * 8:v * 8 + ns_out % 8] = o8[:ns_out % 8]
    return outs, tile, paths


def _emulate_any(xs, model, tile, max_frames):
    ci, co = model.CI, model.CO
    cp = (ci + 1) // 2
    first, order, _ = _compile_two_ended(model)
    counts, slots = _slots(xs, ci, max_frames)

    def halves(W):                                               # (low, high) halves, an odd C_in padded with zero
        lo, hi = np.zeros((co, cp), dtype=np.int64), np.zeros((co, cp), dtype=np.int64)
        lo[:, :] = W[:, 0::2]
        hi[:, :ci // 2] = W[:, 1::2]
        return lo, hi

    outs, paths = [], set()
    for b in range(model.B):
        out = np.full(max_frames * co + 8, UNWRITTEN, dtype=np.int64)
        outs.append(out)
        j0, j1 = first[b], first[b + 1]
        if j0 == j1:
            continue
        F = max(counts[model.stream[order[j]]] for j in range(j0, j1))
        ns_out = F * co
        for f0 in range(0, F, tile):                             # one workgroup each
            nt = min(tile, F - f0)
            acc = np.zeros((tile, co), dtype=np.int64)
            assert (f0 * ci) % 8 == 0 and (f0 * co) % 8 == 0
            for j in range(j0, j1):
                send, s = model.sends[order[j]], model.stream[order[j]]
                c, ins = counts[s], slots[s]
                if c <= f0:
                    continue
                ntj = min(tile, c - f0)
                assert ntj <= nt
                ramp = send.done + f0 < send.R                   # (uniform)
                paths.add(ramp)
                plo = np.full((cp, tile), UNWRITTEN, dtype=np.int64)
                phi = np.full((cp, tile), UNWRITTEN, dtype=np.int64)
                ns_in = c * ci
                vb, nv = f0 * ci // 8, (ntj * ci + 7) // 8
                for w in range(nv):
                    vec = _vector(ins, ns_in, vb + w, True, False)       # whole, or the ragged end: none past it
                    if ci % 2 == 0:
                        for i in range(4):
                            f, k = divmod(w * 4 + i, cp)
                            if f < ntj:
                                plo[k, f], phi[k, f] = vec[2 * i], vec[2 * i + 1]
                    else:
                        for i in range(8):
                            f, ch = divmod(w * 8 + i, ci)
                            if f < ntj:
                                (phi if ch & 1 else plo)[ch >> 1, f] = vec[i]
                lo, hi = plo[:, :ntj], phi[:, :ntj].copy()
                assert (lo != UNWRITTEN).all()
                if ci % 2:
                    assert (hi[cp - 1] == UNWRITTEN).all()
                    hi[cp - 1] = 12345                           # whatever LDS held: it meets a zero weight
                assert (hi != UNWRITTEN).all()
                k1 = halves(send.w1)
                if ramp:
                    k0 = halves(send.w0)
                    inc = -(-(1 << 32) // send.R)
                    p = _dev_pos(send.done + f0 + np.arange(ntj) + 1, send.R, inc)           # one per frame
                    wlo = _dev_w(k0[0][:, :, None], k1[0][:, :, None], p[None, None, :])     # [co][cp][ntj]
                    whi = _dev_w(k0[1][:, :, None], k1[1][:, :, None], p[None, None, :])
                else:
                    wlo = k1[0][:, :, None] * np.ones(ntj, dtype=np.int64)
                    whi = k1[1][:, :, None] * np.ones(ntj, dtype=np.int64)
                if ci % 2:
                    assert not whi[:, cp - 1].any()
                q = (wlo * lo[None]).sum(axis=1) + (whi * hi[None]).sum(axis=1)              # [co][ntj]
                assert np.abs(q).max() < 2 ** 31
                acc[:ntj] += q.T
            ot = np.full(tile * co, UNWRITTEN, dtype=np.int64)
            ot[:nt * co] = np.clip((acc[:nt] + 8192) >> 14, -32768, 32767).reshape(-1)
            vb, nv = f0 * co // 8, (nt * co + 7) // 8
            for w in range(nv):
                v = vb + w
                if v < ns_out // 8:
                    out[v * 8:v * 8 + 8] = ot[w * 8:w * 8 + 8]
                elif v == ns_out // 8:
                    out[v * 8:v * 8 + ns_out % 8] = ot[w * 8:w * 8 + ns_out % 8]
    return outs, paths


def _rehearsal(ci, co, t, heavy):
    """tests/test_gpu_bus_ramp.py's table of the forms: sends at rest, inside ramps that end in the first tile, cross
    a tile edge and outlive the run, one carried from an earlier run; with `heavy` every send its own group"""
    model = TG.BusRampModel(TG.BUSES, ci, co)
    n = len(TG.BUS)
    if heavy:
        W0, W1 = TG.TB.heavy_sends(ci, co, n, 8100 + ci), TG.TB.heavy_sends(ci, co, n, 8200 + ci)
    else:
        W0 = TG.dense_sends(ci, co, n, 4, 8100 + 10 * ci + co)
        W1 = TG.dense_sends(ci, co, n, 4, 8200 + 10 * ci + co)
    model.set(TG.BUS, TG.STREAM, W0)
    for j, R in ((0, t + 300), (1, 7), (3, 3 * t), (4, 2), (5, 50000)):
        model.ramp(j, W1[j:j + 1], R)
    model.sends[5].done = 123
    return model


def _check(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        w = w.astype(np.int64).reshape(-1)
        assert np.array_equal(g[:w.size], w), (what, b)
        assert (g[w.size:] == UNWRITTEN).all(), (what, b)        # nothing past the bus's count


@pytest.mark.parametrize("ci,co", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_emulated_fast_forms_equal_the_model(cm, ci, co):
    t = cm.plan_busramp(TG.BUSES, ci, co, 1).tile_frames
    F = 2 * t + 13
    seen = set()
    for heavy in (False, True):
        xs = [TG.noise(8300 + s, n, ci) >> (4 if heavy else 0) for s, n in enumerate([F, F - 3, t + 5, 1, 0])]
        model = _rehearsal(ci, co, t, heavy)
        got, tile, paths = _emulate_fast(xs, model, F)
        assert tile == t
        seen |= paths
        _check(got, copy.deepcopy(model).run(xs), (ci, co, heavy))
    assert seen == {(r, w) for r in (True, False) for w in (True, False)}


@pytest.mark.parametrize("ci,co", [(3, 2), (6, 2), (5, 5), (16, 16)])
def test_emulated_decomposition_equals_the_model(cm, ci, co):
    p = cm.plan_busramp(TG.BUSES, ci, co, 1)
    assert p.fast == 0
    t = p.tile_frames
    F = 2 * t + 13
    xs = [TG.noise(8400 + s, n, ci) for s, n in enumerate([F, F - 3, t + 5, 1, 0])]
    model = _rehearsal(ci, co, t, False)
    got, paths = _emulate_any(xs, model, t, F)
    assert paths == {True, False}
    _check(got, copy.deepcopy(model).run(xs), (ci, co))


def test_emulated_both_ends_of_the_split():
    """the GPU suite's case: the int32 chain (asserted below 2^31 inside the emulation) holds only with both ends"""
    model = TG.BusRampModel(1, 1, 1)
    model.set([0, 0, 0], [0, 1, 2], [[[30000]], [[30000]], [[2000]]])
    model.ramp(0, [[[2000]]], 4000)
    model.sends[0].done = 8
    model.ramp(2, [[[30000]]], 2)
    assert _compile_two_ended(model)[2] == [1, 0, 1]
    xs = [np.full((64, 1), 32767, dtype=np.int16)] * 3
    got, _, _ = _emulate_fast(xs, model, 64)
    assert (got[0][:64] == 32767).all()


def test_kernel_assembly_house_rules():
    """make asm produces build/k_busramp.s: it holds the kernels and the dot instruction, no scalar load has a register
    AND an immediate offset (tests/test_abi.py tells why), the mono / stereo kernels keep every register out of scratch
    memory, and the output leaves in non-temporal 16-byte stores; no inline assembly in the source."""
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    text = open(os.path.join(PKG, "build", "k_busramp.s")).read()
    assert ".amdhsa_kernel" in text and re.search(r"^\s*v_dot2\w*_i32_i16", text, flags=re.M)
    assert re.search(r"^\s*s_load_dword", text, flags=re.M)
    bad = [ln.strip() for ln in text.splitlines()
           if re.search(r"^\s*s_(buffer_)?load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*s\d+\s+offset:", ln)]
    assert not bad, bad[:5]
    stores = re.findall(r"^\s*global_store_dwordx4[^\n]*", text, flags=re.M)
    assert stores and all(re.search(r"\bnt\b", ln) for ln in stores), [ln for ln in stores if " nt" not in ln][:3]
    usage = open(os.path.join(PKG, "build", "k_busramp.usage.txt")).read()
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", usage, flags=re.S):
        scratch[m.group(1)] = int(m.group(2))
    fast = {k: v for k, v in scratch.items() if "k_busr_fast" in k}
    forms = {re.search(r"k_busr_fastILi(\d)ELi(\d)ELb(\d)E", k).groups() for k in fast}
    assert forms == {(a, b, n) for a in "12" for b in "12" for n in "01"}, sorted(scratch)
    assert any("k_busr_any" in k for k in scratch) and any("k_busr_advance" in k for k in scratch)
    assert all(v == 0 for v in fast.values()), fast
    assert not [k for k in scratch if "k_bus_fast" in k or "k_bus_any" in k]     # (tests/test_bus_host.py counts those)
    src = "".join(open(os.path.join(PKG, "csrc", f)).read() for f in ("k_busramp.hip", "k_bus.h", "k_mix.h"))
    assert "getenv" not in src and not re.search(r"\basm\b|__asm__", src)
    for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, flags=re.M):
        assert not re.findall(r"\bCMHIP_(?!K_(?:BUS|MIX)_H\b)\w+", m.group(1)), m.group(0)   # (but the include guards)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*=.*\bk_busramp\.hip\b", mk, flags=re.M) and "build/k_busramp.s" in mk
