"""The noise suppressor's model for tests/test_denoise_host.py and the device tests: the specification of
include/coolmic_hip.h ("noise suppressor") in numpy int64 and Python integers, written from the header alone.  The window
and the twiddles are taken from the library (cmhip_denoise_window, cmhip_spec_twiddles) so that a last-bit difference
between two libms cannot turn into a parity failure.  Nothing here runs device code or the library's own block.

The model keeps what the header's formulas name and nothing of the kernel's bookkeeping: a row holds every input since
frame 0, the overlap-add sums by absolute frame and the number of blocks done; output frame n is
clamp16(x[n - D] - r[n - D]).  How a stream is cut into runs cannot matter to it by construction.
"""
import functools
import math

import numpy as np

UNITY = 32768
NP_MAX = 1 << 52
CNT_MAX = 65536


@functools.lru_cache(maxsize=None)
def bitrev(n):
    N = 1 << n
    r = np.zeros(N, dtype=np.int64)
    for b in range(n):
        r |= ((np.arange(N) >> b) & 1) << (n - 1 - b)
    return r


def target(p, npk, over, floor):
    """the target gain of a bin, in Python integers"""
    t = (npk * over) >> 4
    if p <= t:
        return floor
    sh = max(0, p.bit_length() - 34)
    ps, ts = p >> sh, t >> sh
    assert ps < 2 ** 34 and ts <= ps
    return max(floor, math.isqrt(((ps - ts) << 30) // ps))


def smooth(g, tg, rise_shift, fall_shift):
    d = tg - g
    if d > 0:
        return g + max(1, d >> rise_shift)
    if d < 0:
        return g - max(1, (-d) >> fall_shift)
    return g


def params(**kw):
    """a parameter set as a dict: the creation defaults (a pure delay) with `kw` over them"""
    p = dict(floor=32768, over=16, rise_shift=0, fall_shift=0)
    p.update(kw)
    return p


class Tables:
    def __init__(self, cm, n):
        self.n, self.N, self.H = n, 1 << n, 1 << (n - 1)
        self.sw = cm.denoise_window(n).astype(np.int64)
        wr, wi = cm.spec_twiddles(n)
        self.wr, self.wi = wr.astype(np.int64), wi.astype(np.int64)

    def forward(self, x):
        """one block x[N] -> (re, im) of X = DFT(x sw) / N, int64 [N] each: the spectrum's transform"""
        n, N = self.n, self.N
        v = np.asarray(x, dtype=np.int64) * self.sw
        assert np.abs(v).max(initial=0) <= 2 ** 30
        zr = v[bitrev(n)].copy()
        zi = np.zeros_like(zr)
        one = np.int64(1) << 30
        for s in range(1, n + 1):
            m, h = 1 << s, 1 << (s - 1)
            k = np.arange(h) * (N // m)
            Wr, Wi = self.wr[k], self.wi[k]
            zr, zi = zr.reshape(N // m, m), zi.reshape(N // m, m)
            ar, ai, br, bi = zr[:, :h], zi[:, :h], zr[:, h:], zi[:, h:]
            pr = br * Wr - bi * Wi
            pi = br * Wi + bi * Wr
            ar, ai = ar * one + one, ai * one + one
            zr = np.concatenate(((ar + pr) >> 31, (ar - pr) >> 31), axis=1).reshape(N)
            zi = np.concatenate(((ai + pi) >> 31, (ai - pi) >> 31), axis=1).reshape(N)
        return zr, zi

    def inverse(self, ur, ui):
        """Z[N] (natural order) -> (t[N], clamped components): the decimation in time with conjugated twiddles, every
        output sat32((a 2^30 +- P + 2^29) >> 30)"""
        n, N = self.n, self.N
        zr, zi = ur[bitrev(n)].copy(), ui[bitrev(n)].copy()
        one, half = np.int64(1) << 30, np.int64(1) << 29
        lo, hi = -(1 << 31), (1 << 31) - 1
        sat = 0
        self.max_imag = 0
        for s in range(1, n + 1):
            m, h = 1 << s, 1 << (s - 1)
            k = np.arange(h) * (N // m)
            Wr, Wi = self.wr[k], -self.wi[k]
            zr, zi = zr.reshape(N // m, m), zi.reshape(N // m, m)
            ar, ai, br, bi = zr[:, :h], zi[:, :h], zr[:, h:], zi[:, h:]
            pr = br * Wr - bi * Wi
            pi = br * Wi + bi * Wr
            ar, ai = ar * one + half, ai * one + half
            out = []
            for v in ((ar + pr) >> 30, (ar - pr) >> 30, (ai + pi) >> 30, (ai - pi) >> 30):
                c = np.clip(v, lo, hi)
                sat += int((c != v).sum())
                out.append(c)
            zr = np.concatenate(out[0:2], axis=1).reshape(N)
            zi = np.concatenate(out[2:4], axis=1).reshape(N)
        self.max_imag = int(np.abs(zi).max(initial=0))
        return zr, sat


class Row:
    """one (stream, channel)"""

    def __init__(self, tab):
        self.t = tab
        self.np = [0] * (tab.H + 1)
        self.acc = [0] * (tab.H + 1)
        self.reset()

    def reset(self):
        self.x = np.zeros(0, dtype=np.int64)        # every input since frame 0
        self.ola = np.zeros(0, dtype=np.int64)      # the sums of c by absolute frame
        self.blocks = 0                             # blocks done
        self.g = [UNITY] * (self.t.H + 1)
        self.out = 0                                # output frames written

    def block(self, par, learn, cnt):
        """the next block; -> clamped components of its inverse transform"""
        N, H = self.t.N, self.t.H
        j = self.blocks
        c, sat = self.removed(self.x[j * H:j * H + N], par, learn, cnt)
        if len(self.ola) < j * H + N:
            self.ola = np.concatenate((self.ola, np.zeros(j * H + N - len(self.ola), dtype=np.int64)))
        self.ola[j * H:j * H + N] += c
        self.blocks += 1
        return sat

    def removed(self, x, par, learn, cnt):
        """one block x[N] under the row's gains and profile, both updated -> (c[N], clamped components)"""
        t = self.t
        N, H = t.N, t.H
        re, im = t.forward(x)
        assert max(np.abs(re).max(), np.abs(im).max()) <= 2 ** 30
        p = [(int(a) * int(a) + int(b) * int(b)) >> 16 for a, b in zip(re[:H + 1], im[:H + 1])]
        for k in range(H + 1):
            self.g[k] = smooth(self.g[k], target(p[k], self.np[k], par["over"], par["floor"]), par["rise_shift"],
                               par["fall_shift"])
            assert 0 <= self.g[k] <= UNITY
        if learn and cnt < CNT_MAX:
            for k in range(H + 1):
                self.acc[k] = (self.acc[k] if cnt else 0) + p[k]
                self.np[k] = self.acc[k] // (cnt + 1)
        w = UNITY - np.array(self.g, dtype=np.int64)
        zr = (re[:H + 1] * w + (1 << 16)) >> 17
        zi = (im[:H + 1] * w + (1 << 16)) >> 17
        zi[0] = zi[H] = 0
        ur, ui = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
        ur[:H + 1], ui[:H + 1] = zr, zi
        ur[H + 1:], ui[H + 1:] = zr[1:H][::-1], -zi[1:H][::-1]
        tt, sat = t.inverse(ur, ui)
        c = (tt * t.sw + (1 << 14)) >> 15
        assert np.abs(c).max(initial=0) < 2 ** 31
        return c, sat

    def emit(self, count):
        """the next `count` output frames -> (int16 [count], clamped samples)"""
        D = self.t.N - 1
        n = np.arange(self.out, self.out + count)
        m = n - D
        ok = m >= 0
        x = np.where(ok, self.x[np.where(ok, m, 0)], 0) if len(self.x) else np.zeros(count, dtype=np.int64)
        r = np.where(ok, (self.ola[np.where(ok, m, 0)] + (1 << 12)) >> 13, 0) if len(self.ola) else np.zeros(count, dtype=np.int64)
        v = x - r
        y = np.clip(v, -32768, 32767)
        self.out += count
        return y.astype(np.int16), int((y != v).sum())


class Stream:
    """one stream of C rows with its parameters, learn flag, learning count and counters"""

    def __init__(self, tab, channels, p=None):
        self.t, self.C = tab, channels
        self.rows = [Row(tab) for _ in range(channels)]
        self.p = dict(p) if p else params()
        self.learning = False
        self.cnt = 0
        self.clips = 0
        self.sat = 0
        self.max_imag = 0

    def set(self, p):
        self.p = dict(p)

    def learn(self, on):
        if on and not self.learning:
            self.cnt = 0
        self.learning = bool(on)

    def set_profile(self, channel, profile):
        assert not self.learning and all(0 <= int(v) <= NP_MAX for v in profile)
        self.rows[channel].np = [int(v) for v in profile]

    def reset(self):
        for r in self.rows:
            r.reset()
        self.learning = False

    def run(self, x):
        """x: int16 [F][C] -> int16 [F][C]"""
        x = np.asarray(x, dtype=np.int64).reshape(-1, self.C)
        F = x.shape[0]
        y = np.zeros((F, self.C), dtype=np.int16)
        if F == 0:
            return y
        N, H = self.t.N, self.t.H
        for r, col in zip(self.rows, x.T):
            r.x = np.concatenate((r.x, col))
        total = len(self.rows[0].x)
        done = self.rows[0].blocks
        complete = (total - N) // H + 1 if total >= N else 0
        for _ in range(done, complete):
            for r in self.rows:
                self.sat += r.block(self.p, self.learning, self.cnt)
                self.max_imag = max(self.max_imag, self.t.max_imag)
            if self.learning and self.cnt < CNT_MAX:
                self.cnt += 1
        for c, r in enumerate(self.rows):
            y[:, c], clips = r.emit(F)
            self.clips += clips
        return y

    def state(self):
        return self.clips, self.sat, self.cnt
