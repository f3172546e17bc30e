"""The spectrum meter's model for tests/test_spec_host.py and tests/test_gpu_spec.py: the specification of
include/coolmic_hip.h ("spectrum") in numpy int64, stage by stage, with the window and the twiddles taken from the
library (cmhip_spec_window, cmhip_spec_twiddles) so that a last-bit difference between two libms cannot turn into a
parity failure.  Nothing here runs device code or the library's own transform.
"""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def _bitrev(n):
    N = 1 << n
    r = np.zeros(N, dtype=np.int64)
    for b in range(n):
        r |= ((np.arange(N) >> b) & 1) << (n - 1 - b)
    return r


class Model:
    def __init__(self, cm, n):
        self.n, self.N, self.H = n, 1 << n, 1 << (n - 1)
        self.win = cm.spec_window(n).astype(np.int64)
        wr, wi = cm.spec_twiddles(n)
        self.wr, self.wi = wr.astype(np.int64), wi.astype(np.int64)
        self.max_component = 0                      # the largest |re|, |im| any stage of any call has produced

    def powers(self, x):
        """x: integers [..., N] (one block per row) -> p[..., N / 2 + 1] as uint64"""
        n, N = self.n, self.N
        x = np.asarray(x, dtype=np.int64)
        lead = x.shape[:-1]
        v = (x * self.win).reshape(-1, N)
        assert np.abs(v).max(initial=0) < 2**30
        zr = v[:, _bitrev(n)]                       # (the permutation is its own inverse)
        zi = np.zeros_like(zr)
        one = np.int64(1) << 30
        for s in range(1, n + 1):
            m, h = 1 << s, 1 << (s - 1)
            k = np.arange(h) * (N // m)
            Wr, Wi = self.wr[k], self.wi[k]
            zr, zi = zr.reshape(-1, N // m, m), zi.reshape(-1, N // m, m)
            ar, ai, br, bi = zr[:, :, :h], zi[:, :, :h], zr[:, :, h:], zi[:, :, h:]
            pr = br * Wr - bi * Wi
            pi = br * Wi + bi * Wr
            ar, ai = ar * one + one, ai * one + one
            zr = np.concatenate(((ar + pr) >> 31, (ar - pr) >> 31), axis=2).reshape(-1, N)
            zi = np.concatenate(((ai + pi) >> 31, (ai - pi) >> 31), axis=2).reshape(-1, N)
            self.max_component = max(self.max_component, int(np.abs(zr).max(initial=0)), int(np.abs(zi).max(initial=0)))
        re, im = zr[:, :self.H + 1], zi[:, :self.H + 1]
        p = (re * re + im * im).astype(np.uint64) >> np.uint64(16)
        return p.reshape(lead + (self.H + 1,))

    def blocks(self, y, first=0, last=None):
        """the blocks of one channel's transformed samples y (from the stream's frame 0): rows [first, last)"""
        y = np.asarray(y, dtype=np.int64)
        total = (len(y) - self.N) // self.H + 1 if len(y) >= self.N else 0
        last = total if last is None else min(last, total)
        if last <= first:
            return np.zeros((0, self.N), dtype=np.int64)
        return np.lib.stride_tricks.sliding_window_view(y, self.N)[::self.H][first:last]

    def count(self, frames):
        """blocks completed by the stream's first `frames` frames"""
        return (frames - self.N) // self.H + 1 if frames >= self.N else 0

    def bands(self, y, edges, first=0, last=None):
        """the band sums (Python integers) over blocks [first, last) of one channel"""
        p = self.powers(self.blocks(y, first, last))
        tot = [int(v) for v in p.sum(axis=0, dtype=np.uint64)] if len(p) else [0] * (self.H + 1)
        return [sum(tot[edges[b]:edges[b + 1]]) for b in range(len(edges) - 1)]


def octaves(n):
    """the default band table"""
    return [1 << b for b in range(n)] + [(1 << (n - 1)) + 1]
