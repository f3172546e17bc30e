"""The drift stage as include/coolmic_hip.h ("clock-drift compensation") states it, in numpy and Python integers:
the model the device tests hold the kernels against.  Written from the header's text alone."""
import numpy as np

ONE = 1 << 32
DELTA_MAX = 1 << 24


def table_valid(H):
    """the header's validity rule for H[P][T]"""
    H = np.asarray(H)
    if H.ndim != 2:
        return False
    P, T = H.shape
    phi = P.bit_length() - 1
    if P != 1 << phi or not 5 <= phi <= 8 or T < 4 or T > 64 or T & 1:
        return False
    return H[0, 0] == 0 and int(np.abs(H.astype(np.int64)).sum(axis=1).max()) <= 65535


def with_row_p(H):
    """the (P + 1)-row table: row P is row 0 moved by one tap"""
    H = np.asarray(H, dtype=np.int64)
    last = np.zeros((1, H.shape[1]), dtype=np.int64)
    last[0, :-1] = H[0, 1:]
    return np.concatenate([H, last])


def out_frames(pos, delta, frames):
    """K = ceil((F * 2^32 - pos) / step), 0 when pos >= F * 2^32"""
    end = frames * ONE
    if pos >= end:
        return 0
    step = ONE + delta
    return -((pos - end) // step)


def next_pos(pos, delta, frames):
    return pos + out_frames(pos, delta, frames) * (ONE + delta) - frames * ONE


def resample(H1, phi, hist, x, pos, delta):
    """One run of one stream: H1 the (P + 1)-row table (int64), hist int [T-1][C] (oldest first), x int [F][C].
    -> (y int16 [K][C], the new history, the new pos, the count of outputs whose rounded value left int16)"""
    T = H1.shape[1]
    x = np.asarray(x, dtype=np.int64).reshape(-1, np.asarray(hist).shape[1])
    F = x.shape[0]
    K = out_frames(pos, delta, F)
    ext = np.concatenate([np.asarray(hist, dtype=np.int64), x])     # x[i] is ext[i + T - 1]
    new_hist = ext[len(ext) - (T - 1):].copy()
    if K == 0:
        return np.zeros((0, x.shape[1]), dtype=np.int16), new_hist, next_pos(pos, delta, F), 0
    t = np.uint64(pos) + np.arange(K, dtype=np.uint64) * np.uint64(ONE + delta)
    n = (t >> np.uint64(32)).astype(np.int64)
    f = (t & np.uint64(ONE - 1)).astype(np.int64)
    p = f >> (32 - phi)
    mu = (f >> (17 - phi)) & 32767
    assert n[-1] < F
    idx = n[:, None] + (T - 1) - np.arange(T)[None, :]               # [K][T]: x[n - k]
    xs = ext[idx]                                                   # [K][T][C]
    a0 = np.einsum("kt,ktc->kc", H1[p], xs)
    a1 = np.einsum("kt,ktc->kc", H1[p + 1], xs)
    assert np.abs(a0).max() < 1 << 31 and np.abs(a1).max() < 1 << 31
    num = a0 * (32768 - mu)[:, None] + a1 * mu[:, None]
    y = (num + (1 << 28)) >> 29
    sat = int(np.count_nonzero((y < -32768) | (y > 32767)))
    return np.clip(y, -32768, 32767).astype(np.int16), new_hist, next_pos(pos, delta, F), sat


class DriftModel:
    """S streams of C channels through the table H[P][T]"""

    def __init__(self, streams, channels, H):
        assert table_valid(H)
        self.S, self.C = streams, channels
        self.H1 = with_row_p(H)
        self.T = self.H1.shape[1]
        self.phi = (self.H1.shape[0] - 1).bit_length() - 1
        self.delta = [0] * streams
        self.saturated = 0
        self.outputs = 0
        for s in range(streams):
            self.reset(s)

    def reset(self, s):
        if s == -1:
            for i in range(self.S):
                self.reset(i)
            return
        if not hasattr(self, "hist"):
            self.hist, self.pos = [None] * self.S, [0] * self.S
            self.in_total, self.out_total = [0] * self.S, [0] * self.S
        self.hist[s] = np.zeros((self.T - 1, self.C), dtype=np.int64)
        self.pos[s] = self.in_total[s] = self.out_total[s] = 0

    def _streams(self, s):
        return range(self.S) if s == -1 else [s]

    def set(self, s, delta):
        assert abs(delta) <= DELTA_MAX
        for i in self._streams(s):
            self.delta[i] = delta

    def seek(self, s, frac):
        assert 0 <= frac < ONE
        for i in self._streams(s):
            self.pos[i] = frac

    def get(self, s):
        return self.delta[s], self.pos[s], self.in_total[s], self.out_total[s]

    def run_stream(self, s, x):
        y, self.hist[s], self.pos[s], sat = resample(self.H1, self.phi, self.hist[s], x, self.pos[s], self.delta[s])
        self.in_total[s] += len(x)
        self.out_total[s] += len(y)
        self.saturated += sat
        self.outputs += y.size
        return y

    def run(self, xs):
        """xs: per stream an int array [F_s][C] -> per stream int16 [K_s][C]"""
        return [self.run_stream(s, xs[s]) for s in range(self.S)]


def dense_table(rng, phi, T):
    """A table whose every tap matters: |h| in [3B/4, B] with B = min(65535 // T, 4096), random signs, H[0][0] = 0.
    (A designed table's edge taps are 2-3 units and would let a halo mistake through.)"""
    B = min(65535 // T, 4096)
    H = rng.integers(3 * B // 4, B + 1, size=(1 << phi, T)) * rng.choice([-1, 1], size=(1 << phi, T))
    H[0, 0] = 0
    return H.astype(np.int16)


def unit_table(phi, T):
    """every row the unit at tap T/2: with delta = 0 the input delayed by T/2 frames, bit for bit"""
    H = np.zeros((1 << phi, T), dtype=np.int16)
    H[:, T // 2] = 16384
    return H


class ServoModel:
    """the header's servo"""

    def __init__(self, target, kp_log2, ki_log2, limit=DELTA_MAX):
        self.target, self.kp, self.ki, self.limit = target, kp_log2, ki_log2, limit
        self.integ = self.delta = self.clamped = 0

    def step(self, fill):
        if fill < 0 or fill >= 1 << 31:
            return self.delta
        e = fill - self.target
        raw = e * (1 << self.kp) + (self.integ + e) * (1 << self.ki)
        if abs(raw) <= self.limit:
            self.integ += e
            self.delta, self.clamped = raw, 0
        else:
            self.delta, self.clamped = (self.limit if raw > 0 else -self.limit), 1
        return self.delta
