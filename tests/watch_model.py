"""The model of the signal watch (include/coolmic_hip.h, "signal watch"): the online definition on the TRANSFORMED
stream, in plain Python (`online`) and in numpy (`run_lengths`, the same recurrence solved for every frame at once;
tests/test_watch_host.py holds the two against each other).  Never the device code, never csrc/watch_plan.h.

    l(n) = l(n - 1) + 1 if P(n) else 0,   l(-1) = the state the stream brought along
"""
import numpy as np

KEYS = ("quiet_frames", "quiet_longest", "quiet_current", "clip_samples", "clip_events", "clip_longest", "sum", "dc")


def online(P, l0, K):
    """plain Python: (count, longest, events, state) of the frames P from the state l0"""
    cnt = longest = ev = 0
    l = l0
    for p in P:
        l = l + 1 if p else 0
        cnt += 1 if p else 0
        longest = max(longest, l)
        ev += 1 if l == K else 0
    return cnt, longest, ev, l


def run_lengths(P, l0):
    """numpy: l(n) for every frame of P.  A frame's run reaches back to the last frame without P; where there is none
    it reaches back into the state."""
    P = np.asarray(P, dtype=bool)
    pos = np.arange(P.size, dtype=np.int64)
    last_zero = np.maximum.accumulate(np.where(P, -1, pos))
    return np.where(last_zero < 0, l0 + pos + 1, pos - last_zero) * P


class Watch:
    """one stream's watch: feed() transformed interleaved samples run by run, result() closes the window and keeps
    the state, reset() clears both"""

    def __init__(self, channels, quiet=32, rail=32767, clip_run=3, rate=48000):
        self.C, self.quiet, self.rail, self.K, self.rate = channels, quiet, rail, clip_run, rate
        self.reset()

    def reset(self):
        self.state = [0] * (2 * self.C + 1)          # dead, quiet per channel, rail per channel
        self._open()

    def configure(self, quiet, rail, clip_run):
        assert self.frames == 0
        self.quiet, self.rail, self.K = quiet, rail, clip_run
        self.reset()

    def _open(self):
        n = 2 * self.C + 1
        self.frames = 0
        self.cnt, self.longest, self.ev = [0] * n, [0] * n, [0] * n
        self.sum = [0] * self.C

    def predicates(self, y):
        f = np.asarray(y, dtype=np.int64).reshape(-1, self.C)
        q = (f >= -self.quiet) & (f <= self.quiet)
        r = (f >= self.rail) | (f <= -self.rail)
        return f, [q.all(axis=1)] + [q[:, c] for c in range(self.C)] + [r[:, c] for c in range(self.C)]

    def feed(self, y):
        f, preds = self.predicates(y)
        if f.shape[0] == 0:
            return
        for p, P in enumerate(preds):
            l = run_lengths(P, self.state[p])
            self.cnt[p] += int(P.sum())
            self.longest[p] = max(self.longest[p], int(l.max()))
            self.ev[p] += int((l == self.K).sum())
            self.state[p] = int(l[-1])
        for c in range(self.C):
            self.sum[c] += int(f[:, c].sum())
        self.frames += f.shape[0]

    def peek(self):
        """the window as WatchResult.as_dict() gives it; None for an empty window"""
        if self.frames == 0:
            return None
        C = self.C
        return {"rate": self.rate, "channels": C, "frames": self.frames, "quiet": self.quiet, "rail": self.rail,
                "clip_run": self.K,
                "dead_frames": self.cnt[0], "dead_longest": self.longest[0], "dead_current": self.state[0],
                "quiet_frames": self.cnt[1:1 + C], "quiet_longest": self.longest[1:1 + C],
                "quiet_current": self.state[1:1 + C],
                "clip_samples": self.cnt[1 + C:], "clip_events": self.ev[1 + C:], "clip_longest": self.longest[1 + C:],
                "sum": list(self.sum),
                "dc": [float(s) / float(self.frames) / 32768.0 for s in self.sum]}

    def result(self):
        d = self.peek()
        self._open()
        return d
