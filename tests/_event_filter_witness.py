"""The refractory and polarity-aware event filter as the contract words it: one sequential walk over the
stream with three maps (the time of every pixel's last event, and of its last kept event of each polarity class).

event_filter is the witness of tests/test_gpu_event_filter.py and of the host check; the generators below build every case those
tests use.  Every generated stream mixes the event-support witness's stream (70 % of a cycle) with chatter phases (30 %): one pixel
fires every 0.4 rho, and every sixth event falls on one of one or two chosen neighbours instead.  Without chatter no input tells
"support from kept events" from "support from all events".  tests/test_event_filter_interface.py asserts, on the CPU and from the
witness alone, the shares of dropped, kept-with-weight-0, supported and in-between events of every case, and that the polarity flag
and the kept-only rule each change the support of a share of the events: a kernel that ignores either cannot pass the GPU tests."""
import numpy as np

import _event_support_witness as ES


class State:
    """What one chunk hands to the next: the three maps, -inf meaning "none"."""

    def __init__(self, shape):
        self.last_any = np.full(shape, -np.inf, dtype=np.float64)
        self.last_kept = np.full((2,) + tuple(shape), -np.inf, dtype=np.float64)

    def copy(self):
        s = State(self.last_any.shape)
        s.last_any[:], s.last_kept[:] = self.last_any, self.last_kept
        return s

    def tobytes(self):
        return self.last_any.tobytes() + self.last_kept.tobytes()


def event_filter(xs, ys, ts, ps, shape, refractory, tau, radius=1, full_support=1, polarity=False, pixel_mask=None, state=None,
                 kept_only=True):
    """(keep uint8, weights float32, support uint8, the carried State afterwards).  ps None: every event in class 0.  ``state``: the
    carried State, None: no event yet (it is not modified).  kept_only=False is NOT the contract: every unmasked event then updates
    the last_kept maps, which is what a filter that forgot the refractory rule in its support stage computes."""
    H, W = shape
    xs, ys, ts = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64), np.asarray(ts, dtype=np.float64)
    n = len(xs)
    cls = np.zeros(n, dtype=np.int64) if ps is None else (np.asarray(ps) > 0).astype(np.int64)
    st = State(shape) if state is None else state.copy()
    masked = np.zeros(shape, dtype=bool) if pixel_mask is None else np.asarray(pixel_mask) != 0
    keep, support = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    r = radius
    with np.errstate(invalid='ignore'):
        for e in range(n):
            x, y, t, c = xs[e], ys[e], ts[e], cls[e]
            kept = (not masked[y, x]) and not (t - st.last_any[y, x] < refractory)
            st.last_any[y, x] = t
            if kept:
                keep[e] = 1
                if r > 0:
                    y0, y1, x0, x1 = max(0, y - r), min(H - 1, y + r), max(0, x - r), min(W - 1, x + r)
                    lk = st.last_kept[c] if polarity else np.maximum(st.last_kept[0], st.last_kept[1])
                    ok = (t - lk[y0:y1 + 1, x0:x1 + 1] <= tau) & ~masked[y0:y1 + 1, x0:x1 + 1]
                    ok[y - y0, x - x0] = False                  # an event's own pixel never supports it
                    support[e] = ok.sum()
            if kept or (not kept_only and not masked[y, x]):
                st.last_kept[c, y, x] = t
    if radius > 0:
        weights = np.minimum(support, full_support).astype(np.float32) / np.float32(full_support)
    else:
        weights = keep.astype(np.float32)
    return keep, weights, support, st


# ---- case generators ---------------------------------------------------------------------------------------------------------
def make_stream(seed, shape, n, radius, full_support, tau, refractory, tie_run=1):
    """(xs, ys, ts, ps) of n events in cycles of about 1500: 70 % from the event-support witness's make_stream, 30 % chatter phases
    of 40 to 120 events in which one pixel fires every 0.4 refractory and every sixth event falls on one of one or two chosen
    neighbours (within ``radius``, at least 1) instead.  With tie_run > 1 time moves on after every second chatter event: the pair
    of equal stamps is what lets a tau = 0 case see the chattering pixel from its neighbour, and a longer run would put the
    neighbour's own events inside one refractory period.  Polarity is uniformly random."""
    rng = np.random.default_rng(seed + 7777)
    H, W = shape
    cycles = max(1, n // 1500)
    per = -(-n // cycles)
    rn = max(1, radius)
    gap = 2.0 * tau + 2.0 * refractory + 1.0
    X, Y, T = [], [], []
    t0 = 0.0
    for c in range(cycles):
        nb = int(0.7 * per)
        xs, ys, ts = ES.make_stream(seed * 131 + c, shape, nb, rn, full_support, tau=tau, tie_run=tie_run)
        X += xs.tolist(); Y += ys.tolist(); T += (ts + t0).tolist()
        t = T[-1] + gap
        m = per - nb
        while m > 0:
            mm = min(m, int(rng.integers(40, 120)))
            cy, cx = int(rng.integers(H)), int(rng.integers(W))
            nbrs = [(y, x) for y in range(max(0, cy - rn), min(H, cy + rn + 1)) for x in range(max(0, cx - rn), min(W, cx + rn + 1))
                    if (y, x) != (cy, cx)]
            nsel = [nbrs[i] for i in rng.permutation(len(nbrs))[:int(rng.integers(1, 3))]]
            for i in range(mm):
                if i % min(tie_run, 2) == 0:
                    t += refractory * 0.4
                y, x = nsel[int(rng.integers(len(nsel)))] if i % 6 == 5 else (cy, cx)
                X.append(x); Y.append(y); T.append(t)
            t += gap
            m -= mm
        t0 = t
    ps = rng.integers(0, 2, n).astype(np.int8) * 2 - 1          # a {-1, +1} recording
    return np.array(X[:n], dtype=np.int16), np.array(Y[:n], dtype=np.int16), np.array(T[:n], dtype=np.float64), ps


def first_chatter(n):
    """The index at which the first chatter phase of make_stream(.., n, ..) begins"""
    cycles = max(1, n // 1500)
    return int(0.7 * -(-n // cycles))


def long_chatter_stream(n_burst, refractory=1.0):
    """One pixel of a 3x3 sensor fires n_burst times, every event inside ``refractory`` of its predecessor (only the first is kept),
    then its neighbour fires once, one step later.  (xs, ys, ts, ps, the burst's duration, the last gap)."""
    step = refractory / 4.0
    xs = np.ones(n_burst + 1, dtype=np.int16)
    ys = np.ones(n_burst + 1, dtype=np.int16)
    xs[-1] = 2
    ts = np.arange(n_burst + 1, dtype=np.float64) * step
    ps = (np.arange(n_burst + 1) % 2).astype(np.int8)
    return xs, ys, ts, ps, float(ts[-1] - ts[0]), step


def two_pixel_stream(n, refractory=1.0):
    """n events alternating on two adjacent pixels of a 3x3 sensor, in phases of 500: steps of refractory / 8 (a pixel's own events
    are a quarter of refractory apart: dropped after the first), then steps of refractory (all kept)."""
    i = np.arange(n)
    xs, ys = (i % 2).astype(np.int16), np.ones(n, dtype=np.int16)
    fast = (i // 500) % 2 == 0
    ts = np.cumsum(np.where(fast, refractory / 8.0, refractory))
    ps = ((i // 3) % 2).astype(np.int8)
    return xs, ys, ts, ps


# name -> dict(shape, n, radius, full_support, tau, refractory, tie_run, seed, mask): every generated case of the GPU module, from
# the specs of the event-support witness (sensors 3x3, 5x7, 33x65, 260x346; r = 1, 2, 3; full_support 1, a middle value, the
# maximum; masks; tie runs; tau = 0) with refractory = tau / 4 (1 where tau is 0), plus a case with the support stage off.
GENERATED = {}
for _name, _s in ES.GENERATED.items():
    if _name.startswith('5x7-r1-k1-n'):
        continue                                             # (the sizes around the kernels' steps have a test of their own)
    GENERATED[_name] = dict(_s, refractory=_s['tau'] / 4.0 if _s['tau'] > 0 else 1.0)
GENERATED['5x7-r0'] = dict(shape=(5, 7), n=900, radius=0, full_support=1, tau=1.0, refractory=0.25, tie_run=1, seed=30, mask=None)


def generated(name):
    """(xs, ys, ts, ps, mask | None, spec) of a generated case."""
    s = GENERATED[name]
    xs, ys, ts, ps = make_stream(s['seed'], s['shape'], s['n'], s['radius'], s['full_support'], s['tau'], s['refractory'], s['tie_run'])
    mask = None if s['mask'] is None else ES.make_mask(s['mask'], s['shape'])
    return xs, ys, ts, ps, mask, s


def run(name, polarity=False, **kw):
    """The witness on a generated case"""
    xs, ys, ts, ps, mask, s = generated(name)
    return event_filter(xs, ys, ts, ps, s['shape'], s['refractory'], s['tau'], s['radius'], s['full_support'], polarity, mask, **kw)
