"""The event-support filter as the contract words it: one sequential walk over the stream with a last-time map.

support_filter is the witness of tests/test_gpu_event_support.py and of the host check; the generators below build every case those
tests use.  tests/test_event_support_interface.py asserts, on the CPU and from the witness alone, that every generated case has at
least 20 % of its events at weight 0, at least 20 % at weight 1 and, where full_support > 1, at least 10 % strictly between: a
kernel that returns a constant cannot pass the GPU tests."""
import numpy as np


def new_map(shape):
    return np.full(shape, -np.inf, dtype=np.float64)


def support_filter(xs, ys, ts, shape, tau, radius=1, full_support=1, pixel_mask=None, last=None):
    """(weights float32, support uint8, the carried map afterwards).  ``last``: the carried map (H, W) float64, None: no event yet."""
    H, W = shape
    xs, ys, ts = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64), np.asarray(ts, dtype=np.float64)
    last = new_map(shape) if last is None else np.array(last, dtype=np.float64)
    masked = np.zeros(shape, dtype=bool) if pixel_mask is None else np.asarray(pixel_mask) != 0
    support = np.zeros(len(xs), dtype=np.uint8)
    r = radius
    for e in range(len(xs)):
        x, y, t = xs[e], ys[e], ts[e]
        if not masked[y, x]:
            y0, y1, x0, x1 = max(0, y - r), min(H - 1, y + r), max(0, x - r), min(W - 1, x + r)
            ok = (t - last[y0:y1 + 1, x0:x1 + 1] <= tau) & ~masked[y0:y1 + 1, x0:x1 + 1]
            ok[y - y0, x - x0] = False                      # an event's own pixel never supports it
            support[e] = ok.sum()
        last[y, x] = t
    weights = np.minimum(support, full_support).astype(np.float32) / np.float32(full_support)
    return weights, support, last


def max_support(radius):
    return (2 * radius + 1) ** 2 - 1


# ---- case generators ---------------------------------------------------------------------------------------------------------
def _border_pixels(H, W):
    """The four corners and the middles of the four edges."""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]


def make_stream(seed, shape, n, radius, full_support, tau=1.0, tie_run=1, unit=None):
    """A stream of n events in cycles of three phases.  quiet: lone events more than tau apart, many of them on corners and edges
    (support 0).  dense: a block of pixels fires pass after pass, all inside one tau (interior events reach every neighbour).
    partial: a few events in a small block inside one tau (support in between).  Time moves on after every ``tie_run`` events of the
    dense and partial phases, so tie_run > 1 gives runs of equal timestamps; tau = 0 leaves those runs as the only support.
    ``unit``: events per cycle (default: n where full_support is the maximum, which needs large blocks, else at most 600)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    if unit is None:
        unit = n if (full_support == max_support(radius) and radius > 1) or n <= 600 else 600
    unit = max(unit, 8)
    xs, ys, ts = [], [], []
    t = 0.0
    gap = 2.0 * tau + 1.0
    border = _border_pixels(H, W)

    def burst(pix, span_events):
        """pix in order, inside one tau (tau = 0: time moves one unit per run of equal stamps)"""
        nonlocal t
        dt = (tau * 0.9 / max(1, span_events // tie_run + 1)) if tau > 0 else 1.0
        for i, (y, x) in enumerate(pix):
            if i and i % tie_run == 0:
                t += dt
            ys.append(y); xs.append(x); ts.append(t)

    while len(xs) < n:
        # quiet: 30 % of the unit
        for _ in range(max(1, int(0.30 * unit))):
            t += gap
            y, x = border[rng.integers(len(border))] if rng.random() < 0.4 else (rng.integers(H), rng.integers(W))
            ys.append(int(y)); xs.append(int(x)); ts.append(t)
        t += gap
        # dense: 45 % of the unit, three passes over a block; the block touches a corner in every other cycle
        reps = 3
        side = int(np.ceil(np.sqrt(0.45 * unit / reps)))
        bh, bw = min(H, side), min(W, max(side, int(np.ceil(0.45 * unit / reps / min(H, side)))))
        y0 = rng.integers(0, H - bh + 1) if rng.random() < 0.5 else (0 if rng.random() < 0.5 else H - bh)
        x0 = rng.integers(0, W - bw + 1) if rng.random() < 0.5 else (0 if rng.random() < 0.5 else W - bw)
        block = [(int(y0 + j), int(x0 + i)) for j in range(bh) for i in range(bw)]
        reps = max(reps, int(np.ceil(0.45 * unit / len(block))))      # (a small sensor: more passes, not fewer dense events)
        pix = []
        for rep in range(reps):
            pix += block if rep % 2 == 0 else [block[k] for k in rng.permutation(len(block))]
        burst(pix, len(pix))
        t += gap
        # partial: 25 % of the unit, in bursts of a few events each on a small block
        left = max(1, int(0.25 * unit))
        while left > 0:
            m = int(min(left, rng.integers(2, 3 + full_support)))
            s = radius + 2
            cy, cx = rng.integers(0, max(1, H - s + 1)), rng.integers(0, max(1, W - s + 1))
            burst([(int(min(H - 1, cy + rng.integers(s))), int(min(W - 1, cx + rng.integers(s)))) for _ in range(m)], m)
            t += gap
            left -= m
    return (np.array(xs[:n], dtype=np.int16), np.array(ys[:n], dtype=np.int16), np.array(ts[:n], dtype=np.float64))


def make_mask(seed, shape, frac=0.08):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < frac).astype(np.uint8)


def two_pixel_stream(n, tau=1.0):
    """n events on two adjacent pixels of a 3x3 sensor: alternating (each supports the other), bursts on one pixel while the other
    stays silent for longer than tau (no support), and runs of equal timestamps.  The lists of both pixels hold ~n / 2 indices."""
    xs, ys, ts = np.zeros(n, dtype=np.int16), np.ones(n, dtype=np.int16), np.zeros(n, dtype=np.float64)
    i = np.arange(n)
    phase = (i // 500) % 4
    # phase 0, 2: alternate at steps of tau / 4; phase 1: pixel 0 only; phase 3: pixel 1 only, at steps of tau (the other pixel's last event ages out)
    xs[:] = np.where(phase == 1, 0, np.where(phase == 3, 1, i % 2))
    step = np.where((phase == 1) | (phase == 3), tau * 1.5, tau * 0.25)
    step[(i % 7 == 0) & (phase == 0)] = 0.0               # equal timestamps inside the alternating phases
    ts[:] = np.cumsum(step)
    return xs, ys, ts


def tie_stream(shape, n_one, n_spread, t0=5.0):
    """Runs of equal timestamps longer than a wave: n_one events at one pixel, then n_spread events walking a 3x3 neighbourhood,
    all at one time; then the same again one time unit later."""
    H, W = shape
    cy, cx = H // 2, W // 2
    xs, ys, ts = [], [], []
    for rep in range(2):
        t = t0 + rep
        xs += [cx] * n_one; ys += [cy] * n_one; ts += [t] * n_one
        for i in range(n_spread):
            xs.append(min(W - 1, max(0, cx + (i % 3) - 1))); ys.append(min(H - 1, max(0, cy + ((i // 3) % 3) - 1))); ts.append(t)
    return np.array(xs, dtype=np.int16), np.array(ys, dtype=np.int16), np.array(ts, dtype=np.float64)


# name -> dict(shape, n, radius, full_support, tau, tie_run, seed, mask): every generated case of the GPU module.  Sensors 3x3, 5x7,
# 33x65 (a 32-pixel tile edge, odd sizes) and 260x346; r = 1, 2, 3; full_support 1, a middle value, the maximum (the maximum needs a
# pixel whose whole window lies inside the sensor and inside a dense block: 33x65).
GENERATED = {}


def _gen(name, shape, n, radius, full_support, tau=1.0, tie_run=1, seed=0, mask=None):
    assert name not in GENERATED
    GENERATED[name] = dict(shape=shape, n=n, radius=radius, full_support=full_support, tau=tau, tie_run=tie_run, seed=seed, mask=mask)


_gen('3x3-r1-k1', (3, 3), 400, 1, 1, seed=1)
_gen('3x3-r1-k3', (3, 3), 600, 1, 3, seed=2)          # (a corner has 3 neighbours)
_gen('3x3-r1-k5', (3, 3), 900, 1, 5, seed=3)          # (an edge pixel has 5: the corners stay in between)
_gen('3x3-r3-k8', (3, 3), 500, 3, 8, seed=4)          # (r = 3 on 3x3: every other pixel is a neighbour)
_gen('5x7-r1-k1', (5, 7), 700, 1, 1, seed=5)
_gen('5x7-r2-k5', (5, 7), 900, 2, 5, seed=6)
_gen('5x7-r3-k6', (5, 7), 900, 3, 6, seed=7)
_gen('5x7-r1-k1-tau0', (5, 7), 800, 1, 1, tau=0.0, tie_run=9, seed=8)
_gen('5x7-r2-k3-ties', (5, 7), 1500, 2, 3, tie_run=150, seed=9)
_gen('33x65-r1-k1', (33, 65), 3000, 1, 1, seed=10)
_gen('33x65-r1-kmax', (33, 65), 3000, 1, 8, seed=11)
_gen('33x65-r2-k12', (33, 65), 3000, 2, 12, seed=12)
_gen('33x65-r2-kmax', (33, 65), 9000, 2, 24, seed=13)
_gen('33x65-r3-k24', (33, 65), 6000, 3, 24, seed=14)
_gen('33x65-r3-kmax', (33, 65), 9000, 3, 48, seed=15)
_gen('33x65-r2-k4-mask', (33, 65), 3000, 2, 4, seed=16, mask=17)
_gen('5x7-r1-k4-mask', (5, 7), 900, 1, 4, seed=18, mask=19)
_gen('260x346-r1-k3', (260, 346), 20000, 1, 3, seed=20)
# n on both sides of the trip and block sizes of the kernels: 64 (a wave, a trip of the sort), 256 (a workgroup), 1024 (a block of the
# sort), 2048 (two blocks), 16384 (16 blocks: one tile of 4096 histogram entries of the scan)
for _n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385):
    _gen(f'5x7-r1-k1-n{_n}', (5, 7), _n, 1, 1, seed=100 + _n)


def generated(name):
    """(xs, ys, ts, mask | None, spec) of a generated case."""
    s = GENERATED[name]
    xs, ys, ts = make_stream(s['seed'], s['shape'], s['n'], s['radius'], s['full_support'], tau=s['tau'], tie_run=s['tie_run'])
    mask = None if s['mask'] is None else make_mask(s['mask'], s['shape'])
    return xs, ys, ts, mask, s


def weight_fractions(weights, full_support):
    """(fraction at 0, fraction at 1, fraction strictly between)"""
    w = np.asarray(weights)
    n = max(1, len(w))
    return (w == 0).sum() / n, (w == 1).sum() / n, ((w > 0) & (w < 1)).sum() / n
