"""Numpy witness of the batched flow-error evaluation, written for this repository.  It restates three things:

  the per-pixel arithmetic   valid(f) = both components not +-inf and sqrt(fx fx + fy fy) > 0; in the intersection of the event plane
                             (and the optional error mask), the valid predicted flow and the valid ground truth:
                             ee = sqrt(dx dx + dy dy), ree = ee / (sqrt(gx gx + gy gy) + eps), six strict comparisons ee > N
  the tap order              a theta below the sensor's size is scaled as v = sum_i a_i (sum_j b_j theta[i0 + i][j0 + j]) over the
                             non-zero runs of the rows of the two resample matrices, j inside i, every product rounded before it is
                             added, every sum starting from +0.0  (``upsample``)
  the summation order        pixel p belongs to thread t = p % 256 of workgroup g = (p // 256) % 32 and is the k-th term of that
                             thread's chain, k = p // 8192; a chain is summed in ascending k from +0.0; the 64 chains of a wave go
                             through the tree v[i] += v[i + o], o = 32, 16, ..., 1; the four waves of a workgroup are added in index
                             order from +0.0; the 32 workgroup partials of a window are added in index order from +0.0
                             (``ordered_sum``)
A term outside the intersection is +0.0 here, where the kernel adds nothing: both leave a non-negative partial sum unchanged.
The module also builds the fields the CPU and the GPU tests share (``random_case``, ``special_case``)."""
import numpy as np

EPSN = 2.0 ** -52
NT, PARTS, WAVE = 256, 32, 64
THRESHOLDS = (1, 2, 3, 5, 10, 20)


def valid(f):
    """flow_eval.py's mask of an (..., 2) flow."""
    with np.errstate(all='ignore'):
        x, y = f[..., 0], f[..., 1]
        return ~np.isinf(x) & ~np.isinf(y) & (np.sqrt(x * x + y * y) > 0)


def event_plane(xs, ys, shape):
    m = np.zeros(shape, dtype=bool)
    m[np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)] = True
    return m


def runs(A):
    """The non-zero run [lo, lo + cnt) of every row of a resample matrix (n_out, n_in); (0, 0) for a row of zeros."""
    out = []
    for row in A:
        nz = np.flatnonzero(row != 0.0)
        out.append((int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.size else (0, 0))
    return out


def upsample(theta, A_H, A_W):
    """theta (h, w, 2) -> (H, W, 2) in the kernel's tap order.  The inner sum of output pixel (y, x) over theta row r depends on (r, x)
    only, so it is formed once per (r, x): the same chain of operations the kernel runs for every y that reads row r."""
    theta = np.asarray(theta, dtype=np.float64)
    h, w = theta.shape[:2]
    H, W = A_H.shape[0], A_W.shape[0]
    with np.errstate(all='ignore'):
        S = np.zeros((h, W, 2))
        for x, (j0, nj) in enumerate(runs(A_W)):
            s = np.zeros((h, 2))
            for j in range(nj):
                s = s + A_W[x, j0 + j] * theta[:, j0 + j, :]
            S[:, x] = s
        V = np.zeros((H, W, 2))
        for y, (i0, ni) in enumerate(runs(A_H)):
            v = np.zeros((W, 2))
            for i in range(ni):
                v = v + A_H[y, i0 + i] * S[i0 + i]
            V[y] = v
    return V


def ordered_sum(terms):
    """The float64 sum of one window's per-pixel terms (flat, +0.0 outside the intersection) in the order of section 18."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    per = PARTS * NT
    k = -(-t.size // per)
    t = np.concatenate([t, np.zeros(k * per - t.size)]).reshape(k, PARTS, NT)
    with np.errstate(all='ignore'):
        acc = np.zeros((PARTS, NT))
        for i in range(k):                                  # the thread chains, ascending pixel index
            acc = acc + t[i]
        v = acc.reshape(PARTS, NT // WAVE, WAVE).copy()
        o = WAVE // 2
        while o >= 1:                                       # the wave tree: lane i takes lane i + o
            v[..., :o] = v[..., :o] + v[..., o:2 * o]
            o //= 2
        wave = v[..., 0]
        part = np.zeros(PARTS)
        for i in range(NT // WAVE):                         # the waves of a workgroup in index order
            part = part + wave[:, i]
        tot = np.float64(0.0)
        for g in range(PARTS):                              # the partials of a window in index order
            tot = tot + part[g]
    return float(tot)


def flow_errors(pred, gt, events, eval_mask=None):
    """One window.  pred (H, W, 2): theta at the sensor's size (``upsample`` of a coarser one); gt (H, W, 2); events (xs, ys);
    eval_mask None or (H, W).  Returns every field of eincm_flow_error_out and 'ee_map'."""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    bit0 = event_plane(events[0], events[1], gt.shape[:2])
    if eval_mask is not None:
        bit0 = bit0 & (np.asarray(eval_mask) != 0)
    pv = bit0 & valid(pred)
    gv = valid(gt)
    both = pv & gv
    with np.errstate(all='ignore'):
        dx, dy = pred[..., 0] - gt[..., 0], pred[..., 1] - gt[..., 1]
        ee = np.sqrt(dx * dx + dy * dy)
        ree = ee / (np.sqrt(gt[..., 0] * gt[..., 0] + gt[..., 1] * gt[..., 1]) + EPSN)
    n_ee = int(both.sum())
    n_over = [int((both & (ee > n)).sum()) for n in THRESHOLDS]
    sum_ee = ordered_sum(np.where(both, ee, 0.0))
    sum_ree = ordered_sum(np.where(both, ree, 0.0))
    return {
        'n_ee': n_ee, 'n_pred': int(pv.sum()), 'n_gt': int(gv.sum()), 'n_over': n_over, 'sum_ee': sum_ee, 'sum_ree': sum_ree,
        'aee': sum_ee / float(n_ee) if n_ee else float('nan'), 'aree': sum_ree / float(n_ee) if n_ee else float('nan'),
        'anpe': [float(np.int64(k) * 100) / (float(n_ee) + EPSN) for k in n_over],
        'ee_map': np.where(both, ee, np.nan),
    }


# -- fields the tests share -----------------------------------------------------------------------------------------------------------
def random_case(seed, H, W, n_events=None, special=True):
    """A window with smooth-ish random flows, events on about a third of the pixels (some pixels several times), and, with ``special``,
    a sprinkling of NaN, +-inf and exact zeros in both fields.  Returns (theta (H, W, 2), gt (H, W, 2), (xs, ys))."""
    rng = np.random.default_rng(seed)
    gt = rng.normal(0.0, 6.0, size=(H, W, 2))
    theta = gt + rng.normal(0.0, 3.0, size=(H, W, 2))
    if special:
        for f in (gt, theta):
            for val in (np.nan, np.inf, -np.inf, 0.0):
                k = max(1, H * W // 40)
                f[rng.integers(0, H, k), rng.integers(0, W, k), rng.integers(0, 2, k)] = val
            z = rng.integers(0, H * W, max(1, H * W // 30))
            f.reshape(-1, 2)[z] = 0.0                        # whole vectors of exact zeros
    n = H * W // 3 if n_events is None else n_events
    xs = rng.integers(0, W, n).astype(np.int16)
    ys = rng.integers(0, H, n).astype(np.int16)
    return theta, gt, (xs, ys)


def special_case():
    """One constructed (7, 13) window.  Row by row, (pred, gt) of pixels that hold events unless said otherwise:
      row 0   the corners (0, 0) and (0, 12) hold ordinary vectors; between them +-inf and NaN in either component of either field
      row 1   exact zeros (+0.0 and -0.0) in either field; 1e-200 vectors whose norm underflows to 0; 1e-160 whose norm does not
      row 2   differences of exactly (0,1) (0,2) (0,3) (3,4) (6,8) (12,16): ee equals a threshold; then each a little above its threshold
      row 3   ordinary vectors WITHOUT events (so outside bit 0), one of them with several events on its right neighbour
      row 6   the corners (6, 0) and (6, 12)
    Returns (theta, gt, (xs, ys), expect) with expect = the counts worked by hand."""
    H, W = 7, 13
    gt = np.zeros((H, W, 2))
    th = np.zeros((H, W, 2))
    ev = []
    inf, nan = np.inf, np.nan

    def put(y, x, p, g, event=True):
        th[y, x], gt[y, x] = p, g
        if event:
            ev.append((x, y))
    # row 0
    put(0, 0, (1.5, -2.0), (1.0, -2.0))                     # in
    put(0, 1, (inf, 1.0), (1.0, 1.0))
    put(0, 2, (1.0, -inf), (1.0, 1.0))
    put(0, 3, (nan, 1.0), (1.0, 1.0))
    put(0, 4, (1.0, nan), (1.0, 1.0))
    put(0, 5, (1.0, 1.0), (inf, 0.0))
    put(0, 6, (1.0, 1.0), (0.0, -inf))
    put(0, 7, (1.0, 1.0), (nan, 1.0))
    put(0, 8, (1.0, 1.0), (1.0, nan))
    put(0, 9, (inf, nan), (nan, inf))
    put(0, 12, (-3.0, 0.25), (-2.0, 0.5))                   # in
    # row 1
    put(1, 0, (0.0, 0.0), (1.0, 1.0))
    put(1, 1, (-0.0, 0.0), (1.0, 1.0))
    put(1, 2, (1.0, 1.0), (0.0, 0.0))
    put(1, 3, (1.0, 1.0), (0.0, -0.0))
    put(1, 4, (1e-200, 1e-200), (1.0, 1.0))                 # pred norm underflows: excluded
    put(1, 5, (1.0, 1.0), (1e-200, 0.0))                    # gt norm underflows: excluded
    put(1, 6, (1e-160, 0.0), (1.0, 1.0))                    # norm 1e-160 > 0: in
    put(1, 7, (0.0, 2.0), (0.0, 1.0))                       # one zero component: in
    # row 2: on and just above every threshold
    base = (1.0, 2.0)
    for k, d in enumerate([(0, 1), (0, 2), (0, 3), (3, 4), (6, 8), (12, 16)]):
        put(2, k, (base[0] + d[0], base[1] + d[1]), base)
        put(2, 6 + k, (base[0] + d[0], np.nextafter(base[1] + d[1], np.inf)), base)
    # row 3: no events on the first two; several on the third
    put(3, 0, (5.0, 5.0), (1.0, 1.0), event=False)
    put(3, 1, (2.0, 2.0), (1.0, 1.0), event=False)
    put(3, 2, (2.0, 2.0), (1.0, 1.0))
    ev += [(2, 3)] * 3
    # row 6
    put(6, 0, (0.5, 0.5), (0.25, 0.5))
    put(6, 12, (30.0, 0.0), (1.0, 0.0))
    xs = np.array([e[0] for e in ev], dtype=np.int16)
    ys = np.array([e[1] for e in ev], dtype=np.int16)
    # by hand: in the intersection are (0,0) (0,12) (1,6) (1,7), the 12 pixels of row 2, (3,2), (6,0), (6,12) = 19
    # pred valid and on an event: those 19 + gt-invalid ones (0,5) (0,6) (0,7) (0,8) (1,2) (1,3) (1,5) = 26
    # gt valid anywhere: 19 + pred-invalid event pixels (0,1) (0,2) (0,3) (0,4) (1,0) (1,1) (1,4) + event-less (3,0) (3,1) = 28
    # ee > N strictly: the at-threshold pixels of row 2 count for the thresholds below their own (5, 4, 3, 2, 1, 0), the ones just above
    # for their own too (6, 5, 4, 3, 2, 1); (6,12) has ee = 29; (0,12), (1,6) and (3,2) have 1 < ee < 2; (1,7) has ee = 1 exactly
    expect = {'n_ee': 19, 'n_pred': 26, 'n_gt': 28, 'n_over': [5 + 6 + 4, 4 + 5 + 1, 3 + 4 + 1, 2 + 3 + 1, 1 + 2 + 1, 0 + 1 + 1]}
    return th, gt, (xs, ys), expect
