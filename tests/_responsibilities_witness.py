"""The E-step operator (eincm_event_responsibilities in include/eincm.h) stated in numpy, three ways:

(a) responsibilities_f32: the rule of the header from given combined scores s, selfs q, weights w and priors pi, every operation one
    numpy float32 operation in the stated order.  Fed with the GPU's own Engine.event_scores output it must give the operator's
    bytes (tests/test_gpu_responsibilities.py).
(b) responsibilities_f64: the same rule in float64 on top of _event_scores_witness.event_scores (imported read-only).
(c) em_witness: the EM loop of segmentation.segment_motions for translations, the M-step scipy's BFGS on
    _event_weights_witness.loss_and_grad at a 1x1 theta, the E-step (b)'s scores through (a)'s rule.

It also holds the case generators of the GPU module; tests/test_responsibilities_interface.py asserts on the CPU, from this file
alone, the conditions that keep that module honest."""
import numpy as np

from oracle import eincm_oracle as O
import _event_scores_witness as ES

NT = ES.NT
MAX_MODELS = 8
FAR = 1e5            # px: a theta that drops every tap


# ---- (a) the rule in float32 ------------------------------------------------------------------------------------------------------------
def responsibilities_f32(s, q, w, pi, exclude_self):
    """s, q (K, n) float32; w (K, n) float32 or None (ones); pi (K,) numbers or None (ones).  Returns dict(weights (K, n) float32,
    labels (n,) uint8, unsupported (n,) bool, p (K, n) float32 before the fallback, a (K, n) float32 after the clamp)."""
    f = np.float32
    s, q = np.asarray(s, dtype=f), np.asarray(q, dtype=f)
    K, n = s.shape
    pi32 = np.ones(K, dtype=f) if pi is None else np.asarray(pi, dtype=np.float64).astype(f)
    with np.errstate(all='ignore'):
        if exclude_self:
            wq = q.copy() if w is None else np.multiply(np.asarray(w, dtype=f), q, dtype=f)
            a = np.subtract(s, wq, dtype=f)
        else:
            a = s.copy()
        a = np.where(a > f(0), a, f(0)).astype(f)                       # a NaN becomes +0, so does -0
        p = np.multiply(pi32[:, None], a, dtype=f)
        T = np.zeros(n, dtype=f)
        for l in range(K):
            T = np.add(T, p[l], dtype=f)
        uns = ~(T > f(0)) | ~np.isfinite(T)
        p_raw = p.copy()
        p = np.where(uns[None, :], np.broadcast_to(pi32[:, None], (K, n)), p).astype(f)
        T2 = np.zeros(n, dtype=f)
        for l in range(K):
            T2 = np.add(T2, p[l], dtype=f)
        T = np.where(uns, T2, T).astype(f)
        labels = np.zeros(n, dtype=np.uint8)
        best = p[0].copy()
        for l in range(1, K):
            up = p[l] > best
            best = np.where(up, p[l], best)
            labels[up] = l
        weights = np.divide(p, T[None, :], dtype=f)
    return dict(weights=weights, labels=labels, unsupported=uns, p=p_raw, a=a)


def ordered_mass(weights):
    """(K,) float64: sum_i w' of (K, n) float32 weights in the operator's order - per 256-event block a wave's 64 values by halving,
    the four waves in ascending order, then the blocks in ascending order from +0."""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    K, n = w.shape
    nb = (n + NT - 1) // NT
    pad = np.zeros((K, nb * NT))
    pad[:, :n] = w
    v = pad.reshape(K, nb, NT // 64, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    waves = v[..., 0]
    blocks = waves[..., 0]
    for j in range(1, NT // 64):
        blocks = blocks + waves[..., j]
    mass = np.zeros(K)
    for j in range(nb):
        mass = mass + blocks[:, j]
    return mass


# ---- (b) the rule in float64 on the score witness ----------------------------------------------------------------------------------------
def weighted_iwes(Theta, xs, ys, ts, edge_ts, shape, w=None):
    """(R,H,W) float64: the splat of the window under a sensor-size Theta with every tap scaled by its event's weight (the oracle's
    warp, rounding, index rule and tap weight, as _event_scores_witness.event_scores takes them)."""
    H, W = shape
    n = len(xs)
    wgt = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    out = []
    for tau in np.atleast_1d(edge_ts):
        wx, wy = O.per_pix_warp(np.asarray(Theta, dtype=np.float64), xs, ys, ts, tau, 1.0)
        rx, ry = O._round_i(wx), O._round_i(wy)
        img = np.zeros(H * W)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qx, qy = (rx + dx) - wx, (ry + dy) - wy
                k = wgt * np.exp(-0.5 * (qx * qx + qy * qy) - np.log(2.0 * np.pi))
                cs, vx = O._tap_index(rx, dx, W)
                rs, vy = O._tap_index(ry, dy, H)
                v = vx & vy
                np.add.at(img, rs[v] * W + cs[v], k[v])
        out.append(img.reshape(H, W))
    return np.stack(out)


def responsibilities_f64(F, Theta, events, edge_ts, omega, w, pi, exclude_self):
    """F (K,R,H,W), Theta (K,H,W,2), events: K (xs, ys, ts) triples of equal length, edge_ts (K,R), omega (R,), w: K arrays or Nones,
    pi (K,) or None.  Returns dict(weights (K,n) float64, a (K,n) before the clamp, M (K,n) the magnitude of a, unsupported)."""
    K = len(events)
    n = len(events[0][0])
    a, M = np.zeros((K, n)), np.zeros((K, n))
    for l, (xs, ys, ts) in enumerate(events):
        r = ES.event_scores(F[l], Theta[l], xs, ys, ts, edge_ts[l], omega)
        wl = np.ones(n) if w is None or w[l] is None else np.asarray(w[l], dtype=np.float64)
        a[l] = r['scores'] - wl * r['selfs'] if exclude_self else r['scores']
        M[l] = r['M'] + (wl * r['M_self'] if exclude_self else 0.0)
    pi64 = np.ones(K) if pi is None else np.asarray(pi, dtype=np.float64).astype(np.float32).astype(np.float64)
    p = pi64[:, None] * np.maximum(a, 0.0)
    T = p.sum(axis=0)
    uns = ~(T > 0)
    p = np.where(uns[None, :], pi64[:, None], p)
    return dict(weights=p / p.sum(axis=0)[None, :], a=a, M=M, unsupported=uns)


# ---- (d) the generated cases ------------------------------------------------------------------------------------------------------------
# name -> (sensor, theta grid or None for a dense theta, R, K, the groups' event counts, seed, the signed stack's lower bound).  One
# window per case, the last, is at theta = FAR.  The stack is uniform in [lo, 1): lo is chosen per case so that between 5 % and 50 % of
# the events are unsupported (no model with a positive score) - the more live models, the more negative the stack has to be.
GENERATED = {
    '60x80-dense-k2-g2': ((60, 80), None, 3, 2, [700, 65], 31, -0.9),
    '33x65-grid-k3': ((33, 65), (3, 5), 3, 3, [257], 32, -0.9),
    '60x80-dense-k8-r1': ((60, 80), None, 1, 8, [256], 33, -1.35),
    '60x80-dense-k1-g2': ((60, 80), None, 3, 1, [255, 64], 34, -0.5),
    '33x65-grid-k3-g3-empty-middle': ((33, 65), (3, 5), 3, 3, [63, 0, 1], 35, -0.95),
}
_cache = {}


def generated(name):
    """dict(shape, grid, R, K, G, ns, windows: B dicts (xs, ys, ts, edges, edge_ts, w float32 | None), theta (B,h,w,2), omega (R,),
    prior (B,), stack (B,R,H,W) float32), read-only, made once.  The windows of a group have equal counts and their OWN events."""
    if name not in _cache:
        shape, grid, R, K, ns, seed, lo = GENERATED[name]
        H, W = shape
        rng = np.random.default_rng(seed + 5000)
        wins, thetas = [], []
        for g, n in enumerate(ns):
            for l in range(K):
                xs, ys, ts, edges, edge_ts = ES.window(shape, n, R, seed * 100 + g * 10 + l) if n else (
                    np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0), rng.uniform(0, 1, (R, H, W)), np.linspace(0.0, 1.0, R) + 0.013)
                w = None
                if l % 2 == 0 and n:                     # every other model carries weights, some of them 0 and some 1
                    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
                    w[::5] = 0.0
                    w[1::7] = 1.0
                wins.append(dict(xs=xs, ys=ys, ts=ts, edges=edges, edge_ts=np.atleast_1d(edge_ts), w=w))
                thetas.append(rng.uniform(-9.0, 9.0, (grid or shape) + (2,)))
        thetas[-1] = np.full_like(thetas[-1], FAR)
        B = len(wins)
        prior = rng.uniform(0.2, 2.0, B)
        if K == 8:
            prior[3] = 0.0                               # a model the prior rules out
        c = dict(shape=shape, grid=grid, R=R, K=K, G=len(ns), ns=list(ns), windows=wins, theta=np.stack(thetas),
                 omega=np.linspace(0.5, 1.0, R) if R > 1 else np.array([0.75]), prior=prior,
                 stack=rng.uniform(lo, 1.0, (B, R, H, W)).astype(np.float32))
        for v in list(c.values()) + [a for w in wins for a in w.values()]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def witness_case(name, source, exclude_self, use_prior):
    """The float64 form of every group of a generated case, the IWEs from weighted_iwes: a list over the groups of
    responsibilities_f64's dicts (None for an empty group)."""
    c = generated(name)
    K, out = c['K'], []
    for g, n in enumerate(c['ns']):
        if n == 0:
            out.append(None)
            continue
        ws = c['windows'][g * K:(g + 1) * K]
        Th = np.stack([ES.sensor_theta(c['theta'][g * K + l], c['shape']) for l in range(K)])
        if source == 'iwe':
            F = np.stack([weighted_iwes(Th[l], w['xs'], w['ys'], w['ts'], w['edge_ts'], c['shape'], w['w']) for l, w in enumerate(ws)])
        else:
            F = c['stack'][g * K:(g + 1) * K]
        out.append(responsibilities_f64(F, Th, [(w['xs'], w['ys'], w['ts']) for w in ws], [w['edge_ts'] for w in ws], c['omega'],
                                        [w['w'] for w in ws], c['prior'][g * K:(g + 1) * K] if use_prior else None, exclude_self))
    return out


# ---- (c) the driver case and the EM loop in numpy ----------------------------------------------------------------------------------------
DRIVER = dict(shape=(64, 96), n_layer=3000, flows=((12.0, 3.0), (-6.0, -9.0)), R=2, alpha=1.0, beta=0.0, gamma=0.0, delta=0.0,
              start=(0.6, 1.4), n_iters=3, seeds=(1, 2))
# em_witness's label accuracy after the last iteration (prior='uniform'), recorded: tests/test_responsibilities_interface.py computes
# it again on the CPU and compares, tests/test_gpu_responsibilities.py holds the GPU driver to it
DRIVER_WITNESS_ACCURACY = 0.8973
_driver = {}


def driver_case(synth):
    """dict(window (xs, ys, ts, edges, edge_ts), truth (n,) the layer of every event, flows (2,2), coeffs0 (1,2,2)): two transparent
    layers of constant flow merged by time"""
    if not _driver:
        d = DRIVER
        H, W = d['shape']
        layers = [synth.make_window(seed, d['shape'], d['n_layer'], d['R'], flow=np.broadcast_to(np.array(v), (H, W, 2)).copy(),
                                    n_segments=8, n_circles=2, jitter_px=0.3, noise_frac=0) for seed, v in zip(d['seeds'], d['flows'])]
        ts = np.concatenate([l['ts'] for l in layers])
        order = np.argsort(ts, kind='stable')
        xs = np.concatenate([l['xs'] for l in layers])[order]
        ys = np.concatenate([l['ys'] for l in layers])[order]
        truth = np.concatenate([np.full(d['n_layer'], i, dtype=np.uint8) for i in range(2)])[order]
        edges = np.maximum(layers[0]['edges'], layers[1]['edges'])
        flows = np.array(d['flows'])
        _driver.update(window=(xs, ys, ts[order], edges, layers[0]['edge_ts']), truth=truth, flows=flows,
                       coeffs0=(flows * np.array(d['start'])[:, None])[None])
    return _driver


def accuracy(labels, truth):
    return float((np.asarray(labels) == np.asarray(truth)).mean())


def em_witness(case, omega, n_iters, maxiter=25, gtol=1e-6, prior='mass'):
    """segment_motions for translations in numpy: an E-step at coeffs0 on unit weights, then n_iters of (M-step, E-step).  Returns a
    list of dict(coeffs (2,2), labels, weights (2,n), mass (2,), n_unsupported)."""
    from scipy.optimize import minimize
    import _event_weights_witness as WW
    d = DRIVER
    xs, ys, ts, edges, edge_ts = case['window']
    H, W = d['shape']
    AH, AW = np.ones((H, 1)), np.ones((W, 1))
    K = 2
    c = case['coeffs0'][0].copy()

    def fun(v, w):
        val, grad, _, _, _ = WW.loss_and_grad(v.reshape(1, 1, 2), xs, ys, ts, edges, edge_ts, d['alpha'], d['beta'], d['gamma'], d['delta'], 1,
                                              AH, AW, weights=w)
        return val, grad.reshape(2)

    def e_step(c, w, pi):
        s, q = np.zeros((K, len(xs)), np.float32), np.zeros((K, len(xs)), np.float32)
        for l in range(K):
            Th = np.broadcast_to(c[l], (H, W, 2))
            F = weighted_iwes(Th, xs, ys, ts, edge_ts, d['shape'], None if w is None else w[l].astype(np.float64))
            r = ES.event_scores(F, Th, xs, ys, ts, edge_ts, omega)
            s[l], q[l] = r['scores'], r['selfs']
        r = responsibilities_f32(s, q, w, pi, True)
        mass = ordered_mass(r['weights'])
        return r, mass, (None if prior == 'uniform' else mass / mass.sum())

    r, mass, pi = e_step(c, None, None)
    out = []
    for _ in range(n_iters):
        w = r['weights']
        for l in range(K):
            c[l] = minimize(fun, c[l], args=(w[l],), jac=True, method='BFGS', options=dict(maxiter=maxiter, gtol=gtol)).x
        r, mass, pi = e_step(c, w, pi)
        out.append(dict(coeffs=c.copy(), labels=r['labels'], weights=r['weights'], mass=mass, n_unsupported=int(r['unsupported'].sum())))
    return out
