"""Segment a window's events into several motions by expectation-maximisation.

K motion models on one event list are K windows of a batch that share the events and carry complementary per-event weights
(section 22).  The M-step solves every model on its weighted events (batch_solver.minimize_motion, section 20); the E-step scores every
event under every model, leave-one-out against that model's image of warped events, and normalises over the models
(Engine.event_responsibilities, one device operation).  Staging keeps no index back to the caller's order, so every iteration stages
the batch again with the new weights."""
import numpy as np

from . import batch_solver as bsol

PRIORS = ('mass', 'uniform')


def check_segment_args(windows, model, coeffs0, n_iters, weights0, prior, min_mass):
    """The arguments of segment_motions, checked without a GPU.  Returns (coeffs0 (G,K,n_coeffs) float64, weights0 as G lists of K
    float32 arrays or None)."""
    G = len(windows)
    if G < 1:
        raise ValueError('windows must hold at least one (xs, ys, ts, edges, edge_ts) tuple')
    for g, w in enumerate(windows):
        if len(w) != 5:
            raise ValueError(f'window {g}: a (xs, ys, ts, edges, edge_ts) tuple, got {len(w)} elements (the weights are the segmentation\'s own)')
    c = np.asarray(coeffs0, dtype=np.float64)
    if c.ndim != 3 or c.shape[0] != G or c.shape[1] < 1 or c.shape[2] != model.n_coeffs:
        raise ValueError(f'coeffs0 must be ({G}, K, {model.n_coeffs}), got {c.shape}')
    if not np.isfinite(c).all():
        raise ValueError('coeffs0 must be finite')
    K = c.shape[1]
    for g in range(G):
        for a in range(K):
            for b in range(a + 1, K):
                if np.array_equal(c[g, a], c[g, b]):
                    raise ValueError(f'window {g}: models {a} and {b} start from equal coefficients and can never separate')
    if isinstance(n_iters, bool) or not isinstance(n_iters, (int, np.integer)) or n_iters < 1:
        raise ValueError(f'n_iters must be a positive integer, got {n_iters!r}')
    if prior not in PRIORS:
        raise ValueError(f'prior {prior!r} not supported; one of {PRIORS}')
    if not (np.isfinite(min_mass) and min_mass >= 0):
        raise ValueError(f'min_mass must be finite and >= 0, got {min_mass!r}')
    if weights0 is not None:
        if len(weights0) != G or any(len(wg) != K for wg in weights0):
            raise ValueError(f'weights0 must be {G} lists of {K} weight arrays')
        weights0 = [[np.ascontiguousarray(w, dtype=np.float32) for w in wg] for wg in weights0]
        for g, wg in enumerate(weights0):
            n = len(windows[g][0])
            if any(w.shape != (n,) for w in wg):
                raise ValueError(f'window {g}: every weights0 array must be ({n},)')
    return c, weights0


def segment_motions(engine, windows, model, coeffs0, params, n_iters=5, maxiter=25, gtol=1e-6, weights0=None, prior='mass',
                    min_mass=1.0, callback=None):
    """EM segmentation of G windows into K motions each.  windows: G (xs, ys, ts, edges, edge_ts) tuples.  model: a
    motion.MotionModel.  coeffs0: (G, K, n_coeffs), the models' starting coefficients; rows equal within a window raise.  params: the
    loss parameters of every M-step (engine.make_params).  weights0: G lists of K per-event weight arrays in [0, 1], or None: an
    E-step at coeffs0 on unit weights comes first.  prior: 'mass' takes every model's share of the previous E-step's mass as its
    mixing weight, 'uniform' leaves them equal.  min_mass: a model whose mass (its sum of weights) falls below this is frozen: left
    out of the later M-steps through ``active``, still staged and still evaluated, so it can still claim events.  callback(it, record)
    is called after every iteration.  The engine's motion path is set to 'expanded' (weights refuse 'fused').

    Each iteration stages the G*K weighted windows, solves the active models (maxiter, gtol), evaluates every window once at the
    solved coefficients so that every IWE is current, and takes the responsibilities as the next weights.  Returns a list of n_iters
    dicts: 'coeffs' (G,K,n_coeffs), 'weights' (G lists of K float32 arrays), 'labels' (G uint8 arrays), 'mass' (G,K),
    'n_unsupported' (G,), 'results' (G lists of K OptimizeResult, None for a frozen model), 'active' (G,K) bool."""
    c, weights = check_segment_args(windows, model, coeffs0, n_iters, weights0, prior, min_mass)
    G, K = c.shape[:2]
    want = ('weights', 'labels', 'mass', 'n_unsupported')
    engine.set_motion_model(model)
    engine.set_motion_path('expanded')

    def stage(wts):
        engine.set_windows([tuple(windows[g]) + (None if wts is None else wts[g][l],) for g in range(G) for l in range(K)])

    def e_step(coeffs, pi):
        engine.loss_grad_motion(coeffs.reshape(G * K, -1), params, want_grad=False, allow_nonfinite=True)
        r = engine.event_responsibilities(K, prior=pi, exclude_self=True, want=want)
        return [[np.array(r['weights'][g * K + l]) for l in range(K)] for g in range(G)], r

    def mixing(mass):
        if prior == 'uniform':
            return None
        share = mass / np.maximum(mass.sum(axis=1, keepdims=True), np.finfo(np.float64).tiny)
        return np.where(mass.sum(axis=1, keepdims=True) > 0, share, 1.0 / K).reshape(-1)

    pi = None
    active = np.ones((G, K), dtype=bool)
    if weights is None:
        stage(None)
        weights, r = e_step(c, None)
        pi = mixing(r['mass'])
        active &= r['mass'] >= min_mass
    history = []
    for it in range(int(n_iters)):
        stage(weights)
        results = [None] * (G * K)
        if active.any():
            results = bsol.minimize_motion(engine, model, c.reshape(G * K, -1), params, maxiter, gtol, active=active.reshape(-1))
        c = np.stack([c.reshape(G * K, -1)[b] if results[b] is None else np.asarray(results[b].x, dtype=np.float64)
                      for b in range(G * K)]).reshape(G, K, -1)
        weights, r = e_step(c, pi)
        pi = mixing(r['mass'])
        record = dict(coeffs=c.copy(), weights=weights, labels=[np.array(a) for a in r['labels']], mass=r['mass'].copy(),
                      n_unsupported=r['n_unsupported'].copy(), results=[results[g * K:(g + 1) * K] for g in range(G)], active=active.copy())
        history.append(record)
        if callback is not None:
            callback(it, record)
        active = active & (r['mass'] >= min_mass)
    return history
