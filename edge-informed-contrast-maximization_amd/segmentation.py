"""Segment a window's events into several motions by expectation-maximisation.

K motion models on one event list are K windows of a batch that share the events and carry complementary per-event weights
(section 22).  The M-step solves every model on its weighted events (batch_solver.minimize_motion, section 20); the E-step scores every
event under every model, leave-one-out against that model's image of warped events, and normalises over the models
(Engine.event_responsibilities, one device operation).  segment_motions stages the batch again with the new weights in every
iteration; segment_motions_in_place stages it once with keep_order=True and lets every E-step write its result
straight into the staged layouts (Engine.apply_responsibilities).  The two return the same bytes.

The EM is local and needs starting coefficients.  seed_motions finds them without a gradient: a coarse-to-fine
grid search on the contrast landscape (Engine.contrast_landscape), one motion after the other, each on the events that the motions
found before it do not explain.

What the EM ends in - K coefficient vectors and one weight per event and model - becomes one flow field and a label image through
segmented_flow (Engine.compose_motions): the form that flow_errors, advect_theta and a submission take.

segment_motions_spatial runs the same loop with a spatially coherent E-step: the staged weights become a
per-pixel label prior on the device (Engine.label_prior) and every event's mixing weights are read at its own pixel.

segment_sequence segments consecutive windows one after the other and hands the segmentation itself on: after
every window the staged weights become a label prior carried along each model's own motion (Engine.carry_label_prior), and the next
window's first E-step reads it (Engine.adopt_carried_prior) instead of a prior formed from unit weights."""
import numpy as np

from . import _lib as L
from . import batch_solver as bsol
from . import motion
from .engine import check_label_prior_args

PRIORS = ('mass', 'uniform')
FIRST_PRIORS = (None, 'carried')


def check_first_prior(first_prior, weights0, spatial=True):
    """first_prior of segment_motions_spatial_primed, checked without a GPU: None or 'carried'; 'carried' replaces the prior of the
    first E-step, the one on unit weights, so it raises together with weights0 (there is no such E-step then) and outside the spatial
    EM."""
    if first_prior not in FIRST_PRIORS:
        raise ValueError(f'first_prior {first_prior!r} not supported; one of {FIRST_PRIORS}')
    if first_prior is not None and not spatial:
        raise ValueError("first_prior='carried' goes with the spatial E-step only (segment_motions_spatial_primed)")
    if first_prior is not None and weights0 is not None:
        raise ValueError("first_prior='carried' together with weights0: there is no first E-step on unit weights to use the carried prior")
    return first_prior


def check_segment_args(windows, model, coeffs0, n_iters, weights0, prior, min_mass, in_place=False, record_weights=True):
    """The arguments of segment_motions and segment_motions_in_place, checked without a GPU.  Returns (coeffs0 (G,K,n_coeffs) float64,
    weights0 as G lists of K float32 arrays or None)."""
    if not isinstance(in_place, (bool, np.bool_)) or not isinstance(record_weights, (bool, np.bool_)):
        raise ValueError(f'in_place and record_weights must be True or False, got {in_place!r} and {record_weights!r}')
    if not in_place and not record_weights:
        raise ValueError('record_weights=False goes with in_place=True: the restaging route holds the weights on the host anyway')
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
    return _segment(engine, windows, model, coeffs0, params, n_iters, maxiter, gtol, weights0, prior, min_mass, callback, False, True)


def segment_motions_in_place(engine, windows, model, coeffs0, params, n_iters=5, maxiter=25, gtol=1e-6, weights0=None, prior='mass',
                             min_mass=1.0, callback=None, record_weights=True):
    """segment_motions with in_place=True: the G*K windows are staged once with keep_order=True, weights0 goes in
    through Engine.set_weights, and every E-step applies its own result on the device (Engine.apply_responsibilities) - no per-event
    download, no restaging.  The history is byte-equal to segment_motions' in 'coeffs', 'weights', 'labels', 'mass', 'n_unsupported' and
    'active': the engine is bit-reproducible and the staged layouts are the same.  A record's 'weights' are fetched by
    Engine.staged_weights(); record_weights=False leaves them out (None), and nothing per-event crosses to the host but the labels."""
    return _segment(engine, windows, model, coeffs0, params, n_iters, maxiter, gtol, weights0, prior, min_mass, callback, True, record_weights)


def segment_motions_spatial(engine, windows, model, coeffs0, params, radius=2, floor_mass=4096, n_iters=5, maxiter=25, gtol=1e-6,
                            weights0=None, prior='mass', min_mass=1.0, callback=None, in_place=True, record_weights=True):
    """segment_motions with a spatially coherent E-step: after every staging, and before every E-step of the
    in-place route, Engine.label_prior(K, radius, floor_mass) turns the staged weights - the ones the E-step is about to replace - into
    a per-pixel prior that stays on the device, and the E-step is Engine.event_responsibilities_spatial (in_place:
    apply_responsibilities_spatial) on that staged prior: model l's mixing weight for an event is its ``prior`` share times its share
    of the mass around the event's pixel.  radius: 0 .. 8, the half-width of the box; floor_mass: what every model's box sum is
    raised by (4096 is one event of weight 1).  in_place and record_weights as segment_motions_in_place takes them; the two routes
    return the same bytes.  Everything else, and the history returned, is segment_motions'."""
    return _segment(engine, windows, model, coeffs0, params, n_iters, maxiter, gtol, weights0, prior, min_mass, callback, in_place, record_weights,
                    spatial=(radius, floor_mass))


def segment_motions_spatial_primed(engine, windows, model, coeffs0, params, radius=2, floor_mass=4096, n_iters=5, maxiter=25, gtol=1e-6,
                                   weights0=None, prior='mass', min_mass=1.0, callback=None, in_place=True, record_weights=True,
                                   first_prior=None):
    """segment_motions_spatial with one keyword more (its own signature is pinned by tests/test_label_prior_interface.py, so the keyword
    lives here).  first_prior: None, or 'carried' (DESIGN.md section 33): the label_prior call after the FIRST staging - the one that
    precedes the E-step at coeffs0 and would form its prior from unit weights, which tells an event nothing - is replaced by
    Engine.adopt_carried_prior(K): that E-step reads the prior a previous window's Engine.carry_label_prior left on the device.  Every
    later staging and iteration is unchanged, and with None the function returns segment_motions_spatial's bytes.  'carried' together
    with weights0 raises: there is no such first E-step then."""
    return _segment(engine, windows, model, coeffs0, params, n_iters, maxiter, gtol, weights0, prior, min_mass, callback, in_place, record_weights,
                    spatial=(radius, floor_mass), first_prior=first_prior)


def _segment(engine, windows, model, coeffs0, params, n_iters, maxiter, gtol, weights0, prior, min_mass, callback, in_place, record_weights,
             spatial=None, first_prior=None):
    """spatial: None, or (radius, floor_mass): the label prior is formed after every staging and the E-step reads it.  first_prior:
    None, or 'carried': after the first staging the engine's carried prior is adopted instead."""
    c, weights = check_segment_args(windows, model, coeffs0, n_iters, weights0, prior, min_mass, in_place, record_weights)
    check_first_prior(first_prior, weights0, spatial is not None)
    if spatial is not None:
        check_label_prior_args(c.shape[1], spatial[0], spatial[1], ())
    G, K = c.shape[:2]
    want = ('weights', 'labels', 'mass', 'n_unsupported')
    engine.set_motion_model(model)
    engine.set_motion_path('expanded')
    staged_once = []
    adopt = [first_prior == 'carried']      # (true until the first staging has taken the carried prior)

    def stage(wts):
        if not in_place:
            engine.set_windows([tuple(windows[g]) + (None if wts is None else wts[g][l],) for g in range(G) for l in range(K)])
        elif not staged_once:           # the one staging: the windows as they are; the weights go in like every later set
            engine.set_windows([tuple(windows[g]) for g in range(G) for l in range(K)], keep_order=True)
            staged_once.append(True)
            if wts is not None:
                engine.set_weights([wts[g][l] for g in range(G) for l in range(K)])
        elif wts is not None:           # (None: the E-step has applied its own result)
            engine.set_weights([wts[g][l] for g in range(G) for l in range(K)])
        if spatial is not None and adopt[0]:       # the first E-step of a window that follows another: the previous window's labels, carried
            adopt[0] = False
            engine.adopt_carried_prior(K)
        elif spatial is not None:       # the prior of the next E-step, from the weights it will replace; it stays on the device
            engine.label_prior(K, spatial[0], spatial[1], want=())

    def e_step(coeffs, pi):
        engine.loss_grad_motion(coeffs.reshape(G * K, -1), params, want_grad=False, allow_nonfinite=True)
        if not in_place:
            respond = engine.event_responsibilities if spatial is None else engine.event_responsibilities_spatial     # (on the staged prior)
            r = respond(K, prior=pi, exclude_self=True, want=want)
            return [[np.array(r['weights'][g * K + l]) for l in range(K)] for g in range(G)], r
        respond = engine.apply_responsibilities if spatial is None else engine.apply_responsibilities_spatial
        r = respond(K, prior=pi, exclude_self=True, want=want[1:])
        return None, r

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
        recorded = weights              # (in place: None, the weights are the device's and the next stage() has nothing to hand over)
        if in_place and record_weights:
            w = engine.staged_weights()
            recorded = [[np.array(w[g * K + l]) for l in range(K)] for g in range(G)]
        record = dict(coeffs=c.copy(), weights=recorded, labels=[np.array(a) for a in r['labels']], mass=r['mass'].copy(),
                      n_unsupported=r['n_unsupported'].copy(), results=[results[g * K:(g + 1) * K] for g in range(G)], active=active.copy())
        history.append(record)
        if callback is not None:
            callback(it, record)
        active = active & (r['mass'] >= min_mass)
    return history


# ---- consecutive windows: the segmentation handed on ------------------------------------------------------------------
def check_sequence_args(windows_seq, coeffs0, tau, em):
    """The arguments of segment_sequence that are its own, checked without a GPU (every step's are checked by check_segment_args when
    it runs).  Returns tau as float64, a number or (G,)."""
    if len(windows_seq) < 1 or any(len(w) != len(windows_seq[0]) or len(w) < 1 for w in windows_seq):
        raise ValueError('windows_seq must hold at least one step, every step the same number G >= 1 of (xs, ys, ts, edges, edge_ts) tuples')
    for name in ('weights0', 'first_prior', 'in_place'):
        if name in em and not (name == 'in_place' and em[name] is True):
            raise ValueError(f'{name} is the sequence\'s own: every step after the first starts from the carried prior, on the batch staged once')
    t = np.asarray(tau, dtype=np.float64)
    if t.shape not in ((), (len(windows_seq[0]),)) or not np.isfinite(t).all():
        raise ValueError(f'tau must be a finite number or ({len(windows_seq[0])},) of them, got {tau!r}')
    return t


def segment_sequence(engine, windows_seq, model, coeffs0, params, tau=1.0, radius=2, floor_mass=4096, **em):
    """segment_motions_spatial over T consecutive steps, the segmentation handed from each to the next.
    windows_seq: T lists of the same G (xs, ys, ts, edges, edge_ts) tuples; coeffs0 (G, K, n_coeffs) starts step 0; radius and
    floor_mass are the label prior's, of the EM and of the carry alike; **em goes to every step (n_iters, maxiter, gtol, prior,
    min_mass, callback, record_weights).  Step 0 is segment_motions_spatial from coeffs0.  After every step but the last,
    Engine.carry_label_prior(K, last coeffs, tau, radius, floor_mass, want=()) runs on the batch that is still staged with the step's
    final weights (the in-place route), and the next step is segment_motions_spatial_primed(coeffs0=last coeffs, first_prior='carried').

    tau: how far the labels move along each model's field between two windows, in the field's own time unit: 1.0 moves them by one
    window's displacement, right for windows that follow each other without a gap.  The coefficients are handed over as they are, as
    the reference hands theta over in place: rescaling them (and tau) for windows of unequal duration is the caller's job.

    Returns the T histories."""
    t = check_sequence_args(windows_seq, coeffs0, tau, em)
    em = {k: v for k, v in em.items() if k != 'in_place'}
    histories, c = [], np.asarray(coeffs0, dtype=np.float64)
    for step, windows in enumerate(windows_seq):
        h = segment_motions_spatial_primed(engine, windows, model, c, params, radius=radius, floor_mass=floor_mass, in_place=True,
                                           first_prior=None if step == 0 else 'carried', **em)
        histories.append(h)
        c = h[-1]['coeffs']
        if step + 1 < len(windows_seq):
            G, K = c.shape[:2]
            engine.carry_label_prior(K, c.reshape(G * K, -1), t, radius, floor_mass, want=())
    return histories


# ---- the segmentation as one flow field and a label image ---------------------------------------------------------
def check_segmented_flow_args(windows, model, record):
    """The arguments of segmented_flow, checked without a GPU.  Returns (coeffs (G, K, n_coeffs) float64, weights as G lists of K
    float32 arrays)."""
    G = len(windows)
    if G < 1:
        raise ValueError('windows must hold at least one (xs, ys, ts, edges, edge_ts) tuple')
    for g, w in enumerate(windows):
        if len(w) != 5:
            raise ValueError(f'window {g}: a (xs, ys, ts, edges, edge_ts) tuple, got {len(w)} elements (the weights are the record\'s)')
    if not isinstance(record, dict) or 'coeffs' not in record or 'weights' not in record:
        raise ValueError("record must be a history record of segment_motions: a dict with 'coeffs' and 'weights'")
    c = np.asarray(record['coeffs'], dtype=np.float64)
    if c.ndim != 3 or c.shape[0] != G or c.shape[1] < 1 or c.shape[2] != model.n_coeffs:
        raise ValueError(f"record['coeffs'] must be ({G}, K, {model.n_coeffs}), got {c.shape}")
    K = c.shape[1]
    weights = record['weights']
    if weights is None:
        raise ValueError("record['weights'] is None (segment_motions_in_place with record_weights=False): the engine still holds the "
                         "weights, call engine.compose_motions")
    if len(weights) != G or any(len(wg) != K for wg in weights):
        raise ValueError(f"record['weights'] must be {G} lists of {K} weight arrays")
    weights = [[np.ascontiguousarray(w, dtype=np.float32) for w in wg] for wg in weights]
    for g, wg in enumerate(weights):
        n = len(windows[g][0])
        if any(w.shape != (n,) for w in wg):
            raise ValueError(f"window {g}: every array of record['weights'] must be ({n},)")
    return c, weights


def segmented_flow(engine, windows, model, record, mode='hard', fill='dominant'):
    """The flow field and the label image of a segmentation (Engine.compose_motions).  windows: the G
    (xs, ys, ts, edges, edge_ts) tuples that were segmented; record: one record of segment_motions' history (its 'coeffs' (G, K,
    n_coeffs) and 'weights').  Stages the G*K windows with the record's weights, sets the model and returns compose_motions' dict
    with all four outputs: 'theta' (G, H, W, 2) is what flow_errors, advect_theta, a dense loss_grad and
    evaluation.dsec_submission_flow take.

    After segment_motions_in_place the engine already holds the final weights in its staged layouts, so
    ``engine.compose_motions(K, record['coeffs'].reshape(G * K, -1))`` gives the last record's result with no staging at all."""
    c, weights = check_segmented_flow_args(windows, model, record)
    G, K = c.shape[:2]
    engine.set_motion_model(model)
    engine.set_windows([tuple(windows[g]) + (weights[g][l],) for g in range(G) for l in range(K)])
    return engine.compose_motions(K, c.reshape(G * K, -1), mode=mode, fill=fill, want=('theta', 'labels', 'mass', 'total'))


def segmented_flow_dense(engine, windows, model, record, mode='hard', fallback='dominant', min_site_mass=1, max_distance=None):
    """segmented_flow with the pixels that hold no event filled from the nearest one that does (Engine.densify_motions, DESIGN.md
    section 31).  windows, model and record as segmented_flow takes them.  Stages the G*K windows with the record's weights, sets the
    model and returns densify_motions' dict with all five outputs: 'theta' (G, H, W, 2) is dense, so the inside of an object takes
    the object's motion and not the background's.

    After segment_motions_in_place the engine already holds the final weights in its staged layouts, so a bare
    ``engine.densify_motions(K, record['coeffs'].reshape(G * K, -1))`` gives the last record's result with no staging at all."""
    c, weights = check_segmented_flow_args(windows, model, record)
    G, K = c.shape[:2]
    engine.set_motion_model(model)
    engine.set_windows([tuple(windows[g]) + (weights[g][l],) for g in range(G) for l in range(K)])
    return engine.densify_motions(K, c.reshape(G * K, -1), mode=mode, fallback=fallback, min_site_mass=min_site_mass,
                                  max_distance=max_distance, want=('theta', 'labels', 'dist2', 'nearest', 'n_sites'))


# ---- seeds for the models: a peeling search on the contrast landscape -------------------------------------------
def landscape_cell(step):
    """The cell size a grid of this step is evaluated at: the smallest of CL_CELLS that is >= the step, 8 beyond."""
    for cell in L.CL_CELLS:
        if cell >= step:
            return cell
    return L.CL_CELLS[-1]


def peel_explained(model, coeffs, xs, ys, ts, t_ref, keep, peel_min_count):
    """The events of one window that the motion ``coeffs`` explains: kept, inside the sensor after the warp, and sharing their pixel of
    the count image of the kept in-sensor events with at least peel_min_count others.  (n,) bool."""
    H, W = model.sensor_size
    rx, ry, inside = motion.warped_pixels(model, coeffs, xs, ys, ts, t_ref)
    part = inside & keep
    pix = ry[part].astype(np.int64) * W + rx[part].astype(np.int64)
    count = np.bincount(pix, minlength=H * W)
    explained = np.zeros(len(keep), dtype=bool)
    explained[part] = count[pix] - 1 >= peel_min_count
    return explained


def check_seed_args(windows, model, n_models, span, axes, base, n, refine_levels, refine_n, t_ref, peel_min_count, min_events):
    """The arguments of seed_motions, checked without a GPU.  Returns (base (G, K) float64, span (len(axes),) float64, t_ref (G,))."""
    G, K = len(windows), model.n_coeffs
    if G < 1:
        raise ValueError('windows must hold at least one (xs, ys, ts, edges, edge_ts) tuple')
    for g, w in enumerate(windows):
        if len(w) != 5:
            raise ValueError(f'window {g}: a (xs, ys, ts, edges, edge_ts) tuple, got {len(w)} elements (the landscape ignores weights)')
    if isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer)) or n_models < 1:
        raise ValueError(f'n_models must be a positive integer, got {n_models!r}')
    b = np.zeros((G, K)) if base is None else np.asarray(base, dtype=np.float64)
    if b.shape == (K,):
        b = np.broadcast_to(b, (G, K))
    if b.shape != (G, K) or not np.isfinite(b).all():
        raise ValueError(f'base must be ({K},) or ({G}, {K}) finite numbers, got {np.shape(base)}')
    for name, v, lo in (('refine_levels', refine_levels, 0), ('peel_min_count', peel_min_count, 0), ('min_events', min_events, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f'{name} must be an integer >= {lo}, got {v!r}')
    motion.coefficient_grid(model, b[0], axes, span, n)                                # (raises for bad axes, span and n)
    motion.coefficient_grid(model, b[0], axes, 1.0, refine_n)
    n_axes = len(np.atleast_1d(np.asarray(axes)))
    t = np.asarray(t_ref, dtype=np.float64)
    if t.shape not in ((), (G,)) or not np.isfinite(t).all():
        raise ValueError(f't_ref must be a finite number or ({G},) of them, got {t_ref!r}')
    return np.array(b), np.array(np.broadcast_to(np.asarray(span, dtype=np.float64), (n_axes,))), np.array(np.broadcast_to(t, (G,)))


def seed_motions(engine, windows, model, n_models, span, axes=(0, 1), base=None, n=17, refine_levels=2, refine_n=9, t_ref=0.5,
                 peel_min_count=2, min_events=16, landscape=None):
    """Starting coefficients for segment_motions, found without a gradient: per window, n_models motions one after the other, each the
    best candidate of a coarse-to-fine grid search on the contrast landscape (Engine.contrast_landscape: the integer sum of squared
    cell counts of the warped events) over the events that the motions found before it do not explain.

    windows: G (xs, ys, ts, edges, edge_ts) tuples.  model: a motion.MotionModel.  The grids run over the coefficient indices ``axes``
    (1 to 3), the other coefficients stay at ``base`` ((K,) or (G, K), zeros by default).  Level 0 is coefficient_grid(base, axes, span,
    n); each of the refine_levels that follow is centred on the level's winner (the largest sumsq, the lowest index on a tie) with the
    previous level's step as its half-range and refine_n values per axis.  A level is evaluated at landscape_cell(its largest step).
    All windows' candidates of a level go into one call, cut into pieces of at most CL_MAX_CANDIDATES.  After a motion is found, the
    events it explains (peel_explained) leave the window's ``keep``; when fewer than min_events remain the window stops, its remaining
    rows NaN.

    landscape: the callable (coeffs (G, V, K), t_ref (G,), cell, keep: G bool arrays) -> sumsq (G, V) that evaluates candidates; None
    stages the windows on ``engine``, sets the model and takes the engine's operator.  With a callable the engine is not touched.

    Returns a dict: 'coeffs0' (G, n_models, K) float64; 'sumsq' (G, n_models) uint64, each winner's sumsq at the last level's cell;
    'n_kept' (G, n_models) int64, the events that took part in each search; 'n_found' (G,) int64, the valid rows."""
    base, span, t_ref = check_seed_args(windows, model, n_models, span, axes, base, n, refine_levels, refine_n, t_ref, peel_min_count,
                                        min_events)
    G, K, M = len(windows), model.n_coeffs, int(n_models)
    if landscape is None:
        engine.set_windows([tuple(w) for w in windows])
        engine.set_motion_model(model)

        def landscape(coeffs, t_ref, cell, keep):
            return engine.contrast_landscape(coeffs, t_ref=t_ref, cell=cell, keep=keep, want='sumsq')['sumsq']

    def best(cands, cell, keep):
        """(winner index (G,), its sumsq (G,)) over the (G, V, K) candidates"""
        V = cands.shape[1]
        s = np.concatenate([np.asarray(landscape(np.ascontiguousarray(cands[:, v:v + L.CL_MAX_CANDIDATES]), t_ref, cell, keep))
                            for v in range(0, V, L.CL_MAX_CANDIDATES)], axis=1)
        j = np.argmax(s, axis=1)                                                       # (the first of equal maxima: the lowest index)
        return j, s[np.arange(G), j]

    keep = [np.ones(len(w[0]), dtype=bool) for w in windows]
    out = dict(coeffs0=np.full((G, M, K), np.nan), sumsq=np.zeros((G, M), dtype=np.uint64), n_kept=np.zeros((G, M), dtype=np.int64),
               n_found=np.zeros(G, dtype=np.int64))
    live = np.ones(G, dtype=bool)
    for m in range(M):
        live &= np.array([int(k.sum()) >= min_events for k in keep])
        if not live.any():
            break
        centre, half, count = base.copy(), span, int(n)
        for level in range(1 + int(refine_levels)):
            step = 2.0 * half / (count - 1)
            cands = np.stack([motion.coefficient_grid(model, centre[g], axes, half, count) for g in range(G)])
            j, s = best(cands, landscape_cell(float(step.max())), keep)
            centre = cands[np.arange(G), j]
            half, count = step, int(refine_n)
        for g in np.flatnonzero(live):
            out['coeffs0'][g, m], out['sumsq'][g, m], out['n_kept'][g, m] = centre[g], s[g], int(keep[g].sum())
            out['n_found'][g] = m + 1
            xs, ys, ts = windows[g][:3]
            keep[g] = keep[g] & ~peel_explained(model, centre[g], xs, ys, ts, t_ref[g], keep[g], int(peel_min_count))
    return out
