"""eincm_densify_motions on the GPU: a motion segmentation composed into a dense flow field and label image,
every pixel taking the label of its nearest labelled pixel.

Every comparison is byte equality of all pixels of all five outputs with tests/_motion_fill_witness.py, whose nearest site is a brute
force over all sites with the key (d2, y', x'); there is no tolerance.  The sensors are small on purpose: 45 x 70 has both sides off
the 32-pixel tile and W off the 64-lane wave, so a row spans two waves with a ragged tail; 33 x 130 has three waves per row and two
tile rows; one case runs at 256 x 336, where a row is longer than the row kernel's workgroup.  Every test runs under its own time
limit."""
import importlib
import signal

import numpy as np
import pytest

import _motion_fill_witness as WIT
import _motion_layers_witness as MLW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
motion = importlib.import_module(pkg + '.motion')
segmentation = importlib.import_module(pkg + '.segmentation')

TIME_LIMIT_S = 60
ALL = ('theta', 'labels', 'dist2', 'nearest', 'n_sites')
COMBOS = [('hard', 'zero'), ('hard', 'dominant'), ('soft', 'zero'), ('soft', 'dominant')]
NONE = 0xFFFFFFFF
_engines, _models = {}, {}


def _model(shape):
    if shape not in _models:
        _models[shape] = motion.MotionModel('affine', shape)
    return _models[shape]


def _new_engine(shape, precision='fp32'):
    return E.Engine(shape, max_events_total=60000, max_refs=1, max_windows=16, precision=precision)


def _eng(shape):
    if shape not in _engines:
        _engines[shape] = _new_engine(shape)
    _engines[shape].set_motion_model(_model(shape))
    return _engines[shape]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f'test exceeded {TIME_LIMIT_S} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TIME_LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


# ---- the cases ----
def _coeffs(seed, n):
    return np.random.default_rng(seed).standard_normal((n, 6)) * np.array([6.0, 6.0, 3.0, 3.0, 3.0, 3.0])


def _window(shape, xs, ys, seed=0):
    """(xs, ys, ts, edges, edge_ts) of the events at these pixels"""
    rng = np.random.default_rng(seed)
    n = len(xs)
    return (np.asarray(xs, dtype=np.int16), np.asarray(ys, dtype=np.int16), np.sort(rng.random(n)), np.ones((1,) + shape), np.array([0.5]))


def _random_group(shape, seed, K, frac=0.03):
    """One group with events on about frac of the pixels, one to three per pixel, and K random weight arrays with exact zeros, ones and
    values that quantise to 0 among them."""
    H, W = shape
    rng = np.random.default_rng(seed)
    pix = rng.choice(H * W, max(1, int(frac * H * W)), replace=False)
    pix = np.repeat(pix, rng.integers(1, 4, len(pix)))
    pix = pix[rng.permutation(len(pix))]
    ws = []
    for _ in range(K):
        w = rng.random(len(pix), dtype=np.float32)
        kind = rng.integers(0, 6, len(pix))
        ws.append(np.where(kind == 0, np.float32(0), np.where(kind == 1, np.float32(1), np.where(kind == 2, np.float32(1e-5), w))).astype(np.float32))
    return _window(shape, pix % W, pix // W, seed), ws


def _pixels_group(shape, sites, K=2):
    """One group with one event on every (x, y) of sites; site i belongs to model i % K alone (one-hot weights), so neighbouring cells
    differ in their label."""
    xs, ys = [s[0] for s in sites], [s[1] for s in sites]
    own = np.arange(len(sites)) % K
    return _window(shape, xs, ys), [(own == l).astype(np.float32) for l in range(K)]


def _stage(eng, groups):
    """groups: (window, [K weight arrays]) each"""
    eng.set_windows([win + (w,) for win, ws in groups for w in ws])


def _wit_groups(groups):
    return [(win[0], win[1], ws) for win, ws in groups]


def _same(got, want, what):
    for name in got:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        assert got[name].tobytes() == want[name].tobytes(), (what, name, int((got[name] != want[name]).sum()))


def _check_combos(eng, shape, groups, coeffs, what, min_site_mass=1, max_dist2=None, combos=COMBOS):
    """All five outputs against the witness for every mode and fallback; returns the last pair (got, want)."""
    K = len(groups[0][1])
    cache = {}
    for mode, fallback in combos:
        got = eng.densify_motions(K, coeffs, mode=mode, fallback=fallback, min_site_mass=min_site_mass,
                                  max_distance=None if max_dist2 is None else np.sqrt(max_dist2 + 0.5), want=ALL)   # (floor(d^2) = max_dist2)
        want = WIT.densify(_model(shape), _wit_groups(groups), coeffs, mode, fallback, min_site_mass,
                           WIT.MD_UNBOUNDED if max_dist2 is None else max_dist2, transforms=cache)
        assert tuple(got) == ALL
        _same(got, want, (what, mode, fallback))
    return got, want


# ---- 1. random events on about 3 % of the pixels ----
@pytest.mark.parametrize('shape,K', [((45, 70), 2), ((45, 70), 3), ((33, 130), 2), ((33, 130), 3), ((256, 336), 2)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f'k{v}')
def test_random_case_equals_the_witness(shape, K):
    groups = [_random_group(shape, 400 + 10 * K + g, K) for g in range(2)]
    coeffs = _coeffs(500 + K, 2 * K)
    eng = _eng(shape)
    _stage(eng, groups)
    got, want = _check_combos(eng, shape, groups, coeffs, ('random', shape, K))
    # the case holds what it claims to: holes to fill, more than one label, every pixel reached
    n = want['n_sites'].astype(np.int64)
    assert (n > 0.015 * shape[0] * shape[1]).all() and (n < 0.04 * shape[0] * shape[1]).all() and want['dist2'].max() > 16
    assert (want['labels'] != 255).all() and all(len(np.unique(want['labels'][g])) == K for g in range(2))
    if shape[0] < 100:
        # a bound and a site threshold: exact squares and others, so pixels sit at d2 == max_dist2
        _check_combos(eng, shape, groups, coeffs, ('random-bounded', shape, K), min_site_mass=4096, max_dist2=10, combos=COMBOS[1:3])


# ---- 2. constructed ties ----
def test_constructed_ties():
    shape = (45, 70)
    W = shape[1]
    four = _pixels_group(shape, [(20, 15), (20, 25), (15, 20), (25, 20)])                 # from (20, 20): d2 25 four times
    diag = _pixels_group(shape, [(45, 30), (37, 26)])                                     # from (40, 30): (5, 0) against (3, 4)
    last = _pixels_group(shape, [(10, 9), (14, 5)])                                       # from (10, 5): 4 down, and 4 right at k^2 == best
    sides = _pixels_group(shape, [(25, 35), (15, 35)])                                    # from (20, 35): 5 right, 5 left
    groups = [four, diag, last, sides]
    eng = _eng(shape)
    _stage(eng, groups)
    got, want = _check_combos(eng, shape, groups, _coeffs(600, 8), 'ties')
    assert got['nearest'][0, 20, 20] == 15 * W + 20 and got['dist2'][0, 20, 20] == 25 and got['labels'][0, 20, 20] == 0    # up: the lowest row
    assert got['nearest'][1, 30, 40] == 26 * W + 37 and got['dist2'][1, 30, 40] == 25 and got['labels'][1, 30, 40] == 1    # row 26 before row 30
    # the pixel's own column holds a site at d2 16; the winner at the same d2 lies 4 columns away: only a search that goes on while
    # k^2 <= best meets it
    assert got['nearest'][2, 5, 10] == 5 * W + 14 and got['dist2'][2, 5, 10] == 16 and got['labels'][2, 5, 10] == 1
    # left against right in one row: the lowest column
    assert got['nearest'][3, 35, 20] == 35 * W + 15 and got['dist2'][3, 35, 20] == 25 and got['labels'][3, 35, 20] == 1


# ---- 3. constructed extremes ----
@pytest.mark.parametrize('shape', [(45, 70), (33, 130)], ids=['45x70', '33x130'])
def test_constructed_extremes(shape):
    H, W = shape
    corner = _pixels_group(shape, [(W - 1, H - 1)])                                       # every row searches its whole width
    column = _pixels_group(shape, [(W // 3, y) for y in (1, H // 2, H // 2 + 1, H - 2)])  # every other column carries "no site"
    empty = (_window(shape, [], []), [np.zeros(0, np.float32)] * 2)
    rand = _random_group(shape, 77, 2)
    groups = [corner, column, empty, rand]
    coeffs = _coeffs(601, 8)
    eng = _eng(shape)
    _stage(eng, groups)
    got, want = _check_combos(eng, shape, groups, coeffs, 'extremes')
    assert got['n_sites'].tolist()[:3] == [1, 4, 0]
    assert (got['nearest'][0] == (H - 1) * W + W - 1).all() and got['dist2'][0, 0, 0] == (H - 1) ** 2 + (W - 1) ** 2
    assert (got['nearest'][1] % W == W // 3).all()
    # the group without events: no site, no label, all fallback - dominant has no model to take either
    assert (got['nearest'][2] == -1).all() and (got['dist2'][2] == NONE).all() and (got['labels'][2] == 255).all() and not got['theta'][2].any()
    # ... and its neighbour is what it is alone
    _stage(eng, [rand])
    alone = eng.densify_motions(2, coeffs[6:], mode='soft', fallback='dominant', want=ALL)
    for name in ALL:
        assert alone[name][0].tobytes() == got[name][3].tobytes(), name


# ---- 4. reach and the site threshold ----
def test_reach_at_the_bound():
    shape = (45, 70)
    g = _pixels_group(shape, [(30, 20), (60, 40)])
    eng = _eng(shape)
    _stage(eng, [g])
    coeffs = _coeffs(602, 2)
    f = _model(shape).field(coeffs)
    for fallback, hole in (('zero', np.zeros(2)), ('dominant', None)):
        at = eng.densify_motions(2, coeffs, fallback=fallback, max_distance=np.sqrt(13.0) + 1e-9, want=ALL)       # (33, 22): d2 = 9 + 4 = 13
        below = eng.densify_motions(2, coeffs, fallback=fallback, max_distance=np.sqrt(12.0) + 1e-9, want=ALL)
        assert at['dist2'][0, 22, 33] == 13 and at['labels'][0, 22, 33] == 0 and below['labels'][0, 22, 33] == 255
        assert at['theta'][0, 22, 33].tobytes() == f[0, 22, 33].tobytes()
        want_hole = f[0, 22, 33] if hole is None else hole                    # dominant: equal totals go to model 0
        assert below['theta'][0, 22, 33].tobytes() == want_hole.tobytes()
        assert below['dist2'].tobytes() == at['dist2'].tobytes() and below['nearest'].tobytes() == at['nearest'].tobytes()
        assert (at['labels'] != 255).sum() == (at['dist2'] <= 13).sum() and (below['labels'] != 255).sum() == (below['dist2'] <= 12).sum()
    _check_combos(eng, shape, [g], coeffs, 'reach-13', max_dist2=13)
    _check_combos(eng, shape, [g], coeffs, 'reach-12', max_dist2=12)


def test_site_threshold():
    shape = (45, 70)
    W = shape[1]
    win = _window(shape, [30, 33], [20, 20])
    ws = [np.array([0.5, 0.0], np.float32), np.array([0.0, 1.0], np.float32)]     # (30, 20): q = 2048 for model 0; (33, 20): 4096 for model 1
    eng = _eng(shape)
    _stage(eng, [(win, ws)])
    coeffs = _coeffs(603, 2)
    low = eng.densify_motions(2, coeffs, min_site_mass=2048, want=ALL)
    assert low['n_sites'].tolist() == [2] and low['labels'][0, 20, 30] == 0 and low['nearest'][0, 20, 30] == 20 * W + 30
    high = eng.densify_motions(2, coeffs, min_site_mass=4096, want=ALL)
    assert high['n_sites'].tolist() == [1] and high['labels'][0, 20, 30] == 1 and high['nearest'][0, 20, 30] == 20 * W + 33
    assert high['dist2'][0, 20, 30] == 9 and (high['labels'] == 1).all()
    for m in (2048, 2049, 4096, 4097):
        _check_combos(eng, shape, [(win, ws)], coeffs, ('threshold', m), min_site_mass=m, combos=COMBOS[2:])


@pytest.mark.parametrize('shape', [(45, 70), (33, 130)], ids=['45x70', '33x130'])
def test_no_reach_is_compose_motions(shape):
    groups = [_random_group(shape, 90 + g, 3, frac=0.2) for g in range(2)]
    coeffs = _coeffs(604, 6)
    eng = _eng(shape)
    _stage(eng, groups)
    for mode, fill in COMBOS:
        a = eng.densify_motions(3, coeffs, mode=mode, fallback=fill, min_site_mass=1, max_distance=0)
        b = eng.compose_motions(3, coeffs, mode=mode, fill=fill)
        assert a['theta'].tobytes() == b['theta'].tobytes() and a['labels'].tobytes() == b['labels'].tobytes(), (mode, fill)
        assert (b['labels'] == 255).any() and (b['labels'] != 255).any()
        c = MLW.compose(_model(shape), _wit_groups(groups), coeffs, mode, fill)
        assert a['theta'].tobytes() == c['theta'].tobytes()


# ---- 5. determinism and weights set in place ----
def test_same_bytes_on_every_run_and_engine():
    shape, K = (45, 70), 3
    groups = [_random_group(shape, 120 + g, K) for g in range(2)]
    coeffs = _coeffs(605, 2 * K)
    eng = _eng(shape)
    _stage(eng, groups)
    a = eng.densify_motions(K, coeffs, mode='soft', want=ALL)
    _same(eng.densify_motions(K, coeffs, mode='soft', want=ALL), a, 'second call')
    with _new_engine(shape) as other:
        other.set_motion_model(_model(shape))
        _stage(other, groups)
        _same(other.densify_motions(K, coeffs, mode='soft', want=ALL), a, 'fresh engine')


def test_after_set_weights_on_a_keep_order_staging():
    shape, K = (33, 130), 2
    groups = [_random_group(shape, 130 + g, K) for g in range(2)]
    coeffs = _coeffs(606, 2 * K)
    eng = _eng(shape)
    _stage(eng, groups)
    fresh = eng.densify_motions(K, coeffs, mode='soft', want=ALL)
    eng.set_windows([win for win, ws in groups for _ in ws], keep_order=True)
    unweighted = eng.densify_motions(K, coeffs, mode='soft', want=ALL)
    eng.set_weights([w for _, ws in groups for w in ws])
    _same(eng.densify_motions(K, coeffs, mode='soft', want=ALL), fresh, 'set_weights')
    assert unweighted['theta'].tobytes() != fresh['theta'].tobytes()
    _same(unweighted, WIT.densify(_model(shape), [(win[0], win[1], [None] * K) for win, _ in groups], coeffs, 'soft', 'dominant'), 'unweighted')


# ---- 6. refusals: nothing written, and the engine answers as before ----
def _raw(eng, K, coeffs, flags, min_site_mass, max_dist2, sent, names=ALL):
    return eng._lib.eincm_densify_motions(eng._ctx, K, None if coeffs is None else coeffs.ctypes.data, flags, min_site_mass, max_dist2,
                                          *[sent[n].ctypes.data if n in names else None for n in ALL])


def test_refusals_write_nothing():
    shape, K = (45, 70), 2
    H, W = shape
    groups = [_random_group(shape, 140, K)]
    coeffs = _coeffs(607, K)
    eng = _eng(shape)
    _stage(eng, groups)
    before = eng.densify_motions(K, coeffs, want=ALL)
    size = dict(theta=H * W * 16, labels=H * W, dist2=H * W * 4, nearest=H * W * 4, n_sites=4)
    nan = coeffs.copy(); nan[1, 3] = np.nan
    cases = [('min_site_mass 0', dict(min_site_mass=0), L.ERR_ARG, b'min_site_mass must be at least 1'),
             ('flag bit 2', dict(flags=4), L.ERR_ARG, b'unknown flag bits'),
             ('flag bit 2 before min_site_mass', dict(flags=6, min_site_mass=0), L.ERR_ARG, b'unknown flag bits'),
             ('all outputs null', dict(names=()), L.ERR_ARG, b'null pointer argument (theta, labels, dist2, nearest and n_sites all)'),
             ('n_models 9', dict(K=9), L.ERR_ARG, b'n_models must lie within'),
             ('n_models 3', dict(K=3), L.ERR_ARG, b'not a whole number of groups'),
             ('coeffs null', dict(coeffs=None), L.ERR_ARG, b'coeffs is required'),
             ('coeffs nan', dict(coeffs=nan), L.ERR_ARG, b'must be finite: window 1, coefficient 3')]
    for what, kw, code, msg in cases:
        sent = {n: np.full(s, 0xA5, np.uint8) for n, s in size.items()}
        a = dict(K=K, coeffs=coeffs, flags=2, min_site_mass=1, max_dist2=NONE, names=ALL)
        a.update(kw)
        rc = _raw(eng, a['K'], a['coeffs'], a['flags'], a['min_site_mass'], a['max_dist2'], sent, a['names'])
        err = eng._lib.eincm_last_error(eng._ctx)
        assert rc == code and msg in err and b'eincm_densify_motions' in err, (what, rc, err)
        assert all((v == 0xA5).all() for v in sent.values()), what
        _same(eng.densify_motions(K, coeffs, want=ALL), before, ('after', what))
    # through Python
    with pytest.raises(ValueError, match='min_site_mass'):
        eng.densify_motions(K, coeffs, min_site_mass=0)
    eng.loss_grad_async(np.zeros((K, 1, 1, 2)), E.make_params(20.0, 35.0, 2.5e-4, 0.0, 1))
    try:
        with pytest.raises(E.EincmError, match='an evaluation is in flight') as err:
            eng.densify_motions(K, coeffs)
    finally:
        eng.loss_grad_wait()
    assert err.value.code == L.ERR_STATE
    _same(eng.densify_motions(K, coeffs, want=ALL), before, 'after the evaluation')
    # compose_motions still answers, and still knows nothing of the new word
    with pytest.raises(ValueError, match="fill 'nearest' unknown"):
        eng.compose_motions(K, coeffs, fill='nearest')
    win, ws = groups[0]
    with _new_engine(shape) as other:
        with pytest.raises(E.EincmError, match='needs staged windows') as err:
            other.densify_motions(K, coeffs)
        assert err.value.code == L.ERR_STATE
        _stage(other, groups)
        with pytest.raises(E.EincmError, match='needs staged windows .* and a motion model'):
            other.densify_motions(K, coeffs)
        other.set_motion_model(_model(shape))
        other.set_windows([win + (ws[0],), (win[0][:50], win[1][:50], win[2][:50], win[3], win[4], ws[1][:50])])
        with pytest.raises(E.EincmError, match='equal n_events'):
            other.densify_motions(K, coeffs)
        _stage(other, groups)
        _same(other.densify_motions(K, coeffs, want=ALL), before, 'the other engine after its refusals')
    with _new_engine(shape, 'fp64') as other:
        other.set_motion_model(_model(shape))
        other.set_windows([win, win])                                          # (an fp64 context takes no per-event weights)
        with pytest.raises(E.EincmError, match='fp64') as err:
            other.densify_motions(K, coeffs)
        assert err.value.code == L.ERR_UNSUPPORTED


# ---- 7. the subsets of the outputs ----
def test_want_subsets():
    shape, K = (33, 130), 2
    groups = [_random_group(shape, 150 + g, K) for g in range(2)]
    coeffs = _coeffs(608, 2 * K)
    eng = _eng(shape)
    _stage(eng, groups)
    kw = dict(mode='soft', fallback='dominant', min_site_mass=3000, max_distance=9.5)
    full = eng.densify_motions(K, coeffs, want=ALL, **kw)
    assert (full['labels'] == 255).any() and (full['labels'] != 255).any()
    for want in (('theta',), ('labels',), ('dist2',), ('nearest',), ('n_sites',), ('n_sites', 'theta'), ('nearest', 'labels'), ('dist2', 'nearest'),
                 'dist2', ALL[::-1]):
        got = eng.densify_motions(K, coeffs, want=want, **kw)
        assert tuple(got) == ((want,) if isinstance(want, str) else want)
        _same(got, full, want)
    assert tuple(eng.densify_motions(K, coeffs)) == ('theta', 'labels')


# ---- 8. segmented_flow_dense ----
def test_segmented_flow_dense_is_stage_then_densify():
    shape, K = (45, 70), 2
    groups = [_random_group(shape, 160 + g, K) for g in range(2)]
    coeffs = _coeffs(609, 2 * K)
    record = dict(coeffs=coeffs.reshape(2, K, 6), weights=[ws for _, ws in groups])
    eng = _eng(shape)
    kw = dict(mode='soft', fallback='zero', min_site_mass=4096, max_distance=6)
    got = segmentation.segmented_flow_dense(eng, [win for win, _ in groups], _model(shape), record, **kw)
    assert tuple(got) == ALL
    _stage(eng, groups)
    _same(got, eng.densify_motions(K, coeffs, want=ALL, **kw), 'segmented_flow_dense')
    _same(got, WIT.densify(_model(shape), _wit_groups(groups), coeffs, 'soft', 'zero', 4096, 36), 'segmented_flow_dense against the witness')
    # the sparse form beside it is untouched
    sparse = segmentation.segmented_flow(eng, [win for win, _ in groups], _model(shape), record, mode='soft', fill='zero')
    assert tuple(sparse) == ('theta', 'labels', 'mass', 'total')
    seen = sparse['labels'] != 255
    assert seen.any() and got['theta'][seen & (got['dist2'] == 0)].tobytes() == sparse['theta'][seen & (got['dist2'] == 0)].tobytes()
