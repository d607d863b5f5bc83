"""The HIP-free rules of the dense composition of a motion segmentation (csrc/eincm_motion_fill.h) on the CPU:
the argument check in its stated order - ml_check's eleven faults, then the two new ones - one refusal at a time and with every later
fault present; the layout of the five outputs against engine.densify_motions_layout; the packed column record at its limits; the key's
order; the site rule; and the feature transform exactly as the kernels run it - the two column sweeps, then the row search with its
k^2 <= best bound - against the brute force of tests/_motion_fill_witness.py on masks of up to 12 x 12.

tests/host/motion_fill_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_motion_layers.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import importlib

import numpy as np
import pytest

import _host_check as HC
import _motion_fill_witness as WIT

(OK, IN_FLIGHT, NULL_OUTPUTS, NOT_READY, FP64, SHARDED, MODELS, GROUPS, UNEQUAL, COEFFS, BAD_FLAGS, CROWDED, SITE_MASS, WIDE) = range(14)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NULL_OUTPUTS: ERR_ARG, NOT_READY: ERR_STATE, FP64: ERR_UNSUPPORTED, SHARDED: ERR_UNSUPPORTED,
        MODELS: ERR_ARG, GROUPS: ERR_ARG, UNEQUAL: ERR_ARG, COEFFS: ERR_ARG, BAD_FLAGS: ERR_ARG, CROWDED: ERR_UNSUPPORTED,
        SITE_MASS: ERR_ARG, WIDE: ERR_UNSUPPORTED}
FULL = 1 << 20                                               # the tile population that is refused
MAX_W = 16384
REC_NONE, KEY_NONE = 0xFFFFFFFF, 2 ** 64 - 1


@pytest.fixture(scope='session')
def motion_fill_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'motion_fill_check')


CASES, EXPECT = {}, {}
NOCO = object()


def _check(name, fault, where=(-1, -1), in_flight=0, has_outputs=1, staged=1, model_set=1, fp64=0, sharded=0, n_models=2, flags=3,
           n_coeffs=2, ne=(5, 5, 0, 0), coeffs=None, ntiles=3, tiles=None, W=640, min_site_mass=1):
    B = len(ne)
    co = [0.5] * (B * n_coeffs) if coeffs is None else ([] if coeffs is NOCO else list(coeffs))
    tc = [0] * (B * ntiles) if tiles is None else list(tiles)
    assert len(tc) == B * ntiles and (coeffs is NOCO or len(co) == B * n_coeffs)
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, has_outputs, staged, model_set, fp64, sharded, n_models, flags, n_coeffs, B, *ne,
                int(coeffs is not NOCO), *[float(v) for v in co], ntiles, *tc, W, min_site_mass)
    EXPECT['check-' + name] = (fault, where)
    return 'check-' + name


# every fault at once: each of the order's thirteen, the later ones still present when the earlier ones are mended
_NAN3 = (1.0, 2.0, 3.0, np.nan, 5.0, 6.0)
ALL_BAD = dict(in_flight=1, has_outputs=0, staged=0, model_set=0, fp64=1, sharded=1, n_models=9, ne=(5, 4, 3), coeffs=_NAN3, flags=7,
               tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0), min_site_mass=0, W=MAX_W + 1)
_order = ['in_flight', 'has_outputs', 'ready', 'fp64', 'sharded', 'n_models', 'groups', 'unequal', 'coeffs', 'flags', 'crowded', 'site_mass',
          'wide']
_mend = {'in_flight': dict(in_flight=0), 'has_outputs': dict(has_outputs=1), 'ready': dict(staged=1, model_set=1), 'fp64': dict(fp64=0),
         'sharded': dict(sharded=0), 'n_models': dict(n_models=2),
         'groups': dict(ne=(5, 4, 3, 3), coeffs=_NAN3 + (7.0, 8.0), tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0, 0, 0, 0)),
         'unequal': dict(ne=(5, 5, 3, 3)), 'coeffs': dict(coeffs=None), 'flags': dict(flags=2), 'crowded': dict(tiles=None),
         'site_mass': dict(min_site_mass=1), 'wide': dict(W=MAX_W)}
_where = {COEFFS: (1, 1), CROWDED: (1, 1)}


def _from(i):
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw.update(_mend[k])
    return kw


CHECKS = [_check('ok', OK), _check('ok-k1', OK, n_models=1, ne=(3, 0, 7)), _check('ok-k8', OK, n_models=8, ne=(2,) * 16),
          _check('ok-no-events', OK, ne=(0, 0)), _check('ok-hard-zero', OK, flags=0), _check('ok-widest', OK, W=MAX_W),
          _check('ok-largest-site-mass', OK, min_site_mass=0xFFFFFFFF), _check('ok-two-events', OK, min_site_mass=8192),
          _check('in-flight', IN_FLIGHT, in_flight=1), _check('null-outputs', NULL_OUTPUTS, has_outputs=0),
          _check('not-staged', NOT_READY, staged=0), _check('no-model', NOT_READY, model_set=0), _check('fp64', FP64, fp64=1),
          _check('sharded', SHARDED, sharded=1), _check('k0', MODELS, n_models=0), _check('k9', MODELS, n_models=9),
          _check('k-does-not-divide', GROUPS, n_models=3), _check('unequal', UNEQUAL, ne=(5, 4, 0, 0)),
          _check('coeffs-null', COEFFS, coeffs=NOCO), _check('coeffs-nan', COEFFS, (2, 1), coeffs=(1, 2, 3, 4, 5, np.nan, 7, 8)),
          _check('flag-bit-2', BAD_FLAGS, flags=4), _check('flag-bit-31', BAD_FLAGS, flags=(1 << 31) | 1),
          _check('crowded', CROWDED, (3, 2), tiles=(0,) * 11 + (FULL,)), _check('site-mass-0', SITE_MASS, min_site_mass=0),
          _check('too-wide', WIDE, W=MAX_W + 1), _check('site-mass-0-and-too-wide', SITE_MASS, min_site_mass=0, W=32767),
          _check('flags-before-site-mass', BAD_FLAGS, flags=4, min_site_mass=0)]
CHECKS += [_check(f'from-{i + 1:02d}-{k}', i + 1, _where.get(i + 1, (-1, -1)), **_from(i)) for i, k in enumerate(_order)]
CHECKS += [_check('all-mended', OK, **_from(len(_order)))]


@pytest.fixture(scope='module')
def out(motion_fill_check, tmp_path_factory):
    return HC.run(motion_fill_check, CASES, tmp_path_factory, 'motion_fill_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code, wb, wi = (int(v) for v in out[name][0])
    assert (fault, (wb, wi)) == EXPECT[name] and code == CODE[fault]


LAYOUTS = [(0, 40, 72), (1, 40, 72), (3, 45, 70), (5, 480, 640), (8, 20000, 16384)]
for _l in LAYOUTS:
    HC.add_case(CASES, 'layout-%d-%d-%d' % _l, 'layout', *_l)


@pytest.mark.parametrize('G,H,W', LAYOUTS)
def test_python_layout_is_the_headers(out, G, H, W):
    eng = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    lay = eng.densify_motions_layout(G, (H, W))
    names = ('theta', 'labels', 'dist2', 'nearest', 'n_sites')
    assert names == eng.MF_OUTPUTS
    assert [lay[n][0] for n in names] == [(G, H, W, 2), (G, H, W), (G, H, W), (G, H, W), (G,)]
    assert [lay[n][1] for n in names] == [np.float64, np.uint8, np.uint32, np.int32, np.uint32]
    for n, got in zip(names, out['layout-%d-%d-%d' % (G, H, W)][1:]):
        assert [int(v) for v in got] == lay[n][2].tolist() and lay[n][2].dtype == np.int64, n


# ---- the packed record: distance 0, the largest distance and row of a sensor side below 32768, and the no-site word ----
_PACKS = {'zero': (0, 0), 'site-in-last-row': (0, 32767), 'far': (32767, 0), 'far-below': (32767, 32767), 'some': (5, 9), 'none': (65535, -1)}
for _n, _p in _PACKS.items():
    HC.add_case(CASES, 'pack-' + _n, 'pack', *_p)


@pytest.mark.parametrize('name', sorted(_PACKS))
def test_packed_record_round_trips(out, name):
    dist, y = _PACKS[name]
    rec, d, yy = (int(v) for v in out['pack-' + name][0])
    assert (d, yy) == (dist, y) and rec == (REC_NONE if y < 0 else dist | y << 16) and (rec == REC_NONE) == (name == 'none')


# ---- the key: its value, and that its unsigned order is (d2, y', x') ----
_KEYS = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0), (0, 7, 1, 3), (3, 2, 4, 9), (5, 2, 0, 9), (4, 1, 3, 0), (4, 1, 3, 16383),
         (32767, 32767, 16383, 16383), (32767, 0, 16383, 0), (65535, -1, 0, 5), (65535, -1, 99, 0)]
for _i, _k in enumerate(_KEYS):
    HC.add_case(CASES, 'key-%d' % _i, 'key', *_k)


def test_key_is_the_tie_rule(out):
    got = [int(out['key-%d' % i][0][0]) for i in range(len(_KEYS))]
    tup = []
    for (dist, y, dx, xs), key in zip(_KEYS, got):
        if y < 0:
            assert key == KEY_NONE
            tup.append((1 << 40, 0, 0))
        else:
            assert key == (dist * dist + dx * dx) << 32 | y << 16 | xs and key < KEY_NONE
            tup.append((dist * dist + dx * dx, y, xs))
    for a in range(len(got)):
        for b in range(len(got)):
            assert (got[a] < got[b]) == (tup[a] < tup[b]), (_KEYS[a], _KEYS[b])
    assert got[5] >> 32 == got[6] >> 32 == 25 and got[5] == got[6]            # (3, 4) against (5, 0) in the same column and row: one site


_SITES = {'one-event': (2, 1, [4096, 0]), 'zero': (2, 1, [0, 0]), 'half-under-4096': (2, 4096, [2048, 0]), 'halves-make-one': (2, 4096, [2048, 2048]),
          'just-under': (3, 8192, [4096, 4095, 0]), 'at': (3, 8192, [4096, 4095, 1]), 'sum-above-2^32': (2, 0xFFFFFFFF, [4294963200, 4294963200]),
          'largest-threshold-missed': (1, 0xFFFFFFFF, [4294963200])}
for _n, (_K, _t, _m) in _SITES.items():
    HC.add_case(CASES, 'site-' + _n, 'site', _K, _t, *_m)


@pytest.mark.parametrize('name', sorted(_SITES))
def test_site_rule(out, name):
    K, t, m = _SITES[name]
    want = bool(WIT.sites(np.array(m, dtype=np.uint32).reshape(K, 1, 1), t)[0, 0])
    assert int(out['site-' + name][0][0]) == int(want) == int(sum(m) >= t)


# ---- the feature transform as the kernels run it, against brute force ----
def _masks():
    rng = np.random.default_rng(31)
    m = {'empty': np.zeros((5, 7), bool), 'full': np.ones((6, 5), bool), '1x1-empty': np.zeros((1, 1), bool), '1x1-site': np.ones((1, 1), bool)}
    one = np.zeros((9, 12), bool); one[8, 11] = True
    m['one-site-in-the-corner'] = one
    one = np.zeros((12, 9), bool); one[0, 0] = True
    m['one-site-at-the-origin'] = one
    col = np.zeros((12, 11), bool); col[[1, 6, 7, 11], 4] = True
    m['one-column'] = col
    row = np.zeros((11, 12), bool); row[5, [0, 3, 4, 10]] = True
    m['one-row'] = row
    cross = np.zeros((9, 9), bool); cross[[1, 7, 4, 4], [4, 4, 1, 7]] = True          # (4, 4): equal distance up, down, left, right
    m['four-way-tie'] = cross
    diag = np.zeros((12, 12), bool); diag[[0, 4], [3, 11]] = True                     # from (x 6, y 4): (3, 4) up-left against (5, 0) right
    m['diagonal-against-axis'] = diag
    # the tie that only the last step meets: from (x 4, y 0) a site 4 rows straight down (column 4, d2 16) and a site in the pixel's
    # own row 4 columns to the right (d2 16, y' 0): the second wins on the row, and the search sees it only at k = 4, where k^2 == best
    last = np.zeros((6, 10), bool); last[[4, 0], [4, 8]] = True
    m['tie-at-the-last-step'] = last
    thin = np.zeros((1, 12), bool); thin[0, [2, 9]] = True
    m['one-pixel-high'] = thin
    tall = np.zeros((12, 1), bool); tall[[2, 9], 0] = True
    m['one-pixel-wide'] = tall
    for i in range(60):
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        m['random-%02d' % i] = rng.random((H, W)) < rng.choice([0.03, 0.1, 0.3, 0.7])
    return m


MASKS = _masks()
for _n, _m in MASKS.items():
    HC.add_case(CASES, 'ft-' + _n, 'ft', _m.shape[0], _m.shape[1], *_m.astype(int).reshape(-1))


@pytest.mark.parametrize('name', sorted(MASKS))
def test_feature_transform_against_brute_force(out, name):
    site = MASKS[name]
    H, W = site.shape
    _, rec, near, d2 = out['ft-' + name]
    rec, near, d2 = (np.array([int(v) for v in a], dtype=np.int64).reshape(H, W) for a in (rec, near, d2))
    want_near, want_d2 = WIT.feature_transform(site)
    assert np.array_equal(near, want_near) and np.array_equal(d2, want_d2.astype(np.int64))
    # the column records: the nearest site of the pixel's own column, the upper one of an up/down tie; no site, no record
    for x in range(W):
        ys = np.nonzero(site[:, x])[0]
        for y in range(H):
            if len(ys) == 0:
                assert rec[y, x] == REC_NONE
            else:
                d, yy = min((abs(int(s) - y), int(s)) for s in ys)
                assert rec[y, x] == d | yy << 16
    if site.any():
        assert (near[site] == np.flatnonzero(site.reshape(-1))).all() and (d2[site] == 0).all()       # a site's nearest site is itself
    else:
        assert (near == -1).all() and (d2 == 0xFFFFFFFF).all()


def test_the_constructed_ties_hold_what_they_claim(out):
    near = lambda name: np.array([int(v) for v in out['ft-' + name][2]]).reshape(MASKS[name].shape)
    assert near('four-way-tie')[4, 4] == 1 * 9 + 4                           # up wins: the lowest row
    assert near('diagonal-against-axis')[4, 6] == 0 * 12 + 3                 # d2 25 both: row 0 wins over row 4
    assert near('tie-at-the-last-step')[0, 4] == 0 * 10 + 8                  # d2 16 both: row 0, met at k = 4 with k^2 == best
    assert near('one-site-in-the-corner')[0, 0] == 8 * 12 + 11
