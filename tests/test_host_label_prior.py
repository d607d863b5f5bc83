"""The HIP-free rules of the per-pixel label prior (csrc/eincm_label_prior.h) and of the E-step with a prior image
(csrc/eincm_responsibilities.h: rs_spatial_check) on the CPU: the argument check in its stated order, one refusal at a time and with
every later fault present; the layout of the two outputs against engine.label_prior_layout; the per-pixel function lp_prior for
K = 1, 2, 8 against tests/_label_prior_witness.py, bit for bit; and the refusals the spatial E-step adds to rs_check's.

tests/host/label_prior_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_motion_layers.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import importlib

import numpy as np
import pytest

import _host_check as HC
import _label_prior_witness as WIT

(OK, IN_FLIGHT, NOT_STAGED, FP64, SHARDED, MODELS, GROUPS, UNEQUAL, RADIUS, BAD_FLAGS, CROWDED) = range(11)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NOT_STAGED: ERR_STATE, FP64: ERR_UNSUPPORTED, SHARDED: ERR_UNSUPPORTED, MODELS: ERR_ARG, GROUPS: ERR_ARG,
        UNEQUAL: ERR_ARG, RADIUS: ERR_ARG, BAD_FLAGS: ERR_ARG, CROWDED: ERR_UNSUPPORTED}
# eincm_compose_motions' codes for the faults the two operators share (tests/test_host_motion_layers.py: CODE)
COMPOSE_CODE = {IN_FLIGHT: ERR_STATE, NOT_STAGED: ERR_STATE, FP64: ERR_UNSUPPORTED, SHARDED: ERR_UNSUPPORTED, MODELS: ERR_ARG, GROUPS: ERR_ARG,
                UNEQUAL: ERR_ARG, BAD_FLAGS: ERR_ARG, CROWDED: ERR_UNSUPPORTED}
FULL = 1 << 20                                               # the tile population that is refused


@pytest.fixture(scope='session')
def label_prior_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'label_prior_check')


CASES, EXPECT = {}, {}


def _check(name, fault, where=(-1, -1), in_flight=0, staged=1, fp64=0, sharded=0, n_models=2, radius=2, flags=0, ne=(5, 5, 0, 0), ntiles=3,
           tiles=None):
    B = len(ne)
    tc = [0] * (B * ntiles) if tiles is None else list(tiles)
    assert len(tc) == B * ntiles
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, staged, fp64, sharded, n_models, radius, flags, B, *ne, ntiles, *tc)
    EXPECT['check-' + name] = (fault, where)
    return 'check-' + name


# every fault at once: each of the order's ten, the later ones still present when the earlier ones are mended
ALL_BAD = dict(in_flight=1, staged=0, fp64=1, sharded=1, n_models=9, ne=(5, 4, 3), radius=9, flags=4, tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0))
_order = ['in_flight', 'staged', 'fp64', 'sharded', 'n_models', 'groups', 'unequal', 'radius', 'flags', 'crowded']
_mend = {'in_flight': dict(in_flight=0), 'staged': dict(staged=1), 'fp64': dict(fp64=0), 'sharded': dict(sharded=0), 'n_models': dict(n_models=2),
         'groups': dict(ne=(5, 4, 3, 3), tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0, 0, 0, 0)), 'unequal': dict(ne=(5, 5, 3, 3)),
         'radius': dict(radius=8), 'flags': dict(flags=0), 'crowded': dict(tiles=None)}
_where = {CROWDED: (1, 1)}


def _from(i):
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw.update(_mend[k])
    return kw


CHECKS = [_check('ok', OK), _check('ok-k1', OK, n_models=1, ne=(3, 0, 7)), _check('ok-k8', OK, n_models=8, ne=(2,) * 16),
          _check('ok-no-events', OK, ne=(0, 0)), _check('ok-radius-0', OK, radius=0), _check('ok-radius-8', OK, radius=8),
          _check('ok-tile-just-below', OK, tiles=(FULL - 1,) * 12), _check('in-flight', IN_FLIGHT, in_flight=1),
          _check('not-staged', NOT_STAGED, staged=0), _check('fp64', FP64, fp64=1), _check('sharded', SHARDED, sharded=1),
          _check('k0', MODELS, n_models=0), _check('k-negative', MODELS, n_models=-2), _check('k9', MODELS, n_models=9),
          _check('k-does-not-divide', GROUPS, n_models=3), _check('k-more-than-windows', GROUPS, n_models=8),
          _check('unequal', UNEQUAL, ne=(5, 4, 0, 0)), _check('unequal-last-group', UNEQUAL, ne=(5, 5, 0, 1)),
          _check('equal-across-groups-only', UNEQUAL, ne=(5, 4, 5, 4)), _check('radius-negative', RADIUS, radius=-1),
          _check('radius-9', RADIUS, radius=9), _check('flag-bit-0', BAD_FLAGS, flags=1), _check('flag-bit-31', BAD_FLAGS, flags=1 << 31),
          _check('crowded', CROWDED, (3, 2), tiles=(0,) * 11 + (FULL,)), _check('crowded-more', CROWDED, (0, 1), tiles=(5, FULL + 9) + (0,) * 10)]
CHECKS += [_check(f'from-{i + 1:02d}-{k}', i + 1, _where.get(i + 1, (-1, -1)), **_from(i)) for i, k in enumerate(_order)]


@pytest.fixture(scope='module')
def out(label_prior_check, tmp_path_factory):
    return HC.run(label_prior_check, CASES, tmp_path_factory, 'label_prior_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code, wb, wi = (int(v) for v in out[name][0])
    assert (fault, (wb, wi)) == EXPECT[name] and code == CODE[fault]
    assert fault not in COMPOSE_CODE or code == COMPOSE_CODE[fault]


LAYOUTS = [(0, 2, 40, 72), (1, 1, 40, 72), (2, 3, 40, 72), (3, 8, 5, 7), (5, 2, 480, 640), (2, 8, 20000, 30000)]
for _l in LAYOUTS:
    HC.add_case(CASES, 'layout-%d-%d-%d-%d' % _l, 'layout', *_l)


@pytest.mark.parametrize('G,K,H,W', LAYOUTS)
def test_python_layout_is_the_headers(out, G, K, H, W):
    eng = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    lay = eng.label_prior_layout(G, K, (H, W))
    _, pr, sm = out['layout-%d-%d-%d-%d' % (G, K, H, W)]
    assert lay['prior'][0] == (G * K, H, W) and lay['smoothed'][0] == (G, K, H, W)
    assert [lay[n][1] for n in ('prior', 'smoothed')] == [np.float32, np.uint64]
    # the header gives every window's block of prior and every (group, model) block of smoothed; Python's are the groups' (model 0)
    assert [int(v) for v in pr] == [int(lay['prior'][2][g]) + l * H * W for g in range(G) for l in range(K)]
    assert [int(v) for v in sm] == [int(lay['smoothed'][2][g]) + l * H * W for g in range(G) for l in range(K)]


# lp_prior: T == 0, a model without mass, equal shares (1/K is not a binary fraction for K = 3 .. 7), the largest sums (17^2 pixels of
# the largest mass per model: sums near 2^41 and a total near 2^44), one unit of difference there, and random sums
_BIG = 289 * 4294963200
_PRIORS = {}
_rng = np.random.default_rng(17)
for _K in (1, 2, 8):
    _sets = [(0, [0] * _K), (1, [0] * _K), (4096, [0] * _K), (0, [0] * (_K - 1) + [7]), (0, [3] * _K), (4096, [_BIG] * _K),
             (0, [_BIG - l for l in range(_K)]), (1, [_BIG] + [0] * (_K - 1)), (0xFFFFFFFF, [_BIG] * _K), (0xFFFFFFFF, [0] * _K)]
    _sets += [(int(_rng.integers(0, 8192)), [int(v) for v in _rng.integers(0, 2 ** int(_rng.integers(1, 42)), _K)]) for _ in range(8)]
    for _j, (_floor, _S) in enumerate(_sets):
        _PRIORS[f'k{_K}-{_j:02d}'] = (_floor, _S)
        HC.add_case(CASES, f'prior-k{_K}-{_j:02d}', 'prior', _K, _floor, *_S)


@pytest.mark.parametrize('name', sorted(_PRIORS))
def test_lp_prior_bit_for_bit(out, name):
    floor, S = _PRIORS[name]
    got = np.array([float(t) for t in out['prior-' + name][1]], dtype=np.float64).astype(np.float32)
    want = WIT.lp_prior(np.array(S, dtype=np.uint64), floor)
    assert got.tobytes() == want.tobytes(), (got, want)
    if floor == 0 and not any(S):
        assert (got == 1.0).all()                            # T == 0
    if len(S) == 1:
        assert got[0] == 1.0                                 # n / n, or T == 0
    if floor == 0 and S[-1] > 0 and not any(S[:-1]) and len(S) > 1:
        assert got[-1] == 1.0 and not got[:-1].any()         # a model without mass and without a floor has no share


def test_the_witness_box_sum_is_the_plain_double_loop():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 2 ** 32, (2, 11, 9), dtype=np.uint64).astype(np.uint32)
    for r in (0, 1, 3, 8):
        want = np.zeros(m.shape, dtype=np.uint64)
        for y in range(11):
            for x in range(9):
                want[:, y, x] = m[:, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].astype(np.uint64).sum(axis=(1, 2), dtype=np.uint64)
        assert WIT.box_sum(m, r).tobytes() == want.tobytes()


# ---- the refusals the spatial E-step adds to rs_check's ----
(S_OK, S_BOTH, S_NEITHER, S_NOT_STAGED, S_VALUE) = range(5)
S_CODE = {S_OK: 0, S_BOTH: ERR_ARG, S_NEITHER: ERR_ARG, S_NOT_STAGED: ERR_STATE, S_VALUE: ERR_ARG}
PRIOR_STAGED = 8                                             # EINCM_RS_PRIOR_STAGED
_GOOD = [0.0, 1.0, 0.5, 3.0e38, 1.0e-45, 2.0]               # (B = 2, npix = 3)
SPATIAL = {}


def _spatial(name, fault, where=(-1, -1), values=_GOOD, flags=0, prior_staged=0):
    v = [] if values is None else list(values)
    HC.add_case(CASES, 'spatial-' + name, 'spatial', int(values is not None), flags, prior_staged, 2, 3, *[float(x) for x in v])
    SPATIAL['spatial-' + name] = (fault, where)
    return 'spatial-' + name


SPATIALS = [_spatial('images', S_OK), _spatial('images-other-flags', S_OK, flags=7), _spatial('staged', S_OK, values=None, flags=PRIOR_STAGED, prior_staged=1),
            _spatial('staged-with-apply', S_OK, values=None, flags=PRIOR_STAGED | 4 | 1, prior_staged=1),
            _spatial('images-beside-a-staged-prior', S_OK, prior_staged=1),
            _spatial('both', S_BOTH, flags=PRIOR_STAGED, prior_staged=1), _spatial('both-bad-value-too', S_BOTH, values=[np.nan] * 6, flags=PRIOR_STAGED),
            _spatial('neither', S_NEITHER, values=None), _spatial('neither-with-a-staged-prior', S_NEITHER, values=None, prior_staged=1),
            _spatial('flag-without-a-staged-prior', S_NOT_STAGED, values=None, flags=PRIOR_STAGED),
            _spatial('nan', S_VALUE, (1, 1), values=[0, 1, 2, 3, np.nan, 5]), _spatial('inf', S_VALUE, (0, 2), values=[0, 1, np.inf, 3, 4, 5]),
            _spatial('negative', S_VALUE, (1, 2), values=[0, 1, 2, 3, 4, -1.0e-30]), _spatial('first-of-two', S_VALUE, (0, 0), values=[-1, 1, 2, 3, np.nan, 5]),
            _spatial('too-large-for-a-float', S_VALUE, (1, 0), values=[0, 1, 2, 1.0e39, 4, 5]), _spatial('minus-zero', S_OK, values=[-0.0] * 6)]


@pytest.mark.parametrize('name', SPATIALS)
def test_the_spatial_e_step_s_added_refusals(out, name):
    fault, code, wb, wp = (int(v) for v in out[name][0])
    assert (fault, (wb, wp)) == SPATIAL[name] and code == S_CODE[fault]


def test_the_added_refusals_are_a_second_function_beside_rs_check():
    import os
    rules = open(os.path.join(HC.CSRC, 'eincm_responsibilities.h')).read()
    assert rules.count('inline RsFault rs_check(') == 1 and rules.count('inline RsSpatialFault rs_spatial_check(') == 1
    assert 'PRIOR_STAGED' not in rules.split('inline RsFault rs_check(')[1].split('\n}\n')[0]
    lp = open(os.path.join(HC.CSRC, 'eincm_label_prior.h')).read()
    import re
    assert 'hip' not in ''.join(re.findall(r'#include\s+[<"]([^>"]+)[>"]', lp)).lower()
