"""The HIP-free rules of the fused motion-model evaluation on the CPU: the support predicate and the slot order
of the moment partials (csrc/eincm_motion.h), and the MOTION plan (csrc/eincm_plan.h: plan_motion).

tests/host/motion_fused_check.cpp is built once per session with the address and undefined-behaviour sanitizers, exactly as
tests/test_host_motion.py builds motion_check, and run once, as a child process, over every case of this module; nothing is preloaded.
Its outputs equal numpy and the launch-policy witness (tests/_launch_policy_witness.py) bit for bit."""
import numpy as np
import pytest

import _host_check as HC
import _launch_policy_witness as LP

ERR_STATE, ERR_UNSUPPORTED = -3, -5
PF_FULL_AUX = 1
SHAPE_MOTION, THETA_ARGS = 3, 1


@pytest.fixture(scope='session')
def motion_fused_check(tmp_path_factory):
    """Path of the sanitized checker."""
    return HC.build(tmp_path_factory, 'motion_fused_check')


CASES = {}


def _case(name, *tokens):
    return HC.add_case(CASES, name, *tokens)


@pytest.fixture(scope='module')
def out(motion_fused_check, tmp_path_factory):
    """name -> the checker's line for that case, split at ' |' into lists of words."""
    return HC.run(motion_fused_check, CASES, tmp_path_factory, 'motion_fused_cases')


_f, _i = HC.f, HC.i

# ---- the support predicate: one row per reason, in the order the predicate asks ----
#             fp64 model staged pending devres flight splat flags lvl gamma -> (code, a word of the reason)
OK_STATE = dict(fp64=0, model=1, staged=1, pending=0, devres=0, flight=0, splat=3, flags=0, lvl=1, gamma=0.0)
PREDICATE = {
    'ok': ({}, 0, 'ok'),
    'ok-gamma-above-level-0': (dict(gamma=2.5e-3, lvl=1), 0, 'ok'),
    'ok-level-0-without-tv': (dict(gamma=0.0, lvl=0), 0, 'ok'),
    'ok-correlation-kind-bits': (dict(flags=2 << 8), 0, 'ok'),
    'fp64': (dict(fp64=1), ERR_UNSUPPORTED, 'fp64'),
    'no-model': (dict(model=0), ERR_STATE, 'no motion model'),
    'not-staged': (dict(staged=0), ERR_STATE, 'eincm_set_windows'),
    'constants-pending': (dict(pending=1), ERR_STATE, 'constants pending'),
    'device-results': (dict(devres=1), ERR_STATE, 'eincm_set_device_results'),
    'in-flight': (dict(flight=1), ERR_STATE, 'in flight'),
    'splat-5': (dict(splat=5), ERR_UNSUPPORTED, '3x3 splat window'),
    'splat-1': (dict(splat=1), ERR_UNSUPPORTED, '3x3 splat window'),
    'full-aux': (dict(flags=PF_FULL_AUX), ERR_UNSUPPORTED, 'EINCM_PF_FULL_AUX'),
    'tv-level-0': (dict(gamma=2.5e-3, lvl=0), ERR_UNSUPPORTED, 'TV term'),
    'tv-level-negative': (dict(gamma=-1.0, lvl=-1), ERR_UNSUPPORTED, 'TV term'),
    # the first reason in the predicate's order wins
    'fp64-before-model': (dict(fp64=1, model=0, splat=5), ERR_UNSUPPORTED, 'fp64'),
    'state-before-parameters': (dict(flight=1, flags=PF_FULL_AUX), ERR_STATE, 'in flight'),
}
for _n, (_kw, _, _) in PREDICATE.items():
    _s = dict(OK_STATE, **_kw)
    _case('pred-' + _n, 'supported', *(_s[k] for k in ('fp64', 'model', 'staged', 'pending', 'devres', 'flight', 'splat', 'flags', 'lvl', 'gamma')))


@pytest.mark.parametrize('name', sorted(PREDICATE))
def test_support_predicate(out, name):
    code, words = out['pred-' + name]
    _, want_code, want_word = PREDICATE[name]
    assert int(code[0]) == want_code and want_word in ' '.join(words), (name, code, words)


RNG = np.random.default_rng(21)
USABLE = {'usable-ok': (3.0, RNG.normal(size=12), 1), 'usable-zero': (0.0, np.zeros(12), 1),
          'usable-nan-q': (3.0, np.where(np.arange(12) == 7, np.nan, 1.0), 0), 'usable-inf-q': (3.0, np.where(np.arange(12) == 0, np.inf, 1.0), 0),
          'usable-inf-bound': (np.inf, np.full(12, 1e308), 0), 'usable-nan-bound': (np.nan, np.ones(12), 0)}
for _n, (_b, _q, _) in USABLE.items():
    _case(_n, 'usable', _b, *_q.tolist())


def test_a_window_takes_part_only_with_finite_q_and_bound(out):
    for name, (_, _, want) in USABLE.items():
        assert int(out[name][0][0]) == want, name


# ---- the MOTION plan ----
def _counts(seed, H, W, n_per_window, B):
    rng = np.random.default_rng(seed)
    return np.stack([LP.tile_counts(rng.integers(0, W, n), rng.integers(0, H, n), H, W) for n in np.broadcast_to(n_per_window, (B,))])


#         name -> (H, W, R, B, events per window, vmax, want_grad, lvl, delta, all_r knob)
PLANS = {
    'tiny-wide': (5, 7, 3, 3, 7, 2.0, 1, 1, 0.0, -1),
    'four-tiles': (37, 53, 3, 3, 4000, 9.0, 1, 1, 0.0, -1),
    'one-sparse-window-wide': (64, 96, 3, 3, [20000, 5, 20000], 12.0, 1, 1, 0.0, -1),
    'forward-only': (64, 96, 3, 3, 20000, 12.0, 0, 1, 0.0, -1),
    'divergence': (64, 96, 3, 3, 20000, 12.0, 1, 0, 0.5, -1),
    '65-windows': (5, 7, 3, 65, 7, 2.0, 1, 1, 0.0, -1),
    '10-windows-in-the-arguments': (37, 53, 3, 10, 4000, 9.0, 1, 1, 0.0, -1),
    '11-windows-beyond-them': (37, 53, 3, 11, 4000, 9.0, 1, 1, 0.0, -1),
    'all-r-by-segments': (37, 53, 3, 176, 400, 9.0, 1, 1, 0.0, -1),
    'all-r-one-short-of-it': (37, 53, 3, 174, 400, 9.0, 1, 1, 0.0, -1),
    'all-r-not-at-one-reference-time': (37, 53, 1, 176, 400, 9.0, 1, 1, 0.0, -1),
    'all-r-by-knob': (37, 53, 3, 3, 4000, 9.0, 1, 1, 0.0, 1),
    'bench-batch': (260, 346, 5, 8, 1_000_000, 30.0, 1, 1, 0.0, -1),
    'unknown-bound': (260, 346, 5, 1, 1_000_000, float('inf'), 1, 1, 0.0, -1),
}
PLAN_COUNTS = {}
for _k, (_n, (_H, _W, _R, _B, _ev, _v, _wg, _lvl, _d, _knob)) in enumerate(PLANS.items()):
    PLAN_COUNTS[_n] = _counts(100 + _k, _H, _W, _ev, _B)
    _case('plan-' + _n, 'plan', _H, _W, _R, _B, _v, _wg, _lvl, _d, _knob, *PLAN_COUNTS[_n].reshape(-1).tolist())
_case('consts', 'consts')

PLAN_FIELDS = ('shape', 'theta_src', 'use_arg', 'need_theta_image', 'host_asm', 'zero_copy_out', 'all_r', 'identity', 'nsrc',
               'events_projected', 'proj', 'grid_tail', 'want_tv', 'want_div', 'div_grad', 'wide', 'n_gather', 'nth')


@pytest.mark.parametrize('name', sorted(PLANS))
def test_motion_plan(out, name):
    H, W, R, B, ev, vmax, want_grad, lvl, delta, knob = PLANS[name]
    counts = PLAN_COUNTS[name]
    got = dict(zip(PLAN_FIELDS, _i(out['plan-' + name][0]).tolist()))
    n_gather = len(LP.segment_lengths(counts, LP.SEG_LONG))
    all_r = bool(want_grad) and R > 1 and (knob != 0 if knob >= 0 else n_gather >= 700)
    want = dict(shape=SHAPE_MOTION, theta_src=THETA_ARGS, use_arg=int(B <= 10), need_theta_image=0, host_asm=0, zero_copy_out=1,
                all_r=int(all_r), identity=1, nsrc=0, events_projected=1, proj=0, grid_tail=0, want_tv=0, want_div=int(delta != 0.0),
                div_grad=int(delta != 0.0 and want_grad), wide=int((counts.sum(axis=1) * R < 4096).any()), n_gather=n_gather, nth=H * W * 2)
    assert got == want, (name, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    # no theta image and no window tables; the capacities are the dense shape's at the motion bound (unknown: the largest windows)
    lp = LP.launch_policy(counts, H, W, R, B, rad=1, vmax=vmax if np.isfinite(vmax) else 1e9, two_dof=False)
    for field, g in zip(LP.FIELDS, _f(out['plan-' + name][1])):
        assert g == lp[field], (name, field, g, lp[field])


def test_the_cases_reach_both_sides_of_every_rule(out):
    got = {n: dict(zip(PLAN_FIELDS, _i(out['plan-' + n][0]).tolist())) for n in PLANS}
    assert {g['wide'] for g in got.values()} == {0, 1} and {g['all_r'] for g in got.values()} == {0, 1}
    assert {g['use_arg'] for g in got.values()} == {0, 1}
    assert got['all-r-by-segments']['n_gather'] >= 700 > got['all-r-one-short-of-it']['n_gather']
    assert _i(out['consts'][0]).tolist() == [10, 128, SHAPE_MOTION, THETA_ARGS]      # q of up to 10 windows beside (cx, cy, s)


# ---- the slots of the moment partials and the order they are added in ----
SLOTS = {}
for _n, (_B, _nt, _seg, _sps) in {'slots-one': (1, 1, 16384, 1), 'slots-r3': (3, 4, 16384, 3), 'slots-several-per-tile': (4, 6, 256, 5),
                                   'slots-65': (65, 2, 4096, 1)}.items():
    _c = np.where(RNG.random((_B, _nt)) < 0.25, 0, RNG.integers(1, 5 * _seg, (_B, _nt)))
    SLOTS[_n] = (_c, _seg, _sps)
    _case(_n, 'slots', _B, _nt, _seg, _sps, *_c.reshape(-1).tolist())
SLOTS['slots-empty'] = (np.zeros((3, 2), dtype=np.int64), 16384, 3)
_case('slots-empty', 'slots', 3, 2, 16384, 3, *[0] * 6)


@pytest.mark.parametrize('name', sorted(SLOTS))
def test_slot_offsets_follow_the_segment_cut(out, name):
    counts, seg, sps = SLOTS[name]
    per_window = np.array([len(LP.segment_lengths(row, seg)) for row in counts], dtype=np.int64)
    total, s0 = int(out[name][0][0]), _i(out[name][1])
    assert total == per_window.sum()
    assert np.array_equal(s0, np.concatenate([[0], np.cumsum(per_window)]) * sps)


SUMS = {'sum-random': RNG.normal(size=(37, 12)) * 10.0 ** RNG.integers(-8, 8, size=(37, 12)),
        'sum-cancelling': np.concatenate([RNG.normal(size=(20, 12)) * 1e9, RNG.normal(size=(20, 12))]),
        'sum-one': RNG.normal(size=(1, 12)), 'sum-none': np.zeros((0, 12))}
for _n, _p in SUMS.items():
    _case(_n, 'sum', _p.shape[0], *_p.reshape(-1).tolist())


@pytest.mark.parametrize('name', sorted(SUMS))
def test_partials_are_added_in_index_order(out, name):
    parts = SUMS[name]
    s = parts[0].copy() if len(parts) else np.zeros(12)
    for g in range(1, parts.shape[0]):
        s = s + parts[g]
    assert np.array_equal(_f(out[name][0]), s)
    if name == 'sum-cancelling':
        assert not np.array_equal(s, parts[::-1].cumsum(axis=0)[-1])   # the order matters on this input: the check can see it
