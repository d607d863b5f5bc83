"""The host's planning (csrc/eincm_plan.h: launch policy, segment cut, resampling tables, host binning, the small rules) on the CPU.

tests/host/plan_check.cpp is built once per session with the address and undefined-behaviour sanitizers and run once, as a child
process, over every case of this module; the tests compare what it printed with numpy, the oracle and the launch-policy witness
(tests/_launch_policy_witness.py).  The GPU modules (test_gpu_launch_policy*.py) guard the wiring of the same rules into the library."""
import math

import numpy as np
import pytest

import _host_check as HC
import _launch_policy_cases as C
import _launch_policy_witness as LP
from oracle import eincm_oracle as O

METHODS = {'bilinear': 0, 'lanczos3': 1, 'lanczos5': 2, 'cubic': 3}
PG_MAXC = 6                            # cells per axis under a tile that k_gather's own projection handles


@pytest.fixture(scope='session')
def plan_check(tmp_path_factory):
    """Path of the sanitized checker."""
    return HC.build(tmp_path_factory, 'plan_check')


# ---- the cases: name -> input line, collected when the module is imported; one run of the checker answers all of them ----
CASES = {}


def _case(name, *tokens):
    return HC.add_case(CASES, name, *tokens)


@pytest.fixture(scope='module')
def out(plan_check, tmp_path_factory):
    """name -> the checker's line for that case, split at ' |' into lists of words."""
    return HC.run(plan_check, CASES, tmp_path_factory, 'plan_cases')


_f, _i = HC.f, HC.i


# ================================================================================================
# launch policy: plan_staging + cut_segments + plan_eval, assembled as eincm_get_launch_policy does, against the witness
# ================================================================================================
def _policy_case(name, counts, H, W, R, B, rad, pitch_env, vmax, hw):
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    return _case(name, 'policy', H, W, R, B, rad, -1 if pitch_env is None else pitch_env, -1.0 if vmax is None else float(vmax), hw[0], hw[1],
                 *counts.tolist())


POLICY = []                            # (case name, the witness's arguments)
for _c in C.CASES:
    for _rad in (1, 2):
        for _pe in (None, 0, 1, 2):
            POLICY.append((_policy_case(f'policy-{_c.id}-r{_rad}-p{_pe}', C.counts(_c.batch), C.H, C.W, C.R, C.B, _rad, _pe, _c.v, _c.hw),
                           dict(counts=C.counts(_c.batch), H=C.H, W=C.W, R=C.R, B=C.B, rad=_rad, vmax=_c.v, two_dof=_c.two_dof, pitch_env=_pe)))
for _b in ('A', 'B'):                  # staged, not evaluated
    POLICY.append((_policy_case(f'policy-{_b}-staged', C.counts(_b), C.H, C.W, C.R, C.B, 1, None, None, (1, 1)),
                   dict(counts=C.counts(_b), H=C.H, W=C.W, R=C.R, B=C.B, rad=1, vmax=None, two_dof=True, pitch_env=None)))


def _uniform_counts(seed, H, W, n, R, B, xy=None):
    """Tile populations of the batches of tests/test_gpu_launch_policy.py: its _window, draw for draw."""
    rng = np.random.default_rng(seed)
    if xy is not None:
        return xy(rng)
    out = []
    for _ in range(B):
        xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
        rng.uniform(0.0, 1.0, n); rng.uniform(0.0, 1.0, (R, H, W))
        out.append(LP.tile_counts(xs, ys, H, W))
    return np.stack(out)


def _sparse_dense(rng):
    xs = np.concatenate([rng.integers(0, 32, 200_000), rng.integers(0, 224, 34_000)])
    ys = np.concatenate([rng.integers(0, 32, 200_000), rng.integers(0, 160, 34_000)])
    return LP.tile_counts(xs, ys, 160, 224)[None]


# the three batches whose numbers tests/test_gpu_launch_policy.py pins: (shape, evaluations (vmax, theta shape, pinned fields))
PINNED = {
    'bench': (dict(H=260, W=346, R=5, B=8), _uniform_counts(1, 260, 346, 1_000_000, 5, 8), [
        (None, (1, 1), dict(seg_splat=16384, seg_gather_2dof=16384, seg_splat_short=8192, pitch_policy=1, span_splat=1.0, cap_splat=0)),
        (20.0, (1, 1), dict(cap_splat=4608, cap_gather_2dof=4608, pitch_aligned=1, splat_short=0)),
        (29.0, (1, 1), dict(cap_splat=4608, pitch_aligned=0)),
        (117.0, (1, 1), dict(splat_short=1)),
        (6.0, (4, 4), dict(cap_splat=2304, cap_gather=4608, pitch_aligned=0)),
        (24.0, (4, 4), dict(cap_splat=4608, pitch_aligned=1))]),
    'several': (dict(H=96, W=96, R=5, B=1), _uniform_counts(2, 96, 96, 5_000_000, 5, 1), [
        (None, (1, 1), dict(seg_splat=8192, seg_gather_2dof=8192, seg_splat_short=0, pitch_policy=0, seg_gather=16384)),
        (20.0, (4, 4), dict(cap_splat=2304, pitch_aligned=0))]),
    'sparse': (dict(H=160, W=224, R=3, B=1), _uniform_counts(3, 160, 224, 0, 3, 1, _sparse_dense), [
        (None, (1, 1), dict(span_splat=1.0, span_gather=1.0, span_gather_2dof=1.0)),
        (25.0, (4, 4), dict(cap_splat=4608))]),
}
PINNED_CASES = []
for _name, (_shape, _counts, _evals) in PINNED.items():
    for _k, (_v, _hw, _want) in enumerate(_evals):
        PINNED_CASES.append((_policy_case(f'pinned-{_name}-{_k}', _counts, _shape['H'], _shape['W'], _shape['R'], _shape['B'], 1, None, _v, _hw),
                             dict(counts=_counts, rad=1, vmax=_v, two_dof=_hw == (1, 1), pitch_env=None, **_shape), _want))


def test_launch_policy_equals_the_witness(out):
    for name, kw in POLICY + [(n, kw) for n, kw, _ in PINNED_CASES]:
        got = _f(out[name][0])
        want = LP.launch_policy(**kw)
        assert len(got) == len(LP.FIELDS) == 13
        for field, g in zip(LP.FIELDS, got):
            assert g == want[field], (name, field, g, want[field])


def test_pinned_batches_keep_their_numbers(out):
    for name, _, want in PINNED_CASES:
        got = dict(zip(LP.FIELDS, _f(out[name][0])))
        for field, v in want.items():
            assert got[field] == v, (name, field, got[field], v)
    several = dict(zip(LP.FIELDS, _f(out['pinned-several-0'][0])))
    assert several['span_splat'] < 0.02 and several['span_gather'] < 0.04


# ================================================================================================
# launch forms of the event kernels: plan_forms, the one decision that selects the machine code (DESIGN.md sections 5 and 22)
# ================================================================================================
CONST, TILE, POLY = 1, 2, 3                                  # THETA_CONST / THETA_TILE / THETA_POLY (csrc/eincm_types.h)
L_GATHER, L_SPLAT, L_SPLAT_SHORT, L_GATHER_2DOF = range(4)   # ListId
COPY_SPLAT, COPY_GATHER = range(2)                           # EventCopy
SW_CAP = {CONST: 6912, TILE: 4608}                           # SW_CAP_CONST / SW_CAP_TILE
THETA_TILE_BYTES, ACCUM_BYTES, POLY_SCRATCH_BYTES = 32 * 32 * 16, 32 * 32 * 2 * 8, (2 * 32 + 4 * 8) * 8
PH, PW, PR, PB = 120, 160, 3, 3                              # the batches of tests/_switch_probe.py and tests/_weighted_switch_probe.py


def _forms_case(name, *, H=PH, W=PW, R=PR, B=PB, rad=1, weighted=0, wide=0, proj=1, itembase=1, n=(100, 100, 0, 100), all_r=None,
                no_host_asm=0, motion=0, hw=(4, 4), vmax=9.0, want_grad=1, counts=()):
    """n: segments of the gather's, the splat's, the splat's short and the 2-DoF gather's list; counts: the staged tile populations
    instead (wide = -1: as staged)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    return _case(name, 'forms', H, W, R, B, rad, weighted, wide, proj, itembase, *n, -1 if all_r is None else all_r, no_host_asm, motion,
                 hw[0], hw[1], float(vmax), want_grad, *counts.tolist())


def S(mode, rad=1, threads=512, wt=0, lst=L_SPLAT):
    """What a test expects of a SplatForm: the key (mode, rad, threads, weighted) and the list."""
    return (mode, rad, threads, wt), lst


def G(mode, rad=1, wide=0, threads=512, proj=0, all_r=0, wt=0, lst=L_GATHER, copy=COPY_GATHER, wg=PR):
    """... of a GatherForm: the key (mode, rad, wide, threads, proj, all_r, weighted), the list, the event copy, workgroups per segment."""
    return (mode, rad, wide, threads, proj, all_r, wt), lst, copy, wg


def G2(rad=1, wt=0, wg=PR):
    """The 2-DoF gather: 256 threads, its own list on the splat's copy of the events."""
    return G(CONST, rad, 0, 256, 0, 0, wt, L_GATHER_2DOF, COPY_SPLAT, wg)


_case('formrows', 'formrows')
NAMED = {}                             # case name -> (expected SplatForm, expected GatherForm), literals read off the parent's ladders


def _named(name, want_s, want_g, **kw):
    NAMED[_forms_case(name, **kw)] = (want_s, want_g)


# DESIGN.md section 22's table (weighted: wt = 1) with its unweighted twin, on the context of the switch probes: narrow and wide batch
for _wt in (0, 1):
    for _wide in (0, 1):
        _t, _k = f'w{_wt}-wide{_wide}', dict(weighted=_wt, wide=_wide)
        _named(f'forms-2dof-{_t}', S(CONST, wt=_wt), G2(wt=_wt), hw=(1, 1), **_k)
        for _hw in ((4, 4), (16, 16), (8, 8)):         # default run: the in-gather projection
            _named(f'forms-grid{_hw[0]}-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, proj=1, wt=_wt), hw=_hw, **_k)
        _named(f'forms-noproj-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, wt=_wt), proj=0, **_k)                 # EINCM_NO_PROJ_IN_GATHER
        _named(f'forms-allr-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, proj=1, all_r=1, wt=_wt, wg=1), all_r=1, **_k)   # EINCM_GATHER_ALL_R=1
        _named(f'forms-allr-noproj-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, wt=_wt), all_r=1, proj=0, **_k)   # (all_r goes with proj)
        _named(f'forms-allr0-800-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, proj=1, wt=_wt), all_r=0, n=(800, 800, 0, 800), **_k)
        _named(f'forms-800-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, proj=1, all_r=1, wt=_wt, wg=1), n=(800, 800, 0, 800), **_k)
        _named(f'forms-dense-{_t}', S(TILE, wt=_wt), G(TILE, wide=_wide, wt=_wt), hw=(PH, PW), n=(800, 800, 0, 800), **_k)
        _named(f'forms-forward-{_t}', S(TILE, wt=_wt), None, want_grad=0, **_k)
# the fused motion forms: narrow and wide, all reference times on and off
for _wide in (0, 1):
    _k = dict(motion=1, wide=_wide, hw=(0, 0))
    _named(f'forms-motion-wide{_wide}', S(POLY), G(POLY, wide=_wide), **_k)
    _named(f'forms-motion-800-wide{_wide}', S(POLY), G(POLY, wide=_wide, all_r=1, wg=1), n=(800, 800, 0, 800), **_k)
    _named(f'forms-motion-allr-wide{_wide}', S(POLY), G(POLY, wide=_wide, all_r=1, wg=1), all_r=1, **_k)
    _named(f'forms-motion-allr0-wide{_wide}', S(POLY), G(POLY, wide=_wide), all_r=0, n=(800, 800, 0, 800), **_k)
    _named(f'forms-motion-R1-wide{_wide}', S(POLY), G(POLY, wide=_wide, wg=1), R=1, n=(800, 800, 0, 800), **_k)   # (one reference time: nothing to fold)
    _named(f'forms-motion-forward-wide{_wide}', S(POLY), None, want_grad=0, **_k)
# the three other splat windows, at 2-DoF and at a grid: k_splat_r / k_gather_r take neither `wide` nor the projection nor all_r
for _rad in (0, 2, 3):
    _named(f'forms-rad{_rad}-2dof', S(CONST, _rad, 256), G2(_rad), rad=_rad, hw=(1, 1), vmax=150.0)
    _named(f'forms-rad{_rad}-grid', S(TILE, _rad, 256), G(TILE, _rad, 0, 256), rad=_rad, vmax=150.0)
    _named(f'forms-rad{_rad}-grid-wide-allr', S(TILE, _rad, 256), G(TILE, _rad, 0, 256), rad=_rad, wide=1, all_r=1, n=(800, 800, 0, 800))
    _named(f'forms-rad{_rad}-dense', S(TILE, _rad, 256), G(TILE, _rad, 0, 256), rad=_rad, hw=(PH, PW))
# the cells of tests/_launch_policy_cases.py, unweighted and weighted (tests/test_gpu_launch_policy_parity.py,
# tests/test_gpu_event_weights_cells.py): 2-DoF on the long and on the short list; every grid has 700 gather segments and more
for _c in C.CASES:
    for _wt in (0, 1):
        _k = dict(H=C.H, W=C.W, R=C.R, B=C.B, weighted=_wt, wide=-1, hw=_c.hw, vmax=_c.v, counts=C.counts(_c.batch))
        if _c.two_dof:
            _named(f'forms-cell-{_c.id}-w{_wt}', S(CONST, wt=_wt, lst=L_SPLAT_SHORT if _c.list == 'short' else L_SPLAT), G2(wt=_wt, wg=C.R), **_k)
        else:
            _named(f'forms-cell-{_c.id}-w{_wt}', S(TILE, wt=_wt), G(TILE, proj=1, all_r=1, wt=_wt, wg=1), **_k)

# closure: everything the entry points accept, on a small sensor
SWEEP = []
_E = None


def _refused(shape, weighted, rad):
    """What check_staging / eincm_set_splat_window (engine.event_weights_refusal) and motion_fused_supported (engine.motion_fused_refusal) refuse."""
    global _E
    if _E is None:
        import importlib
        _E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    size = 2 * rad + 1
    if weighted and _E.event_weights_refusal('fp32', size) is not None:
        return True
    return shape == 'motion' and _E.motion_fused_refusal('fp32', size, _E.make_params(20.0, 35.0, 0.0, 0.0, 2), bool(weighted)) is not None


SWEEP_HW = {'identity': (40, 48), '2dof': (1, 1), 'grid': (2, 2), 'motion': (0, 0)}
for _shape, _hw in SWEEP_HW.items():
    for _wt in (0, 1):
        for _rad in (0, 1, 2, 3):
            if _refused(_shape, _wt, _rad):
                continue
            for _wide in (0, 1):
                for _proj in (0, 1):
                    for _allr in (None, 0, 1):
                        for _n in (699, 700, 701):
                            for _wg in (0, 1):
                                for _v in (3.0, 200.0):
                                    SWEEP.append(_forms_case(
                                        f'sweep-{_shape}-w{_wt}-r{_rad}-wide{_wide}-p{_proj}-a{_allr}-n{_n}-g{_wg}-v{_v:g}', H=40, W=48, R=3, B=2,
                                        rad=_rad, weighted=_wt, wide=_wide, proj=_proj, n=(_n, 50, 50, 50), all_r=_allr,
                                        motion=int(_shape == 'motion'), hw=_hw, vmax=_v, want_grad=_wg))


def _form(parts):
    """The checker's line as (splat, gather, plan) dicts; gather None where none was planned."""
    s = dict(zip(('mode', 'rad', 'threads', 'weighted', 'row', 'lds', 'list', 'wincap', 'winmaxw'), _i(parts[0]).tolist()))
    g = dict(zip(('mode', 'rad', 'wide', 'threads', 'proj', 'all_r', 'weighted', 'row', 'lds', 'list', 'copy', 'wg', 'wincap', 'winmaxw', 'pal'),
                 _i(parts[1]).tolist()))
    p = dict(zip(('wincap', 'winmaxw', 'wincap_a', 'winmaxw_a', 'pal', 'cap_2', 'maxw_2', 'pal_2', 'splat_short', 'proj', 'all_r', 'host_asm'),
                 _i(parts[2]).tolist()))
    s['key'] = tuple(s[k] for k in ('mode', 'rad', 'threads', 'weighted'))
    g['key'] = tuple(g[k] for k in ('mode', 'rad', 'wide', 'threads', 'proj', 'all_r', 'weighted'))
    return s, (g if g['row'] >= 0 or any(g['key']) else None), p


def _rows(out):
    """The four form lists as lists of key tuples: k_splat's, k_splat_r's, k_gather's, k_gather_r's."""
    sp, spr, ga, gar = out['formrows']
    return [[tuple(r) for r in _i(part).reshape(-1, n).tolist()] for part, n in ((sp, 4), (spr, 4), (ga, 7), (gar, 7))]


def _check_form(name, s, g, p, rows):
    """What must hold of every planned form: it is a row of its family's list, at that row; its threads, LDS bytes and window
    geometry are the ones the parent's launch code computed beside its ladders."""
    sp, spr, ga, gar = rows
    fam = sp if s['rad'] == 1 else spr
    assert 0 <= s['row'] < len(fam) and fam[s['row']] == s['key'], (name, s)
    tile = 0 if s['mode'] == CONST else THETA_TILE_BYTES
    scratch = POLY_SCRATCH_BYTES if s['mode'] == POLY else 0
    if s['rad'] == 1:
        assert s['threads'] == 512 and (s['wincap'], s['winmaxw']) == (p['wincap'], p['winmaxw']), (name, s, p)
        assert s['lds'] == s['wincap'] * 4 + tile + scratch, (name, s)
    else:                              # u64 windows, capped to fit beside the Theta tile; the plan keeps the uncapped capacity
        assert s['threads'] == 256 and s['wincap'] == min(p['wincap'], SW_CAP[s['mode']]), (name, s, p)
        assert s['winmaxw'] == max(40, round(math.sqrt(s['wincap'] * 1.4))) and s['lds'] == s['wincap'] * 8 + tile, (name, s)
    assert s['lds'] <= 65536 and s['list'] == (L_SPLAT_SHORT if p['splat_short'] else L_SPLAT), (name, s, p)
    if g is None:
        return
    fam = ga if g['rad'] == 1 else gar
    assert 0 <= g['row'] < len(fam) and fam[g['row']] == g['key'], (name, g)
    two_dof = g['mode'] == CONST
    assert g['threads'] == (256 if two_dof or g['rad'] != 1 else 512), (name, g)
    want_geom = (p['cap_2'], p['maxw_2'], p['pal_2']) if two_dof else (p['wincap_a'], p['winmaxw_a'], p['pal'])
    assert (g['wincap'], g['winmaxw'], g['pal']) == want_geom, (name, g, p)
    assert g['lds'] == g['wincap'] * 4 + (0 if two_dof else ACCUM_BYTES + THETA_TILE_BYTES) + scratch and g['lds'] <= 65536, (name, g)
    assert (g['list'], g['copy']) == ((L_GATHER_2DOF, COPY_SPLAT) if two_dof else (L_GATHER, COPY_GATHER)), (name, g)
    assert g['proj'] == p['proj'] and g['all_r'] == p['all_r'], (name, g, p)


def test_the_form_lists_are_the_instantiations_of_the_library(out):
    """5 k_splat, 6 k_splat_r, 18 k_gather and 6 k_gather_r kernels, as the parent's code object holds them (profiles/launch_forms.md)."""
    sp, spr, ga, gar = _rows(out)
    assert sorted(sp) == sorted([(m, 1, 512, wt) for m in (CONST, TILE) for wt in (0, 1)] + [(POLY, 1, 512, 0)])
    assert sorted(spr) == sorted((m, r, 256, 0) for m in (CONST, TILE) for r in (0, 2, 3))
    assert sorted(ga) == sorted([(CONST, 1, 0, 256, 0, 0, wt) for wt in (0, 1)] +
                                [(TILE, 1, wide, 512, pr, ar, wt) for wide in (0, 1) for pr, ar in ((0, 0), (1, 0), (1, 1)) for wt in (0, 1)] +
                                [(POLY, 1, wide, 512, 0, ar, 0) for wide in (0, 1) for ar in (0, 1)])
    assert sorted(gar) == sorted((m, r, 0, 256, 0, 0, 0) for m in (CONST, TILE) for r in (0, 2, 3))
    for fam in (sp, spr, ga, gar):
        assert len(set(fam)) == len(fam)


def test_named_cells_take_their_forms(out):
    rows = _rows(out)
    for name, (want_s, want_g) in NAMED.items():
        s, g, p = _form(out[name])
        assert (s['key'], s['list']) == want_s, (name, s, want_s)
        if want_g is None:
            assert g is None, (name, g)
        else:
            assert g is not None and (g['key'], g['list'], g['copy'], g['wg']) == want_g, (name, g, want_g)
        _check_form(name, s, g, p, rows)
    # the capped window of k_splat_r lives in the form alone
    for rad in (0, 2, 3):
        s, _, p = _form(out[f'forms-rad{rad}-grid'])
        assert p['wincap'] == 6912 and s['wincap'] == 4608
        s, _, p = _form(out[f'forms-rad{rad}-2dof'])
        assert p['wincap'] == s['wincap'] == 6912
    # the launch-policy cells: the splat's capacity class and pitch are the case's
    for c in C.CASES:
        s, g, p = _form(out[f'forms-cell-{c.id}-w0'])
        assert s['wincap'] == c.cap and p['pal'] == int(c.aligned), (c.id, s, p)


def test_every_reachable_form_is_a_row_and_every_row_is_reached(out):
    rows = _rows(out)
    reached = [set(), set(), set(), set()]
    assert len(SWEEP) > 2000
    for name in SWEEP:
        s, g, p = _form(out[name])
        _check_form(name, s, g, p, rows)
        assert (g is not None) == name.split('-')[8].endswith('1'), name       # a gather form exactly for a gradient evaluation
        reached[0 if s['rad'] == 1 else 1].add(s['key'])
        if g is not None:
            reached[2 if g['rad'] == 1 else 3].add(g['key'])
    for fam, got in zip(rows, reached):
        assert got == set(fam), (sorted(set(fam) - got), sorted(got - set(fam)))


def test_a_refused_combination_has_no_row(out):
    """Weights or a motion model with another splat window, weights with a motion model: the entry points refuse them, and the plan
    names no kernel for them (row -1: the launch reports it instead of running some kernel)."""
    for name in ('refused-weighted-rad2', 'refused-motion-rad2', 'refused-weighted-motion'):
        s, g, _ = _form(out[name])
        assert s['row'] == -1 and g is not None and g['row'] == -1, (name, s, g)


_forms_case('refused-weighted-rad2', weighted=1, rad=2)
_forms_case('refused-motion-rad2', motion=1, rad=2, hw=(0, 0))
_forms_case('refused-weighted-motion', weighted=1, motion=1, hw=(0, 0))


# ================================================================================================
# segment cut
# ================================================================================================
CUTS = {}                              # name -> (counts (nbins,), ntiles, seg)


def _cut_case(name, counts, ntiles, seg, want_items=True):
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    CUTS[name] = (counts, ntiles, seg, want_items)
    _case(name, 'cut', seg, ntiles, int(counts.sum()), want_items, *counts.tolist())


for _H, _W in ((33, 31), (260, 346), (480, 640)):
    for _B in (1, 3, 16):
        _rng = np.random.default_rng(_H * 100 + _B)
        _nt = int(np.prod(LP.tiles_of(_H, _W)))
        _seg = int(_rng.choice([64, 256, 4096]))
        # empty tiles, sparse ones, tiles near one segment and tiles of several
        _pop = np.where(_rng.random((_B, _nt)) < 0.3, 0, _rng.integers(1, _seg // 2, (_B, _nt)))
        _pop = np.where(_rng.random((_B, _nt)) < 0.2, _seg + _rng.integers(-2, 3, (_B, _nt)), _pop)
        _pop = np.where(_rng.random((_B, _nt)) < 0.1, _rng.integers(_seg, 9 * _seg, (_B, _nt)), _pop)
        _cut_case(f'cut-{_H}x{_W}-B{_B}', _pop, _nt, _seg)
_cut_case('cut-empty', np.zeros(6), 2, 4096)
_cut_case('cut-one-event', [0, 0, 1, 0], 4, 4096)
_cut_case('cut-one-tile', [0, 50_000, 0, 0, 0, 0], 3, 8192)
_cut_case('cut-1e7-seg64', [3, 10_000_000], 2, 64)
_cut_case('cut-1e7-seg2^20', [10_000_000, 0, 5], 3, 1 << 20)
_cut_case('cut-counts-only', [10_000_000, 70_000], 2, 16384, want_items=False)
for _seg in (64, 1 << 20):
    _cut_case(f'cut-exactly-seg{_seg}', [_seg, 0, _seg + 1, _seg - 1], 2, _seg)
_cut_case('cut-3pc-hit', [9700 * 2, 300, 300], 3, 8192)
_cut_case('cut-3pc-missed', [9699 * 2, 301, 301], 3, 8192)


@pytest.mark.parametrize('name', list(CUTS))
def test_segment_cut(out, name):
    counts, ntiles, seg, want_items = CUTS[name]
    head, lens, order, win_item0, items = out[name]
    n, tspan = int(head[0]), float(head[1])
    lens, order, win_item0, items = _i(lens), _i(order), _i(win_item0), _i(items).reshape(-1, 4)
    # every length is min(balanced_seg_len, what is left of the bin), the segments of a bin partition it in order
    want_lens, bins = [], []
    for idx, c in enumerate(counts.tolist()):
        ln = LP.balanced_seg_len(c, seg)
        k = [min(ln, c - s) for s in range(0, c, ln)]
        want_lens += k; bins += [idx] * len(k)
    want_lens, bins = np.array(want_lens, dtype=np.int64), np.array(bins, dtype=np.int64)
    assert n == len(lens) and np.array_equal(lens, want_lens) and lens.sum() == counts.sum()
    assert (lens <= seg).all() and (lens > 0).all()
    assert np.array_equal(np.bincount(bins, weights=lens, minlength=counts.size).astype(np.int64), counts)
    assert np.array_equal(order, np.argsort(-lens, kind='stable'))           # the stable permutation by decreasing length
    assert tspan == LP.list_span(counts, seg)
    if not want_items:
        assert items.size == 0 and win_item0.size == 0
        return
    assert np.array_equal(items[:, 0], bins // ntiles) and np.array_equal(items[:, 1], bins % ntiles) and np.array_equal(items[:, 3], lens)
    assert np.array_equal(items[:, 2], np.cumsum(lens) - lens)     # bins are contiguous, so the segments are too
    B = counts.size // ntiles
    assert win_item0.size == B + 1 and (np.diff(win_item0) >= 0).all() and win_item0[-1] == n
    assert np.array_equal(win_item0, np.searchsorted(bins // ntiles, np.arange(B + 1)))


def test_span_follows_all_but_three_percent(out):
    assert float(out['cut-3pc-hit'][0][1]) == 1.0 / 3 and float(out['cut-3pc-missed'][0][1]) == 1.0
    assert float(out['cut-empty'][0][1]) == 1.0 / 64


# ================================================================================================
# resampling tables
# ================================================================================================
RESAMPLE = [(h, h, 260, 346) for h in (1, 2, 4, 16)] + [(33, 33, 33, 33), (40, 40, 31, 31), (3, 40, 33, 31)]
for _m, _mi in METHODS.items():
    for _h, _w, _H, _W in RESAMPLE:
        _case(f'resample-{_m}-{_h}x{_w}-{_H}x{_W}', 'resample', _mi, _h, _w, _H, _W)
        _case(f'taps-{_m}-{_h}x{_w}-{_H}x{_W}', 'taps', _mi, _h, _w, _H, _W)
FITS_SENSOR = (64, 96)
for _k in range(1, 41):
    _case(f'fits-{_k}', 'resample', 0, _k, _k, *FITS_SENSOR)


def _extents(A):
    """(lo, hi) of the non-zero entries of every row of A; (0, 0) for a row of zeros."""
    nz = A != 0.0
    lo, hi = nz.argmax(axis=1), A.shape[1] - nz[:, ::-1].argmax(axis=1)
    some = nz.any(axis=1)
    return np.where(some, lo, 0), np.where(some, hi, 0)


def _tile_ranges(rows, cols, H, W):
    ty, tx = LP.tiles_of(H, W)
    out = []
    for y0 in range(0, ty * LP.TS, LP.TS):
        for x0 in range(0, tx * LP.TS, LP.TS):
            q = []
            for (lo, hi), s in ((rows, slice(y0, min(y0 + LP.TS, H))), (cols, slice(x0, min(x0 + LP.TS, W)))):
                lo, hi = lo[s][hi[s] > lo[s]], hi[s][hi[s] > lo[s]]
                q += [int(lo.min()), int(hi.max() - lo.min())] if lo.size else [0, 0]
            out.append(q)
    return np.array(out, dtype=np.int64)


def _check_tables(parts, method, h, w, H, W):
    AH, AW = _f(parts[0]).reshape(H, h), _f(parts[1]).reshape(W, w)
    assert np.abs(AH - O.resample_matrix(h, H, H / h, method)).max() <= 1e-15
    assert np.abs(AW - O.resample_matrix(w, W, W / w, method)).max() <= 1e-15
    rows, cols = _extents(AH), _extents(AW)
    assert np.array_equal(_i(parts[2]).reshape(H, 2), np.stack(rows, axis=1))
    assert np.array_equal(_i(parts[3]).reshape(W, 2), np.stack(cols, axis=1))
    tr = _tile_ranges(rows, cols, H, W)
    assert np.array_equal(_i(parts[4]).reshape(-1, 4), tr)
    fits = bool((tr[:, 1] <= PG_MAXC).all() and (tr[:, 3] <= PG_MAXC).all())
    assert int(parts[5][0]) == fits
    return AH, AW, rows, cols, fits


@pytest.mark.parametrize('method', list(METHODS))
def test_resample_tables(out, method):
    for h, w, H, W in RESAMPLE:
        AH, AW, rows, cols, _ = _check_tables(out[f'resample-{method}-{h}x{w}-{H}x{W}'], method, h, w, H, W)
        # build_taps: the same extents as runs (lo, count) and the weights padded to the longest run, out of one packed block
        strides, rlo, rcnt, clo, ccnt, rw, cw = out[f'taps-{method}-{h}x{w}-{H}x{W}']
        rstride, cstride = int(strides[0]), int(strides[1])
        for A, (lo, hi), glo, gcnt, gw, stride in ((AH, rows, rlo, rcnt, rw, rstride), (AW, cols, clo, ccnt, cw[:-1], cstride)):
            assert np.array_equal(_i(glo), lo) and np.array_equal(_i(gcnt), hi - lo) and stride == max(1, int((hi - lo).max()))
            want = np.zeros((A.shape[0], stride))
            for o in range(A.shape[0]):
                want[o, :hi[o] - lo[o]] = A[o, lo[o]:hi[o]]
            assert np.array_equal(_f(gw).reshape(A.shape[0], stride), want)
        assert int(cw[-1]) == 8 * (H * rstride + W * cstride) + 8 * (H + W)          # the block holds exactly the six tables


def test_fits_flag_flips_at_pg_maxc(out):
    H, W = FITS_SENSOR
    fits = [_check_tables(out[f'fits-{k}'], 'bilinear', k, k, H, W)[4] for k in range(1, 41)]
    over = fits.index(False) + 1                                   # the first grid with more than PG_MAXC cells under a tile
    assert over > 2 and all(fits[:over - 1])
    most = [max(tr[:, 1].max(), tr[:, 3].max()) for tr in (_i(out[f'fits-{k}'][4]).reshape(-1, 4) for k in (over - 1, over))]
    assert most[0] <= PG_MAXC < most[1]


# ================================================================================================
# host binning
# ================================================================================================
BINS = {}


def _bin_case(name, H, W, R, windows, edge_ts):
    """windows: a list of (xs, ys, ts) per window."""
    BINS[name] = (H, W, R, windows, np.asarray(edge_ts, dtype=np.float64))
    ev = [v for xs, ys, ts in windows for x, y, t in zip(xs, ys, ts) for v in (int(x), int(y), repr(float(t)))]
    _case(name, 'bin', H, W, R, len(windows), *[len(w[0]) for w in windows], *[float(v) for v in np.ravel(edge_ts)], *ev)


def _events(rng, H, W, n):
    xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
    k = n // 4
    xs[:k], ys[:k] = xs[k:2 * k], ys[k:2 * k]                          # repeated pixels
    xs[-4:], ys[-4:] = [0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1]      # the corners
    p = rng.permutation(n)
    return xs[p], ys[p], np.sort(rng.uniform(-0.2, 1.3, n))


_EMPTY = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
for _H, _W in ((33, 31), (70, 100)):
    _rng = np.random.default_rng(_H)
    _wins = [_events(_rng, _H, _W, 300), _EMPTY, _events(_rng, _H, _W, 1000), _EMPTY, _EMPTY, _events(_rng, _H, _W, 40)]
    _ets = _rng.uniform(0.0, 1.0, (len(_wins), 3))
    _bin_case(f'bin-{_H}x{_W}', _H, _W, 3, _wins, _ets)
    _bin_case(f'bin-{_H}x{_W}-none', _H, _W, 3, [_EMPTY, _EMPTY], _ets[:2])
    # refusals: the first one wins, at its own (window, index); an outside event before a NaN timestamp and the other way round
    for _k, (_bad_xy_at, _bad_t_at, _xy) in enumerate((((2, 17), (2, 400), (_W, 3)), ((5, 30), (2, 9), (-1, 0)), ((2, 0), None, (4, _H)),
                                                       (None, (5, 39), None))):
        _w = [tuple(np.array(a, dtype=np.float64 if a.dtype.kind == 'f' else np.int64) for a in w) for w in _wins]
        if _bad_xy_at:
            _w[_bad_xy_at[0]][0][_bad_xy_at[1]], _w[_bad_xy_at[0]][1][_bad_xy_at[1]] = _xy
        if _bad_t_at:
            _w[_bad_t_at[0]][2][_bad_t_at[1]] = (np.nan, np.inf, -np.inf, np.nan)[_k]
        _first = min(p for p in (_bad_xy_at, _bad_t_at) if p)
        _bin_case(f'refuse-{_H}x{_W}-{_k}', _H, _W, 3, _w, _ets)
        BINS[f'refuse-{_H}x{_W}-{_k}'] += ((_first[0], _first[1], 1 if _first == _bad_xy_at else 0),)


@pytest.mark.parametrize('name', [n for n in BINS if n.startswith('bin-')])
def test_host_binning(out, name):
    H, W, R, wins, edge_ts = BINS[name]
    _, counts, sxy, st, cntmax, dtmax = out[name]
    assert out[name][0] == ['ok']
    tx = LP.tiles_of(H, W)[1]
    want_xy, want_t, want_counts, want_cm, want_dt = [], [], [], [], []
    for b, (xs, ys, ts) in enumerate(wins):
        tile = (ys // LP.TS) * tx + xs // LP.TS
        p = np.argsort(tile, kind='stable')                          # windows are concatenated in order: the sort by (window, tile)
        want_xy.append((xs | (ys << 16))[p]); want_t.append(ts[p])
        want_counts.append(LP.tile_counts(xs, ys, H, W))
        want_cm.append(np.bincount(ys * W + xs).max() if xs.size else 0)
        want_dt.append(np.abs(ts[:, None] - edge_ts[b][None, :]).max() if xs.size else 0.0)
    assert np.array_equal(_i(counts), np.concatenate(want_counts))
    assert np.array_equal(_i(sxy), np.concatenate(want_xy)) and np.array_equal(_f(st), np.concatenate(want_t))
    assert np.array_equal(_i(cntmax), want_cm) and np.array_equal(_f(dtmax), want_dt)
    if sum(len(w[0]) for w in wins):
        assert max(want_cm) > 1 and min(want_cm) == 0


@pytest.mark.parametrize('name', [n for n in BINS if n.startswith('refuse-')])
def test_host_binning_reports_the_first_refused_event(out, name):
    win, index, bad_xy = BINS[name][5]
    assert out[name][0] == ['refused', str(win), str(index), str(bad_xy)]


def test_edge_moments(out):
    f = _f(out['edges'][1]).astype(np.float32)
    assert np.array_equal(f, EDGE_VALUES.astype(np.float32))
    d = f.astype(np.float64)
    got = _f(out['edges'][0])
    assert got[0] == pytest.approx(d.sum(), rel=1e-14) and got[1] == pytest.approx((d * d).sum(), rel=1e-14) and got[2] == np.abs(d).max()


EDGE_VALUES = np.random.default_rng(5).normal(0.0, 3.0, 33 * 31)
_case('edges', 'edges', *EDGE_VALUES.tolist())


# ================================================================================================
# small functions
# ================================================================================================
for _R in range(1, 17):
    _case(f'mrw-{_R}', 'mrw', _R)
# the largest window a float64 staging accepts (check_staging: f64_ishift >= 40), the first it refuses, the largest eincm_create allows
ISHIFT = (1, 6, 7, 1 << 20, 26_353_589, 26_353_590, 2_000_000_000)
for _n in ISHIFT:
    _case(f'ishift-{_n}', 'ishift', _n)
for _tw in (1, 3, 7, 8, 21):
    _case(f'nlm-{_tw}', 'nlm', _tw)
PACK = ((3, 1), (8, 8), (0, 4), (5, 4), (0, 1), (16, 8), (1, 256))
_case('packer', 'packer', *[v for p in PACK for v in p])


def test_multi_ref_weights(out):
    for R in range(1, 17):
        assert np.abs(_f(out[f'mrw-{R}'][0]) - O.compute_weights_for_multi_reference(R)).max() <= 1e-15


def test_f64_ishift_and_nlm_shift(out):
    for n in ISHIFT:
        bound = max(1.0, n * 0.15915494309189535)
        assert int(out[f'ishift-{n}'][0][0]) == min(52, 62 - math.ceil(math.log2(bound))), n
    assert [int(out[f'ishift-{n}'][0][0]) for n in (1, 1 << 20, 26_353_589, 26_353_590)] == [52, 44, 40, 39]
    for tw in (1, 3, 7, 8, 21):
        s = int(out[f'nlm-{tw}'][0][0])
        assert (1 << s) >= tw * tw and (s == 0 or (1 << (s - 1)) < tw * tw)


def test_packer_offsets_and_padding(out):
    offs, (block,) = out['packer']
    buf = bytes.fromhex(block)
    want, end = bytearray(), 0
    for k, ((n, align), off) in enumerate(zip(PACK, _i(offs)), 1):
        assert off == -(-end // align) * align                       # the next multiple of align
        want += bytes(off - len(want)) + bytes([k]) * n              # zero padding, then the piece
        end = off + n
    assert buf == bytes(want) and len(buf) == end
