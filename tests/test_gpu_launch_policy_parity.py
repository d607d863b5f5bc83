"""Value parity of every cell of the event kernels' launch policy (the table "cells of the launch policy").

tests/test_gpu_launch_policy.py pins which cell the library picks; this module checks what the kernels compute there.  Two batches
of 16 windows (tests/_launch_policy_cases.py) are staged once per binning mode - on the device, and on the host, which builds the
segment lists and the short list itself and fills the window tables by k_windows - and evaluated at thetas chosen to sit in one cell
each: the long and the short splat list, the four LDS capacity classes, windows at the bank-aligned pitch and at pitch = width,
windows that fill their class exactly, windows clamped to a multiple of 32 words, and thetas no window holds.

Every case first asserts that eincm_get_launch_policy equals the numpy witness (tests/_launch_policy_witness.py) field by field,
so that no case passes in another cell than the one it is named for (tests/test_launch_policy_witness.py holds the names to the
witness on the CPU).  Then every window is compared with the C port of the oracle at gamma = delta = 0, as
tests/test_gpu_fullsize.py::check_window does: value, IWE stack and dL/dIWE at 1e-5; the gradient at 1e-5 where the windows of the
long list hold the theta and at 5e-5 where they do not (the bar of
tests/test_gpu_parity.py::test_huge_displacement_takes_the_direct_path).

The tests are ordered case by case with both binning modes of a case next to each other, and the C port's results are kept for
the last (batch, theta) only: all of them at once would be 4 GB of float64 images.
"""
import importlib
import os

import numpy as np
import pytest

import _launch_policy_cases as C
import _launch_policy_witness as LP
from oracle import eincm_c_port as CP
from oracle import eincm_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5                     # value, IWE stack, dL/dIWE; the gradient where the long list's windows hold the theta
TOL_GRAD_DIRECT = 5e-5         # the gradient where they do not
TOL_SAME_V, TOL_SAME_G = 1e-6, 2e-5        # between two configurations of the library (tests/test_gpu_switches.py)

engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')

NTHREADS = min(os.cpu_count() or 1, 16)
ENV = ('EINCM_HOST_BINNING', 'EINCM_WINCAP', 'EINCM_PITCH_ALIGNED', 'EINCM_SEG', 'EINCM_SEG_SPLAT', 'EINCM_SEG_2DOF')


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def params(case, **kw):
    return engine.make_params(C.ALPHA, C.BETA, 0.0, 0.0, case.lvl, **kw)


def stage(batch, binning='device', wincap=None, pitch=None, splat_window=None):
    """A context with the batch staged.  EINCM_HOST_BINNING and EINCM_WINCAP are read when the context is created,
    EINCM_PITCH_ALIGNED at every staging."""
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)
        if binning == 'host':
            mp.setenv('EINCM_HOST_BINNING', '1')
        if wincap is not None:
            mp.setenv('EINCM_WINCAP', str(wincap))
        if pitch is not None:
            mp.setenv('EINCM_PITCH_ALIGNED', str(pitch))
        eng = engine.Engine((C.H, C.W), sum(len(w['xs']) for w in C.batch(batch)), max_refs=C.R, max_windows=C.B)
        try:
            if splat_window is not None:
                eng.set_splat_window(splat_window)
            eng.set_windows([C.win_args(w) for w in C.batch(batch)])
        except Exception:
            eng.close()
            raise
    return eng


@pytest.fixture(scope='module')
def staged(built_lib):
    """staged(batch, binning, wincap) -> the context of that configuration, staged once for the module."""
    made = {}

    def get(batch, binning='device', wincap=None):
        key = (batch, binning, wincap)
        if key not in made:
            made[key] = stage(batch, binning, wincap)
        return made[key]
    yield get
    for e in made.values():
        e.close()


_REF = {}


def reference(case):
    """The C port's (value, gradient, IWE stack, dL/dIWE) of every window at the case's theta; the last case's are kept."""
    if case.id not in _REF:
        _REF.clear()
        th = C.theta(case)
        out = []
        for b, win in enumerate(C.batch(case.batch)):
            v, g, im = CP.loss_and_grad(th[b], *C.win_args(win), C.ALPHA, C.BETA, (C.H, C.W), nthreads=NTHREADS, return_images=True)
            out.append((v, g, im['iwes'], im['G']))
        _REF[case.id] = out
    return _REF[case.id]


def assert_policy(eng, batch, vmax, two_dof, rad=1, pitch_env=None):
    """The library's thirteen fields against the witness, field by field; returns the witness's evaluation half."""
    pol = eng.launch_policy()
    wit = LP.launch_policy(C.counts(batch), C.H, C.W, C.R, C.B, rad=rad, vmax=vmax, two_dof=two_dof, pitch_env=pitch_env)
    assert set(pol) == set(LP.FIELDS)
    for k in LP.FIELDS:
        assert pol[k] == wit[k], (k, pol[k], wit[k])
    return LP.eval_policy(LP.stage_policy(C.counts(batch), C.H, C.W, C.R, C.B, pitch_env), vmax, two_dof, rad)


def check_against_port(tag, case, v, g, iwes, G, long_fits):
    ref = reference(case)
    err = np.array([[abs(v[b] - r[0]) / abs(r[0]), rel(g[b], r[1]), rel(iwes[b], r[2]), rel(G[b], r[3])] for b, r in enumerate(ref)])
    worst = err.max(axis=0)
    print(f'CELL {tag} list={case.list} cap={case.cap} aligned={int(case.aligned)} fits={int(case.fits)} '
          f'value={worst[0]:.2e} grad={worst[1]:.2e} iwe={worst[2]:.2e} G={worst[3]:.2e} |g|={max(np.abs(r[1]).max() for r in ref):.2e}')
    tol_g = TOL if long_fits else TOL_GRAD_DIRECT
    for b, e in enumerate(err):
        assert e[0] <= TOL, (tag, b, 'value', e[0])
        assert e[2] <= TOL, (tag, b, 'iwes', e[2])
        assert e[3] <= TOL, (tag, b, 'G', e[3])
        assert e[1] <= tol_g, (tag, b, 'grad', e[1], tol_g)


PARITY = [(c, m) for c in C.CASES for m in ('device', 'host')]


@pytest.mark.parametrize('case,binning', PARITY, ids=[f'{c.id}-{m}' for c, m in PARITY])
def test_cell_parity(staged, case, binning):
    eng = staged(case.batch, binning)
    th = C.theta(case)
    v, g, _ = eng.loss_grad(th, params(case))
    ev = assert_policy(eng, case.batch, np.abs(th).max(), case.two_dof)
    assert (ev['splat_short'] == 1) == (case.list == 'short') and ev['splat']['cap'] == case.cap
    assert ev['splat']['aligned'] == case.aligned and ev['splat']['fits'] == case.fits
    check_against_port(f'{case.id}-{binning}', case, v, g, eng.iwes(), eng.image_grad(), ev['long_fits'])


@pytest.mark.parametrize('v', [56, 70])
def test_aligned_two_dof_gather(built_lib, v):
    """EINCM_PITCH_ALIGNED=2: the 2-DoF gather's windows at the bank-aligned pitch too, the clamped ones of the sparse tiles'
    full-span segments included (batch B: 92 px clamp to 64, 106 px to 96)."""
    case = C.BY_ID[f'B-2dof1x1-v{v}']
    eng = stage('B', pitch=2)
    try:
        th = C.theta(case)
        val, g, _ = eng.loss_grad(th, params(case))
        ev = assert_policy(eng, 'B', float(v), True, pitch_env=2)
        assert ev['pitch_aligned'] == 3 and ev['gather_2dof']['aligned'] and ev['gather_2dof']['cap'] == case.cap
        assert C.widest_window(case, 1.0) > ev['gather_2dof']['maxw']
        check_against_port(f'{case.id}-pitch2', case, val, g, eng.iwes(), eng.image_grad(), ev['long_fits'])
    finally:
        eng.close()


def test_device_assembly_and_forward_only(staged):
    """The same theta through k_final + k_theta_const (EINCM_PF_FULL_AUX: scalar assembly on the device instead of the host's) and
    without a gradient, on the short list at 6912 words (A / v = 70)."""
    case = C.BY_ID['A-2dof1x1-v70']
    eng = staged('A')
    th = C.theta(case)
    v, g, _ = eng.loss_grad(th, params(case))
    ev = assert_policy(eng, 'A', case.v, True)
    assert ev['splat_short'] == 1 and ev['cap_splat'] == 6912
    v2, g2, aux = eng.loss_grad(th, params(case, full_aux=True), want_aux=True)
    assert_policy(eng, 'A', case.v, True)
    v3, g3, _ = eng.loss_grad(th, params(case), want_grad=False)
    assert g3 is None
    dv2, dv3 = np.abs(v2 - v) / np.abs(v), np.abs(v3 - v) / np.abs(v)
    dg2 = max(rel(g2[b], g[b]) for b in range(C.B))
    print(f'ROUTE k_final value={dv2.max():.2e} grad={dg2:.2e} forward-only value={dv3.max():.2e}')
    assert dv2.max() <= TOL_SAME_V and dg2 <= TOL_SAME_G
    assert dv3.max() <= TOL_SAME_V
    for b in range(C.B):
        assert aux[b]['final_loss'] == pytest.approx(v2[b], rel=1e-12)


def test_splat_window_five_on_the_short_list(built_lib):
    """Splat window size 5 at A / v = 70: k_splat_r on the short list, margin 6, windows capped at 6912 words; windows 0, 7 and 15
    against the torch float64 witness of the sized splat."""
    import _splat_window_witness as SW
    case = C.BY_ID['A-2dof1x1-v70']
    eng = stage('A', splat_window=5)
    try:
        th = C.theta(case)
        v, g, _ = eng.loss_grad(th, params(case))
        ev = assert_policy(eng, 'A', case.v, True, rad=2)
        assert ev['splat_short'] == 1 and ev['cap_splat'] == 6912 and ev['splat']['side'] == 73 and not ev['long_fits']
        iwes, G = eng.iwes(), eng.image_grad()
    finally:
        eng.close()
    for b in (0, 7, 15):
        win = [np.array(a) for a in C.win_args(C.batch('A')[b])]            # (writable copies: torch.as_tensor)
        v_w, g_w, G_w, I_w, _ = SW.loss_and_grad(th[b], *win, C.ALPHA, C.BETA, 0.0, 0.0, case.lvl, np.ones((C.H, 1)),
                                                 np.ones((C.W, 1)), window_size=5)
        e = (abs(v[b] - v_w) / abs(v_w), rel(g[b], g_w), rel(iwes[b], I_w), rel(G[b], G_w))
        print(f'SPLAT5 window {b} value={e[0]:.2e} grad={e[1]:.2e} iwe={e[2]:.2e} G={e[3]:.2e}')
        assert e[0] <= TOL and e[2] <= TOL and e[3] <= TOL, (b, e)
        assert e[1] <= TOL_GRAD_DIRECT, (b, e)


def test_strided_vmax_sampling_misses_the_spikes(built_lib):
    """A dense theta of 24 576 doubles is sampled with stride 3 for max|theta|; its 60 px spikes sit between the samples, so the
    policy sizes the windows for the 4 px field (class 2304) and the spikes' taps leave the windows.  Capacity does not affect
    correctness: the result is the oracle's.  The gradient is held to the direct path's 5e-5, the bar of a theta the windows do
    not hold (the witness at the true maximum: nothing fits)."""
    win, th, stride = C.strided_case()
    Hs, Ws = win['sensor_size']
    Rs = len(win['edge_ts'])
    a = (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])
    v_o, g_o, aux = O.loss_and_grad(th, *a, C.ALPHA, C.BETA, 0.0, 0.0, 0, 5, (Hs, Ws), return_intermediates=True)
    with engine.Engine((Hs, Ws), len(win['xs']), max_refs=Rs) as eng:
        eng.set_window(*a)
        v, g, _ = eng.loss_grad(th, engine.make_params(C.ALPHA, C.BETA, 0.0, 0.0, 0))
        pol = eng.launch_policy()
        iwes, G = eng.iwes(), eng.image_grad()
    sampled = np.abs(th.reshape(-1)[::stride]).max()
    wit = LP.launch_policy(LP.tile_counts(win['xs'], win['ys'], Hs, Ws)[None], Hs, Ws, Rs, 1, vmax=sampled, two_dof=False)
    for k in LP.FIELDS:
        assert pol[k] == wit[k], (k, pol[k], wit[k])
    assert pol['cap_splat'] == 2304
    e = (abs(v[0] - v_o) / abs(v_o), rel(g[0], g_o), rel(iwes[0], aux['_iwes']), rel(G[0], aux['_G']))
    print(f'STRIDED value={e[0]:.2e} grad={e[1]:.2e} iwe={e[2]:.2e} G={e[3]:.2e}')
    assert e[0] <= TOL and e[2] <= TOL and e[3] <= TOL, e
    assert e[1] <= TOL_GRAD_DIRECT, e


@pytest.mark.parametrize('case', C.CASES, ids=[c.id for c in C.CASES])
def test_pinned_capacity_gives_the_same_accumulators(staged, case):
    """EINCM_WINCAP=1024 and 6912 against the automatic policy.  A pinned context walks the long list with every window clamped
    to 1024 words, or none below 83 px: the IWE stack is a sum of integers, so it is bit-identical to the automatic policy's
    wherever that walked the long list too - a tap lost or doubled at a window edge changes it, whatever the float tolerances -
    and equal to 1e-6 where the automatic policy took the short list (other segments: another fixed-point scale per tap).
    Value, gradient and that 1e-6 are the bars and the measure of tests/test_gpu_switches.py between two configurations: max-norm
    relative over the whole batch's array.  Window by window the two lists' IWE stacks differ by up to 1.05e-6 (A / v = 150: a tap
    is rounded to 2^-21 on a 12 000-event segment and to 2^-22 on a 6144-event one, and 150 px of flow smear a tile's events
    so thin that the window's largest pixel is a few taps); the figures of both measures are printed."""
    th = C.theta(case)
    auto = staged(case.batch)
    v0, g0, _ = auto.loss_grad(th, params(case))
    short = assert_policy(auto, case.batch, case.v, case.two_dof)['splat_short'] == 1
    I0 = auto.iwes()
    for cap in (1024, 6912):
        e = staged(case.batch, wincap=cap)
        v, g, _ = e.loss_grad(th, params(case))
        pol = e.launch_policy()
        assert pol['cap_splat'] == cap and pol['cap_gather'] == cap and pol['cap_gather_2dof'] == cap and pol['splat_short'] == 0
        I = e.iwes()
        dv, dg, di = rel(v, v0), rel(g, g0), rel(I, I0)
        print(f'PINNED {case.id} cap={cap} auto_short={int(short)} iwe={di:.2e} value={dv:.2e} grad={dg:.2e} per window: '
              f'iwe={max(rel(I[b], I0[b]) for b in range(C.B)):.2e} grad={max(rel(g[b], g0[b]) for b in range(C.B)):.2e}')
        if short:
            assert di <= TOL_SAME_V, (cap, di)
        else:
            assert np.array_equal(I, I0), (cap, di)
        assert dv <= 2 * TOL_SAME_V and dg <= TOL_SAME_G, (cap, dv, dg)
