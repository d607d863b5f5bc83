"""Theta in and results out at every transport limit (the table of _transport_cases.py, checked against the sources by
test_transport_table.py): every window of a batch against the fp64 oracle, at two thetas, through both scalar assemblies, masked and
asynchronous where a regime has its own handling of those.

Every window has its own events, event count and theta, so that a mixed-up window index, a theta left over from the previous call or a
gradient row that was not written fails.  The windows are uniformly random events (cheap to make at 2049 windows), 2000-3000 per window
so that events * R >= 4096 keeps the gather's wide variant off except in the `tiny` cases.
"""
import importlib

import numpy as np
import pytest

from oracle import eincm_c_port as CP
from oracle import eincm_oracle as O
from _transport_cases import CASES, H, R, W

pytestmark = pytest.mark.gpu

TOL = 1e-5
ALPHA, BETA, GAMMA = 20.0, 35.0, 0.05
N_THREADS = 4          # the C port per (small) window
N_SAMPLE = 200         # windows checked against the oracle in the largest batches
N_AUX = 16             # windows whose aux scalars are checked against the Python oracle

engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')


@pytest.fixture(scope='module', autouse=True)
def _lib(built_lib):
    return built_lib


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_windows(rng, B, tiny=False):
    """B windows of uniformly random events (as test_gpu_launch_policy._window), 2000-3000 each; `tiny`: window B // 2 has 40."""
    wins = []
    for b in range(B):
        n = 40 if (tiny and b == B // 2) else int(rng.integers(2000, 3001))
        xs = rng.integers(0, W, n).astype(np.int16)
        ys = rng.integers(0, H, n).astype(np.int16)
        wins.append((xs, ys, np.sort(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 1.0, (R, H, W)), np.linspace(0.0, 1.0, R)))
    return wins


def make_theta(rng, B, hw):
    """A distinct theta per window: a flow of a few pixels over the window plus per-cell variation."""
    mean = rng.uniform(-6.0, 6.0, (B, 1, 1, 2))
    return mean + rng.uniform(-2.0, 2.0, (B,) + tuple(hw) + (2,)) * (hw != (1, 1))


def other_theta(rng, theta):
    """A second theta that differs from the first in every component by 0.5 to 2 px."""
    return theta + rng.choice([-1.0, 1.0], theta.shape) * rng.uniform(0.5, 2.0, theta.shape)


def sample(B):
    """Every window, or a fixed sample of the largest batches that holds the mask limit (63 | 64) and both ends."""
    if B <= 2 * N_SAMPLE:
        return np.arange(B)
    rng = np.random.default_rng(B)
    fixed = [0, 1, 62, 63, 64, 65, B // 2, B - 2, B - 1]
    rest = rng.choice(np.setdiff1d(np.arange(B), fixed), N_SAMPLE - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, rest]))


def oracle(win, theta, tv):
    if tv:
        v, g, _ = O.loss_and_grad(theta, *win, ALPHA, BETA, GAMMA, 0.0, 0, 5, (H, W))
        return v, g
    return CP.loss_and_grad(theta, *win, ALPHA, BETA, (H, W), nthreads=N_THREADS)


def check_oracle(what, wins, theta, v, g, idx, tv=False):
    bad = []
    for b in idx:
        v_ref, g_ref = oracle(wins[b], theta[b], tv)
        ev = abs(v[b] - v_ref) / abs(v_ref)
        eg = rel(g[b], g_ref)
        if not (ev <= TOL and eg <= TOL):
            bad.append(f'window {b}: value {v[b]!r} (oracle {v_ref!r}, rel {ev:.1e}), gradient rel {eg:.1e}')
    assert not bad, f'{what}: {len(bad)} of {len(idx)} windows disagree with the oracle:\n  ' + '\n  '.join(bad[:8])


def check_aux(what, wins, theta, v, aux, idx, tv=False):
    for b in idx[:: max(1, len(idx) // N_AUX)]:
        v_ref, a_ref = O.loss_func(theta[b], *wins[b], ALPHA, BETA, GAMMA if tv else 0.0, 0.0, 0 if tv else 1, 5, (H, W))
        assert abs(v[b] - v_ref) <= TOL * abs(v_ref), f'{what}: window {b} value {v[b]} vs {v_ref}'
        for k in ('mean_rel_corr', 'mean_rel_contrast'):
            assert abs(aux[b][k] - a_ref[k]) <= TOL * abs(a_ref[k]), f'{what}: window {b} {k} {aux[b][k]} vs {a_ref[k]}'


def mask_of(B):
    """Inactive windows among the first 64 and, with more than 64 windows, from 64 on (those are evaluated all the same)."""
    act = np.ones(B, dtype=bool)
    act[[b for b in (1, 5, 17, 33, 62) if b < B]] = False
    if B > 64:
        act[64] = False
        act[B - 1] = False
    return act


def params(case, full_aux=False):
    if case.tv:
        return engine.make_params(ALPHA, BETA, GAMMA, 0.0, 0, full_aux=full_aux)
    return engine.make_params(ALPHA, BETA, 0.0, 0.0, 1, full_aux=full_aux)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_transport_matches_the_oracle(case):
    rng = np.random.default_rng(1000 + case.B * 7 + case.hw[0] + 3 * case.tv + 5 * case.tiny)
    B, hw = case.B, case.hw
    wins = make_windows(rng, B, case.tiny)
    th1 = make_theta(rng, B, hw)
    th2 = other_theta(rng, th1)
    idx = sample(B)
    p, p_aux = params(case), params(case, full_aux=True)
    with engine.Engine((H, W), sum(len(w[0]) for w in wins), max_refs=R, max_windows=case.cap) as e:
        e.set_windows(wins)
        v1, g1, _ = e.loss_grad(th1, p)
        check_oracle('theta1', wins, th1, v1, g1, idx, case.tv)
        v2, g2, _ = e.loss_grad(th2, p)
        check_oracle('theta2', wins, th2, v2, g2, idx, case.tv)
        # k_final with every auxiliary scalar, right after the default assembly at another theta
        v3, g3, aux3 = e.loss_grad(th1, p_aux, want_aux=True)
        check_oracle('theta1, full_aux', wins, th1, v3, g3, idx, case.tv)
        check_aux('theta1, full_aux', wins, th1, v3, aux3, idx, case.tv)
        v4, g4, aux4 = e.loss_grad(th2, p_aux, want_aux=True)
        check_oracle('theta2, full_aux', wins, th2, v4, g4, idx, case.tv)

        if case.mask:
            # right after a full evaluation at theta2: a row that is not written this time would hold theta2's gradient
            e.loss_grad(th2, p)
            act = mask_of(B)
            vm, gm, _ = e.loss_grad(th1, p, active=act, allow_nonfinite=False)
            honoured = act | (np.arange(B) >= 64)
            skipped = ~honoured
            assert np.array_equal(vm[honoured], v1[honoured]) and np.array_equal(gm[honoured], g1[honoured])
            assert np.all(np.isnan(vm[skipped])) and np.all(gm[skipped] == 0.0)
            v5, g5, _ = e.loss_grad(th1, p)
            assert np.array_equal(v5, v1) and np.array_equal(g5, g1)

        if case.run_async:
            e.loss_grad(th2, p)
            e.loss_grad_async(th1, p)
            va, ga, _ = e.loss_grad_wait()
            assert np.array_equal(va, v1) and np.array_equal(ga, g1)
            if case.mask:
                act = mask_of(B)
                e.loss_grad_async(th1, p, active=act)
                va, ga, _ = e.loss_grad_wait(allow_nonfinite=False)
                honoured = act | (np.arange(B) >= 64)
                assert np.array_equal(va[honoured], v1[honoured]) and np.array_equal(ga[honoured], g1[honoured])
                assert np.all(np.isnan(va[~honoured])) and np.all(ga[~honoured] == 0.0)


@pytest.mark.timeout(600)
def test_restaging_after_a_theta_grid():
    """The window constants of set_windows come from a theta = 0 pass of the 2-DoF route.  After a 16x16 evaluation has filled the pinned
    theta buffer, re-staging 65 windows must still compute them at theta = 0: the zero-warp IWE and every later value depend on them."""
    B = 65
    rng = np.random.default_rng(77)
    first, second = make_windows(rng, B), make_windows(rng, B)
    n_max = max(sum(len(w[0]) for w in first), sum(len(w[0]) for w in second))
    p = engine.make_params(ALPHA, BETA, 0.0, 0.0, 1)
    with engine.Engine((H, W), n_max, max_refs=R, max_windows=B) as e:
        e.set_windows(first)
        e.loss_grad(make_theta(rng, B, (16, 16)), p)
        e.set_windows(second)
        z = e.zero_iwe()
        for b in range(B):
            xs, ys = (np.asarray(a, dtype=np.float64) for a in second[b][:2])
            ref = O.events_to_pdf_frame(xs, ys, (H, W))
            assert rel(z[b], ref) <= TOL, f'window {b}: zero-warp IWE differs from the oracle'
        for hw in ((1, 1), (16, 16)):
            th = make_theta(rng, B, hw)
            v, g, _ = e.loss_grad(th, p)
            check_oracle(f'{hw} after re-staging', second, th, v, g, np.arange(B))
