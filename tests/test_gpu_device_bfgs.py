"""The device-resident BFGS (csrc/eincm_bfgs.hip.h) on the GPU: every step against its written contract
``batch_solver.NumpyBFGSState``, whole minimisations of a device-side objective against SciPy, determinism, and the multi-level solver
with ``bfgs_state='device'`` against ``'host'``."""
import importlib

import numpy as np
import pytest
import scipy.optimize as spo
import torch      # at import, before any fixture loads the engine's library: a torch wheel brings its own HIP runtime under the same soname,
                  # and whichever copy is loaded first serves both; loaded second, torch's finds no GPU

import _bfgs_cases as CASES

pytestmark = pytest.mark.gpu

engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
bsol = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
sol = importlib.import_module('edge-informed-contrast-maximization_amd.solver')
synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
L = engine.L


U = 2.0 ** -53
SHAPES = {2: (1, 1), 30: (3, 5), 128: (8, 8), 130: (5, 13), 512: (16, 16)}
MASKS = {1: [1], 3: [1, 0, 1], 8: [1, 1, 0, 1, 0, 1, 1, 1]}
SENSOR = (32, 40)


def small_engine(B, **kw):
    eng = engine.Engine(SENSOR, 400 * B, max_refs=2, max_windows=B, **kw)
    wins = [synth.make_window(300 + b, SENSOR, 300, 2, flow='constant', flow_mag=1.0) for b in range(B)]
    eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
    return eng


def one_blas_thread():
    """dsymv / dsyr2 on one thread, as the solver's drivers run them"""
    import contextlib
    return bsol.threadpool_limits(limits=1, user_api='blas') if bsol.threadpool_limits is not None else contextlib.nullcontext()


def to_dev(t, a):
    import torch
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    torch.cuda.synchronize()


def snapshot(eng):
    import torch
    ts = eng.bfgs_state_tensors() + eng.bfgs_trial_tensors()
    torch.cuda.synchronize()
    return [t.clone() for t in ts]


def step_bounds(n, H, g, p, gt, alpha):
    """First-order bounds of |device - numpy| for one UPDATE of one window, from the magnitude sums (see test_step_parity)."""
    nu = n * U
    s, y = alpha * p, gt - g
    aH = np.abs(H)
    ys = float(y @ s)
    e_ys = 2 * nu * float(np.abs(y * s).sum())
    Hy = H @ y
    e_Hy = 2 * nu * (aH @ np.abs(y))
    yhy = float(y @ Hy)
    e_yhy = 2 * nu * float(np.abs(y) @ np.abs(Hy)) + float(np.abs(y) @ e_Hy)
    rho = 1.0 / ys
    e_rho = rho * rho * e_ys + 2 * U * abs(rho)
    t = 1.0 + rho * yhy
    e_t = abs(yhy) * e_rho + abs(rho) * e_yhy + 2 * U * (abs(rho * yhy) + abs(t))
    coef = 0.5 * rho * t
    e_coef = 0.5 * (abs(t) * e_rho + abs(rho) * e_t) + 4 * U * abs(coef)
    w = coef * s - rho * Hy
    e_w = np.abs(s) * e_coef + np.abs(Hy) * e_rho + abs(rho) * e_Hy + 4 * U * (np.abs(coef * s) + np.abs(rho * Hy))
    H1 = H + np.outer(s, w) + np.outer(w, s)
    e_H = np.outer(np.abs(s), e_w) + np.outer(e_w, np.abs(s)) + 6 * U * (aH + np.abs(np.outer(s, w)) + np.abs(np.outer(w, s)))
    P1 = -(H1 @ gt)
    e_P = 2 * nu * (np.abs(H1) @ np.abs(gt)) + e_H @ np.abs(gt)
    pn = float(np.linalg.norm(P1))
    gn = float(np.linalg.norm(gt))
    return dict(ys=e_ys, yhy=e_yhy, H=e_H, P=e_P, e_ys_rel=e_ys / abs(ys),
                dphi0=2 * nu * float(np.abs(gt * P1).sum()) + float(np.abs(gt) @ e_P),
                pnorm=(2 * nu * pn * pn + 2 * float(np.abs(P1) @ e_P)) / (2 * pn) + 2 * U * pn,
                pmax=float(e_P.max()), gnorm=(nu + 2 * U) * gn)


@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('n', [2, 30, 128, 130, 512])
def test_step_parity(built_lib, n, B):
    """trial, reduce and accept(UPDATE) of the GPU state against NumpyBFGSState from the same random state: a random symmetric H, gradients
    and steps spanning 1e-6 .. 1e3, some windows masked out.

    Tolerance.  Both sides round every n-term sum once, in their own order; a computed n-term sum differs from the exact one by at most
    n 2^-53 sum|a_i b_i| (any order), so two computed sums differ by at most FACTOR = 2 times that.  The bound is chained to first order
    through the update: y.s -> rho = 1 / y.s, H y (a sum) -> y.Hy (a sum over sums: the inner bound enters weighted by |y|) -> c, w ->
    H' = H + s w^T + w s^T -> P' = -H' Gt (a sum whose terms carry H's bound) -> G.P', |P'|.  Elementwise operations (the same
    operands on both sides up to the bounds above) add 2^-53 of their magnitude per rounding and side.  Nothing here was fitted to
    measured errors; the measured error / bound ratios are printed (worst over these cases: DESIGN.md section 17).  The trial point,
    max|G| and max|X| involve no sum: bit for bit.  H' is bit-symmetric; windows outside the mask keep every bit of their state."""
    import torch
    rng = np.random.default_rng(1000 * n + B)
    h, w = SHAPES[n]
    mask = np.array(MASKS[B], bool)
    x0 = rng.standard_normal((B, n))
    gs, al = 10.0 ** rng.uniform(-6, 3, B), 10.0 ** rng.uniform(-6, 3, B)
    G = rng.standard_normal((B, n)) * gs[:, None]
    Gt = G + rng.standard_normal((B, n)) * gs[:, None]
    P = rng.standard_normal((B, n)) * 10.0 ** rng.uniform(-3, 1, B)[:, None]
    A = rng.standard_normal((B, n, n))
    Hs = 0.5 * (A + A.transpose(0, 2, 1)) + np.eye(n)
    ratios = {}

    def check(name, dev, ref, bound):
        err = np.abs(np.asarray(dev) - np.asarray(ref))
        bound = np.asarray(bound, dtype=np.float64)
        assert np.all(err <= bound), (name, n, B, float((err / np.maximum(bound, 1e-300)).max()))
        ratios[name] = max(ratios.get(name, 0.0), float((err / np.maximum(bound, 1e-300)).max()))

    st = bsol.NumpyBFGSState(lambda X, m: (np.zeros(B), Gt))
    with small_engine(B) as eng, one_blas_thread():
        eng.bfgs_begin(x0.reshape(B, h, w, 2))
        tx, tg, tp, tH = eng.bfgs_state_tensors()
        for t, a in ((tg, G), (tp, P), (tH, Hs)):
            to_dev(t, a)
        st.begin(x0)
        for b in range(B):
            st.set_state(b, g=G[b], p=P[b], H=Hs[b])
        before = snapshot(eng)
        # trial
        eng.bfgs_trial(al, mask)
        txt, tgt = eng.bfgs_trial_tensors()
        _, d_ref, gm_ref = st.eval(al, mask)
        torch.cuda.synchronize()
        assert np.array_equal(txt.cpu().numpy()[mask], st.xt[mask])
        # the caller's gradient at the trial point, then reduce
        rows = torch.from_numpy(np.flatnonzero(mask)).cuda()
        tgt[rows] = torch.from_numpy(Gt[mask]).cuda()
        d_dev, gm_dev = eng.bfgs_reduce(mask)
        for b in np.flatnonzero(mask):
            check('reduce_dphi', d_dev[b], d_ref[b], 2 * n * U * np.abs(Gt[b] * P[b]).sum())
            assert gm_dev[b] == gm_ref[b]
        # accept
        modes = np.where(mask, L.BFGS_UPDATE, L.BFGS_SKIP).astype(np.uint8)
        sc_dev = eng.bfgs_accept(al, modes)
        sc_ref = st.accept(al, modes)
        x_d, g_d, H_d = eng.bfgs_fetch(True)
        x_d, g_d = x_d.reshape(B, n), g_d.reshape(B, n)
        p_d = tp.cpu().numpy()
        x_r, g_r, H_r = st.fetch(True)
        for b in np.flatnonzero(mask):
            bd = step_bounds(n, Hs[b], G[b], P[b], Gt[b], al[b])
            assert bd['e_ys_rel'] < 1e-6                         # the first-order chain holds: y.s is far from cancelling
            assert np.array_equal(x_d[b], x_r[b]) and np.array_equal(g_d[b], Gt[b]) and np.array_equal(g_r[b], Gt[b])
            assert np.array_equal(H_d[b], H_d[b].T), 'H lost its bit symmetry'
            check('H', H_d[b], H_r[b], bd['H'])
            check('P', p_d[b], st.p[b], bd['P'])
            for name, k in (('dphi0', L.BFGS_S_DPHI0), ('pnorm', L.BFGS_S_PNORM), ('pmax', L.BFGS_S_PMAX), ('gnorm', L.BFGS_S_GNORM),
                            ('ys', L.BFGS_S_YS), ('yhy', L.BFGS_S_YHY)):
                check(name, sc_dev[b, k], sc_ref[b, k], bd[name])
            assert sc_dev[b, L.BFGS_S_GMAX] == sc_ref[b, L.BFGS_S_GMAX] and sc_dev[b, L.BFGS_S_XMAX] == sc_ref[b, L.BFGS_S_XMAX]
        after = snapshot(eng)
        for b in np.flatnonzero(~mask):
            for t0, t1 in zip(before, after):
                assert torch.equal(t0[b], t1[b]), 'a masked window changed'
    print(f'step parity n={n} B={B} error/bound: ' + ' '.join(f'{k}={v:.3f}' for k, v in sorted(ratios.items())))


def test_accept_modes_and_refusals(built_lib):
    """INIT takes P = -G with H = I, MOVE moves the point alone, SKIP nothing; the entry points refuse out-of-order and unsupported calls
    with a message."""
    import torch
    B, n, (h, w) = 3, 30, SHAPES[30]
    rng = np.random.default_rng(3)
    x0, g1 = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    with engine.Engine(SENSOR, 1200, max_refs=2, max_windows=B) as eng:
        assert eng._lib.eincm_bfgs_begin(eng._ctx, x0.ctypes.data, h, w, None) == L.ERR_STATE      # (the wrapper has no B yet)
        assert b'before eincm_set_windows' in eng._lib.eincm_last_error(eng._ctx)
    with small_engine(B) as eng:
        with pytest.raises(engine.EincmError, match='before eincm_bfgs_begin'):
            eng.bfgs_accept(np.zeros(B), np.zeros(B, np.uint8))
        with pytest.raises(engine.EincmError, match='before eincm_bfgs_begin'):
            eng.bfgs_trial(np.zeros(B))
        with pytest.raises(engine.EincmError, match='EINCM_BFGS_MAX_N'):
            eng.bfgs_begin(np.zeros((B, 23, 23, 2)))
        eng.set_device_results(True)
        with pytest.raises(engine.EincmError, match='eincm_set_device_results'):
            eng.bfgs_begin(x0.reshape(B, h, w, 2))
        eng.set_device_results(False)
        eng.bfgs_begin(x0.reshape(B, h, w, 2))
        with pytest.raises(engine.EincmError, match='unknown'):
            eng.bfgs_accept(np.zeros(B), np.array([1, 4, 0], np.uint8))
        eng.bfgs_trial(np.zeros(B))
        xt, gt = eng.bfgs_trial_tensors()
        assert np.array_equal(xt.cpu().numpy(), x0)
        to_dev(gt, g1)
        d, gm = eng.bfgs_reduce()
        assert not d.any() and np.array_equal(gm, np.abs(g1).max(1))             # P = 0 after begin
        sc = eng.bfgs_accept(np.zeros(B), np.array([L.BFGS_INIT, L.BFGS_MOVE, L.BFGS_SKIP], np.uint8))
        x, g, H = eng.bfgs_fetch(True)
        tx, tg, tp, tH = eng.bfgs_state_tensors()
        p = tp.cpu().numpy()
        assert np.array_equal(x.reshape(B, n), x0) and np.array_equal(g.reshape(B, n)[:2], g1[:2]) and not g.reshape(B, n)[2].any()
        assert np.array_equal(p[0], -g1[0]) and not p[1].any() and not p[2].any()
        assert np.array_equal(H, np.stack([np.eye(n)] * B))
        assert sc[0, L.BFGS_S_GMAX] == np.abs(g1[0]).max() and sc[0, L.BFGS_S_XMAX] == np.abs(x0[0]).max()
        assert sc[0, L.BFGS_S_GNORM] == pytest.approx(np.linalg.norm(g1[0]), rel=1e-14)
        assert sc[0, L.BFGS_S_DPHI0] == pytest.approx(-g1[0] @ g1[0], rel=1e-14) and sc[0, L.BFGS_S_PNORM] == sc[0, L.BFGS_S_GNORM]
        # a new batch drops the state
        wins = [synth.make_window(400 + b, SENSOR, 300, 2, flow='constant', flow_mag=1.0) for b in range(B)]
        eng.set_windows([(v['xs'], v['ys'], v['ts'], v['edges'], v['edge_ts']) for v in wins])
        with pytest.raises(engine.EincmError, match='before eincm_bfgs_begin'):
            eng.bfgs_fetch()
    with small_engine(1, precision='fp64') as eng:
        with pytest.raises(engine.EincmError, match='fp64') as ei:
            eng.bfgs_begin(np.zeros((1, 1, 1, 2)))
        assert ei.value.code == L.ERR_UNSUPPORTED


class TorchBowlState:
    """The state interface with the quartic bowl of _bfgs_cases evaluated by torch on the GPU, through the views of the trial point and
    its gradient: no vector crosses PCIe between begin and fetch."""

    def __init__(self, eng, seeds, n):
        import torch
        self.eng, self.n, self.shape = eng, n, SHAPES[n]
        terms = [CASES.bowl_terms(s, n) for s in seeds]
        self.A = torch.from_numpy(np.stack([a for a, _ in terms])).cuda()
        self.b = torch.from_numpy(np.stack([b for _, b in terms])).cuda()

    def begin(self, x0, active=None):
        self.B = x0.shape[0]
        self.eng.bfgs_begin(np.asarray(x0).reshape((self.B,) + self.shape + (2,)), active)

    def eval(self, alpha, mask):
        import torch
        self.eng.bfgs_trial(alpha, mask)
        xt, gt = self.eng.bfgs_trial_tensors()
        rows = torch.from_numpy(np.flatnonzero(mask)).cuda()
        x, A, b = xt[rows], self.A[rows], self.b[rows]
        Ax = (A * x[:, None, :]).sum(-1)
        f = 0.5 * (x * Ax).sum(-1) - (b * x).sum(-1) + 0.25 * (x ** 4).sum(-1)
        gt[rows] = Ax - b + x ** 3
        d, gm = self.eng.bfgs_reduce(mask)
        fv = np.full(self.B, np.nan)
        fv[np.flatnonzero(mask)] = f.cpu().numpy()
        return fv, d, gm

    def accept(self, alpha, modes):
        return self.eng.bfgs_accept(alpha, modes)

    def fetch(self, want_hess_inv=False):
        x, g, H = self.eng.bfgs_fetch(want_hess_inv)
        return x.reshape(self.B, self.n), g.reshape(self.B, self.n), H


SEEDS = (1, 2, 3, 4)


def solve_bowls(n):
    x0 = np.random.default_rng(5).uniform(-0.5, 0.5, (len(SEEDS), n))
    with small_engine(len(SEEDS)) as eng:
        drv = bsol.DeviceLockstepBFGS(TorchBowlState(eng, SEEDS, n), x0, 400, 1e-6)
        return x0, drv.run(), drv


@pytest.mark.parametrize('n', [30, 128, 512])
def test_device_side_objective_against_scipy(built_lib, n):
    """Whole minimisations with the state on the GPU and the objective evaluated there, four seeds in lockstep, against
    scipy.optimize.minimize(BFGS) on the host: the same status, nit and nfev, x within 1e-6 and f within 1e-10 (the tolerances of
    test_rank_two_update_beyond_64_dimensions)."""
    x0, res, drv = solve_bowls(n)
    assert drv.n_fetches == 1
    for b, seed in enumerate(SEEDS):
        ref = spo.minimize(CASES.quartic_bowl(seed, n), x0[b], jac=True, method='BFGS', options={'maxiter': 400, 'gtol': 1e-6})
        a = res[b]
        dx, df = np.abs(a.x - ref.x).max(), abs(a.fun - ref.fun)
        print(f'bowl n={n} seed={seed}: nit {a.nit}/{ref.nit} nfev {a.nfev}/{ref.nfev} status {a.status}/{ref.status} dx {dx:.2e} df {df:.2e}')
        assert (a.status, a.nit, a.nfev) == (ref.status, ref.nit, ref.nfev), (n, seed)
        assert dx < 1e-6 and df < 1e-10, (n, seed, dx, df)
        assert np.array_equal(a.hess_inv, a.hess_inv.T)


def test_two_solves_from_fresh_contexts_are_bit_identical(built_lib):
    _, r1, _ = solve_bowls(128)
    _, r2, _ = solve_bowls(128)
    for a, b in zip(r1, r2):
        assert np.array_equal(a.x, b.x) and a.fun == b.fun and (a.nit, a.nfev, a.status) == (b.nit, b.nfev, b.status)
        assert np.array_equal(a.jac, b.jac) and np.array_equal(a.hess_inv, b.hess_inv)


# ---- on the engine: the multi-level solver with bfgs_state='device' against 'host' ---------------------------------------------------
LOSS = dict(alpha=20.0, beta=35.0, gamma=0.0, delta=0.0, scale_to_sensor_size_method='bilinear')
N_LVLS = 4                       # theta pyramid 1 -> 2 -> 4 -> 8: the 8x8 level (128 unknowns) runs on the device state


def level_solver(B, H, W, bfgs_state, maxiters, extra=None, hs=None, callbacks=None):
    return bsol.BatchedMultipleLevelEINCMSolver(
        B, (H, W), N_LVLS, maxiters, LOSS,
        {'method': 'BFGS', 'options': {'gtol': 1e-7}, 'n_extra_attempts': extra or {}},
        handover_opt_maxiters=sol.growing_maxiters(N_LVLS, 4, 20), handover_opt_solver_params={'method': 'L-BFGS-B', 'options': {'gtol': 1e-6}},
        handover_settings=hs, pyramid_downscale_method='lanczos3', pyramid_upscale_method='repeat', pyramid_bases=[2] * (N_LVLS - 1),
        bfgs_state=bfgs_state, theta_solver_callbacks=callbacks)


def instrument(solver):
    """Log every evaluation of the solver's engine with the bytes its arrays carry across the C boundary (what crosses PCIe)."""
    eng, B = solver.engine, solver.B
    log = dict(evals=[], bytes={}, fetches=0, begins=0)

    def add(shape, nbytes):
        log['bytes'][shape] = log['bytes'].get(shape, 0) + int(nbytes)
    lg, be, ba, bb, bf = eng.loss_grad, eng.bfgs_eval, eng.bfgs_accept, eng.bfgs_begin, eng.bfgs_fetch

    def loss_grad(theta, params, *a, **k):
        v, g, aux = lg(theta, params, *a, **k)
        th = np.asarray(theta)
        add(th.shape[1:3], th.nbytes + v.nbytes + g.nbytes + B)
        log['evals'].append((th.shape[1:3], 'host', v.copy(), np.abs(g.reshape(B, -1)).max(1), np.array(k.get('active'), bool)))
        return v, g, aux

    def bfgs_eval(params, alpha, active=None, **k):
        v, d, gm = be(params, alpha, active, **k)
        shape = eng._bfgs_shape[1:3]
        add(shape, 8 * B + B + 3 * 8 * B)
        log['evals'].append((shape, 'device', v.copy(), gm.copy(), np.array(active, bool)))
        return v, d, gm

    def bfgs_accept(alpha, modes):
        add(eng._bfgs_shape[1:3], 8 * B + B + 8 * B * L.BFGS_NS)
        return ba(alpha, modes)

    def bfgs_begin(x0, active=None):
        log['begins'] += 1
        add(np.asarray(x0).shape[1:3], np.asarray(x0).nbytes + B)
        return bb(x0, active)

    def bfgs_fetch(want_hess_inv=False):
        log['fetches'] += 1
        x, g, H = bf(want_hess_inv)
        add(eng._bfgs_shape[1:3], x.nbytes + g.nbytes + (H.nbytes if H is not None else 0))
        return x, g, H
    eng.loss_grad, eng.bfgs_eval, eng.bfgs_accept, eng.bfgs_begin, eng.bfgs_fetch = loss_grad, bfgs_eval, bfgs_accept, bfgs_begin, bfgs_fetch
    return log


def windows(B, H, W, N, R, seed0=60):
    wins = [synth.make_window(seed0 + b, (H, W), N, R, flow='constant', flow_mag=3.0 + 0.5 * b) for b in range(B)]
    return [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def test_solver_device_state_against_host_state(built_lib):
    """Eight synthetic windows (as test_gpu_batch_solver.py), pyramid 1 -> 2 -> 4 -> 8.  The levels below 8x8 run on the host in both
    solvers, so the 8x8 level starts from the same point: its first evaluation agrees to the tolerance between loss_grad_device and
    loss_grad (test_gpu_device_io.py: value 1e-10, gradient 1e-9, relative to the largest entry); at the end of every level the two
    agree at test_gpu_batch_solver.py's tolerances (objective 1e-4 relative, theta 0.05 px).  On the device level no gradient comes down
    (one fetch per begin) and fewer bytes cross PCIe."""
    B, H, W, N, R = 8, 96, 128, 12000, 3
    args = windows(B, H, W, N, R)
    maxiters = sol.growing_maxiters(N_LVLS, 16 / 5, 16)
    outs, logs = {}, {}
    for mode in ('host', 'device'):
        s = level_solver(B, H, W, mode, maxiters)
        s.set_datasamples(args)
        logs[mode] = instrument(s)
        outs[mode] = s.solve()
        s.close()
    first = {m: next(e for e in logs[m]['evals'] if e[0] == (8, 8)) for m in logs}
    assert first['host'][1] == 'host' and first['device'][1] == 'device'
    assert first['device'][4].all() and first['host'][4].all()
    print('first 8x8 evaluation: value rel', rel(first['device'][2], first['host'][2]), 'max|g| rel', rel(first['device'][3], first['host'][3]))
    assert rel(first['device'][2], first['host'][2]) <= 1e-10 and rel(first['device'][3], first['host'][3]) <= 1e-9
    assert not any(e[1] == 'device' for e in logs['device']['evals'] if e[0] != (8, 8))       # below 8x8: the host's bit-exact update
    for b in range(B):
        for k in range(N_LVLS):
            key = f'pyr_lvl_{k}'
            sh, sd = outs['host'][b]['theta_opt_state_pyr'][key], outs['device'][b]['theta_opt_state_pyr'][key]
            dth = np.abs(outs['device'][b]['final_theta_pyr'][key] - outs['host'][b]['final_theta_pyr'][key]).max()
            print(f'window {b} {key}: fun {sd.fun_val:.9f} / {sh.fun_val:.9f} nit {sd.iter_num}/{sh.iter_num} nfev '
                  f'{sd.num_fun_eval}/{sh.num_fun_eval} status {sd.status}/{sh.status} dtheta {dth:.2e}')
    for b in range(B):
        for k in range(N_LVLS):
            key = f'pyr_lvl_{k}'
            sh, sd = outs['host'][b]['theta_opt_state_pyr'][key], outs['device'][b]['theta_opt_state_pyr'][key]
            assert sd.fun_val == pytest.approx(sh.fun_val, rel=1e-4), (b, key)
            assert np.abs(outs['device'][b]['final_theta_pyr'][key] - outs['host'][b]['final_theta_pyr'][key]).max() < 0.05, (b, key)
        assert set(outs['device'][b]) == set(outs['host'][b])
    lg = logs['device']
    assert lg['begins'] >= 1 and lg['fetches'] == lg['begins']         # x comes down once per begin, never per tick
    print('bytes across PCIe at 8x8: host', logs['host']['bytes'][(8, 8)], 'device', lg['bytes'][(8, 8)])
    assert lg['bytes'][(8, 8)] < logs['host']['bytes'][(8, 8)]
    for shape in ((1, 1), (2, 2), (4, 4)):
        assert lg['bytes'][shape] == logs['host']['bytes'][shape]


def test_solver_device_state_retry_callbacks_and_handover(built_lib):
    """A retry restarts the unconverged windows from their last iterate with H = I; a collecting callback gets every iterate (x is
    fetched for it); a second set_datasamples / solve hands over from the first.  Against the host state at the tolerances of
    test_two_sequences_with_handover."""
    B, H, W, N, R = 2, 96, 128, 8000, 3
    hs = {'use_handover': True, 'solve_handover_for_levels': [1, 0], 'use_downscaled_finest_priors': True, 'handover_limits': [0.0, 1.0],
          'clip_solved_handover': False, 'alpha_handover': 0.67}
    maxiters = sol.growing_maxiters(N_LVLS, 10 / 5, 10)

    class Collect(sol.EmptyCallback):
        def __init__(self):
            super().__init__()
            self.seen = []

        def __call__(self, r):
            super().__call__(r)
            self.seen.append((self.cur_key, np.array(r.x, copy=True), float(r.fun)))
    outs, cbs, logs, marks = {}, {}, {}, {}
    for mode in ('host', 'device'):
        cbs[mode] = [Collect(), sol.EmptyCallback()]
        s = level_solver(B, H, W, mode, maxiters, extra={'pyr_lvl_0': 1, 'pyr_lvl_1': 1}, hs=hs, callbacks=cbs[mode])
        outs[mode] = []
        for i in range(2):
            s.set_datasamples(windows(B, H, W, N, R, seed0=70 + 10 * i))
            logs[mode] = instrument(s)
            marks[mode] = len(cbs[mode][0].seen)
            outs[mode].append(s.solve())
        s.close()
    lg = logs['device']
    assert lg['begins'] >= 1
    seen = cbs['device'][0].seen[marks['device']:]                # the second solve's iterates of window 0
    n_seen0 = sum(1 for k, _, _ in seen if k == 'pyr_lvl_0')
    assert n_seen0 >= 1
    assert lg['fetches'] == lg['begins'] + n_seen0              # the collecting callback's iterates, and one fetch per begin
    for key, x, f in seen:
        assert x.shape == {'pyr_lvl_3': (1, 1, 2), 'pyr_lvl_2': (2, 2, 2), 'pyr_lvl_1': (4, 4, 2), 'pyr_lvl_0': (8, 8, 2)}[key]
        assert np.isfinite(x).all() and np.isfinite(f)
    # the counting-only callback counted every iteration of the device level without an x
    assert cbs['device'][1].get_iters()['pyr_lvl_0'] >= outs['device'][1][1]['theta_opt_state_pyr']['pyr_lvl_0'].iter_num >= 1
    retried = lg['begins'] > 1
    print('device begins at 8x8 in the second solve:', lg['begins'], '(retry ran)' if retried else '(no retry needed)')
    for b in range(B):
        od, oh = outs['device'][1][b], outs['host'][1][b]
        assert set(od['ho_opt_state_pyr']) == set(oh['ho_opt_state_pyr']) == {'pyr_lvl_1', 'pyr_lvl_0'}
        for k in range(N_LVLS):
            key = f'pyr_lvl_{k}'
            print(f'window {b} {key}: handover {od["final_handover_weight_pyr"][key]:.4f}/{oh["final_handover_weight_pyr"][key]:.4f} dtheta '
                  f'{np.abs(od["final_theta_pyr"][key] - oh["final_theta_pyr"][key]).max():.2e}')
            assert od['final_handover_weight_pyr'][key] == pytest.approx(oh['final_handover_weight_pyr'][key], abs=0.05), (b, key)
            assert np.abs(od['final_theta_pyr'][key] - oh['final_theta_pyr'][key]).max() < 0.1, (b, key)


def test_retry_restarts_from_the_last_iterate(built_lib):
    """maxiter 3 at a level with an extra attempt: every window stops unconverged after 3 iterations and is begun again from where it
    stopped, with H = I."""
    n, B = 128, 2
    x0 = np.random.default_rng(5).uniform(-0.5, 0.5, (B, n))
    with small_engine(B) as eng:
        st = TorchBowlState(eng, (1, 2), n)
        r1 = bsol.DeviceLockstepBFGS(st, x0, 3, 1e-6).run()
        assert all(r.status == 1 and r.nit == 3 for r in r1)
        x1 = np.stack([r.x for r in r1])
        r2 = bsol.DeviceLockstepBFGS(st, x1, 400, 1e-6, active=[True, False]).run()
        assert r2[1] is None and r2[0].status == 0 and r2[0].fun < r1[0].fun
        x, _, _ = st.fetch()
        assert np.array_equal(x[1], x1[1])                           # the rider's point never moved
        # the restart is what SciPy does from that point with a fresh inverse Hessian
        ref = spo.minimize(CASES.quartic_bowl(1, n), x1[0], jac=True, method='BFGS', options={'maxiter': 400, 'gtol': 1e-6})
        assert (r2[0].nit, r2[0].nfev, r2[0].status) == (ref.nit, ref.nfev, ref.status)
        assert np.abs(r2[0].x - ref.x).max() < 1e-6
