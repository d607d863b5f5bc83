"""The limited-memory form of the device-resident BFGS (csrc/eincm_lbfgs.hip.h) on the GPU: every accept, stage by
stage, against its written contract ``batch_solver.NumpyLBFGSState``; whole minimisations of a device-side objective against that
contract; and the engine's objective on theta shapes the dense form refuses (a 24x24 grid, a dense per-pixel theta)."""
import importlib

import numpy as np
import pytest
import torch      # at import, before any fixture loads the engine's library (see test_gpu_device_bfgs.py)

import _bfgs_cases as CASES

pytestmark = pytest.mark.gpu

engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
bsol = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
sol = importlib.import_module('edge-informed-contrast-maximization_amd.solver')
synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
L = engine.L

U = 2.0 ** -53
CHUNK = 512        # LBFGS_CHUNK: unknowns per workgroup of the sweeps (256 theta cells).  n = 2 h w is even, so the smallest n above one chunk
                   # is one chunk and one cell: 514.  130 is one partial chunk, 1040 two chunks and a partial third.
SHAPES = {2: (1, 1), 130: (5, 13), CHUNK + 2: (1, 257), 1040: (20, 26)}
MASKS = {1: [1], 3: [1, 0, 1], 8: [1, 1, 0, 1, 0, 1, 1, 1]}
SENSOR = (32, 40)


def small_engine(B, sensor=SENSOR, n_events=300, **kw):
    eng = engine.Engine(sensor, (n_events + 100) * B, max_refs=2, max_windows=B, **kw)
    wins = [synth.make_window(300 + b, sensor, n_events, 2, flow='constant', flow_mag=1.0) for b in range(B)]
    eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
    return eng


def device_state(eng):
    """Every array of the limited state as numpy copies."""
    tx, tg, tp, tH = eng.bfgs_state_tensors()
    assert tH is None
    S, Y, D, delta, head, count, m = eng.lbfgs_history_tensors()
    xt, gt = eng.bfgs_trial_tensors()
    torch.cuda.synchronize()
    return dict(x=tx.cpu().numpy(), g=tg.cpu().numpy(), p=tp.cpu().numpy(), S=S.cpu().numpy(), Y=Y.cpu().numpy(), D=D.cpu().numpy(),
                delta=delta.cpu().numpy(), head=head.cpu().numpy(), count=count.cpu().numpy(), xt=xt.cpu().numpy(), gt=gt.cpu().numpy())


def mirror(st, dev):
    """Put the host contract's windows into the GPU's state, bit for bit."""
    for b, w in enumerate(st.windows):
        w.x, w.g, w.p = dev['x'][b].copy(), dev['g'][b].copy(), dev['p'][b].copy()
        w.S, w.Y, w.D, w.delta = dev['S'][b].copy(), dev['Y'][b].copy(), dev['D'][b].copy(), dev['delta'][b].copy()
        w.head, w.count = int(dev['head'][b]), int(dev['count'][b])


def basis_vectors(S, Y, g, m):
    return {**{k: S[k] for k in range(m)}, **{m + k: Y[k] for k in range(m)}, 2 * m: g}


@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('n', sorted(SHAPES))
def test_accept_parity_by_stage(built_lib, n, B):
    """For m in {1, 3, 10}: INIT, then m + 3 accepts (the ring fills and wraps) in which the windows take part by a pattern that leaves
    them at different ring fills, one of them with y = 0 (a skipped pair).  Before every step the host contract is put into the GPU's own
    state, so each accept is compared from identical bits:

    * bit-equal: the trial point, the stored s and y, the ring's head and count, max|G|, max|X|, max|P|, and every array of the windows
      outside the mask;
    * within 2 n 2^-53 sum|a_i b_i| of numpy's dot (two computed n-term sums, each within n 2^-53 sum|a_i b_i| of the exact one - the
      bound of test_gpu_device_bfgs.py, nothing fitted): every entry of D, Gt.P of the reduce, G.P, y.s, y.y; |P| and |G| within the
      same bound passed through the square root ((n + 2) 2^-53 relative);
    * delta bit-equal to batch_solver.lbfgs_delta run on the GPU's own D, P bit-equal to batch_solver.lbfgs_combine of the GPU's own
      delta and basis."""
    h, w = SHAPES[n]
    rng = np.random.default_rng(5000 + 10 * n + B)
    ratios = {}

    def check(name, dev, ref, bound):
        err = np.abs(np.asarray(dev) - np.asarray(ref))
        bound = np.asarray(bound, dtype=np.float64)
        assert np.all(err <= bound), (name, n, B, float((err / np.maximum(bound, 1e-300)).max()))
        ratios[name] = max(ratios.get(name, 0.0), float((err / np.maximum(bound, 1e-300)).max()))

    with small_engine(B) as eng:
        for m, scale in ((1, 'last_pair'), (3, 'identity'), (10, 'last_pair')):
            x0 = rng.standard_normal((B, n))
            feed = np.zeros((B, n))
            st = bsol.NumpyLBFGSState(lambda X, mk: (np.zeros(B), feed.copy()), m, scale)
            st.begin(x0)
            eng.lbfgs_begin(x0.reshape(B, h, w, 2), history=m, initial_scale=scale)
            everyone, sc_prev = np.ones(B, bool), None
            for step in range(m + 4):
                init = step == 0
                mask = everyone if init else np.array([(step + b) % 3 != 0 for b in range(B)]) if B > 1 else everyone
                if not init and B == 8:
                    mask = mask & np.array(MASKS[8], bool) if step % 2 else mask
                mode = L.BFGS_INIT if init else L.BFGS_UPDATE
                before = device_state(eng)
                mirror(st, before)
                alpha = np.zeros(B) if init else 10.0 ** rng.uniform(-2, 0.5, B)
                # trial
                eng.bfgs_trial(alpha, mask)
                xt, gt = eng.bfgs_trial_tensors()
                torch.cuda.synchronize()
                xt_np = xt.cpu().numpy()
                # the gradient at the trial point: y = A s with a random positive diagonal A (y = 0 for one window at step 2)
                for b in np.flatnonzero(mask):
                    s = alpha[b] * before['p'][b]
                    feed[b] = rng.standard_normal(n) if init else before['g'][b] + rng.uniform(0.5, 2.0, n) * s
                    if step == 2 and b == int(np.flatnonzero(mask)[0]):
                        feed[b] = before['g'][b]
                _, d_ref, gm_ref = st.eval(alpha, mask)
                assert np.array_equal(xt_np[mask], st.xt[mask])
                rows = torch.from_numpy(np.flatnonzero(mask)).cuda()
                gt[rows] = torch.from_numpy(feed[mask]).cuda()
                d_dev, gm_dev = eng.bfgs_reduce(mask)
                for b in np.flatnonzero(mask):
                    check('reduce_dphi', d_dev[b], d_ref[b], 2 * n * U * np.abs(feed[b] * before['p'][b]).sum())
                    assert gm_dev[b] == gm_ref[b]
                # accept
                modes = np.where(mask, mode, L.BFGS_SKIP).astype(np.uint8)
                sc_dev = eng.bfgs_accept(alpha, modes)
                sc_ref = st.accept(alpha, modes)
                after = device_state(eng)
                for b in np.flatnonzero(mask):
                    hw = st.windows[b]
                    assert (int(after['head'][b]), int(after['count'][b])) == (hw.head, hw.count), (m, step, b)
                    if step == 2 and b == int(np.flatnonzero(mask)[0]):
                        assert hw.count == int(before['count'][b]), 'the pair with y = 0 was stored'
                    slots, order = bsol.lbfgs_basis(hw.head, hw.count, m)
                    assert np.array_equal(after['x'][b], hw.x) and np.array_equal(after['g'][b], feed[b])
                    for k in slots:
                        assert np.array_equal(after['S'][b, k], hw.S[k]) and np.array_equal(after['Y'][b, k], hw.Y[k]), (m, step, b, k)
                    vec = basis_vectors(hw.S, hw.Y, hw.g, m)
                    for u in order:
                        for v in order:
                            check('D', after['D'][b, u, v], hw.D[u, v], 2 * n * U * np.abs(vec[u] * vec[v]).sum())
                            assert after['D'][b, u, v] == after['D'][b, v, u]
                    delta = bsol.lbfgs_delta(after['D'][b], hw.head, hw.count, m, scale)
                    assert np.array_equal(after['delta'][b][order], delta[order]), (m, step, b)
                    p_np = bsol.lbfgs_combine(after['delta'][b], after['S'][b], after['Y'][b], after['g'][b], hw.head, hw.count, m)
                    assert np.array_equal(after['p'][b], p_np), (m, step, b)
                    g_d, p_d, x_d = after['g'][b], after['p'][b], after['x'][b]
                    check('dphi0', sc_dev[b, L.BFGS_S_DPHI0], g_d @ p_d, 2 * n * U * np.abs(g_d * p_d).sum())
                    check('pnorm', sc_dev[b, L.BFGS_S_PNORM], np.linalg.norm(p_d), (n + 2) * U * np.linalg.norm(p_d))
                    check('gnorm', sc_dev[b, L.BFGS_S_GNORM], np.linalg.norm(g_d), (n + 2) * U * np.linalg.norm(g_d))
                    assert sc_dev[b, L.BFGS_S_GMAX] == np.abs(g_d).max() and sc_dev[b, L.BFGS_S_XMAX] == np.abs(x_d).max()
                    assert sc_dev[b, L.BFGS_S_PMAX] == np.abs(p_d).max()
                    if not init:
                        s, y = alpha[b] * before['p'][b], feed[b] - before['g'][b]
                        check('ys', sc_dev[b, L.BFGS_S_YS], sc_ref[b, L.BFGS_S_YS], 2 * n * U * np.abs(y * s).sum())
                        check('yy', sc_dev[b, L.BFGS_S_YHY], sc_ref[b, L.BFGS_S_YHY], 2 * n * U * (y * y).sum())
                    else:
                        assert hw.count == 0 and np.array_equal(p_d, -g_d)
                for b in np.flatnonzero(~mask):
                    for k in before:
                        assert np.array_equal(before[k][b], after[k][b]), ('a masked window changed', k, m, step, b)
                    assert np.array_equal(sc_dev[b], sc_prev[b])
                sc_prev = sc_dev.copy()
            fills = after['count']
            if B > 1 and m == 10:
                assert len(set(int(c) for c in fills)) > 1, fills          # the pattern left the windows at different ring fills
    print(f'accept parity n={n} B={B} error/bound: ' + ' '.join(f'{k}={v:.3f}' for k, v in sorted(ratios.items())))


def test_refusals_and_the_way_back_to_the_dense_form(built_lib):
    B, n, (h, w) = 2, 130, SHAPES[130]
    x0 = np.random.default_rng(1).standard_normal((B, h, w, 2))
    with engine.Engine(SENSOR, 800, max_refs=2, max_windows=B) as eng:
        assert eng._lib.eincm_lbfgs_begin(eng._ctx, x0.ctypes.data, h, w, None, 3, 1) == L.ERR_STATE
        assert b'before eincm_set_windows' in eng._lib.eincm_last_error(eng._ctx)
    with small_engine(B) as eng:
        with pytest.raises(engine.EincmError, match='before eincm_bfgs_begin'):
            eng.bfgs_trial(np.zeros(B))
        for bad in (0, 17):
            assert eng._lib.eincm_lbfgs_begin(eng._ctx, x0.ctypes.data, h, w, None, bad, 1) == L.ERR_ARG
            assert b'EINCM_LBFGS_MAX_HISTORY' in eng._lib.eincm_last_error(eng._ctx)
        assert eng._lib.eincm_lbfgs_begin(eng._ctx, x0.ctypes.data, h, w, None, 3, 2) == L.ERR_ARG
        assert b'initial_scale' in eng._lib.eincm_last_error(eng._ctx)
        eng.set_device_results(True)
        with pytest.raises(engine.EincmError, match='eincm_set_device_results'):
            eng.lbfgs_begin(x0)
        eng.set_device_results(False)
        eng.lbfgs_begin(x0, history=3)
        assert eng.bfgs_state_tensors()[3] is None
        with pytest.raises(engine.EincmError, match='hess_inv must be NULL'):
            eng.bfgs_fetch(True)
        x, g, H = eng.bfgs_fetch()
        assert np.array_equal(x, x0) and not g.any() and H is None
        # back to the dense form on the same context
        with pytest.raises(engine.EincmError, match='EINCM_BFGS_MAX_N'):
            eng.bfgs_begin(np.zeros((B, 23, 23, 2)))
        eng.bfgs_begin(x0)
        with pytest.raises(engine.EincmError, match='dense form'):
            eng.lbfgs_history_tensors()
        x, g, H = eng.bfgs_fetch(True)
        assert np.array_equal(x, x0) and np.array_equal(H, np.stack([np.eye(n)] * B))
    with small_engine(1, precision='fp64') as eng:
        with pytest.raises(engine.EincmError, match='fp64') as ei:
            eng.lbfgs_begin(np.zeros((1, 1, 1, 2)))
        assert ei.value.code == L.ERR_UNSUPPORTED


# ---- whole minimisations of a device-side objective ---------------------------------------------------------------------------------
class TorchBowlLimited:
    """The quartic bowl of _bfgs_cases evaluated by torch on the GPU through the views of the trial point and its gradient, the state in
    the limited form."""

    def __init__(self, eng, seeds, n, history, scale):
        self.eng, self.n, self.shape, self.history, self.scale = eng, n, SHAPES[n], history, scale
        terms = [CASES.bowl_terms(s, n) for s in seeds]
        self.A = torch.from_numpy(np.stack([a for a, _ in terms])).cuda()
        self.b = torch.from_numpy(np.stack([b for _, b in terms])).cuda()

    def begin(self, x0, active=None):
        self.B = x0.shape[0]
        self.eng.lbfgs_begin(np.asarray(x0).reshape((self.B,) + self.shape + (2,)), active, self.history, self.scale)

    def eval(self, alpha, mask):
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
        x, g, _ = self.eng.bfgs_fetch(False)
        return x.reshape(self.B, self.n), g.reshape(self.B, self.n), None


SEEDS = (1, 2, 3, 4)


@pytest.mark.parametrize('n', [130, 1040])
def test_device_side_objective_against_the_host_contract(built_lib, n):
    """Four bowls in lockstep, gtol 1e-6, history 10, 'last_pair': the device state and NumpyLBFGSState both end with status 0, within
    2 sqrt(n) gtol of each other (both end points have max|g| <= gtol, each within sqrt(n) gtol of the minimiser: the bowl's Hessian is
    >= I)."""
    gtol = 1e-6
    x0 = np.random.default_rng(5).uniform(-0.5, 0.5, (len(SEEDS), n))
    with small_engine(len(SEEDS)) as eng:
        drv = bsol.DeviceLockstepBFGS(TorchBowlLimited(eng, SEEDS, n, 10, 'last_pair'), x0, 400, gtol, want_hess_inv=False)
        dev = drv.run()
        assert drv.n_fetches == 1
    host = bsol.DeviceLockstepBFGS(bsol.NumpyLBFGSState(CASES.batch_of([CASES.quartic_bowl(s, n) for s in SEEDS]), 10, 'last_pair'),
                                   x0, 400, gtol, want_hess_inv=False).run()
    for b, (a, r) in enumerate(zip(dev, host)):
        dx = float(np.linalg.norm(a.x - r.x))
        print(f'bowl n={n} seed={SEEDS[b]}: status {a.status}/{r.status} nit {a.nit}/{r.nit} nfev {a.nfev}/{r.nfev} |dx| {dx:.2e}')
        assert a.status == 0 and r.status == 0, (n, b)
        assert dx <= 2 * np.sqrt(n) * gtol, (n, b, dx)


# ---- on the engine's objective: theta shapes the dense form refuses -----------------------------------------------------------------
B_ENG = 3
CASES_ENG = {
    'grid24': dict(sensor=(48, 64), shape=(24, 24), lvl=1, gamma=0.0),            # n = 1152
    'dense': dict(sensor=(20, 26), shape=(20, 26), lvl=0, gamma=2.5e-4),          # n = 1040: one unknown pair per pixel, TV term on
}


def eng_params(case):
    return engine.make_params(20.0, 35.0, case['gamma'], 0.0, case['lvl'], 'bilinear')


def eng_windows(case):
    wins = [synth.make_window(80 + b, case['sensor'], 3000, 2, flow='constant', flow_mag=1.5 + 0.5 * b) for b in range(B_ENG)]
    return [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]


def eng_solve(case, maxiter=12):
    with engine.Engine(case['sensor'], 3000 * B_ENG, max_refs=2, max_windows=B_ENG) as eng:
        eng.set_windows(eng_windows(case))
        theta0 = np.zeros((B_ENG,) + case['shape'] + (2,))
        v0, _, _ = eng.loss_grad(theta0, eng_params(case))
        res = bsol.minimize_thetas(eng, theta0, eng_params(case), maxiter, 1e-7, hessian='auto', history=5, bfgs_state='device')
        return v0, res


@pytest.mark.parametrize('name', sorted(CASES_ENG))
def test_engine_first_evaluation_and_refusal_of_the_dense_form(built_lib, name):
    """The first evaluation through the limited state agrees with loss_grad at the tolerances between loss_grad_device and loss_grad
    (value 1e-10, gradient 1e-9 of the largest entry); eincm_bfgs_begin refuses the shape with its message and still works afterwards."""
    case = CASES_ENG[name]
    p = eng_params(case)
    rng = np.random.default_rng(9)
    theta0 = rng.uniform(-1.0, 1.0, (B_ENG,) + case['shape'] + (2,))
    n = theta0[0].size
    assert n > L.BFGS_MAX_N
    with engine.Engine(case['sensor'], 3000 * B_ENG, max_refs=2, max_windows=B_ENG) as eng:
        eng.set_windows(eng_windows(case))
        v_ref, g_ref, _ = eng.loss_grad(theta0, p)
        eng.lbfgs_begin(theta0, history=4)
        v, d, gm = eng.bfgs_eval(p, np.zeros(B_ENG))
        xt, gt = eng.bfgs_trial_tensors()
        torch.cuda.synchronize()
        g = gt.cpu().numpy().reshape(g_ref.shape)
        assert np.array_equal(xt.cpu().numpy().reshape(theta0.shape), theta0)
        ev = np.abs(v - v_ref).max() / np.abs(v_ref).max()
        eg = np.abs(g - g_ref).max() / np.abs(g_ref).max()
        print(f'{name}: first evaluation value rel {ev:.2e} gradient rel {eg:.2e}')
        assert ev <= 1e-10 and eg <= 1e-9
        assert np.array_equal(gm, np.abs(g.reshape(B_ENG, -1)).max(1)) and not d.any()          # P = 0 after begin
        with pytest.raises(engine.EincmError, match='more than EINCM_BFGS_MAX_N = 1024'):
            eng.bfgs_begin(theta0)
        eng.bfgs_begin(theta0[:, :4, :4])
        v4, _, _ = eng.bfgs_eval(p, np.zeros(B_ENG))
        assert np.isfinite(v4).all() and eng.bfgs_state_tensors()[3] is not None


@pytest.mark.parametrize('name', sorted(CASES_ENG))
def test_engine_minimisation_descends_and_repeats_bit_for_bit(built_lib, name):
    """minimize_thetas on the device state: every window's final objective is at most its first, its status is 0, 1 or 2, and two solves
    from fresh contexts are bit-identical.  (End points are not compared between drivers on this objective: DESIGN.md sections 8, 17.)"""
    case = CASES_ENG[name]
    v0, r1 = eng_solve(case)
    _, r2 = eng_solve(case)
    for b, (a, c) in enumerate(zip(r1, r2)):
        print(f'{name} window {b}: f {v0[b]:.9f} -> {a.fun:.9f} nit {a.nit} nfev {a.nfev} status {a.status}')
        assert a.fun <= v0[b] and a.status in (0, 1, 2) and a.nit >= 1
        assert np.array_equal(a.x, c.x) and a.fun == c.fun and (a.nit, a.nfev, a.status) == (c.nit, c.nfev, c.status)
        assert np.array_equal(a.jac, c.jac) and a.hess_inv is None


def test_solver_one_level_deeper_than_the_default_pyramid(built_lib):
    """BatchedMultipleLevelEINCMSolver(hessian='auto') with a 32x32 level on top of the default 1 .. 16x16 pyramid: the levels up to
    16x16 keep the matrix, the 32x32 level (2048 unknowns) runs in the limited form; both device and host states run through."""
    n_lvls, B, sensor = 6, B_ENG, (48, 64)
    case = dict(sensor=sensor)
    for state in ('device', 'host'):
        s = bsol.BatchedMultipleLevelEINCMSolver(
            B, sensor, n_lvls, sol.growing_maxiters(n_lvls, 2, 4), dict(alpha=20.0, beta=35.0, gamma=0.0, delta=0.0,
                                                                       scale_to_sensor_size_method='bilinear'),
            {'method': 'BFGS', 'options': {'gtol': 1e-7}}, pyramid_bases=[2] * (n_lvls - 1), bfgs_state=state, hessian='auto', history=5)
        s.set_datasamples(eng_windows(case))
        begun = []
        lb = s.engine.lbfgs_begin
        s.engine.lbfgs_begin = lambda x0, *a, **k: (begun.append(np.asarray(x0).shape), lb(x0, *a, **k))[1]
        out = s.solve()
        s.close()
        assert (begun and all(sh == (B, 32, 32, 2) for sh in begun)) if state == 'device' else not begun
        for b in range(B):
            st = out[b]['theta_opt_state_pyr']['pyr_lvl_0']
            assert out[b]['final_theta_pyr']['pyr_lvl_0'].shape == (32, 32, 2) and np.isfinite(st.fun_val)
            assert st.status in (0, 1, 2) and st.hess_inv is None
