"""Cases of tests/test_gpu_loss_assembly.py, and the run that both the test and the recording of its golden file make.

Every path that turns per-image scalars into a window's loss and its gradient weights (csrc/eincm_loss.h): host assembly, k_final,
k_final_dense, the float64 engine, the objective kinds, the handover blend, objectives() and the device-resident entry point.  The
arithmetic depends on R, the tile count and the path, not on size: sensor 37x53 (2x2 ragged tiles), R = 3, three windows of 1500, 0
and 700 events.
"""
import hashlib
import importlib

import numpy as np
import torch      # at import, before anything loads the engine's library: the HIP runtime loaded first serves both

H, W, R = 37, 53, 3
COUNTS = (1500, 0, 700)
B = len(COUNTS)
ALPHA, BETA, GAMMA, DELTA = 20.0, 35.0, 2.5e-4, 0.5
HANDOVER = (0.3, 0.5, 0.9)
AUX = ('final_loss', 'mean_rel_corr', 'mean_rel_contrast', 'mean_rel_iwe_divergence', 'theta_total_variation')
_CACHE = {}


def engine_module():
    return importlib.import_module('edge-informed-contrast-maximization_amd.engine')


def windows():
    if 'w' not in _CACHE:
        synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
        out = []
        for b, n in enumerate(COUNTS):
            w = synth.make_window(60 + b, (H, W), n, R, flow='smooth', flow_mag=4.0)
            out.append((w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']))
        _CACHE['w'] = out
    return _CACHE['w']


def theta(shape, nan=False):
    """(B, h, w, 2): a fixed offset per window plus a ripple; nan: one NaN in window 2's theta."""
    h, w = shape
    rng = np.random.default_rng(101 + h)
    th = np.array([[1.5, -0.75], [-1.0, 0.5], [0.75, 2.0]]).reshape(B, 1, 1, 2) + (0.4 * rng.uniform(-1.0, 1.0, (B, h, w, 2)) if h * w > 1 else 0.0)
    th = np.ascontiguousarray(np.broadcast_to(th, (B, h, w, 2)), dtype=np.float64).copy()
    if nan:
        th[2].reshape(-1)[-1] = np.nan
    return th


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def _put(rec, name, v, g=None, aux=None):
    rec[name + '/value'] = np.array(v, dtype=np.float64)
    if g is not None:
        g = np.array(g, dtype=np.float64)
        if g.size > 512:                # the dense gradients: digest and the first entries of every window
            rec[name + '/grad_sha256'] = digest(g)
            rec[name + '/grad_head'] = g.reshape(B, -1)[:, :8].copy()
        else:
            rec[name + '/grad'] = g
    if aux is not None:
        for k in AUX:
            rec[name + '/aux_' + k] = np.array([a[k] for a in aux], dtype=np.float64)


def _evals(E):
    """name -> (theta shape, params, keyword arguments of loss_grad) of the fp32 engine's evaluations."""
    P = E.make_params
    two, grid, dense = (1, 1), (4, 4), (H, W)
    c1 = (two, P(ALPHA, BETA, 0.0, 0.0, 2))
    c3 = (grid, P(ALPHA, BETA, GAMMA, 0.0, 0))
    c4 = (grid, P(ALPHA, BETA, GAMMA, DELTA, 0))
    return {
        '01_2dof_lvl2': c1 + ({},),
        '02_2dof_tv': (two, P(ALPHA, BETA, GAMMA, 0.0, 0), {}),
        '03_grid_tv': c3 + ({},),
        '04_grid_delta': c4 + ({},),
        '05_grid_full_aux': (grid, P(ALPHA, BETA, GAMMA, DELTA, 0, full_aux=True), {}),
        '05_grid_full_aux_lvl1': (grid, P(ALPHA, BETA, GAMMA, 0.0, 1, full_aux=True), {}),
        '06_dense_tv': (dense, P(ALPHA, BETA, GAMMA, 0.0, 0), {}),
        '07_forward_1': c1 + ({'want_grad': False},),
        '07_forward_3': c3 + ({'want_grad': False},),
        '08_active_1': c1 + ({'active': [1, 0, 1]},),
        '08_active_3': c3 + ({'active': [1, 0, 1]},),
        '09_variance_1': (two, P(ALPHA, BETA, 0.0, 0.0, 2, contrast_kind='variance'), {}),
        '10_nan_1': c1 + ({'nan': True},),
        '10_nan_4': c4 + ({'nan': True},),
        '12_adaptive_hadamard_3': (grid, P(ALPHA, BETA, GAMMA, 0.0, 0, contrast_kind='adaptive_grad_mag', correlation_kind='hadamard'), {}),
        '12_joint_delta': (grid, P(ALPHA, BETA, GAMMA, DELTA, 0, correlation_kind='joint_contrast'), {}),
    }


def _run(eng, shape, params, kw, rec, name):
    kw = dict(kw)
    th = theta(shape, nan=kw.pop('nan', False))
    v, g, aux = eng.loss_grad(th, params, want_aux=True, **kw)
    _put(rec, name, v, g, aux)


def record():
    """Every case -> {name/field: array}.  Needs a GPU."""
    E = engine_module()
    rec = {}
    n = max(sum(COUNTS), 1)
    with E.Engine((H, W), n, max_refs=R, max_windows=B) as eng:
        eng.set_windows(windows())
        for name, (shape, params, kw) in _evals(E).items():
            _run(eng, shape, params, kw, rec, name)
        # 13: the handover blend and chain rule
        P = E.make_params
        v, dv = eng.handover_loss_grad(np.array(HANDOVER), theta((4, 4)) * 0.5 + 0.25, theta((4, 4)), P(ALPHA, BETA, GAMMA, 0.0, 0))
        rec['13_handover/value'], rec['13_handover/dvalue'] = np.array(v, dtype=np.float64), np.array(dv, dtype=np.float64)
        # 14: objectives() on a full-resolution Theta
        for b, d in enumerate(eng.objectives(theta((H, W)))):
            for k, a in d.items():
                rec[f'14_objectives/w{b}_{k}'] = np.array(a, dtype=np.float64)
        # 15: theta and gradient resident in HBM
        tdev = torch.from_numpy(theta((4, 4))).to('cuda:0')
        v, g, aux = eng.loss_grad_device(tdev, P(ALPHA, BETA, GAMMA, 0.0, 0), want_aux=True)
        _put(rec, '15_device_3', v, g.cpu().numpy(), aux)
    # 11: a float64 engine
    with E.Engine((H, W), n, max_refs=R, max_windows=B, precision='fp64') as eng:
        eng.set_windows(windows())
        P = E.make_params
        _run(eng, (1, 1), P(ALPHA, BETA, 0.0, 0.0, 2), {}, rec, '11_fp64_1')
        _run(eng, (4, 4), P(ALPHA, BETA, GAMMA, DELTA, 0), {}, rec, '11_fp64_grid_tv_delta')
    return rec
