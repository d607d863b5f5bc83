"""Record the reference's own loss path on fixed inputs: tests/golden/ref_*.npz.

PROVENANCE.  Every recorded number in a ref_*.npz is an output of the reference's unmodified Python modules
(src/eincm/losses.py, event_warpers.py, contrast_metrics.py, regularizers.py, objectives/*.py, src/utils/event_utils.py,
theta_utils.py, img_utils.py of robotic-vision-lab/Edge-Informed-Contrast-Maximization), imported from the path given
by --reference-src and run in float64 (the reference sets jax_enable_x64).  jax is not installed here, so the JAX
primitives they call are served by oracle/jax_standin.py: the pin rests on the stand-in's reading of those primitives,
each tested in tests/test_jax_standin.py.  Gradients are by torch autograd through the reference's own code.
The inputs are stored explicitly (edges at fp32-representable values), so no fixture depends on the synthetic
generator's RNG stream.  No test runs this script or reads the reference; the tests read only the fixtures.

Convolution order.  jax.scipy.signal.convolve is recorded in the stand-in's 'exact' mode (the exact sum rounded once),
what the reference computes when no summation order can flip a `> 0` test.  Each loss case is also evaluated under the
'taps' and 'reversed' orders; `order_sensitive` lists every output that moves by more than 1e-13 relative under either
order.  Such an output depends on XLA's summation order in the real reference (regularizers.py:26-29 counts pixels whose
Scharr flow gradient is non-zero; on locally constant flow that count flips on +-1e-16 residues).  The flags document
the finding only; the tests compare every output with the 'exact' recording.

Run from the repo root:
    python tests/golden/make_reference_golden.py --reference-src <reference checkout>/src            (write)
    python tests/golden/make_reference_golden.py --reference-src <reference checkout>/src --check    (compare)
--check regenerates into a temporary directory and compares with the committed files: bit for bit, except values that
pass through a torch scatter-add or reduction whose order may vary between torch builds, which must agree to 1e-15
relative (max-norm).
"""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import jax_standin as JS          # noqa: E402

synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')

CMD = 'python tests/golden/make_reference_golden.py --reference-src <reference>/src'
ORDER_RTOL = 1e-13
CHECK_RTOL = 1e-15

# name, (H, W), N, R, theta spec, method, flow, flow magnitude, alpha, beta, gamma, delta, level, handover
LOSS_CASES = [
    ('2dof_lvl2_37x53', (37, 53), 1800, 3, (1, 1), 'bilinear', 'constant', 6.0, 20.0, 35.0, 0.0, 0.0, 2, None),
    ('2dof_lvl0_tv_20x26', (20, 26), 300, 1, (1, 1), 'bilinear', 'constant', 4.0, 20.0, 35.0, 2.5e-3, 0.0, 0, None),
    ('2dof_lvl0_tv_div_r3_20x26', (20, 26), 300, 3, (1, 1), 'bilinear', 'constant', 4.0, 20.0, 35.0, 2.5e-3, 0.7, 0, None),
    ('bilinear4x4_lvl0_40x54', (40, 54), 3500, 5, (4, 4), 'bilinear', 'smooth', 6.0, 20.0, 35.0, 2.5e-3, 0.5, 0, None),
    ('lanczos3_8x8_lvl1_37x53', (37, 53), 1600, 3, (8, 8), 'lanczos3', 'smooth', 5.0, 60.0, 60.0, 0.0, 0.0, 1, None),
    ('cubic5x3_lvl0_37x53', (37, 53), 1500, 3, (5, 3), 'cubic', 'smooth', 5.0, 20.0, 35.0, 1e-3, 0.3, 0, None),
    ('lanczos5_6x6_r16_alpha0_20x26', (20, 26), 400, 16, (6, 6), 'lanczos5', 'smooth', 3.0, 0.0, 35.0, 0.0, 0.0, 2, None),
    ('finer_than_sensor_2x12_5x7', (5, 7), 7, 1, (2, 12), 'bilinear', 'smooth', 1.5, 20.0, 35.0, 2.5e-3, 0.7, 0, None),
    ('dense_tv_div_24x30', (24, 30), 1500, 3, 'dense', 'bilinear', 'smooth', 4.0, 2000.0, 4000.0, 2.5e-3, 1.0, 0, None),
    ('bigflow_wrapdrop_beta0_30x40', (30, 40), 1500, 2, (2, 2), 'bilinear', 'smooth', 45.0, 20.0, 0.0, 0.0, 0.0, 3, None),
    ('halfpixel_2dof_37x53', (37, 53), 1500, 3, 'halfpixel', 'bilinear', 'constant', 4.0, 20.0, 35.0, 0.0, 0.0, 1, None),
    ('one_event_5x7', (5, 7), 1, 1, (1, 1), 'bilinear', 'constant', 1.0, 20.0, 35.0, 0.0, 0.0, 2, None),
    ('handover_lvl0_20x26', (20, 26), 400, 3, (2, 3), 'bilinear', 'smooth', 3.0, 20.0, 35.0, 2.5e-3, 0.0, 0, 0.3),
    ('handover_lvl2_37x53', (37, 53), 1200, 3, (4, 4), 'bilinear', 'smooth', 5.0, 20.0, 35.0, 0.0, 0.0, 2, 0.6),
]
WARPED_MAX_N = 3000
SPLAT_SIZES = (1, 2, 3, 5, 7)
TILES = ((7, 9), (1, 13), (6, 1), 'sensor')
EDT_FORMULATIONS = ('linear', 'linear-bound', 'logarithmic', 'exponential')


def _case_inputs(i, case):
    name, (H, W), N, R, spec, method, flow, mag = case[:8]
    win = synth.make_window(300 + i, (H, W), N, R, flow=flow, flow_mag=mag)
    edges = win['edges'].astype(np.float32)                      # stored fp32: the recorded inputs are exactly these
    ts = win['ts']
    rng = np.random.default_rng(900 + i)
    if spec == 'dense':
        theta = win['flow_gt'] * rng.uniform(0.5, 1.5, (H, W, 2))
    elif spec == 'halfpixel':
        # theta * dt lands on half-pixels: dyadic times, theta a multiple of 4 -> round-half-even decisions everywhere
        ts = np.sort(rng.integers(0, 9, N)) / 8.0
        theta = np.array([[[4.0, -12.0]]])
    else:
        theta = synth.theta_near_truth(300 + i, win, spec)
    prev = None
    if case[13] is not None:
        prev = theta * rng.uniform(0.6, 1.4, theta.shape)
    return dict(xs=win['xs'], ys=win['ys'], ts=np.asarray(ts, dtype=np.float64), edges=edges,
                edge_ts=win['edge_ts'].astype(np.float64), theta=theta, prev_theta=prev)


def _np(a):
    if isinstance(a, JS.Array):
        a = a.t
    if isinstance(a, torch.Tensor):
        return a.detach().numpy().copy()
    return np.asarray(a)


def _loss_once(ref, inp, case):
    """Run the reference's loss_func (+ objectives, IWEs, handover) under the current convolve mode."""
    name, (H, W), N, R, spec, method = case[:6]
    al, be, ga, de, lvl, ho = case[8:14]
    jnp = JS
    xs, ys = jnp.array(inp['xs']), jnp.array(inp['ys'])
    ts, edge_ts = jnp.array(inp['ts']), jnp.array(inp['edge_ts'])
    edges = jnp.array(inp['edges'].astype(np.float64))
    th = torch.tensor(inp['theta'], dtype=torch.float64, requires_grad=True)
    val, aux = ref['losses'].loss_func(JS.Array(th), xs, ys, ts, edges, edge_ts, al, be, ga, de, lvl, 5, (H, W), method)
    val.t.backward()
    out = {'value': _np(val), 'grad': th.grad.numpy().copy()}
    for k in ('scaled_theta', 'mean_rel_corr', 'mean_rel_contrast', 'mean_rel_iwe_divergence', 'theta_total_variation',
              'multi_ref_weights'):
        out[k] = np.asarray(_np(aux[k]), dtype=np.float64)
    Theta = JS.Array(aux['scaled_theta'].t.detach())
    lo = ref['losses'].compute_loss_objectives(Theta, xs, ys, ts, edges, edge_ts, (H, W))
    for k, v in lo.items():
        if k in ('warped_xs', 'warped_ys'):
            continue
        out['obj_' + k] = np.asarray(_np(v), dtype=np.float64)
    wx, wy = lo['warped_xs'], lo['warped_ys']
    if N <= WARPED_MAX_N:
        out['warped_xs'], out['warped_ys'] = _np(wx), _np(wy)
    pdf = ref['event_utils'].events_to_pdf_frame
    out['iwes'] = np.stack([_np(pdf(wx[r], wy[r], (H, W))) for r in range(R)])
    out['zero_iwe'] = _np(pdf(xs, ys, (H, W)))
    if ho is not None:
        a = torch.tensor(float(ho), dtype=torch.float64, requires_grad=True)
        hv = ref['losses'].handover_loss_func(JS.Array(a), jnp.array(inp['prev_theta']), jnp.array(inp['theta']), xs, ys,
                                              ts, edges, edge_ts, al, be, ga, de, lvl, 5, (H, W), method)
        hv.t.backward()
        out['ho_value'], out['ho_dalpha'] = _np(hv), a.grad.numpy().copy()
    return out


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def record_loss_case(ref, i, case):
    inp = _case_inputs(i, case)
    res = {}
    for mode in JS.CONVOLVE_MODES:
        JS.set_convolve_mode(mode)
        res[mode] = _loss_once(ref, inp, case)
    JS.set_convolve_mode('exact')
    ex = res['exact']
    flagged = sorted(k for k in ex if any(_rel(res[m][k], ex[k]) > ORDER_RTOL for m in ('taps', 'reversed')))
    name, (H, W), N, R, spec, method = case[:6]
    al, be, ga, de, lvl, ho = case[8:14]
    d = dict(xs=inp['xs'], ys=inp['ys'], ts=inp['ts'], edges=inp['edges'], edge_ts=inp['edge_ts'], theta=inp['theta'],
             params=np.array([al, be, ga, de, lvl], dtype=np.float64), method=np.array(method),
             order_sensitive=np.array(flagged, dtype='U64'))
    if ho is not None:
        d['prev_theta'] = inp['prev_theta']
        d['alpha_handover'] = np.float64(ho)
    d.update(ex)
    for m in ('taps', 'reversed'):          # the float-order recordings of the scalar outputs and the gradient
        d[f'{m}_value'] = res[m]['value']
        d[f'{m}_grad'] = res[m]['grad']
        d[f'{m}_theta_total_variation'] = res[m]['theta_total_variation']
    return d, flagged


def record_splat_window(ref):
    """events_to_pdf_frame(..., window_size=s) on one window's warped coordinates, with d sum(IWE * Wt) / d(wx, wy)."""
    H, W, N = 20, 26, 300
    win = synth.make_window(401, (H, W), N, 1, flow='smooth', flow_mag=4.0)
    theta = synth.theta_near_truth(401, win, (2, 2))
    dt = win['ts'] - 1.0
    Th = theta[0, 0]
    wx = win['xs'] - Th[0] * dt + np.random.default_rng(5).normal(0, 0.2, N)
    wy = win['ys'] - Th[1] * dt + np.random.default_rng(6).normal(0, 0.2, N)
    wx[:3] = [-1.4, W + 0.3, 2.5]; wy[:3] = [3.0, H - 0.6, -0.5]          # taps that wrap, drop, and half-pixels
    Wt = np.random.default_rng(7).standard_normal((H, W))
    d = dict(sensor_size=np.array([H, W]), wx=wx, wy=wy, cotangent=Wt, window_sizes=np.array(SPLAT_SIZES))
    for s in SPLAT_SIZES:
        tx = torch.tensor(wx, requires_grad=True)
        ty = torch.tensor(wy, requires_grad=True)
        img = ref['event_utils'].events_to_pdf_frame(JS.Array(tx), JS.Array(ty), (H, W), window_size=s)
        (img.t * torch.from_numpy(Wt)).sum().backward()
        d[f'iwe_s{s}'] = _np(img)
        d[f'gwx_s{s}'] = tx.grad.numpy().copy()
        d[f'gwy_s{s}'] = ty.grad.numpy().copy()
    return d


def record_objective_kinds(ref):
    """The reference's tiled and pairwise objectives on a recorded IWE / edge pair; values and d/d(IWE)."""
    H, W = 20, 26
    win = synth.make_window(402, (H, W), 600, 1, flow='smooth', flow_mag=3.0)
    iwe = _np(ref['event_utils'].events_to_pdf_frame(JS.array(win['xs']), JS.array(win['ys']), (H, W)))
    edge = win['edges'][0].astype(np.float32).astype(np.float64)
    co, cr = ref['contrast'], ref['correlation']
    d = dict(iwe=iwe, edge=edge.astype(np.float32))
    tiles = []
    for tile in TILES:
        tile = (H, W) if tile == 'sensor' else tile
        tiles.append(tile)
        tag = f'{tile[0]}x{tile[1]}'
        fns = {
            'adaptive_mean_gradient_magnitude': lambda x: co.compute_adaptive_mean_gradient_magnitude(x, tile),
            'adaptive_variance': lambda x: co.compute_adaptive_variance(x, tile),
            'adaptive_mean_squared_error': lambda x: cr.compute_adaptive_mean_squared_error(JS.array(edge), x, tile),
        }
        for k, f in fns.items():
            t = torch.tensor(iwe, requires_grad=True)
            v = f(JS.Array(t))
            v.t.backward()
            d[f'{k}_{tag}'] = _np(v)
            d[f'd_{k}_{tag}'] = t.grad.numpy().copy()
    for k, f in (('mean_hadamard_product', cr.compute_mean_hadamard_product), ('joint_contrast', cr.compute_joint_contrast)):
        t = torch.tensor(iwe, requires_grad=True)
        v = f(JS.array(edge), JS.Array(t))
        v.t.backward()
        d[k] = _np(v)
        d['d_' + k] = t.grad.numpy().copy()
    d['tiles'] = np.array(tiles)
    return d


def record_edge_maps(ref):
    """eincm_inv_exp_dist_transform and RTEF_IEDT(...).compute_edge_iedt on two small binary edge images (numpy/scipy only)."""
    img = ref['img_utils']
    e1 = np.zeros((9, 11), dtype=np.uint8)
    e1[2, 1:7] = 1; e1[6, 8] = 1; e1[3:8, 4] = 1
    e0 = np.zeros((6, 7), dtype=np.uint8)                      # no edge pixel at all
    d = dict(edge_a=e1, edge_empty=e0)
    d['eincm_a'] = img.eincm_inv_exp_dist_transform(e1)
    d['eincm_empty'] = img.eincm_inv_exp_dist_transform(e0)
    for f in EDT_FORMULATIONS:
        d[f'rtef_{f}_a'] = img.RTEF_IEDT(6.0, None, f).compute_edge_iedt(e1)
        # compute_edge_iedt asserts a two-valued image, so the empty image has no RTEF recording (img_utils.py:403-405)
    return d


def load_reference(src):
    sys.dont_write_bytecode = True
    JS.install()
    sys.path.insert(0, os.path.abspath(src))
    mods = dict(losses='eincm.losses', event_utils='utils.event_utils', contrast='eincm.objectives.contrast_objectives',
                correlation='eincm.objectives.correlation_objectives', img_utils='utils.img_utils')
    return {k: importlib.import_module(v) for k, v in mods.items()}


def _header(kind):
    return np.array(f'ref_{kind}: recorded from the reference\'s own code (float64, jax primitives served by '
                    f'oracle/jax_standin.py, convolve mode exact) by: {CMD}')


def write_all(ref, out_dir):
    written = []
    for i, case in enumerate(LOSS_CASES):
        d, flagged = record_loss_case(ref, i, case)
        d['provenance'] = _header(case[0])
        path = os.path.join(out_dir, f'ref_{case[0]}.npz')
        np.savez_compressed(path, **d)
        written.append(path)
        print(f'{case[0]:34s} value {float(d["value"]): .17g}  order-sensitive: {", ".join(flagged) or "-"}')
    for kind, fn in (('splat_window', record_splat_window), ('objective_kinds', record_objective_kinds),
                     ('edge_maps', record_edge_maps)):
        d = fn(ref)
        d['provenance'] = _header(kind)
        path = os.path.join(out_dir, f'ref_{kind}.npz')
        np.savez_compressed(path, **d)
        written.append(path)
        print(f'{kind:34s} recorded')
    return written


def compare(new_dir, old_dir):
    bad = []
    for p in sorted(os.listdir(new_dir)):
        a = dict(np.load(os.path.join(new_dir, p), allow_pickle=False))
        op = os.path.join(old_dir, p)
        if not os.path.exists(op):
            bad.append(f'{p}: not committed')
            continue
        b = dict(np.load(op, allow_pickle=False))
        if set(a) != set(b):
            bad.append(f'{p}: keys differ {sorted(set(a) ^ set(b))}')
            continue
        for k in a:
            if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
                bad.append(f'{p}:{k}: shape/dtype')
            elif a[k].dtype.kind in 'fc':
                if not np.array_equal(a[k], b[k]) and _rel(a[k], b[k]) > CHECK_RTOL:
                    bad.append(f'{p}:{k}: rel {_rel(a[k], b[k]):.3g}')
            elif not np.array_equal(a[k], b[k]):
                bad.append(f'{p}:{k}: differs')
    committed = {p for p in os.listdir(old_dir) if p.startswith('ref_') and p.endswith('.npz')}
    bad += [f'{p}: committed but no longer produced' for p in sorted(committed - set(os.listdir(new_dir)))]
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-src', required=True)
    ap.add_argument('--check', action='store_true')
    a = ap.parse_args()
    ref = load_reference(a.reference_src)
    if not a.check:
        for p in write_all(ref, HERE):
            print(os.path.basename(p), os.path.getsize(p))
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        write_all(ref, tmp)
        bad = compare(tmp, HERE)
    for b in bad:
        print('MISMATCH', b)
    print('check:', 'FAILED' if bad else 'all fixtures reproduced')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
