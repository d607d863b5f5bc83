"""The repository's CPU references against outputs recorded from the reference's own code (tests/golden/ref_*.npz;
provenance in tests/golden/make_reference_golden.py).  Reads only the fixtures; no GPU.

numpy oracle and torch witness: value <= 1e-12 relative, gradient <= 1e-10 max-norm relative, IWEs, scaled theta and the
objectives dict <= 1e-12.  Every output is compared with the 'exact'-convolution recording, the order-sensitive ones included:
this is what checks the oracle's difference-first Scharr form on locally constant flow.
"""
import numpy as np
import pytest
import torch

from oracle import eincm_c_port as CP
from oracle import eincm_oracle as O
from oracle import eincm_torch as T
from oracle import edge_smoothing as ES
import _objective_kinds_witness as WIT
import _splat_window_witness as SW
from _reference_golden import edge_maps, load_loss_case, loss_case_names, objective_kinds, splat_window

NAMES = loss_case_names()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _oracle(d, theta=None):
    k = d['kw']
    return O.loss_and_grad(d['theta'] if theta is None else theta, *d['window'], k['alpha'], k['beta'], k['gamma'], k['delta'],
                           k['cur_pyr_lvl'], 5, d['sensor_size'], k['method'], return_intermediates=True)


def _mats(d):
    h, w = d['theta'].shape[:2]
    H, W = d['sensor_size']
    m = d['kw']['method']
    return O.resample_matrix(h, H, H / h, m), O.resample_matrix(w, W, W / w, m)


def test_fixture_set():
    assert len(NAMES) >= 12
    flagged = [n for n in NAMES if load_loss_case(n)['order_sensitive']]
    # the case matrix must hold outputs that depend on the convolution's summation order (2-DoF and bilinear grids at level 0)
    assert any(n.startswith('2dof_lvl0') for n in flagged) and any(n.startswith('bilinear') for n in flagged), flagged


@pytest.mark.parametrize('name', NAMES)
def test_numpy_oracle_reproduces_the_reference(name):
    d = load_loss_case(name)
    H, W = d['sensor_size']
    val, grad, aux = _oracle(d)
    assert abs(val - d['value']) <= 1e-12 * abs(d['value']), (val, d['value'])
    assert rel(grad, d['grad']) <= 1e-10
    assert rel(aux['scaled_theta'], d['scaled_theta']) <= 1e-12
    assert rel(aux['_iwes'], d['iwes']) <= 1e-12
    assert rel(aux['_zero_iwe'], d['zero_iwe']) <= 1e-12
    for k in ('mean_rel_corr', 'mean_rel_contrast', 'mean_rel_iwe_divergence', 'theta_total_variation'):
        assert aux[k] == pytest.approx(d[k], rel=1e-12, abs=1e-300), k
    assert rel(aux['multi_ref_weights'], d['multi_ref_weights']) <= 1e-12
    lo = O.compute_loss_objectives(d['scaled_theta'], *d['window'], (H, W))
    for k, want in d['objectives'].items():
        assert rel(lo[k], want) <= 1e-12 or (np.abs(want).max() == 0 and np.abs(lo[k]).max() == 0), k
    if 'warped_xs' in d:
        assert rel(lo['warped_xs'], d['warped_xs']) <= 1e-12 and rel(lo['warped_ys'], d['warped_ys']) <= 1e-12
        for r in range(len(d['edge_ts'])):
            wx, wy = d['warped_xs'][r], d['warped_ys'][r]
            # count image built directly with numpy: round half to even, wrap [-n, -1], drop the rest
            cx, cy = np.rint(wx).astype(np.int64), np.rint(wy).astype(np.int64)
            cx = np.where(cx < 0, cx + W, cx)
            cy = np.where(cy < 0, cy + H, cy)
            ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            want = np.zeros((H, W), dtype=np.int64)
            np.add.at(want, (cy[ok], cx[ok]), 1)
            assert np.array_equal(O.rounded_count_image(wx, wy, (H, W)), want), r


@pytest.mark.parametrize('name', NAMES)
def test_torch_witness_reproduces_the_reference(name):
    d = load_loss_case(name)
    k = d['kw']
    v, g = T.loss_and_grad(d['theta'], *d['window'], k['alpha'], k['beta'], k['gamma'], k['delta'], k['cur_pyr_lvl'],
                           d['sensor_size'], *_mats(d))
    assert abs(v - d['value']) <= 1e-12 * abs(d['value'])
    assert rel(g, d['grad']) <= 1e-10


@pytest.mark.parametrize('name', NAMES)
def test_objective_kinds_and_splat_witnesses_reproduce_the_reference(name):
    d = load_loss_case(name)
    k = d['kw']
    args = (d['theta'], *d['window'], k['alpha'], k['beta'], k['gamma'], k['delta'], k['cur_pyr_lvl'], *_mats(d))
    v, g = WIT.loss_and_grad(*args, 0, 0)[:2]
    assert abs(v - d['value']) <= 1e-12 * abs(d['value'])
    assert rel(g, d['grad']) <= 1e-10
    v, g = SW.loss_and_grad(*args, window_size=3)[:2]
    assert abs(v - d['value']) <= 1e-12 * abs(d['value'])
    assert rel(g, d['grad']) <= 1e-10


C_PORT = [n for n in NAMES if load_loss_case(n)['kw']['delta'] == 0.0
          and (load_loss_case(n)['kw']['gamma'] == 0.0 or load_loss_case(n)['kw']['cur_pyr_lvl'] > 0)]


@pytest.mark.parametrize('name', C_PORT)
def test_c_port_reproduces_the_reference(name):
    """The C port computes loss_func with gamma = delta = 0 (tests/test_oracle_c_port.py's tolerances)."""
    d = load_loss_case(name)
    k = d['kw']
    v, g = CP.loss_and_grad(d['theta'], *d['window'], k['alpha'], k['beta'], d['sensor_size'], k['method'], nthreads=2)
    assert v == pytest.approx(d['value'], rel=1e-12)
    assert np.abs(g - d['grad']).max() <= 1e-10 * np.abs(d['grad']).max()


@pytest.mark.parametrize('name', [n for n in NAMES if n.startswith('handover')])
def test_oracle_handover_reproduces_the_reference(name):
    d = load_loss_case(name)
    k = d['kw']
    v, dv = O.handover_loss_and_grad(d['alpha_handover'], d['prev_theta'], d['theta'], *d['window'], k['alpha'], k['beta'],
                                     k['gamma'], k['delta'], k['cur_pyr_lvl'], 5, d['sensor_size'], k['method'])
    assert abs(v - d['ho_value']) <= 1e-12 * abs(d['ho_value'])
    assert abs(dv - d['ho_dalpha']) <= 1e-10 * abs(d['ho_dalpha'])


def test_splat_window_witness_reproduces_the_reference():
    d = splat_window()
    H, W = (int(v) for v in d['sensor_size'])
    for s in d['window_sizes']:
        wx = torch.tensor(d['wx'], requires_grad=True)
        wy = torch.tensor(d['wy'], requires_grad=True)
        img = SW.splat(wx, wy, H, W, int(s))
        (img * torch.from_numpy(d['cotangent'])).sum().backward()
        assert rel(img.detach().numpy(), d[f'iwe_s{s}']) <= 1e-12, s
        assert rel(wx.grad.numpy(), d[f'gwx_s{s}']) <= 1e-12, s
        assert rel(wy.grad.numpy(), d[f'gwy_s{s}']) <= 1e-12, s
        if s == 3:
            assert rel(O.events_to_pdf_frame(d['wx'], d['wy'], (H, W)), d['iwe_s3']) <= 1e-12
            gx, gy = O.events_to_pdf_frame_adjoint(d['cotangent'], d['wx'], d['wy'])
            assert rel(gx, d['gwx_s3']) <= 1e-12 and rel(gy, d['gwy_s3']) <= 1e-12


def test_objective_kinds_witness_reproduces_the_reference():
    d = objective_kinds()
    E = torch.from_numpy(d['edge'])
    for tile in d['tiles']:
        tile = (int(tile[0]), int(tile[1]))
        tag = f'{tile[0]}x{tile[1]}'
        for key, fn in (('adaptive_mean_gradient_magnitude', lambda x: WIT.contrast_t(x, 2, tile)),
                        ('adaptive_variance', lambda x: WIT.contrast_t(x, 3, tile)),
                        ('adaptive_mean_squared_error', lambda x: -WIT.correlation_t(E, x, 1, tile))):
            for form in ('vector', 'loop'):
                x = torch.tensor(d['iwe'], requires_grad=True)
                f = fn(x) if form == 'vector' else {'adaptive_mean_gradient_magnitude': lambda: WIT.contrast_t(x, 2, tile, 'loop'),
                                                     'adaptive_variance': lambda: WIT.contrast_t(x, 3, tile, 'loop'),
                                                     'adaptive_mean_squared_error': lambda: -WIT.correlation_t(E, x, 1, tile, 'loop')}[key]()
                f.backward()
                assert float(f) == pytest.approx(float(d[f'{key}_{tag}']), rel=1e-12), (key, tag, form)
                assert rel(x.grad.numpy(), d[f'd_{key}_{tag}']) <= 1e-12, (key, tag, form)
    for key, kind in (('mean_hadamard_product', 2), ('joint_contrast', 3)):
        x = torch.tensor(d['iwe'], requires_grad=True)
        f = WIT.correlation_t(E, x, kind)
        f.backward()
        assert float(f) == pytest.approx(float(d[key]), rel=1e-12), key
        assert rel(x.grad.numpy(), d['d_' + key]) <= 1e-12, key


def test_edge_map_oracle_reproduces_the_reference():
    d = edge_maps()
    assert rel(ES.eincm_inv_exp_dist_transform(d['edge_a']), d['eincm_a']) <= 1e-15
    # an edge-free image: scipy's transform has no background pixel to measure to; the oracle calls it the same way
    assert rel(ES.eincm_inv_exp_dist_transform(d['edge_empty']), d['eincm_empty']) <= 1e-15
    for f in ('linear', 'linear-bound', 'logarithmic', 'exponential'):
        assert rel(ES.rtef_inv_exp_dist_transform(d['edge_a'], 6.0, None, f), d[f'rtef_{f}_a']) <= 1e-15, f
