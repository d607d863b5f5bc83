"""Canny without a GPU: known answers of the numpy witness, argument checks that run before any GPU call,
the C-ABI symbol, and the staging path with ready edges."""
import importlib
import os
import re

import numpy as np
import pytest

import _canny_witness as CW

pkg = 'edge-informed-contrast-maximization_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(shape, axis, at, lo=20, hi=220):
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((xx if axis == 1 else yy) >= at, hi, lo).astype(np.uint8)


def test_vertical_step_gives_one_line_at_the_expected_column():
    img = _step((12, 16), 1, 8)
    out = CW.canny(img, 30, 80)
    # dx is 4 * 200 at columns 7 and 8 (equal magnitudes): the tie rule keeps the first, column 7
    assert np.array_equal(np.nonzero(out.any(axis=0))[0], [7])
    assert np.all(out[:, 7] == 255)


def test_horizontal_step_uses_the_vertical_branch():
    out = CW.canny(_step((16, 12), 0, 8), 30, 80)
    assert np.array_equal(np.nonzero(out.any(axis=1))[0], [7]) and np.all(out[7] == 255)


def test_diagonal_step_uses_the_diagonal_branch():
    H = W = 16
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.where(xx - yy >= 0, 200, 20).astype(np.uint8)         # 45 degree step: |dx| = |dy| inside
    surv, _ = CW.survivors(img, 30, 80)
    dx, dy = CW.sobel(img)
    inner = (slice(2, -2), slice(2, -2))
    d = (np.abs(dx) == np.abs(dy)) & (dx != 0)
    assert d[inner].any()
    assert np.all((dx[inner] ^ dy[inner])[d[inner]] < 0)              # s = -1: neighbours (r-1, c+1) and (r+1, c-1)
    assert (surv & d)[inner].any()                                     # survivors decided by the diagonal test
    out = CW.canny(img, 30, 80)
    on = np.argwhere(out[inner] == 255) + 2
    assert len(on) > 0 and set((on[:, 1] - on[:, 0]).tolist()) == {-1, 0}     # one staircase along the diagonal


def test_two_pixel_plateau_keeps_the_pixel_the_tie_rule_names():
    img = np.zeros((7, 10), np.uint8)
    img[:, 5:] = 100                                                # magnitude plateau over columns 4 and 5
    dx, _ = CW.sobel(img)
    assert dx[3, 4] == dx[3, 5] == 400
    out = CW.canny(img, 10, 20)
    assert np.all(out[:, 4] == 255) and not out[:, 5].any()
    # the same plateau along y keeps the upper row
    out_t = CW.canny(np.ascontiguousarray(img.T), 10, 20)
    assert np.all(out_t[4] == 255) and not out_t[5].any()


def test_swapped_thresholds_equal_the_ordered_call():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 31)).astype(np.uint8)
    assert np.array_equal(CW.canny(img, 200, 100), CW.canny(img, 100, 200))
    assert np.array_equal(CW.canny(img, 80, 30, False), CW.canny(img, 30, 80, False))
    assert CW.thresholds(80, 30) == (900, 6400) and CW.thresholds(1e6, 0.5, False) == (0, 32767)


def test_constant_and_single_pixel_images_are_empty():
    assert not CW.canny(np.full((9, 13), 77, np.uint8), 1, 2).any()
    assert not CW.canny(np.full((1, 1), 200, np.uint8), 0, 0).any()
    row = np.array([[0, 0, 0, 200, 200, 200]], np.uint8)            # 1 x N and N x 1: replicate borders, first of the tie
    assert CW.canny(row, 30, 80).tolist() == [[0, 0, 255, 0, 0, 0]]
    assert CW.canny(np.ascontiguousarray(row.T), 30, 80)[:, 0].tolist() == [0, 0, 255, 0, 0, 0]


def _chain_image(cut):
    """A diagonal-free weak chain along row 5, strong only at its left end; `cut` removes one pixel of the chain."""
    img = np.zeros((11, 30), np.uint8)
    img[6:, :] = 20                                                 # weak step: |dy| = 80, m = 6400
    img[6:, :3] = 60                                                # strong at the left end
    if cut:
        img[6:, 15] = 0                                             # no gradient at column 15: the chain breaks there
        img[:, 15] = 0
    return img


def test_weak_chain_survives_through_a_strong_pixel_and_dies_when_cut():
    surv, strong = CW.survivors(_chain_image(False), 50, 150)
    assert strong.any() and (surv & ~strong).sum() > 20
    out = CW.canny(_chain_image(False), 50, 150)
    assert np.array_equal(out == 255, surv)
    surv_c, strong_c = CW.survivors(_chain_image(True), 50, 150)
    out_c = CW.canny(_chain_image(True), 50, 150)
    assert not surv_c[:, 15].any() and strong_c[:, :15].any() and not strong_c[:, 16:].any()
    assert out_c[:, :15].any() and not out_c[:, 16:].any() and surv_c[:, 16:].any()


@pytest.mark.parametrize('kw, match', [
    ({'apert_size': 5}, 'aperture_size'), ({'apert_size': 7}, 'aperture_size'), ({'apert_size': -1}, 'aperture_size'),
    ({'th1': -1.0}, 'threshold1'), ({'th2': -0.5}, 'threshold2'), ({'th1': float('nan')}, 'threshold1'),
    ({'th2': float('inf')}, 'threshold2')])
def test_arguments_refused_before_any_gpu_call(kw, match):
    edges = importlib.import_module(pkg + '.edges')
    with pytest.raises(ValueError, match=match):
        edges.image_to_edge(np.zeros((8, 8), np.uint8), **kw)
    E = importlib.import_module(pkg + '.engine')
    with pytest.raises(ValueError, match=match):
        E.check_canny_args(kw.get('th1', 30), kw.get('th2', 80), kw.get('apert_size', 3))


def test_symbol_in_header_and_binding():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    assert re.search(r'int eincm_canny\(eincm_ctx\* ctx, const uint8_t\* src, int n, double threshold1, double threshold2, '
                     r'int aperture_size, int l2_gradient,\s*uint8_t\* dst\);', txt)
    L = importlib.import_module(pkg + '._lib')
    assert [n for n, _, _ in L.SIGNATURES].count('eincm_canny') == 1


def test_to_canny_input_min_max_and_truncation():
    edges = importlib.import_module(pkg + '.edges')
    a = np.array([[0.0, 0.5], [0.25, 1.0]])
    assert edges.to_canny_input(a).tolist() == [[0, 127], [63, 255]]
    assert edges.to_canny_input(np.full((3, 3), 0.4)).tolist() == [[0] * 3] * 3     # range <= DBL_EPSILON: scale 0
    img = np.random.default_rng(0).random((20, 30))
    assert np.array_equal(edges.to_canny_input(img), CW.to_canny_input(img))


def test_stage_datasample_with_ready_edges_is_unchanged():
    staging = importlib.import_module(pkg + '.staging')
    rng = np.random.default_rng(1)
    ds = {'events': {'x': np.array([1, 2, 3]), 'y': np.array([4, 5, 6]), 't': np.array([1000.0, 1500.0, 2000.0])},
          'image_ts': np.array([1000.0, 2000.0]), 'eval_ts': (1000.0, 2000.0),
          'images': rng.integers(0, 256, (2, 6, 7)).astype(np.uint8)}
    e = [rng.random((6, 7)) * 3.0, rng.random((6, 7))]
    xs, ys, ts, edges, ets = staging.stage_datasample(ds, e)
    ts_ref, ets_ref = staging.normalize_times(ds['events']['t'], ds['image_ts'], 1000.0, 2000.0)
    assert np.array_equal(edges, staging.normalize_edges(e)) and np.array_equal(ts, ts_ref) and np.array_equal(ets, ets_ref)
    assert xs.tolist() == [1, 2, 3] and ys.tolist() == [4, 5, 6]
    for k in range(2):
        eps = np.finfo(np.float64).eps
        assert np.array_equal(edges[k], (e[k] - e[k].min()) / (e[k].max() - e[k].min() + eps))
    with pytest.raises(TypeError, match='ready edges'):
        staging.stage_datasample(ds, e, k_size=1)
