"""The witness of the batched flow-error evaluation (tests/_flow_error_witness.py) against evaluation.sparse_flow_error, the numpy
restatement of the reference's flow_eval.py that the package already has.  No GPU.

Counts and the six over-threshold counts are integers and must be equal; A{N}PE is one division of equal integers and must have equal
bits.  AEE and AREE are means of the SAME non-negative float64 terms summed in two orders (numpy's pairwise order there, the kernel's
thread chains and trees here).  A sum of n non-negative terms in any order is within (n - 1) u of the exact sum, relative, u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, to first order), so two orders differ by at most 2 (n - 1) u <
n 2^-52 relative; the division by n_ee rounds once more on each side, which the slack between 2 (n - 1) u and n 2^-52 = 2 n u covers
(2 u).  The tolerance is derived, not measured; the measured differences are printed."""
import importlib

import numpy as np
import pytest

import _flow_error_witness as FW

pkg = 'edge-informed-contrast-maximization_amd'
ev = importlib.import_module(pkg + '.evaluation')


def reference(theta, gt, events, mask=None):
    """sparse_flow_error on per_pix_theta_to_flow, and the reference's own per-pixel terms for the counts it does not return."""
    with np.errstate(all='ignore'):
        pred = ev.per_pix_theta_to_flow(theta, events[0], events[1])
        r = ev.sparse_flow_error(pred, gt, mask)
        mp = (~np.isinf(pred[..., 0])) & (~np.isinf(pred[..., 1])) & (np.linalg.norm(pred, axis=-1) > 0)
        if mask is not None:
            mp = mp & np.asarray(mask, dtype=bool)
        mg = (~np.isinf(gt[..., 0])) & (~np.isinf(gt[..., 1])) & (np.linalg.norm(gt, axis=-1) > 0)
        both = mp & mg
        ee = np.linalg.norm(pred[both] - gt[both], axis=-1)
    return r, both, ee


def compare(theta, gt, events, mask=None):
    w = FW.flow_errors(theta, gt, events, mask)
    r, both, ee = reference(theta, gt, events, mask)
    assert {k: w[k] for k in ('n_ee', 'n_pred', 'n_gt')} == r['counts']
    assert w['n_over'] == [int((ee > n).sum()) for n in FW.THRESHOLDS]
    for k, n in enumerate(FW.THRESHOLDS):
        assert np.float64(w['anpe'][k]).tobytes() == np.float64(r['errors'][f'A{n}PE']).tobytes(), n
    # numpy's own terms, bit for bit, and NaN exactly outside the intersection
    assert np.array_equal(np.isnan(w['ee_map']), ~both)
    assert w['ee_map'][both].tobytes() == ee.tobytes()
    n_ee = w['n_ee']
    if n_ee == 0:
        assert np.isnan(w['aee']) and np.isnan(w['aree']) and np.isnan(r['errors']['AEE']) and np.isnan(r['errors']['AREE'])
        assert w['anpe'] == [0.0] * 6
        return w
    tol = n_ee * 2.0 ** -52
    for mine, theirs in ((w['aee'], r['errors']['AEE']), (w['aree'], r['errors']['AREE'])):
        rel = abs(mine - theirs) / abs(theirs)
        print(f'n_ee {n_ee}: relative difference {rel:.3g}, bound {tol:.3g}')
        assert rel <= tol
    return w


@pytest.mark.parametrize('shape', [(37, 53), (64, 80)])
@pytest.mark.parametrize('special', [False, True])
def test_random_fields(shape, special):
    H, W = shape
    for seed in range(3):
        theta, gt, events = FW.random_case(seed, H, W, special=special)
        compare(theta, gt, events)
        mask = np.random.default_rng(100 + seed).random((H, W)) < 0.6
        compare(theta, gt, events, mask)
        a = FW.flow_errors(theta, gt, events)
        b = FW.flow_errors(theta, gt, events, np.ones((H, W), np.uint8))
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_constructed_window():
    theta, gt, events, expect = FW.special_case()
    w = compare(theta, gt, events)
    for k, v in expect.items():
        assert w[k] == v, k
    # strict comparison: the six pixels whose ee equals a threshold
    assert w['ee_map'][2, :6].tolist() == [1.0, 2.0, 3.0, 5.0, 10.0, 20.0]
    assert all(w['ee_map'][2, 6 + k] > n for k, n in enumerate(FW.THRESHOLDS))
    # an underflowing predicted flow is excluded, as the reference excludes it; a tiny one whose norm survives is not
    assert np.isnan(w['ee_map'][1, 4]) and not np.isnan(w['ee_map'][1, 6])
    # the event-less pixels are outside, whatever their vectors
    assert np.isnan(w['ee_map'][3, 0]) and np.isnan(w['ee_map'][3, 1]) and w['ee_map'][3, 2] == np.sqrt(2.0)


def test_empty_windows():
    theta, gt, _ = FW.random_case(5, 9, 11, special=False)
    none = (np.zeros(0, np.int16), np.zeros(0, np.int16))
    w = compare(theta, gt, none)
    assert (w['n_ee'], w['n_pred']) == (0, 0) and w['n_gt'] == 99
    # events, but an empty intersection: the mask removes every event pixel
    _, _, events = FW.random_case(5, 9, 11, special=False)
    w = compare(theta, gt, events, np.zeros((9, 11), bool))
    assert w['n_ee'] == 0 and np.isnan(w['aee']) and w['anpe'] == [0.0] * 6


def test_ordered_sum_is_the_stated_order():
    """Known answers of the order itself: with terms 2^53 and 1 the result depends on who meets whom first."""
    big = 2.0 ** 53
    t = np.zeros(3 * 8192)
    t[0], t[8192], t[2 * 8192] = big, 1.0, 1.0            # one thread's chain: (big + 1) + 1 loses both ones
    assert FW.ordered_sum(t) == big
    t = np.zeros(8192)
    t[0], t[1], t[33] = big, 1.0, 1.0                     # lanes 0, 1, 33 of one wave: 1 + 33 meet at o = 32, then join lane 0 at o = 1
    assert FW.ordered_sum(t) == big + 2.0
    t = np.zeros(8192)
    t[0], t[64], t[128] = big, 1.0, 1.0                   # waves 0, 1, 2 of one workgroup, added in index order: both ones are lost
    assert FW.ordered_sum(t) == big
    t = np.zeros(8192)
    t[0], t[256], t[512] = big, 1.0, 1.0                  # workgroups 0, 1, 2 in index order: lost again
    assert FW.ordered_sum(t) == big
    t[0], t[256], t[257] = big, 1.0, 1.0                  # two ones in ONE workgroup meet first
    t[512] = 0.0
    assert FW.ordered_sum(t) == big + 2.0


def test_upsample_tap_order_matches_the_matrix_product(built_lib):
    """The tap-ordered field is within 1e-13 of A_H theta A_W^T (the project's tolerance for scaled_theta), for every method."""
    E = importlib.import_module(pkg + '.engine')
    rng = np.random.default_rng(3)
    H, W = 37, 53
    for method in ('bilinear', 'cubic', 'lanczos3', 'lanczos5'):
        for h, w in ((1, 1), (2, 2), (4, 4), (5, 3), (16, 16)):
            theta = rng.normal(0, 5, size=(h, w, 2))
            A_H, A_W = E.resample_matrix(h, H, method), E.resample_matrix(w, W, method)
            got = FW.upsample(theta, A_H, A_W)
            want = np.einsum('yi,xj,ijc->yxc', A_H, A_W, theta)
            assert np.abs(got - want).max() <= 1e-13, (method, h, w)
