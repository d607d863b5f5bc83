"""The bound of the fused motion path's gradient, stated once for tests/test_gpu_motion_fused.py and the motion
sweep of tests/dev/fuzz_gpu.py: the slots of a window's moment partials, the exact moments of a dense gradient, and the bound of
|fused gradient - (exact moments) M| that follows from the summation scheme built.  Nothing in the bound is fitted."""
import math

import numpy as np

import _launch_policy_witness as LP

U = 2.0 ** -53


def slots_per_window(wins, shape, R):
    """(slots of every window's moment partials, all_r): a slot per (segment of the gather's list, reference time), or per segment where
    one workgroup walks all reference times (700 segments and more: csrc/eincm_plan.h, plan_motion)."""
    H, W = shape
    segs = np.array([len(LP.segment_lengths(LP.tile_counts(w['xs'], w['ys'], H, W), LP.SEG_LONG)) for w in wins])
    all_r = R > 1 and segs.sum() >= 700
    return segs * (1 if all_r else R), all_r


def exact_moments(model, dense_grad):
    """(mu (B, 12), sum|m_j g| (B, 12)): the moments of a dense gradient, every sum exact (math.fsum) and rounded once."""
    H, W = model.sensor_size
    mono = [np.broadcast_to(m, (H, W)) for m in (np.ones((1, 1)),) + model.monomials()]
    G = np.asarray(dense_grad, dtype=np.float64)
    mu = np.array([[math.fsum((m * G[b, :, :, a]).ravel().tolist()) for a in range(2) for m in mono] for b in range(G.shape[0])])
    mu_abs = np.array([[math.fsum((np.abs(m) * np.abs(G[b, :, :, a])).ravel().tolist()) for a in range(2) for m in mono] for b in range(G.shape[0])])
    return mu, mu_abs


def moment_bound(model, dense_grad, slots):
    """|fused gradient - (exact moments) M| is at most this.  A moment is an ordered float64 sum of rounded products m_j(p) g: a thread
    adds its 2 pixels (512 threads, 1024 pixels), the wave tree has 6 levels, the 8 waves are added in index order, and the host adds
    the window's `slots` partials in index order - the longest chain of additions an addend goes through is n = 2 + 6 + 8 + slots; the
    rounding of the product and of the i64 -> fp64 conversion of a 61-bit sum make it n + 2.  Such a sum is within n 2^-53 sum|m_j g|
    of the exact one to first order; the bound has the form of sections 17 and 20, 2 n 2^-53 sum|m_j g|, carried through |M|, plus the
    2 * 12 * 2^-53 sum_j |M_jk mu_j| of the two 12-term sums M^T mu (the fused one and this reference's).  Nothing is fitted."""
    mu, mu_abs = exact_moments(model, dense_grad)
    n = 2 + 6 + 8 + np.asarray(slots, dtype=np.float64) + 2
    absM = np.abs(model.matrix)
    return mu @ model.matrix, (2.0 * n[:, None] * U * mu_abs) @ absM + 2.0 * 12 * U * (np.abs(mu) @ absM)
