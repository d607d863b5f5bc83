"""Independent fp64 witness of the loss with per-event weights: torch float64 forward, gradient by autograd.

Test helper only.  tests/_splat_window_witness.py's loss_from_Theta / loss_and_grad / objectives at the 3x3 splat window with three
changes: every tap of event e is w_e * exp(-|q|^2 / 2) / (2 pi), in the zero-warp IWE too; the TV event mask is built from the events
with w_e > 0; and the weights are the float32 values the engine stages (check_event_weights' rounding), widened to fp64.  No weights
stands for ones.  Normalisation, Scharr, divergence and TV come from oracle/eincm_torch.py, the kinds from
tests/_objective_kinds_witness.py (both imported read-only).
"""
import math

import numpy as np
import torch

from oracle import eincm_torch as T
import _objective_kinds_witness as WIT

EPSN = T.EPSN
_DT = torch.float64
LOG_2PI = math.log(2.0 * math.pi)


def staged_weights(weights, n):
    """The weights as the engine sees them: float32 once, widened to fp64 (ones when None)."""
    if weights is None:
        return np.ones(int(n), dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).astype(np.float32).astype(np.float64)
    assert w.shape == (int(n),)
    return w


def splat(wx, wy, wgt, H, W):
    """sum_e wgt_e * k_e(p) as an (H, W) tensor: events_to_pdf_frame(wx, wy, (H, W), 3) with every tap scaled by its event's weight."""
    rx = torch.round(wx.detach()).to(torch.int64)
    ry = torch.round(wy.detach()).to(torch.int64)
    frame = torch.zeros(H * W, dtype=_DT)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            px = rx + dx
            py = ry + dy
            qx = px.to(_DT) - wx
            qy = py.to(_DT) - wy
            k = wgt * torch.exp(-0.5 * (qx * qx + qy * qy) - LOG_2PI)
            px = torch.where(px < 0, px + W, px)
            py = torch.where(py < 0, py + H, py)
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            idx = torch.where(ok, py * W + px, torch.zeros_like(px))
            frame = frame.index_put((idx,), torch.where(ok, k, torch.zeros_like(k)), accumulate=True)
    return frame.reshape(H, W)


def loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, weights=None, contrast_kind=0,
                    correlation_kind=0, tile=WIT.DEFAULT_TILE, images=None, terms=None):
    """losses.py:162-193 on a full-resolution Theta (H,W,2) tensor with weighted events.  images: receives the IWE tensors
    (retain_grad: .grad is dL/dIWE after backward).  terms: receives the zero-warp values and the per-image values as floats."""
    H, W, _ = Theta.shape
    xi = torch.as_tensor(np.asarray(xs).astype(np.int64))
    yi = torch.as_tensor(np.asarray(ys).astype(np.int64))
    t = torch.as_tensor(np.asarray(ts, dtype=np.float64))
    E = torch.as_tensor(np.asarray(edges, dtype=np.float64))
    tau = np.atleast_1d(np.asarray(edge_ts, dtype=np.float64))
    wn = staged_weights(weights, len(xi))
    wgt = torch.as_tensor(wn)
    R = len(tau)
    w = T._weights(R)
    with torch.no_grad():
        I0 = splat(xi.to(_DT), yi.to(_DT), wgt, H, W)
    n0 = T._normalize(I0)
    c0 = WIT.contrast_t(I0, contrast_kind, tile)
    d0 = T._iwe_div(n0)
    vx = Theta[yi, xi, 0]
    vy = Theta[yi, xi, 1]
    rel_con, rel_corr, rel_div, per = [], [], [], []
    for r in range(R):
        dts = t - float(tau[r])
        I = splat(xi.to(_DT) - vx * dts, yi.to(_DT) - vy * dts, wgt, H, W)
        if images is not None:
            if I.requires_grad:
                I.retain_grad()
            images.append(I)
        n = T._normalize(I)
        zc = WIT.correlation_t(E[r], n0, correlation_kind, tile)
        corr = WIT.correlation_t(E[r], n, correlation_kind, tile)
        con = WIT.contrast_t(I, contrast_kind, tile)
        div = T._iwe_div(n)
        rel_corr.append(w[r] * corr / (zc + EPSN))
        rel_con.append(w[r] * con / (c0 + EPSN))
        rel_div.append(w[r] * div / (d0 + EPSN))
        if terms is not None:
            per.append(dict(correlation=float(corr.detach()), zero_correlation=float(zc.detach()), contrast=float(con.detach()),
                            divergence=float(div.detach()), variance=float(torch.var(I.detach(), unbiased=False))))
    mrc = torch.stack(rel_con).mean()
    mrr = torch.stack(rel_corr).mean()
    mrd = torch.stack(rel_div).mean()
    tv = torch.zeros((), dtype=_DT)
    if cur_pyr_lvl <= 0:
        present = torch.as_tensor(wn > 0.0)                  # an event of weight 0 is not in the TV mask
        mask = torch.zeros(H, W, dtype=_DT)
        mask[yi[present], xi[present]] = 1.0
        tot = torch.zeros((), dtype=_DT)
        nz = torch.zeros(H, W, dtype=torch.bool)
        for c in (0, 1):
            gx, gy = T._scharr_diff(Theta[:, :, c] * mask)
            tot = tot + (gx.abs() * 0.25 + gy.abs() * 0.25).sum()
            nz |= (gx.detach().abs() > 0) | (gy.detach().abs() > 0)
        tv = tot / (float(nz.sum()) + EPSN)
    val = (alpha * (-mrc) + beta * (-mrr)) + (gamma * tv + delta * mrd)
    if terms is not None:
        terms.update(theta_total_variation=float(tv.detach()), mean_rel_iwe_divergence=float(mrd.detach()),
                     mean_rel_corr=float(mrr.detach()), mean_rel_contrast=float(mrc.detach()), zero_contrast=float(c0),
                     zero_variance=float(torch.var(I0, unbiased=False)), zero_iwe_divergence=float(d0), per_ref=per,
                     zero_iwe=I0.numpy().copy())
    return val


def loss_and_grad(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, A_H, A_W, weights=None,
                  contrast_kind=0, correlation_kind=0, tile=WIT.DEFAULT_TILE):
    """(value, grad (h,w,2), dL/dIWE (R,H,W), IWEs (R,H,W), terms) for a coarse theta (h,w,2); A_H (H,h), A_W (W,w) the resampling
    matrices (identity matrices for a dense theta)."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    AH = torch.as_tensor(np.asarray(A_H, dtype=np.float64))
    AW = torch.as_tensor(np.asarray(A_W, dtype=np.float64))
    Theta = torch.einsum('yi,xj,ijc->yxc', AH, AW, th)
    imgs, terms = [], {}
    val = loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, weights, contrast_kind,
                          correlation_kind, tile, imgs, terms)
    val.backward()
    G = np.stack([i.grad.numpy() for i in imgs])
    I = np.stack([i.detach().numpy() for i in imgs])
    return float(val.detach()), th.grad.numpy().copy(), G, I, terms


def loss_and_grad_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, weights=None, contrast_kind=0,
                        correlation_kind=0, tile=WIT.DEFAULT_TILE, full=False):
    """(value, dL/dTheta (H,W,2)) on a full-resolution Theta: what a motion model's gradient is projected from.
    full: (value, dL/dTheta, dL/dIWE (R,H,W), IWEs (R,H,W), terms), as loss_and_grad returns them."""
    Th = torch.tensor(np.asarray(Theta, dtype=np.float64), requires_grad=True)
    imgs, terms = [], {}
    val = loss_from_Theta(Th, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, weights, contrast_kind, correlation_kind,
                          tile, imgs, terms)
    val.backward()
    if not full:
        return float(val.detach()), Th.grad.numpy().copy()
    return (float(val.detach()), Th.grad.numpy().copy(), np.stack([i.grad.numpy() for i in imgs]),
            np.stack([i.detach().numpy() for i in imgs]), terms)


def loss_value(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, A_H, A_W, weights=None, **kw):
    """The value alone, without autograd (finite differences, forward-only checks)."""
    with torch.no_grad():
        Theta = torch.einsum('yi,xj,ijc->yxc', torch.as_tensor(np.asarray(A_H, dtype=np.float64)),
                             torch.as_tensor(np.asarray(A_W, dtype=np.float64)), torch.as_tensor(np.asarray(theta, dtype=np.float64)))
        return float(loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, weights, **kw))


def objectives(Theta, xs, ys, ts, edges, edge_ts, weights=None):
    """The terms compute_loss_objectives reports (losses.py:49-105) for a full-resolution Theta (H,W,2), default kinds."""
    terms = {}
    with torch.no_grad():
        loss_from_Theta(torch.as_tensor(np.asarray(Theta, dtype=np.float64)), xs, ys, ts, edges, edge_ts, 1.0, 1.0, 0.0, 0.0, 0,
                        weights, terms=terms)
    return terms


def handover_loss_and_grad(alpha_handover, prev_theta, theta, *args, **kw):
    """value and d/d(alpha_handover) of the handover loss (losses.py:269-276): <dL/dtheta_ho, prev - theta>."""
    prev_theta = np.asarray(prev_theta, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    val, grad, _, _, _ = loss_and_grad(alpha_handover * prev_theta + (1 - alpha_handover) * theta, *args, **kw)
    return val, float(np.sum(grad * (prev_theta - theta)))


def count_images(Theta, xs, ys, ts, edge_ts, weights=None):
    """(R, H, W) integer images of the rounded warped coordinates of the events with w > 0 (JAX index rule, half-to-even rounding)."""
    Theta = np.asarray(Theta, dtype=np.float64)
    H, W, _ = Theta.shape
    xi = np.asarray(xs).astype(np.int64)
    yi = np.asarray(ys).astype(np.int64)
    keep = staged_weights(weights, len(xi)) > 0.0
    out = []
    for tau in np.atleast_1d(np.asarray(edge_ts, dtype=np.float64)):
        dt = np.asarray(ts, dtype=np.float64) - tau
        rx = np.rint(xi - Theta[yi, xi, 0] * dt).astype(np.int64)
        ry = np.rint(yi - Theta[yi, xi, 1] * dt).astype(np.int64)
        rx = np.where(rx < 0, rx + W, rx)
        ry = np.where(ry < 0, ry + H, ry)
        ok = keep & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        img = np.zeros(H * W, dtype=np.uint32)
        np.add.at(img, ry[ok] * W + rx[ok], 1)
        out.append(img.reshape(H, W))
    return np.stack(out)
