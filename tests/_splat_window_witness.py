"""Independent fp64 witness of the loss with a selectable splat window size: torch float64 forward, gradient by autograd.

Test helper only.  Generalises the 3x3 splat of oracle/eincm_torch.py to events_to_pdf_frame's window_size (event_utils.py:13-61):
radius w = window_size // 2, every event adds exp(-|q|^2 / 2) / (2 pi) at the (2w+1)^2 pixels round(x) + d, d in [-w, w]^2,
q = round(x) + d - x, scattered with the same index rule (a negative index wraps once, an index past the end is dropped).  The
objective is losses.py:162-193 with the kinds of tests/_objective_kinds_witness.py; normalisation, Scharr, divergence and TV come
from oracle/eincm_torch.py (imported read-only).  The splat of long event lists runs in chunks under torch.utils.checkpoint, so that
autograd keeps one chunk's taps at a time (10^6 events x 5 reference times x 25 taps would not fit otherwise); the arithmetic is the
same.
"""
import math

import numpy as np
import torch
from torch.utils.checkpoint import checkpoint

from oracle import eincm_torch as T
import _objective_kinds_witness as WIT

EPSN = T.EPSN
_DT = torch.float64
CHUNK = 1 << 16
LOG_2PI = math.log(2.0 * math.pi)


def radius(window_size):
    return int(window_size) // 2


def _splat_chunk(wx, wy, H, W, rad):
    rx = torch.round(wx.detach()).to(torch.int64)
    ry = torch.round(wy.detach()).to(torch.int64)
    frame = torch.zeros(H * W, dtype=_DT)
    for dx in range(-rad, rad + 1):
        for dy in range(-rad, rad + 1):
            px = rx + dx
            py = ry + dy
            qx = px.to(_DT) - wx
            qy = py.to(_DT) - wy
            k = torch.exp(-0.5 * (qx * qx + qy * qy) - LOG_2PI)
            px = torch.where(px < 0, px + W, px)
            py = torch.where(py < 0, py + H, py)
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            idx = torch.where(ok, py * W + px, torch.zeros_like(px))
            frame = frame.index_put((idx,), torch.where(ok, k, torch.zeros_like(k)), accumulate=True)
    return frame


def splat(wx, wy, H, W, window_size=3):
    """events_to_pdf_frame(wx, wy, (H, W), window_size) as an (H, W) tensor."""
    rad = radius(window_size)
    n = wx.shape[0]
    if n <= CHUNK:
        return _splat_chunk(wx, wy, H, W, rad).reshape(H, W)
    frame = torch.zeros(H * W, dtype=_DT)
    for s in range(0, n, CHUNK):
        a, b = wx[s:s + CHUNK], wy[s:s + CHUNK]
        if a.requires_grad or b.requires_grad:
            frame = frame + checkpoint(_splat_chunk, a, b, H, W, rad, use_reentrant=False)
        else:
            frame = frame + _splat_chunk(a, b, H, W, rad)
    return frame.reshape(H, W)


def loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, window_size=3, contrast_kind=0,
                    correlation_kind=0, tile=WIT.DEFAULT_TILE, images=None, terms=None):
    """losses.py:162-193 on a full-resolution Theta (H,W,2) tensor with the given splat window.  images: receives the IWE tensors
    (retain_grad: .grad is dL/dIWE after backward).  terms: receives the zero-warp values and the per-image values as floats."""
    H, W, _ = Theta.shape
    xi = torch.as_tensor(np.asarray(xs).astype(np.int64))
    yi = torch.as_tensor(np.asarray(ys).astype(np.int64))
    t = torch.as_tensor(np.asarray(ts, dtype=np.float64))
    E = torch.as_tensor(np.asarray(edges, dtype=np.float64))
    tau = np.asarray(edge_ts, dtype=np.float64)
    R = len(tau)
    w = T._weights(R)
    with torch.no_grad():
        I0 = splat(xi.to(_DT), yi.to(_DT), H, W, window_size)
    n0 = T._normalize(I0)
    c0 = WIT.contrast_t(I0, contrast_kind, tile)
    d0 = T._iwe_div(n0)
    vx = Theta[yi, xi, 0]
    vy = Theta[yi, xi, 1]
    rel_con, rel_corr, rel_div, per = [], [], [], []
    for r in range(R):
        dts = t - float(tau[r])
        I = splat(xi.to(_DT) - vx * dts, yi.to(_DT) - vy * dts, H, W, window_size)
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
        mask = torch.zeros(H, W, dtype=_DT)
        mask[yi, xi] = 1.0
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
                     zero_variance=float(torch.var(I0, unbiased=False)), zero_iwe_divergence=float(d0), per_ref=per)
    return val


def loss_and_grad(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, A_H, A_W, window_size=3,
                  contrast_kind=0, correlation_kind=0, tile=WIT.DEFAULT_TILE):
    """(value, grad (h,w,2), dL/dIWE (R,H,W), IWEs (R,H,W), terms) for a coarse theta (h,w,2); A_H (H,h), A_W (W,w) the resampling
    matrices (identity matrices for a dense theta)."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    AH = torch.as_tensor(np.asarray(A_H, dtype=np.float64))
    AW = torch.as_tensor(np.asarray(A_W, dtype=np.float64))
    Theta = torch.einsum('yi,xj,ijc->yxc', AH, AW, th)
    imgs, terms = [], {}
    val = loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, window_size, contrast_kind,
                          correlation_kind, tile, imgs, terms)
    val.backward()
    G = np.stack([i.grad.numpy() for i in imgs])
    I = np.stack([i.detach().numpy() for i in imgs])
    return float(val.detach()), th.grad.numpy().copy(), G, I, terms


def loss_value(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, A_H, A_W, window_size=3, **kw):
    """The value alone, without autograd (finite differences, forward-only checks)."""
    with torch.no_grad():
        Theta = torch.einsum('yi,xj,ijc->yxc', torch.as_tensor(np.asarray(A_H, dtype=np.float64)),
                             torch.as_tensor(np.asarray(A_W, dtype=np.float64)), torch.as_tensor(np.asarray(theta, dtype=np.float64)))
        return float(loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, window_size, **kw))


def objectives(Theta, xs, ys, ts, edges, edge_ts, window_size=3):
    """The terms compute_loss_objectives reports (losses.py:49-105) for a full-resolution Theta (H,W,2), default kinds."""
    terms = {}
    with torch.no_grad():
        loss_from_Theta(torch.as_tensor(np.asarray(Theta, dtype=np.float64)), xs, ys, ts, edges, edge_ts, 1.0, 1.0, 0.0, 0.0, 0,
                        window_size, terms=terms)
    return terms


def handover_loss_and_grad(alpha_handover, prev_theta, theta, *args, **kw):
    """value and d/d(alpha_handover) of the handover loss (losses.py:269-276): <dL/dtheta_ho, prev - theta>."""
    prev_theta = np.asarray(prev_theta, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    val, grad, _, _, _ = loss_and_grad(alpha_handover * prev_theta + (1 - alpha_handover) * theta, *args, **kw)
    return val, float(np.sum(grad * (prev_theta - theta)))


def tap_moment_bound(rad, n_f=2001):
    """max over f in [-1/2, 1/2] of sum_d |d - f| k(d) * sum_d k(d) / (2 pi), k(d) = exp(-(d - f)^2 / 2), d = -rad..rad: the bound of
    |dL/dw| / max|G| per component behind the gradient's fixed-point scale."""
    f = np.linspace(-0.5, 0.5, n_f)[:, None]
    q = np.arange(-rad, rad + 1)[None, :] - f
    k = np.exp(-0.5 * q * q)
    return float(((np.abs(q) * k).sum(1) * k.sum(1)).max() / (2.0 * math.pi))
