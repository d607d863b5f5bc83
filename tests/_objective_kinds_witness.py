"""Independent fp64 witness of the loss with every (contrast kind x correlation kind): torch float64 forward, gradient by autograd.

Test helper only.  Restates losses.py:162-193 with the objective selected by kind, on top of the splat,
normalisation and Scharr of oracle/eincm_torch.py (imported read-only):
  contrast kinds     0 grad_mag  1 variance  2 adaptive_grad_mag  3 adaptive_variance   (on the raw IWE)
  correlation kinds  0 mse (-K)  1 adaptive_mse (-K)  2 hadamard (+K)  3 joint_contrast (+K)   (on the edges and the normalised IWE)
Tiles are extract_tiles' (img_utils.py:105-120): whole th x tw tiles, the ragged remainder ignored; the tile-local Scharr zero-pads
at the tile border.  amin / amax share their cotangent among ties, as JAX does.

Two forms of the tiled terms: 'loop' (one slice per tile, the literal restatement) and 'vector' (the default: the cropped whole-tile
region reshaped to a (tiles, th, tw) batch, the tile-local Scharr a batched zero-padded convolution), which keeps 1x1 tiles on a
large sensor affordable under autograd.  tests/test_objective_kinds_interface.py checks that the two agree.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import eincm_torch as T

EPSN = T.EPSN
_DT = torch.float64
DEFAULT_TILE = (32, 42)
FORMS = ('vector', 'loop')


def _tiles(a, tile):
    th, tw = tile
    H, W = a.shape
    return [a[i * th:(i + 1) * th, j * tw:(j + 1) * tw] for i in range(H // th) for j in range(W // tw)]


def _tile_batch(a, tile):
    """The whole tiles of a as one (nty * ntx, th, tw) tensor, in the order of _tiles (row of tiles by row of tiles)."""
    th, tw = tile
    H, W = a.shape
    nty, ntx = H // th, W // tw
    return a[:nty * th, :ntx * tw].reshape(nty, th, ntx, tw).permute(0, 2, 1, 3).reshape(nty * ntx, th, tw)


def _mean_gm(a):
    gx, gy = T._scharr(a)
    return (gx * gx + gy * gy).mean()


def _mean_gm_batch(t):
    """_mean_gm of every image of a (n, th, tw) batch, each zero-padded at its own border: (n,)"""
    k = torch.stack([torch.flip(T._SX, dims=(0, 1)), torch.flip(T._SY, dims=(0, 1))])[:, None]      # as T._conv_same
    g = F.conv2d(t[:, None], k, padding=1)
    return (g * g).sum(dim=1).mean(dim=(1, 2))


def _check_form(form):
    if form not in FORMS:
        raise ValueError(f'form {form!r}: one of {FORMS}')


def contrast_t(img, kind, tile=DEFAULT_TILE, form='vector'):
    _check_form(form)
    if kind == 0:
        return _mean_gm(img)
    if kind == 1:
        return torch.var(img, unbiased=False)
    if kind == 2:
        if form == 'vector':
            return _mean_gm_batch(_tile_batch(img, tile)).sum()
        return sum(_mean_gm(t) for t in _tiles(img, tile))
    if kind == 3:
        if form == 'vector':
            return torch.var(_tile_batch(img, tile), dim=(1, 2), unbiased=False).sum()
        return sum(torch.var(t, unbiased=False) for t in _tiles(img, tile))
    raise ValueError(kind)


def correlation_t(E, n, kind, tile=DEFAULT_TILE, form='vector'):
    """The signed correlation term: -K for the error-type kinds, +K for the similarity-type kinds."""
    _check_form(form)
    if kind == 0:
        return -((E - n) ** 2).mean()
    if kind == 1:
        if form == 'vector':
            return -((_tile_batch(E, tile) - _tile_batch(n, tile)) ** 2).mean(dim=(1, 2)).sum()
        return -sum(((a - b) ** 2).mean() for a, b in zip(_tiles(E, tile), _tiles(n, tile)))
    if kind == 2:
        return (E * n).mean()
    if kind == 3:
        return _mean_gm(E + n)
    raise ValueError(kind)


def contrast_value(arr, kind, tile=DEFAULT_TILE, form='vector'):
    return float(contrast_t(torch.as_tensor(np.asarray(arr, dtype=np.float64)), kind, tile, form))


def correlation_value(E, n, kind, tile=DEFAULT_TILE, form='vector'):
    return float(correlation_t(torch.as_tensor(np.asarray(E, dtype=np.float64)), torch.as_tensor(np.asarray(n, dtype=np.float64)),
                               kind, tile, form))


def loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, contrast_kind=0, correlation_kind=0,
                    tile=DEFAULT_TILE, images=None, form='vector', terms=None):
    """losses.py:162-193 with the selected kinds on a full-resolution Theta (H,W,2) tensor.  images: a list that receives the IWE
    tensors (retain_grad: their .grad is dL/dIWE after backward).  terms: a dict that receives the TV and divergence terms as floats.
    Returns (value, mean_rel_corr, mean_rel_contrast) tensors."""
    H, W, _ = Theta.shape
    xi = torch.as_tensor(np.asarray(xs).astype(np.int64))
    yi = torch.as_tensor(np.asarray(ys).astype(np.int64))
    t = torch.as_tensor(np.asarray(ts, dtype=np.float64))
    E = torch.as_tensor(np.asarray(edges, dtype=np.float64))
    tau = np.asarray(edge_ts, dtype=np.float64)
    R = len(tau)
    w = T._weights(R)
    I0 = T._splat(xi.to(_DT), yi.to(_DT), H, W)
    n0 = T._normalize(I0)
    c0 = contrast_t(I0, contrast_kind, tile, form)
    d0 = T._iwe_div(n0)
    vx = Theta[yi, xi, 0]
    vy = Theta[yi, xi, 1]
    rel_con, rel_corr, rel_div = [], [], []
    for r in range(R):
        dts = t - float(tau[r])
        I = T._splat(xi.to(_DT) - vx * dts, yi.to(_DT) - vy * dts, H, W)
        if images is not None:
            I.retain_grad()
            images.append(I)
        n = T._normalize(I)
        rel_corr.append(w[r] * correlation_t(E[r], n, correlation_kind, tile, form)
                        / (correlation_t(E[r], n0, correlation_kind, tile, form) + EPSN))
        rel_con.append(w[r] * contrast_t(I, contrast_kind, tile, form) / (c0 + EPSN))
        rel_div.append(w[r] * T._iwe_div(n) / (d0 + EPSN))
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
        terms.update(theta_total_variation=float(tv.detach()), mean_rel_iwe_divergence=float(mrd.detach()))
    return val, mrr, mrc


def loss_and_grad(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, A_H, A_W, contrast_kind=0,
                  correlation_kind=0, tile=DEFAULT_TILE, form='vector'):
    """(value, grad (h,w,2), dL/dIWE (R,H,W), aux) for a coarse theta (h,w,2); A_H (H,h), A_W (W,w) the resampling matrices.
    form: 'vector' or 'loop', the two forms of the tiled terms."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    AH = torch.as_tensor(np.asarray(A_H, dtype=np.float64))
    AW = torch.as_tensor(np.asarray(A_W, dtype=np.float64))
    Theta = torch.einsum('yi,xj,ijc->yxc', AH, AW, th)
    imgs, terms = [], {}
    val, mrr, mrc = loss_from_Theta(Theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, contrast_kind,
                                    correlation_kind, tile, imgs, form, terms)
    val.backward()
    G = np.stack([i.grad.numpy() for i in imgs])
    return float(val.detach()), th.grad.numpy().copy(), G, dict(terms, mean_rel_corr=float(mrr.detach()),
                                                                mean_rel_contrast=float(mrc.detach()))


def handover_loss_and_grad(alpha_handover, prev_theta, theta, *args, **kw):
    """value and d/d(alpha_handover) of the handover loss (losses.py:269-276): <dL/dtheta_ho, prev - theta>."""
    prev_theta = np.asarray(prev_theta, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    val, grad, _, _ = loss_and_grad(alpha_handover * prev_theta + (1 - alpha_handover) * theta, *args, **kw)
    return val, float(np.sum(grad * (prev_theta - theta)))
