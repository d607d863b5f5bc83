"""numpy witness of eincm_canny: OpenCV's integer Canny, aperture 3, restated in five plain steps.

int64 arithmetic throughout, explicit padding, and hysteresis as scipy.ndimage.label over the survivors with a 3x3 structure:
a formulation independent of the GPU's union-find.  Also the host chain of edges.frames_to_edges, built from this witness and
the package's smoothing entry points."""
import sys

import numpy as np
from scipy import ndimage


def thresholds(th1, th2, l2_gradient=True):
    """Step 2: swap, clamp to 32767, square the positive ones for L2, floor."""
    th1, th2 = float(th1), float(th2)
    if th1 > th2:
        th1, th2 = th2, th1
    th1, th2 = min(th1, 32767.0), min(th2, 32767.0)
    if l2_gradient:
        th1 = th1 * th1 if th1 > 0 else th1
        th2 = th2 * th2 if th2 > 0 else th2
    return int(np.floor(th1)), int(np.floor(th2))


def sobel(img):
    """Step 1: dx = [-1 0 1] x [1 2 1]^T, dy its transpose, BORDER_REPLICATE."""
    s = np.pad(np.asarray(img, dtype=np.int64), 1, mode='edge')
    H, W = img.shape
    a = lambda dy, dx: s[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]        # noqa: E731  source at offset (dy, dx)
    gx = (a(-1, 1) + 2 * a(0, 1) + a(1, 1)) - (a(-1, -1) + 2 * a(0, -1) + a(1, -1))
    gy = (a(1, -1) + 2 * a(1, 0) + a(1, 1)) - (a(-1, -1) + 2 * a(-1, 0) + a(-1, 1))
    return gx, gy


def survivors(img, th1, th2, l2_gradient=True):
    """Steps 1-4: (survivor mask, strong mask)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    low, high = thresholds(th1, th2, l2_gradient)
    dx, dy = sobel(img)
    m = dx * dx + dy * dy if l2_gradient else np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1, mode='constant', constant_values=0)                  # magnitude 0 outside the image
    nb = lambda oy, ox: mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]          # noqa: E731  m(r + oy, c + ox)
    x = np.abs(dx)
    y = np.abs(dy) << 15
    tg22x = x * 13573
    tg67x = tg22x + (x << 16)
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    pos = (dx ^ dy) >= 0                                                    # s = +1
    keep_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    keep_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    keep_d = np.where(pos, (m > nb(-1, -1)) & (m > nb(1, 1)), (m > nb(-1, 1)) & (m > nb(1, -1)))
    keep = (m > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    return keep, keep & (m > high)


def canny(img, th1, th2, l2_gradient=True):
    """cv.Canny(img, th1, th2, None, 3, l2_gradient) for one uint8 image: uint8 0 / 255."""
    surv, strong = survivors(img, th1, th2, l2_gradient)
    lab, _ = ndimage.label(surv, structure=np.ones((3, 3), dtype=int))   # step 5: 8-connected components of the survivors
    hit = np.unique(lab[strong])
    return np.where(surv & np.isin(lab, hit[hit > 0]), 255, 0).astype(np.uint8)


def canny_stack(imgs, th1, th2, l2_gradient=True):
    return np.stack([canny(im, th1, th2, l2_gradient) for im in imgs])


def to_canny_input(image):
    """jnp_to_ocv_n255 as edges.to_canny_input states it (float32 minmax to [0, 255], truncating cast)."""
    x = np.asarray(image).astype(np.float32)
    lo, hi = float(x.min()), float(x.max())
    scale = 255.0 * (1.0 / (hi - lo)) if hi - lo > sys.float_info.epsilon else 0.0
    return (x * np.float32(scale) + np.float32(-lo * scale)).astype(np.uint8)


def unit_range(a):
    """img_utils.py:24-25."""
    a = np.asarray(a, dtype=np.float64)
    return (a - a.min()) / (a.max() - a.min() + sys.float_info.epsilon)


def chain_edge_images(images, th1=30, th2=80):
    """exp_mgr.py:334-346 up to Canny: unit range (float64) -> to_canny_input -> canny."""
    return np.stack([canny(to_canny_input(unit_range(im)), th1, th2) for im in images])
