"""Edge extraction on the GPU: grayscale frames -> the ``edges`` stack the loss consumes (SURVEY f-4).

Mirrors the callables the reference's hydra group ``edge_extraction`` binds (src/experiments/e00/configs/edge_extraction/),
same names and arguments:

  to_canny_input(image)                                                jnp_to_ocv_n255, src/utils/img_utils.py:87-93 (host)
  image_to_edge(img, apert_size=3, th1=30, th2=80)                     src/utils/img_utils.py:192-208 (cv.Canny, L2)
  smoothen_edges(edge_img, k_size=1, sigma=1)                         src/utils/img_utils.py:210-220
  eincm_inv_exp_dist_transform(edge_img, alpha=6)                      src/utils/img_utils.py:229-233
  rtef_inv_exp_dist_transform(edge_img, d_sat, alpha_iedt, formulation)   src/utils/img_utils.py:223-226, :236-410
  preprocess_image(img, denoise_h=4, ..., bilateral_filter_sigma_space=15)   src/utils/img_utils.py:131-189
  frames_to_edges(images, ...)                                         the chain of src/experiments/e00/exp_mgr.py:334-350

preprocess_image is the photometric clean-up in front of Canny (NL-means, CLAHE, unsharp masking, bilateral filter), restated
from OpenCV's algorithms as DESIGN.md section 14 writes them down; parity with OpenCV itself is unpinned.  frames_to_edges
runs it when it is passed as preprocess_image_func (default None: no clean-up).  Preprocessing, Canny and the smoothing run in
libeincm_hip.so; no CPU fallback.
"""
import sys

import numpy as np

from .engine import Engine, check_canny_args, make_preprocess_params

_engines = {}


def _engine(shape, device=0):
    """A small context per sensor size: these entry points only need its stream and scratch buffers."""
    key = (int(shape[0]), int(shape[1]), int(device))
    if key not in _engines:
        _engines[key] = Engine(key[:2], max_events_total=1, max_refs=1, max_windows=1, device=device)
    return _engines[key]


def clear_engines():
    for e in _engines.values():
        e.close()
    _engines.clear()


def smoothen_edges(edge_img, k_size=1, sigma=1, engine=None):
    """Gaussian smoothing as the reference's call performs it.  The reference passes its arguments to OpenCV positionally
    (``cv.GaussianBlur(edge_img, None, k_size, sigma, 0)``, img_utils.py:218), which binds ``k_size`` to sigmaX and
    ``sigma`` to the (ignored) output array; the kernel size is then derived from sigmaX.  ``sigma`` is therefore accepted
    and unused here too.  preprocess_image's unsharp mask inherits the same binding (sharpen_kernel_size -> sigmaX)."""
    del sigma
    img = np.asarray(edge_img).astype(np.float64)
    eng = engine or _engine(img.shape[-2:])
    return eng.gaussian_blur(img, float(k_size))


def eincm_inv_exp_dist_transform(edge_img, alpha=6, engine=None):
    e = np.asarray(edge_img)
    eng = engine or _engine(e.shape[-2:])
    return eng.inv_dist_transform(e.astype('bool'), 'exponential', alpha=float(alpha))


def rtef_inv_exp_dist_transform(edge_img, dist_surf_saturation_distance=None, alpha_iedt=None, formulation='exponential',
                                engine=None):
    e = np.asarray(edge_img)
    vals = np.unique(e)
    assert e.ndim == 2 and len(vals) == 2 and 0 in vals.astype('int'), 'Need 2D binary edge image'    # img_utils.py:397-399
    d_sat = 6.0 if dist_surf_saturation_distance is None else float(dist_surf_saturation_distance)   # img_utils.py:256
    alpha = d_sat / 5.541 if alpha_iedt is None else float(alpha_iedt)                               # img_utils.py:257
    eng = engine or _engine(e.shape)
    return eng.inv_dist_transform(e.astype('bool'), formulation, alpha=alpha, d_sat=d_sat)


def smooth_edge_stack(edge_imgs, smoothen_edges_func=smoothen_edges, **kw):
    """exp_mgr.py:343-350 for a stack of binary edge images: smooth each, then min-max normalise each to [0, 1]."""
    from .staging import normalize_edges
    return normalize_edges([smoothen_edges_func(e, **kw) for e in edge_imgs])


def to_canny_input(image):
    """jnp_to_ocv_n255 (img_utils.py:87-93): the image as float32, cv.normalize(NORM_MINMAX) to [0, 255], then .astype(uint8).
    cv.normalize takes scale = 255 * (1 / (max - min)), or 0 when max - min <= DBL_EPSILON, and shift = -min * scale (in double),
    and converts with x * scale + shift; here that is float32 arithmetic with scale and shift rounded to float32, then numpy's
    truncating cast.  Whether this equals OpenCV's float32 conversion bit for bit at pixels that land exactly on an integer is not
    checked (no OpenCV to compare with)."""
    x = np.asarray(image).astype(np.float32)
    lo, hi = float(x.min()), float(x.max())
    scale = 255.0 * (1.0 / (hi - lo)) if hi - lo > sys.float_info.epsilon else 0.0
    shift = -lo * scale
    return (x * np.float32(scale) + np.float32(shift)).astype(np.uint8)


def image_to_edge(img, apert_size=3, th1=30, th2=80, engine=None):
    """cv.Canny(img, th1, th2, None, apert_size, L2gradient=True) (img_utils.py:192-208) on the GPU.  img: (H,W) or (n,H,W)
    uint8; returns 0 / 255 uint8 of the same shape.  Only apert_size 3 is implemented (the reference's only setting)."""
    th1, th2, apert_size = check_canny_args(th1, th2, apert_size)
    e = np.asarray(img)
    eng = engine or _engine(e.shape[-2:])
    return eng.canny(e, th1, th2, apert_size, l2_gradient=True)


def preprocess_image(img, denoise_h=4, denoise_template_win_size=3, denoise_search_win_size=11, clahe_clip_limit=5,
                     clahe_tile_grid_size=(10, 10), sharpen_kernel_size=3, sharpen_sigma_x=2, sharpen_alpha=1.5, sharpen_beta=-0.5,
                     bilateral_filter_neigh_diameter=5, bilateral_filter_sigma_color=15, bilateral_filter_sigma_space=15, engine=None):
    """The reference's preprocess_image (img_utils.py:131-189) on the GPU, same names and defaults: cv.fastNlMeansDenoising ->
    CLAHE (clahe_tile_grid_size[0] splits the width) -> unsharp mask -> cv.bilateralFilter.
    img: (H,W) or (n,H,W); input that is not a uint8 ndarray goes through to_canny_input first, image by image
    (img_utils.py:146-147).  Returns uint8 of the same shape.

    The unsharp mask's blur is ``cv.GaussianBlur(img, None, sharpen_kernel_size, sharpen_sigma_x, 0)``: as in smoothen_edges,
    the positional arguments bind ``sharpen_kernel_size`` to sigmaX and ``sharpen_sigma_x`` to the (ignored) output array, and
    OpenCV derives the kernel size from sigmaX (cvRound(6 sigma + 1) | 1: 19 taps of sigma 3 for the defaults).
    ``sharpen_sigma_x`` is therefore accepted and unused here too."""
    del sharpen_sigma_x
    a = np.asarray(img)
    shape = a.shape[-2:]
    p = dict(denoise_h=denoise_h, denoise_template_win=denoise_template_win_size, denoise_search_win=denoise_search_win_size,
             clahe_clip_limit=clahe_clip_limit, clahe_tiles=tuple(clahe_tile_grid_size), sharpen_sigma=sharpen_kernel_size,
             sharpen_alpha=sharpen_alpha, sharpen_beta=sharpen_beta, bilateral_d=bilateral_filter_neigh_diameter,
             bilateral_sigma_color=bilateral_filter_sigma_color, bilateral_sigma_space=bilateral_filter_sigma_space)
    if a.ndim not in (2, 3):
        raise ValueError(f'images must be (H,W) or (n,H,W), got {a.shape}')
    make_preprocess_params(shape, 'all', **p)                  # argument checks before any GPU call
    if not isinstance(img, np.ndarray) or a.dtype != np.uint8:
        a = to_canny_input(a) if a.ndim == 2 else np.stack([to_canny_input(im) for im in a])
    eng = engine or _engine(shape)
    return eng.preprocess_image(a, 'all', **p)


def _is_batched(func, batched):
    """func is `batched` itself or a functools.partial of it: such callables take the whole stack in one call."""
    return func is batched or getattr(func, 'func', None) is batched


def _normalize_to_unit_range(a):
    """img_utils.py:24-25."""
    from .staging import EPSN
    return (a - a.min()) / (a.max() - a.min() + EPSN)


def frames_to_edges(images, image_to_edge_func=image_to_edge, smoothen_edges_func=smoothen_edges, preprocess_image_func=None,
                    **smoothen_kw):
    """exp_mgr.py:334-350 for a stack of grayscale frames: [preprocess_image_func] -> normalize_to_unit_range (float64) ->
    to_canny_input -> image_to_edge_func -> smoothen_edges_func(**smoothen_kw) -> normalize_to_unit_range.  Returns the (R,H,W)
    float64 stack in [0, 1].  preprocess_image and image_to_edge (or a functools.partial of either) run once for the whole stack."""
    if preprocess_image_func is not None and _is_batched(preprocess_image_func, preprocess_image):
        u8 = [im if isinstance(im, np.ndarray) and im.dtype == np.uint8 else to_canny_input(im) for im in images]  # per image, as
        images = list(preprocess_image_func(np.stack(u8)))                                                          # one call would
        preprocess_image_func = None
    frames = [_normalize_to_unit_range(np.asarray(im if preprocess_image_func is None else preprocess_image_func(im)).astype(np.float64))
              for im in images]
    canny_in = np.stack([to_canny_input(f) for f in frames])
    if _is_batched(image_to_edge_func, image_to_edge):
        edge_imgs = list(image_to_edge_func(canny_in))
    else:
        edge_imgs = [image_to_edge_func(c) for c in canny_in]
    return smooth_edge_stack(edge_imgs, smoothen_edges_func, **smoothen_kw)
