"""GPU image preprocessing (eincm_preprocess_image) against the numpy witness tests/_preprocess_witness.py:
every stage alone and the whole chain bit-exact on scenes, noise, ramps, constant and saturated images from 3x3 to 480x640,
non-default parameters, batching, determinism, fp32 / fp64 contexts, the C-ABI's refusals, and the frames -> edges chain with
edges.preprocess_image as its clean-up."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _canny_witness as CW
import _preprocess_witness as PW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
edges_mod = importlib.import_module(pkg + '.edges')
staging = importlib.import_module(pkg + '.staging')
synth = importlib.import_module(pkg + '.synth')

_engines = {}


def _eng(shape, precision='fp32'):
    key = (tuple(shape), precision)
    if key not in _engines:
        _engines[key] = E.Engine(shape, max_events_total=1, max_refs=1, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    edges_mod.clear_engines()


def _scene(shape, seed, noise=6.0):
    rng = np.random.default_rng(seed)
    win = synth.make_window(seed, shape, 10, 1, flow='zero', n_segments=24, n_circles=6)
    f = 40.0 + 170.0 * win['edges'][0] + rng.normal(0.0, noise, shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _inputs(shape, seed):
    H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    sat = np.where((xx // 5 + yy // 4) % 3 == 0, 255, np.where((xx + yy) % 7 < 3, 0, 128))      # 0 and 255 plateaus
    imgs = [rng.integers(0, 256, shape),                                  # uniform noise
            (xx * 3 + yy) % 256,                                          # ramps
            np.full(shape, 91),                                           # constant
            sat]
    if H >= 16 and W >= 16:
        imgs = [_scene(shape, seed), _scene(shape, seed + 1, noise=15.0)] + imgs
    return np.stack(imgs).astype(np.uint8)


def _grid(shape):
    H, W = shape
    return (10, 10) if H >= 10 and W >= 10 else (min(W, 4), min(H, 3))


def _witness(img, stages, **kw):
    """Keywords of Engine.preprocess_image, mapped onto the witness's."""
    m = {'denoise_h': 'h', 'denoise_template_win': 'tw', 'denoise_search_win': 'sw', 'clahe_clip_limit': 'clip',
         'clahe_tiles': 'tiles', 'sharpen_sigma': 'sigma', 'sharpen_alpha': 'alpha', 'sharpen_beta': 'beta', 'bilateral_d': 'd',
         'bilateral_sigma_color': 'sc', 'bilateral_sigma_space': 'ss'}
    return PW.preprocess(img, stages, **{m[k]: v for k, v in kw.items()})


def _check(eng, imgs, stages, **kw):
    got = eng.preprocess_image(imgs, stages, **kw)
    assert got.dtype == np.uint8 and got.shape == imgs.shape
    for k in range(len(imgs)):
        ref = _witness(imgs[k], stages, **kw)
        assert np.array_equal(got[k], ref), (imgs.shape, k, stages, kw, int((got[k] != ref).sum()))
    return got


STAGE_SETS = [PW.NLMEANS, PW.CLAHE, PW.UNSHARP, PW.BILATERAL, PW.ALL]
SHAPES = [(3, 3), (3, 64), (40, 3), (37, 53), (260, 346), (256, 336), (480, 640)]


@pytest.mark.parametrize('shape', SHAPES)
def test_each_stage_and_the_chain_bit_exact(shape):
    imgs = _inputs(shape, sum(shape))
    if shape == (480, 640):
        imgs = imgs[[0, 2, 5]]                                            # scene, noise, saturated: keeps the witness quick
    eng = _eng(shape)
    for stages in STAGE_SETS:
        _check(eng, imgs, stages, clahe_tiles=_grid(shape))


NON_DEFAULT = [
    (PW.NLMEANS, dict(denoise_template_win=1)), (PW.NLMEANS, dict(denoise_template_win=5, denoise_h=10.0)),
    (PW.NLMEANS, dict(denoise_template_win=7, denoise_search_win=21)), (PW.NLMEANS, dict(denoise_search_win=3)),
    (PW.NLMEANS, dict(denoise_h=4.3)), (PW.NLMEANS, dict(denoise_h=0.7, denoise_search_win=21)),
    (PW.CLAHE, dict(clahe_clip_limit=0.0)), (PW.CLAHE, dict(clahe_tiles=(1, 1))), (PW.CLAHE, dict(clahe_tiles=(4, 7))),
    (PW.CLAHE, dict(clahe_tiles=(16, 16), clahe_clip_limit=2.0)), (PW.CLAHE, dict(clahe_clip_limit=-1.0, clahe_tiles=(7, 4))),
    (PW.UNSHARP, dict(sharpen_sigma=1.0)), (PW.UNSHARP, dict(sharpen_sigma=0.8, sharpen_alpha=2.0, sharpen_beta=-1.0)),
    (PW.UNSHARP, dict(sharpen_sigma=7.5, sharpen_alpha=1.3, sharpen_beta=-0.3)),
    (PW.BILATERAL, dict(bilateral_d=0)), (PW.BILATERAL, dict(bilateral_d=3)), (PW.BILATERAL, dict(bilateral_d=9)),
    (PW.BILATERAL, dict(bilateral_d=9, bilateral_sigma_color=40.0, bilateral_sigma_space=3.0)),
    (PW.BILATERAL, dict(bilateral_d=0, bilateral_sigma_color=-1.0, bilateral_sigma_space=-1.0)),
    (PW.ALL, dict(denoise_template_win=5, denoise_search_win=7, clahe_tiles=(4, 7), clahe_clip_limit=0.0, sharpen_sigma=1.5,
                  bilateral_d=9)),
]


@pytest.mark.parametrize('stages, kw', NON_DEFAULT)
def test_non_default_parameters(stages, kw):
    shape = (37, 53)
    kw = dict({'clahe_tiles': (10, 10)}, **kw)
    _check(_eng(shape), _inputs(shape, 7), stages, **kw)


def test_non_default_parameters_on_a_narrow_image():
    shape = (3, 40)
    imgs = _inputs(shape, 8)
    eng = _eng(shape)
    _check(eng, imgs, PW.NLMEANS, denoise_template_win=7, denoise_search_win=21)
    _check(eng, imgs, PW.BILATERAL, bilateral_d=0)
    _check(eng, imgs, PW.ALL, clahe_tiles=(16, 3), sharpen_sigma=7.5)


def test_batch_equals_single_calls_repeats_and_precision():
    shape = (65, 129)
    imgs = _inputs(shape, 11)
    eng = _eng(shape)
    batch = eng.preprocess_image(imgs)
    for k in range(len(imgs)):
        assert np.array_equal(batch[k], eng.preprocess_image(imgs[k]))
    for _ in range(3):
        assert np.array_equal(eng.preprocess_image(imgs), batch)
    assert np.array_equal(_eng(shape, 'fp64').preprocess_image(imgs), batch)
    for stages in STAGE_SETS[:4]:
        assert np.array_equal(_eng(shape, 'fp64').preprocess_image(imgs, stages), eng.preprocess_image(imgs, stages))
    big = np.tile(imgs, (54, 1, 1))                                       # 324 images in one call
    assert np.array_equal(eng.preprocess_image(big), np.tile(batch, (54, 1, 1)))
    # the NL-means table follows h: a call with another h between two equal calls changes nothing
    a = eng.preprocess_image(imgs, 'nlmeans', denoise_h=4.3)
    eng.preprocess_image(imgs, 'nlmeans', denoise_h=9.0)
    assert np.array_equal(eng.preprocess_image(imgs, 'nlmeans', denoise_h=4.3), a)


def _params(**kw):
    p = L.PreprocessParams()
    base = dict(stages=15, denoise_h=4.0, denoise_template_win=3, denoise_search_win=11, clahe_clip_limit=5.0, clahe_tiles_x=10,
                clahe_tiles_y=10, sharpen_sigma=3.0, sharpen_alpha=1.5, sharpen_beta=-0.5, bilateral_d=5, bilateral_sigma_color=15.0,
                bilateral_sigma_space=15.0)
    for k, v in dict(base, **kw).items():
        setattr(p, k, v)
    return p


def test_c_abi_errors():
    lib = L.load()
    u8 = C.POINTER(C.c_uint8)
    shape = (3, 40)
    eng = _eng(shape)
    src = _inputs(shape, 3)[:2].copy()
    dst = np.empty_like(src)
    call = lambda p, n=2: lib.eincm_preprocess_image(eng._ctx, src.ctypes.data_as(u8), n, C.byref(p), dst.ctypes.data_as(u8))  # noqa: E731
    assert call(_params()) == L.ERR_ARG                                   # the default (10, 10) grid on a 3 x N image
    assert call(_params(clahe_tiles_x=40, clahe_tiles_y=3)) == L.OK
    assert call(_params(clahe_tiles_x=41, clahe_tiles_y=3)) == L.ERR_ARG
    assert call(_params(stages=13)) == L.OK                               # no CLAHE: its grid is not read
    ok = dict(clahe_tiles_x=4, clahe_tiles_y=3)
    for bad in [dict(stages=0), dict(stages=16), dict(denoise_h=0.0), dict(denoise_h=float('nan')), dict(denoise_template_win=4),
                dict(denoise_search_win=0), dict(clahe_tiles_x=0), dict(clahe_clip_limit=float('inf')), dict(sharpen_sigma=0.0),
                dict(sharpen_beta=float('nan')), dict(bilateral_sigma_space=float('inf'))]:
        assert call(_params(**dict(ok, **bad))) == L.ERR_ARG, bad
    for unsup in [dict(denoise_template_win=9), dict(denoise_search_win=23), dict(sharpen_sigma=30.0), dict(bilateral_d=67),
                  dict(bilateral_d=0, bilateral_sigma_space=30.0)]:
        assert call(_params(**dict(ok, **unsup))) == L.ERR_UNSUPPORTED, unsup
    assert call(_params(**ok), n=0) == L.ERR_ARG
    assert lib.eincm_preprocess_image(eng._ctx, None, 1, C.byref(_params(**ok)), dst.ctypes.data_as(u8)) == L.ERR_ARG
    # src and dst may alias
    a = src.copy()
    assert lib.eincm_preprocess_image(eng._ctx, a.ctypes.data_as(u8), 2, C.byref(_params(**ok)), a.ctypes.data_as(u8)) == L.OK
    assert np.array_equal(a, eng.preprocess_image(src, clahe_tiles=(4, 3)))
    with pytest.raises(ValueError, match='uint8'):
        eng.preprocess_image(src.astype(np.int16), clahe_tiles=(4, 3))
    with pytest.raises(ValueError, match='clahe_tiles'):
        eng.preprocess_image(src)


def test_edges_preprocess_image_names_and_conversion():
    shape = (96, 128)
    rng = np.random.default_rng(4)
    img = _scene(shape, 4)
    ref = PW.preprocess(img)
    assert np.array_equal(edges_mod.preprocess_image(img), ref)
    assert np.array_equal(edges_mod.preprocess_image(np.stack([img, img])), np.stack([ref, ref]))
    kw = dict(denoise_h=6, denoise_template_win_size=5, denoise_search_win_size=7, clahe_clip_limit=2, clahe_tile_grid_size=(4, 7),
              sharpen_kernel_size=2, sharpen_sigma_x=99, sharpen_alpha=1.8, sharpen_beta=-0.8, bilateral_filter_neigh_diameter=3,
              bilateral_filter_sigma_color=30, bilateral_filter_sigma_space=5)
    ref2 = PW.preprocess(img, h=6, tw=5, sw=7, clip=2, tiles=(4, 7), sigma=2, alpha=1.8, beta=-0.8, d=3, sc=30, ss=5)
    assert np.array_equal(edges_mod.preprocess_image(img, **kw), ref2)
    f = rng.random(shape) * 3.0 - 1.0                                     # not uint8: to_canny_input first
    assert np.array_equal(edges_mod.preprocess_image(f), PW.preprocess(CW.to_canny_input(f)))
    fs = np.stack([f, 2.0 * f + 5.0, f ** 2])
    assert np.array_equal(edges_mod.preprocess_image(fs), PW.preprocess_stack([CW.to_canny_input(x) for x in fs]))


def _frames(shape, R, seed):
    rng = np.random.default_rng(seed)
    win = synth.make_window(seed, shape, 10, R, flow='constant', flow_mag=8.0, n_segments=24, n_circles=6)
    return 0.1 + 0.7 * win['edges'] + rng.normal(0.0, 0.02, win['edges'].shape), win


def _ref_chain(frames, th1=30, th2=80, **pre):
    pre_imgs = [PW.preprocess(CW.to_canny_input(f) if f.dtype != np.uint8 else f, **pre) for f in frames]
    return CW.chain_edge_images(pre_imgs, th1, th2)


def test_frames_to_edges_with_preprocessing_equals_the_witness_chain():
    shape = (96, 128)
    frames, _ = _frames(shape, 4, 21)
    ref_edges = _ref_chain(frames)
    assert all(e.any() for e in ref_edges)
    ref = np.stack([CW.unit_range(edges_mod.smoothen_edges(e, k_size=1)) for e in ref_edges])
    got = edges_mod.frames_to_edges(frames, preprocess_image_func=edges_mod.preprocess_image, k_size=1)
    assert got.shape == (4,) + shape and np.array_equal(got, ref)
    assert not np.array_equal(got, edges_mod.frames_to_edges(frames, k_size=1))
    # the reference's config binds the clean-up through a partial; a per-frame wrapper gives the same stack
    part = functools.partial(edges_mod.preprocess_image, denoise_h=7, clahe_tile_grid_size=(4, 7))
    got_p = edges_mod.frames_to_edges(frames, image_to_edge_func=functools.partial(edges_mod.image_to_edge, th1=100, th2=200),
                                      preprocess_image_func=part)
    ref_p = np.stack([CW.unit_range(edges_mod.smoothen_edges(e)) for e in _ref_chain(frames, 100, 200, h=7, tiles=(4, 7))])
    assert np.array_equal(got_p, ref_p)
    per_frame = edges_mod.frames_to_edges(frames, image_to_edge_func=functools.partial(edges_mod.image_to_edge, th1=100, th2=200),
                                          preprocess_image_func=lambda im: part(im))
    assert np.array_equal(per_frame, ref_p)


def test_stage_datasample_with_preprocessing():
    shape = (96, 128)
    frames, win = _frames(shape, 5, 33)
    images = np.stack([CW.to_canny_input(CW.unit_range(f)) for f in frames])
    sample = {'events': {'x': win['xs'], 'y': win['ys'], 't': win['ts'] * 1e6, 'p': np.ones(len(win['xs']), bool)},
              'images': images, 'image_ts': win['edge_ts'] * 1e6, 'eval_ts': (0.0, 1e6)}
    smoothed = [edges_mod.smoothen_edges(e, k_size=1) for e in _ref_chain(images)]
    got = staging.stage_datasample(sample, preprocess_image_func=edges_mod.preprocess_image)
    ref = staging.stage_datasample(sample, smoothed)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
