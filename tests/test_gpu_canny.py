"""GPU Canny (eincm_canny) against the numpy witness tests/_canny_witness.py: bit-exact on every input,
hysteresis through arbitrarily long weak chains, batching, determinism, fp32 / fp64 contexts, and the frames -> edges chain
(edges.frames_to_edges, staging.stage_datasample without ready edges)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
from scipy import ndimage

import _canny_witness as CW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
edges_mod = importlib.import_module(pkg + '.edges')
staging = importlib.import_module(pkg + '.staging')
synth = importlib.import_module(pkg + '.synth')

THRESHOLDS = [(30, 80, True), (100, 200, True), (30, 80, False), (100, 200, False)]

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
    """A grayscale frame: a synth edge scene (segments and circles, blurred) plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    win = synth.make_window(seed, shape, 10, 1, flow='zero', n_segments=24, n_circles=6)
    f = 40.0 + 170.0 * win['edges'][0] + rng.normal(0.0, noise, shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _inputs(shape, seed):
    H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = [rng.integers(0, 256, shape),                                  # uniform random
            (xx * 3 + yy) % 256,                                          # smooth ramps: NMS ties everywhere
            (xx // 2 + 2 * yy) % 256,
            np.full(shape, 91)]                                           # constant
    if H >= 16 and W >= 16:
        imgs = [_scene(shape, seed), _scene(shape, seed + 1, noise=15.0)] + imgs
    return np.stack(imgs).astype(np.uint8)


SHAPES = [(3, 64), (3, 200), (130, 3), (3, 3), (17, 31), (37, 53), (65, 129), (96, 128), (16, 64), (260, 346), (480, 640)]


@pytest.mark.parametrize('shape', SHAPES)
def test_bit_exact_against_the_witness(shape):
    imgs = _inputs(shape, sum(shape))
    eng = _eng(shape)
    for th1, th2, l2 in THRESHOLDS:
        got = eng.canny(imgs, th1, th2, l2_gradient=l2)
        assert got.dtype == np.uint8 and got.shape == imgs.shape
        for k in range(len(imgs)):
            ref = CW.canny(imgs[k], th1, th2, l2)
            assert np.array_equal(got[k], ref), (shape, k, th1, th2, l2, int((got[k] != ref).sum()))


def test_thresholds_edge_cases():
    shape = (37, 53)
    imgs = _inputs(shape, 4)
    eng = _eng(shape)
    for th1, th2, l2 in [(0, 0, True), (0, 0, False), (80, 30, True), (29.7, 80.2, True), (1e9, 1e9, True), (0.5, 1e6, False),
                         (2040, 2040, False)]:
        got = eng.canny(imgs, th1, th2, l2_gradient=l2)
        for k in range(len(imgs)):
            assert np.array_equal(got[k], CW.canny(imgs[k], th1, th2, l2)), (th1, th2, l2, k)
    assert np.array_equal(eng.canny(imgs, 200, 100), eng.canny(imgs, 100, 200))


def _spiral(N=256, gap=6, width=3):
    """A rectangular spiral band of value 30 (a weak step edge at thresholds 100 / 200) over the whole image, with one brighter
    pixel at the path's inner end: the only strong survivors sit there, thousands of pixels of chain away from the far end."""
    path = np.zeros((N, N), bool)
    y, x = 2, 2
    top, bottom, left, right = 2, N - 3, 2, N - 3
    k = 0
    path[y, x] = True
    while True:
        d = k % 4
        end = [(y, right), (bottom, x), (y, left), (top + gap, x)][d]
        n = abs(end[0] - y) + abs(end[1] - x)
        if n <= gap:
            break
        dy, dx = [(0, 1), (1, 0), (0, -1), (-1, 0)][d]
        for _ in range(n):
            y += dy
            x += dx
            path[y, x] = True
        if d == 1:
            right -= gap
        elif d == 2:
            bottom -= gap
        elif d == 3:
            left += gap
            top += gap
        k += 1
    img = np.where(ndimage.binary_dilation(path, structure=np.ones((width, width), bool)), 30, 0).astype(np.uint8)
    img[y, x] = 90
    return img, (y, x)


def test_weak_spiral_is_kept_whole():
    img, (ey, ex) = _spiral()
    surv, strong = CW.survivors(img, 100, 200)
    _, n_comp = ndimage.label(surv, structure=np.ones((3, 3), int))
    ys, xs = np.nonzero(strong)
    assert n_comp == 1 and surv.sum() > 17000 and 0 < len(ys) <= 9
    assert np.abs(ys - ey).max() <= 1 and np.abs(xs - ex).max() <= 1
    got = _eng(img.shape).canny(img, 100, 200)
    assert np.array_equal(got == 255, surv)
    assert np.array_equal(got, CW.canny(img, 100, 200))


def test_batch_equals_single_calls_and_repeats_bitwise():
    shape = (96, 128)
    rng = np.random.default_rng(11)
    imgs = np.concatenate([_inputs(shape, 11), rng.integers(0, 256, (1,) + shape).astype(np.uint8)])
    assert len(imgs) == 7
    eng = _eng(shape)
    batch = eng.canny(imgs, 30, 80)
    for k in range(7):
        assert np.array_equal(batch[k], eng.canny(imgs[k], 30, 80))
    for _ in range(3):
        assert np.array_equal(eng.canny(imgs, 30, 80), batch)
    big = np.tile(imgs, (46, 1, 1))                                    # 322 images in one call
    out = eng.canny(big, 30, 80)
    assert np.array_equal(out, np.tile(batch, (46, 1, 1)))


def test_fp32_and_fp64_contexts_agree():
    shape = (65, 129)
    imgs = _inputs(shape, 2)
    for th1, th2, l2 in THRESHOLDS:
        assert np.array_equal(_eng(shape, 'fp32').canny(imgs, th1, th2, l2_gradient=l2),
                              _eng(shape, 'fp64').canny(imgs, th1, th2, l2_gradient=l2))


def test_c_abi_errors():
    shape = (17, 31)
    eng = _eng(shape)
    lib = L.load()
    src = np.zeros((2,) + shape, np.uint8)
    dst = np.empty_like(src)
    u8 = C.POINTER(C.c_uint8)
    call = lambda n, t1, t2, ap, l2=1: lib.eincm_canny(eng._ctx, src.ctypes.data_as(u8), n, t1, t2, ap, l2,  # noqa: E731
                                                        dst.ctypes.data_as(u8))
    assert call(2, 30.0, 80.0, 3) == L.OK
    assert call(2, 30.0, 80.0, 5) == L.ERR_UNSUPPORTED
    assert call(2, 30.0, 80.0, -1) == L.ERR_UNSUPPORTED
    assert call(0, 30.0, 80.0, 3) == L.ERR_ARG
    assert call(2, -1.0, 80.0, 3) == L.ERR_ARG
    assert call(2, 30.0, float('nan'), 3) == L.ERR_ARG
    assert call(2, float('inf'), 80.0, 3) == L.ERR_ARG
    assert lib.eincm_canny(eng._ctx, None, 1, 30.0, 80.0, 3, 1, dst.ctypes.data_as(u8)) == L.ERR_ARG
    with pytest.raises(ValueError, match='uint8'):
        eng.canny(src.astype(np.int16), 30, 80)
    with pytest.raises(ValueError):
        eng.canny(np.zeros((16, 31), np.uint8), 30, 80)


def _frames(shape, R, seed):
    """R float frames (photometric values, not uint8) from one moving synth scene plus noise."""
    rng = np.random.default_rng(seed)
    win = synth.make_window(seed, shape, 10, R, flow='constant', flow_mag=8.0, n_segments=24, n_circles=6)
    return 0.1 + 0.7 * win['edges'] + rng.normal(0.0, 0.02, win['edges'].shape), win


@pytest.mark.parametrize('smoothing', ['gaussian', 'iedt'])
def test_frames_to_edges_equals_the_witness_chain(smoothing):
    shape = (96, 128)
    frames, _ = _frames(shape, 5, 21)
    ref_edges = CW.chain_edge_images(frames, 30, 80)
    assert all(e.any() for e in ref_edges)
    if smoothing == 'gaussian':
        got = edges_mod.frames_to_edges(frames, k_size=1)
        ref = np.stack([CW.unit_range(edges_mod.smoothen_edges(e, k_size=1)) for e in ref_edges])
    else:
        got = edges_mod.frames_to_edges(frames, smoothen_edges_func=edges_mod.eincm_inv_exp_dist_transform, alpha=6)
        ref = np.stack([CW.unit_range(edges_mod.eincm_inv_exp_dist_transform(e, alpha=6)) for e in ref_edges])
    assert got.shape == (5,) + shape and got.dtype == np.float64
    assert np.array_equal(got, ref)
    assert got.min() == 0.0 and got.max() <= 1.0
    # the reference's config binds other thresholds through a partial; a per-frame callable and a preprocessing hook
    part = edges_mod.frames_to_edges(frames, image_to_edge_func=functools.partial(edges_mod.image_to_edge, th1=100, th2=200))
    per_frame = edges_mod.frames_to_edges(frames, image_to_edge_func=lambda im: edges_mod.image_to_edge(im, th1=100, th2=200))
    ref_100 = np.stack([CW.unit_range(edges_mod.smoothen_edges(e)) for e in CW.chain_edge_images(frames, 100, 200)])
    assert np.array_equal(part, ref_100) and np.array_equal(per_frame, ref_100)
    pre = edges_mod.frames_to_edges(frames, preprocess_image_func=np.sqrt)
    assert np.array_equal(pre, edges_mod.frames_to_edges(np.sqrt(frames))) and not np.array_equal(pre, got)


def test_stage_datasample_from_frames():
    shape = (96, 128)
    frames, win = _frames(shape, 5, 33)
    images = np.stack([CW.to_canny_input(CW.unit_range(f)) for f in frames])       # uint8 frames as a loader hands them out
    sample = {'events': {'x': win['xs'], 'y': win['ys'], 't': win['ts'] * 1e6, 'p': np.ones(len(win['xs']), bool)},
              'images': images, 'image_ts': win['edge_ts'] * 1e6, 'eval_ts': (0.0, 1e6)}
    smoothed = [edges_mod.smoothen_edges(e, k_size=1) for e in CW.chain_edge_images(images, 30, 80)]
    got = staging.stage_datasample(sample)
    ref = staging.stage_datasample(sample, smoothed)
    assert len(got) == 5
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    got_iedt = staging.stage_datasample(sample, smoothen_edges_func=edges_mod.eincm_inv_exp_dist_transform, alpha=6)
    iedt = [edges_mod.eincm_inv_exp_dist_transform(e, alpha=6) for e in CW.chain_edge_images(images, 30, 80)]
    assert np.array_equal(got_iedt[3], staging.normalize_edges(iedt))
