"""Image preprocessing without a GPU: known answers of the numpy witness, argument checks that run before
any GPU call, the C-ABI symbol and struct layout, and frames_to_edges without preprocessing."""
import ctypes as C
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _preprocess_witness as PW

pkg = 'edge-informed-contrast-maximization_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reflect101_on_narrow_images():
    assert [PW.reflect101(p, 1) for p in range(-5, 6)] == [0] * 11
    assert [PW.reflect101(p, 2) for p in range(-4, 6)] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [PW.reflect101(p, 3) for p in range(-6, 9)] == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert PW.pad101(np.array([[1, 2, 3]]), 0, 0, 4, 4).tolist() == [[1, 2, 3, 2, 1, 2, 3, 2, 1, 2, 3]]


def test_constant_image_is_fixed_by_nlmeans_unsharp_and_bilateral():
    for shape in ((3, 3), (3, 17), (20, 31)):
        for v in (0, 77, 255):
            img = np.full(shape, v, np.uint8)
            assert np.array_equal(PW.nlmeans(img), img)
            assert np.array_equal(PW.nlmeans(img, 2.5, 7, 21), img)
            assert np.array_equal(PW.unsharp(img), img)
            assert np.array_equal(PW.bilateral(img), img)
            assert np.array_equal(PW.bilateral(img, 0, 15, 15), img)


def test_clahe_of_a_constant_image_equals_the_hand_computed_lut():
    # 20 x 30 at (3, 2): no padding, 10 x 10 tiles, total 100; limit max(int(5 * 100 / 256), 1) = 1, so 99 counts are clipped,
    # batch 0, residual 99, step 256 // 99 = 2: bins 0, 2, ..., 196 gain one.  cum(77) = 39 (even bins below 77) + 1 = 40;
    # rne(40 * (255 / 100)) = 102.
    img = np.full((20, 30), 77, np.uint8)
    assert np.unique(PW.clahe(img, 5.0, 3, 2)).tolist() == [102]
    # without clipping the whole tile is in bin 77: cum = 100 -> 255
    assert np.unique(PW.clahe(img, 0.0, 3, 2)).tolist() == [255]


def test_clip_and_redistribution_on_a_hand_sized_histogram():
    hist = np.zeros(256, np.int64)
    hist[10], hist[20], hist[30] = 700, 5, 3                         # limit 6: 694 clipped -> batch 2, residual 182, step 1
    out = PW.clip_histogram(hist, 6)
    assert out[10] == 6 + 2 + 1 and out[20] == 5 + 2 + 1 and out[30] == 3 + 2 + 1
    assert np.all(out[:182] >= 3) and np.all(out[182:] == np.where(np.arange(182, 256) == 30, 5, 2)[:])
    assert out.sum() == hist.sum()
    hist = np.zeros(256, np.int64)
    hist[0] = 50                                                     # limit 10: 40 clipped -> batch 0, residual 40, step 6
    out = PW.clip_histogram(hist, 10)
    assert out[0] == 11 and out.sum() == 50
    assert np.array_equal(np.nonzero(out[1:])[0] + 1, np.arange(6, 6 * 40, 6))


def test_clahe_padding_quirk_and_grid_orientation():
    assert PW.clahe_geometry(260, 346, 10, 10) == (270, 350, 27, 35)   # 260 divides by 10 and still gets 10 rows
    assert PW.clahe_geometry(260, 340, 10, 10) == (260, 340, 26, 34)   # both divide: no padding
    assert PW.clahe_geometry(256, 336, 4, 7) == (259, 340, 37, 85)      # (tiles_x, tiles_y) = (4, 7): x splits the width
    luts, (th, tw) = PW.clahe_luts(np.zeros((256, 336), np.uint8), 5.0, 4, 7)
    assert luts.shape == (7, 4, 256) and (th, tw) == (37, 85)


def test_add_weighted_rounds_half_to_even():
    a = np.array([3, 2, 0, 255, 1], np.uint8)
    b = np.array([2, 1, 255, 0, 0], np.uint8)
    # 1.5 * 3 - 0.5 * 2 = 3.5 -> 4;  1.5 * 2 - 0.5 * 1 = 2.5 -> 2;  saturation at both ends; 1.5 -> 2
    assert PW.add_weighted(a, 1.5, b, -0.5).tolist() == [4, 2, 0, 255, 2]


def test_unsharp_kernel_derived_from_sharpen_kernel_size():
    k = PW.unsharp_taps(3.0)                                        # sharpen_kernel_size = 3 lands in sigmaX
    assert len(k) == 19 and k.sum() == 256 and np.array_equal(k, k[::-1])
    assert k.tolist() == [0, 1, 3, 4, 9, 14, 20, 28, 32, 34, 32, 28, 20, 14, 9, 4, 3, 1, 0]
    assert len(PW.unsharp_taps(2.0)) == 13 and len(PW.unsharp_taps(0.5)) == 5
    edges = importlib.import_module(pkg + '.edges')
    assert 'sharpen_sigma_x' in edges.preprocess_image.__doc__


def test_nlmeans_table_constants():
    tab, s, fpm = PW.nlm_table(4, 3, 11)
    assert (s, fpm, len(tab)) == (4, 69599, 36577) and tab[0] == fpm
    assert [PW.nlm_shift(t) for t in (1, 3, 5, 7)] == [0, 4, 5, 6]
    hh = float(np.float32(4.3) * np.float32(4.3))                  # float32 square, not 18.49
    assert hh != 4.3 * 4.3
    tab2, _, _ = PW.nlm_table(4.3, 3, 11)
    assert tab2[5] == round(fpm * math.exp(-(5 * 16 / 9) / hh))


def test_bilateral_taps():
    r, cw, taps = PW.bilateral_setup(5, 15, 15)
    # sqrt(i^2 + j^2) <= 2 keeps 13 of the 25 offsets: rows of 1, 3, 5, 3 and 1, in row-major order
    assert r == 2 and len(taps) == 13 and cw[0] == 1.0 and taps[6][:2] == (0, 0) and taps[6][2] == 1.0
    assert [t[:2] for t in taps[:5]] == [(-2, 0), (-1, -1), (-1, 0), (-1, 1), (0, -2)]
    assert taps[1][2] == np.float32(math.exp(math.sqrt(2.0) * math.sqrt(2.0) * (-0.5 / 225.0)))
    assert len(PW.bilateral_setup(9, 15, 15)[2]) == 49 and len(PW.bilateral_setup(3, 15, 15)[2]) == 5
    assert PW.bilateral_setup(0, 15, 15)[0] == 22                     # cvRound(22.5) = 22
    assert PW.bilateral_setup(3, -1, -1)[0] == 1 and PW.bilateral_setup(1, 0, 0)[0] == 1


@pytest.mark.parametrize('kw, match', [
    ({'denoise_h': 0}, 'denoise_h'), ({'denoise_h': float('nan')}, 'denoise_h'), ({'denoise_template_win_size': 4}, 'template'),
    ({'denoise_search_win_size': 10}, 'search'), ({'denoise_template_win_size': 9}, 'template'),
    ({'denoise_search_win_size': 23}, 'search'), ({'clahe_tile_grid_size': (0, 4)}, 'clahe_tiles'),
    ({'clahe_tile_grid_size': (9, 4)}, 'clahe_tiles'), ({'clahe_clip_limit': float('inf')}, 'clahe_clip_limit'),
    ({'sharpen_kernel_size': 0}, 'sharpen_sigma'), ({'sharpen_kernel_size': 30}, 'taps'),
    ({'sharpen_alpha': float('nan')}, 'sharpen_alpha'), ({'bilateral_filter_neigh_diameter': 71}, 'radius'),
    ({'bilateral_filter_sigma_color': float('inf')}, 'sigma_color')])
def test_arguments_refused_before_any_gpu_call(kw, match):
    edges = importlib.import_module(pkg + '.edges')
    with pytest.raises(ValueError, match=match):
        edges.preprocess_image(np.zeros((6, 8), np.uint8), **dict({'clahe_tile_grid_size': (2, 2)}, **kw))


def test_default_grid_on_a_three_row_image_is_refused():
    E = importlib.import_module(pkg + '.engine')
    with pytest.raises(ValueError, match='clahe_tiles'):
        E.make_preprocess_params((3, 40))
    E.make_preprocess_params((3, 40), stages=['nlmeans', 'unsharp', 'bilateral'])       # other stages need no grid
    E.make_preprocess_params((3, 40), clahe_tiles=(10, 3))
    with pytest.raises(ValueError, match='stage'):
        E.make_preprocess_params((8, 8), stages=0)
    with pytest.raises(ValueError, match='stage'):
        E.make_preprocess_params((8, 8), stages=['sharpen'])
    with pytest.raises(TypeError, match='unknown'):
        E.make_preprocess_params((8, 8), sigma=3)


def test_symbol_struct_and_binding():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    assert re.search(r'int eincm_preprocess_image\(eincm_ctx\* ctx, const uint8_t\* src, int n, '
                     r'const eincm_preprocess_params\* params, uint8_t\* dst\);', txt)
    assert re.search(r'#define EINCM_ABI_VERSION 6\b', txt)
    L = importlib.import_module(pkg + '._lib')
    assert [n for n, _, _ in L.SIGNATURES].count('eincm_preprocess_image') == 1
    assert (L.PRE_NLMEANS, L.PRE_CLAHE, L.PRE_UNSHARP, L.PRE_BILATERAL, L.PRE_ALL) == (1, 2, 4, 8, 15)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    L = importlib.import_module(pkg + '._lib')
    fields = [f for f, _ in L.PreprocessParams._fields_]
    src = tmp_path / 'pp.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eincm.h"\nint main(void){'
                   'printf("%zu %d %d %d %d %d", sizeof(eincm_preprocess_params), EINCM_PRE_NLMEANS, EINCM_PRE_CLAHE, '
                   'EINCM_PRE_UNSHARP, EINCM_PRE_BILATERAL, EINCM_PRE_ALL);'
                   + ''.join(f'printf(" %zu", offsetof(eincm_preprocess_params, {f}));' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'pp'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.PreprocessParams) == 88
    assert vals[1:6] == [1, 2, 4, 8, 15]
    assert vals[6:] == [getattr(L.PreprocessParams, f).offset for f in fields]


def test_frames_to_edges_without_preprocessing_is_unchanged(monkeypatch):
    edges = importlib.import_module(pkg + '.edges')
    import inspect
    assert inspect.signature(edges.frames_to_edges).parameters['preprocess_image_func'].default is None
    seen = []
    # a stand-in for the GPU stages: the chain must hand Canny the same uint8 stack as before and never call preprocess_image
    monkeypatch.setattr(edges, 'preprocess_image', lambda *a, **k: seen.append('pre'))
    fake_canny = lambda c: (np.asarray(c) > 128).astype(np.uint8) * 255                       # noqa: E731
    fake_smooth = lambda e, **kw: np.asarray(e, dtype=np.float64) + 1.0                       # noqa: E731
    rng = np.random.default_rng(5)
    frames = rng.random((3, 9, 12))
    got = edges.frames_to_edges(frames, image_to_edge_func=fake_canny, smoothen_edges_func=fake_smooth)
    staging = importlib.import_module(pkg + '.staging')
    ref = staging.normalize_edges([fake_smooth(fake_canny(edges.to_canny_input(edges._normalize_to_unit_range(f))))
                                   for f in frames])
    assert np.array_equal(got, ref) and not seen
    # a batched preprocessing callable is recognised through functools.partial, a per-frame one is called per frame
    assert edges._is_batched(functools.partial(edges.preprocess_image, denoise_h=3), edges.preprocess_image)
    calls = []
    edges.frames_to_edges(frames, image_to_edge_func=fake_canny, smoothen_edges_func=fake_smooth,
                          preprocess_image_func=lambda im: calls.append(im.shape) or im)
    assert calls == [(9, 12)] * 3
