"""The launch policy of a staged batch (eincm_get_launch_policy; DESIGN.md 4.2 "where those rules hold"): which segment lengths, LDS
pitch regime and window capacities the library picks is not part of the results - any choice is correct, tests/test_gpu_launch_policy_parity.py checks the values cell by cell -
but it is what the measured configurations rely on, so the rules are pinned here on cheap synthetic batches (uniformly random events)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')


def _window(rng, H, W, n, R, xs=None, ys=None):
    xs = rng.integers(0, W, n).astype(np.int16) if xs is None else xs
    ys = rng.integers(0, H, n).astype(np.int16) if ys is None else ys
    return xs, ys, np.sort(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 1.0, (R, H, W)), np.linspace(0.0, 1.0, R)


def test_many_windows_one_segment_per_tile(built_lib):
    """The bench regime: 8 windows of 10^6 events on 260x346 (99 tiles, ~10^4 events each): long splat segments, aligned pitch for k_splat
    as long as the padded window stays in its capacity class."""
    rng = np.random.default_rng(1)
    H, W, N, R, B = 260, 346, 1_000_000, 5, 8
    with engine.Engine((H, W), N * B, max_refs=R, max_windows=B) as e:
        assert e.launch_policy()['cap_splat'] == 0
        e.set_windows([_window(rng, H, W, N, R) for _ in range(B)])
        p = engine.make_params(20.0, 35.0, 0.0, 0.0, 4)
        pol = e.launch_policy()
        assert pol['seg_splat'] == 16384 and pol['seg_gather_2dof'] == 16384 and pol['seg_splat_short'] == 8192 and pol['pitch_policy'] == 1
        assert pol['span_splat'] == 1.0                                           # a tile is one segment (staging has evaluated theta = 0 for the window constants)
        e.loss_grad(np.tile([20.0, -7.0], (B, 1, 1, 1)), p)                       # 36 + 20 = 56 px: 56^2 and 64 * 56 both fit 4608 words
        pol = e.launch_policy()
        assert pol['cap_splat'] == 4608 and pol['cap_gather_2dof'] == 4608 and pol['pitch_aligned'] == 1 and pol['splat_short'] == 0
        e.loss_grad(np.tile([29.0, 5.0], (B, 1, 1, 1)), p)                        # 65 px: 65^2 = 4225 fits 4608, 96 * 65 does not
        pol = e.launch_policy()
        assert pol['cap_splat'] == 4608 and pol['pitch_aligned'] == 0
        e.loss_grad(np.tile([117.0, 0.0], (B, 1, 1, 1)), p)                       # 153 px outgrow every window: the short list
        assert e.launch_policy()['splat_short'] == 1
        e.loss_grad(np.tile([[[6.0, 2.0]] * 4] * 4, (B, 1, 1, 1)), p)             # a theta grid: the splat takes what it needs (42 px)
        pol = e.launch_policy()
        assert pol['cap_splat'] == 2304 and pol['cap_gather'] == 4608 and pol['pitch_aligned'] == 0       # 64 * 42 words would need the next class
        e.loss_grad(np.tile([[[24.0, 3.0]] * 4] * 4, (B, 1, 1, 1)), p)            # 60 px: 3600 words, 64 * 60 = 3840 - both in the 4608 class
        pol = e.launch_policy()
        assert pol['cap_splat'] == 4608 and pol['pitch_aligned'] == 1


def test_tiles_of_several_segments(built_lib, monkeypatch):
    """5 * 10^6 events on 9 tiles: a long segment would double every workgroup, so 8192-event lists and pitch = width; a segment spans
    1 / 68 of the window, so a 20 px theta needs the smallest windows only.  An EINCM_SEG_SPLAT above the 16384 events whose u32 sums
    k_splat can hold is ignored: the default stands."""
    monkeypatch.setenv('EINCM_SEG_SPLAT', '32768')                              # read by eincm_create
    rng = np.random.default_rng(2)
    H, W, N, R = 96, 96, 5_000_000, 5
    with engine.Engine((H, W), N, max_refs=R) as e:
        e.set_window(*_window(rng, H, W, N, R))
        pol = e.launch_policy()
        assert pol['seg_splat'] == 8192 and pol['seg_gather_2dof'] == 8192 and pol['seg_splat_short'] == 0 and pol['pitch_policy'] == 0
        assert pol['seg_gather'] == 16384 and pol['span_splat'] < 0.02 and pol['span_gather'] < 0.04
        e.loss_grad(np.full((1, 4, 4, 2), 20.0), engine.make_params(20.0, 35.0, 0.0, 0.0, 2))
        pol = e.launch_policy()
        assert pol['cap_splat'] == 2304 and pol['pitch_aligned'] == 0


def test_sparse_tiles_set_the_span(built_lib):
    """One dense tile (200 000 events) among 34 sparse ones (1000 each, 15 % of the events): the mean tile would size the windows for a
    fraction of the time, but the sparse tiles' single segments span the whole window - the capacity follows them."""
    rng = np.random.default_rng(3)
    H, W, R = 160, 224, 3
    n_dense, n_sparse = 200_000, 34_000
    xs = np.concatenate([rng.integers(0, 32, n_dense), rng.integers(0, W, n_sparse)]).astype(np.int16)
    ys = np.concatenate([rng.integers(0, 32, n_dense), rng.integers(0, H, n_sparse)]).astype(np.int16)
    perm = rng.permutation(xs.size)
    with engine.Engine((H, W), xs.size, max_refs=R) as e:
        e.set_window(*_window(rng, H, W, xs.size, R, xs[perm], ys[perm]))
        pol = e.launch_policy()
        assert pol['span_splat'] == 1.0 and pol['span_gather'] == 1.0 and pol['span_gather_2dof'] == 1.0
        e.loss_grad(np.full((1, 4, 4, 2), 25.0), engine.make_params(20.0, 35.0, 0.0, 0.0, 2))
        assert e.launch_policy()['cap_splat'] == 4608                             # (36 + 25)^2 = 3721 words
