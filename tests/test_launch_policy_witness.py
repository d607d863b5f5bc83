"""The launch-policy witness (tests/_launch_policy_witness.py) against what is known without a GPU: the staging table of the two
parity batches, the cell every parity case is named for (tests/_launch_policy_cases.py), and the numbers
tests/test_gpu_launch_policy.py pins on its three batches.  A case that drifts out of its cell fails here; the GPU module
(tests/test_gpu_launch_policy_parity.py) then holds the library to the witness field by field before it compares any number."""
import math

import numpy as np
import pytest

import _launch_policy_cases as C
import _launch_policy_witness as LP


def _window(rng, H, W, n, R):
    """The draws of tests/test_gpu_launch_policy.py::_window in its order (coordinates, timestamps, edge images): (xs, ys)."""
    xs, ys = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
    rng.uniform(0.0, 1.0, n)
    rng.uniform(0.0, 1.0, (R, H, W))
    return xs, ys


def test_window_geometry_rules():
    assert [LP.win_maxw(c) for c in LP.CAPS] == [57, 66, 80, 98] and LP.win_maxw(1024) == 40
    assert LP.balanced_seg_len(12_004, 16384) == 16384 and LP.balanced_seg_len(12_004, 8192) == 6144
    assert LP.balanced_seg_len(20_004, 8192) == 6912 and LP.balanced_seg_len(16385, 16384) == 8448
    assert LP.segment_lengths([12_004, 0, 3], 8192) == [6144, 5860, 3]
    # 48 x 48 fills the smallest class, one more pixel takes the next; the aligned pitch only where it stays in the class
    assert LP.fit_window(12.0, 1.0, 4.0, 0, 1) == dict(cap=2304, maxw=57, aligned=False, fits=True, side=48)
    assert LP.fit_window(12.01, 1.0, 4.0, 0, 1)['cap'] == 3072
    assert LP.fit_window(28.0, 1.0, 4.0, 2, 1)['aligned'] and not LP.fit_window(28.0, 1.0, 4.0, 2, 0)['aligned']
    assert LP.fit_window(47.0, 1.0, 4.0, 2, 1)['fits'] and not LP.fit_window(48.0, 1.0, 4.0, 2, 1)['fits']
    # the theta-grid gather's rule: the unrounded side (47.1 px of flow: 83.1^2 = 6906 fits 6912, the rounded 84^2 does not)
    assert LP.fit_window(47.1, 1.0, 4.0, 2, -1)['fits'] and not LP.fit_window(47.1, 1.0, 4.0, 2, 0)['fits']
    assert not LP.fit_window(47.2, 1.0, 4.0, 2, -1)['fits']
    assert LP.fit_window(11.5, 1.0, 4.0, 2, -1)['cap'] == 4608                       # the floor class
    # a splat window of size 5: margin 6
    assert LP.fit_window(35.0, 1.0, 6.0, 2, 1)['side'] == 73


def test_span_follows_all_but_three_percent():
    # 97 % of the events in tiles of three segments, 3 % in single-segment tiles: inside the allowance
    assert LP.list_span([9700 * 2, 300, 300], 8192) == 1.0 / 3
    assert LP.list_span([9699 * 2, 301, 301], 8192) == 1.0                          # one event over
    assert LP.list_span([0, 0], 8192) == 1.0 / 64 and LP.list_span([8192 * 100], 8192) == 1.0 / 64


@pytest.mark.parametrize('name', ['A', 'B'])
def test_parity_batches_stage_as_tabulated(name):
    st = LP.stage_policy(C.counts(name), C.H, C.W, C.R, C.B)
    want = C.STAGED[name]
    assert st['n_events'] == want['n_events'] and math.floor(st['x_wg'] + 0.5) == want['x_wg']
    for k in ('seg_splat', 'seg_gather_2dof', 'seg_splat_short', 'pitch_policy', 'span_splat', 'span_splat_short'):
        assert st[k] == want[k], k
    assert st['seg_gather'] == 16384 and st['span_gather'] == st['span_gather_2dof'] == st['span_splat']
    # the batch is what the cases' comments say: two dense tiles per window, none in the 4-pixel-tall last tile row, window 0 with
    # tile (0, 0) and a tile of the 26-pixel-wide last column; the sparse tiles inside the 3 % allowance
    cnt = C.counts(name).reshape(C.B, C.TILES_Y, C.TILES_X)
    dense = cnt >= C.DENSE[name]
    assert (dense.sum(axis=(1, 2)) == 2).all() and not dense[:, -1].any()
    assert dense[0, 0, 0] and dense[0, 3, C.TILES_X - 1]
    assert len({tuple(np.flatnonzero(d)) for d in dense}) > C.B // 2                 # the dense tiles differ between the windows
    assert 0 < cnt[~dense].sum() <= 0.03 * cnt.sum() and cnt[~dense].max() < 4096
    assert LP.stage_policy(C.counts(name), C.H, C.W, C.R, C.B, pitch_env=2)['pitch_policy'] == 2


@pytest.mark.parametrize('case', C.CASES, ids=[c.id for c in C.CASES])
def test_every_case_sits_in_its_cell(case):
    th = C.theta(case)
    assert th.shape == (C.B,) + case.hw + (2,)
    a = np.abs(th)
    assert a.max() == case.v
    if case.kind == '2dof':
        assert tuple(th[0, 0, 0]) == (case.v, -case.v) and (a[..., 0] == case.v).all()
    else:
        assert a.min() >= 0.6 * case.v and ((a[..., 0] == case.v) & (a[..., 1] == case.v)).any(axis=(1, 2)).all()
        s = np.sign(th)
        if case.kind == 'checker':
            assert (s[:, :-1] == -s[:, 1:]).all() and (s[:, :, :-1] == -s[:, :, 1:]).all()
        else:
            assert (s == s[:, :1, :1]).all()
    st = LP.stage_policy(C.counts(case.batch), C.H, C.W, C.R, C.B)
    ev = LP.eval_policy(st, a.max(), case.two_dof)
    s = ev['splat']
    assert ('short' if ev['splat_short'] else 'long') == case.list
    assert (s['cap'], s['aligned'], s['fits'], s['side']) == (case.cap, case.aligned, case.fits, case.side)
    assert ev['long_fits'] == (case.fits and case.list == 'long')
    span = st['span_splat_short'] if ev['splat_short'] else st['span_splat']
    assert case.side == math.ceil(LP.window_side(case.v, span))
    if case.fits:
        assert case.side ** 2 <= case.cap and (case.cap == LP.CAPS[0 if not case.two_dof else 2] or case.side ** 2 > LP.CAPS[LP.CAPS.index(case.cap) - 1])
        assert case.aligned == (-(-case.side // 32) * 32 * case.side <= case.cap)
    else:
        assert case.side ** 2 > LP.CAPS[-1] and case.cap == LP.CAPS[-1] and not case.aligned
    if not case.two_dof:
        assert case.list == 'long'                                                   # a grid has no short list
    # the clamped cells: windows wider than the class was sized for
    if case.kind == 'checker':
        widest, clamped = C.tile_windows(case, s['cap'], s['maxw'])
        if case.hw == (16, 16):
            assert widest == C.widest_window(case, span) == 76 and clamped > 0.75
        else:
            assert widest == 57 and clamped < 0.01
    if case.batch == 'B' and case.two_dof and case.list == 'long' and case.aligned:
        full = C.widest_window(case, 1.0)                                            # the sparse tiles' segments span the window
        assert full > s['maxw'] >= 64 and (s['maxw'] & ~31) in (64, 96)


def test_named_cells_are_all_there():
    """Every cell of the table in DESIGN.md 4.2 has a case: list x class x aligned / unaligned, filled classes, overflow."""
    cells = {(c.two_dof, c.list, c.cap, c.aligned, c.fits) for c in C.CASES}
    for cap in (4608, 6912):
        for lst in ('long', 'short'):
            assert (True, lst, cap, True, True) in cells, (lst, cap)
            assert (True, lst, cap, False, True) in cells, (lst, cap)
    assert (True, 'short', 6912, False, False) in cells
    for cap, aligned in ((2304, False), (3072, False), (4608, True), (4608, False), (6912, True), (6912, False)):
        assert (False, 'long', cap, aligned, True) in cells, (cap, aligned)
    assert (False, 'long', 6912, False, False) in cells
    # A cell the rules cannot reach: the 2304 and 3072 classes at the aligned pitch.  A window is at least 36 px (the tile and its
    # margin) and is padded to 64 words per row: 64 * 36 = 2304 holds at theta = 0 only (the staging's own evaluation), and a
    # window of 37..48 px takes 2304 unpadded, where 64 * side > 2304; 3072 is the class of 49..55 px, where 64 * side > 3072.
    for side in range(37, 56):
        f = LP.fit_window(side - 36.0, 1.0, 4.0, 0, 1)
        assert f['cap'] < 4608 and not f['aligned'], side
    assert LP.fit_window(0.0, 1.0, 4.0, 0, 1) == dict(cap=2304, maxw=57, aligned=True, fits=True, side=36)


def test_staging_stride_case_is_sampled_past_its_spikes():
    win, th, stride = C.strided_case()
    assert th.size == 24_576 and th.size // 8192 == stride
    flat = np.abs(th.reshape(-1))
    assert flat.max() == 60.0 and flat[::stride].max() <= 4.0 and (flat == 60.0).sum() >= 150
    Hs, Ws = win['sensor_size']
    cnt = LP.tile_counts(win['xs'], win['ys'], Hs, Ws)[None]
    pol = LP.launch_policy(cnt, Hs, Ws, len(win['edge_ts']), 1, vmax=flat[::stride].max(), two_dof=False)
    assert pol['cap_splat'] == 2304 and pol['seg_splat'] == 4096 and pol['span_splat'] == 1.0
    assert not LP.eval_policy(LP.stage_policy(cnt, Hs, Ws, len(win['edge_ts']), 1), 60.0, False)['long_fits']


def _uniform_counts(seed, H, W, N, R, B):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        xs, ys = _window(rng, H, W, N, R)[:2]
        out.append(LP.tile_counts(xs, ys, H, W))
    return np.stack(out)


def test_witness_gives_the_pinned_numbers_of_the_bench_regime():
    """tests/test_gpu_launch_policy.py::test_many_windows_one_segment_per_tile, recomputed from its tile counts."""
    H, W, N, R, B = 260, 346, 1_000_000, 5, 8
    cnt = _uniform_counts(1, H, W, N, R, B)
    pol = LP.launch_policy(cnt, H, W, R, B)
    assert pol['cap_splat'] == 0
    assert pol['seg_splat'] == 16384 and pol['seg_gather_2dof'] == 16384 and pol['seg_splat_short'] == 8192 and pol['pitch_policy'] == 1
    assert pol['span_splat'] == 1.0
    pol = LP.launch_policy(cnt, H, W, R, B, vmax=20.0, two_dof=True)
    assert pol['cap_splat'] == 4608 and pol['cap_gather_2dof'] == 4608 and pol['pitch_aligned'] == 1 and pol['splat_short'] == 0
    pol = LP.launch_policy(cnt, H, W, R, B, vmax=29.0, two_dof=True)
    assert pol['cap_splat'] == 4608 and pol['pitch_aligned'] == 0
    assert LP.launch_policy(cnt, H, W, R, B, vmax=117.0, two_dof=True)['splat_short'] == 1
    pol = LP.launch_policy(cnt, H, W, R, B, vmax=6.0, two_dof=False)
    assert pol['cap_splat'] == 2304 and pol['cap_gather'] == 4608 and pol['pitch_aligned'] == 0
    pol = LP.launch_policy(cnt, H, W, R, B, vmax=24.0, two_dof=False)
    assert pol['cap_splat'] == 4608 and pol['pitch_aligned'] == 1


def test_witness_gives_the_pinned_numbers_of_tiles_of_several_segments():
    """tests/test_gpu_launch_policy.py::test_tiles_of_several_segments."""
    H, W, N, R = 96, 96, 5_000_000, 5
    cnt = _uniform_counts(2, H, W, N, R, 1)
    pol = LP.launch_policy(cnt, H, W, R, 1, vmax=20.0, two_dof=False)
    assert pol['seg_splat'] == 8192 and pol['seg_gather_2dof'] == 8192 and pol['seg_splat_short'] == 0 and pol['pitch_policy'] == 0
    assert pol['seg_gather'] == 16384 and pol['span_splat'] < 0.02 and pol['span_gather'] < 0.04
    assert pol['cap_splat'] == 2304 and pol['pitch_aligned'] == 0


def test_witness_gives_the_pinned_numbers_of_sparse_tiles():
    """tests/test_gpu_launch_policy.py::test_sparse_tiles_set_the_span."""
    rng = np.random.default_rng(3)
    H, W, R = 160, 224, 3
    n_dense, n_sparse = 200_000, 34_000
    xs = np.concatenate([rng.integers(0, 32, n_dense), rng.integers(0, W, n_sparse)]).astype(np.int16)
    ys = np.concatenate([rng.integers(0, 32, n_dense), rng.integers(0, H, n_sparse)]).astype(np.int16)
    cnt = LP.tile_counts(xs, ys, H, W)[None]
    pol = LP.launch_policy(cnt, H, W, R, 1, vmax=25.0, two_dof=False)
    assert pol['span_splat'] == 1.0 and pol['span_gather'] == 1.0 and pol['span_gather_2dof'] == 1.0
    assert pol['cap_splat'] == 4608
