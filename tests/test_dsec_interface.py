"""The DSEC data path without a GPU: known answers of the numpy witness tests/_dsec_witness.py worked by hand,
the remap contract's table and its distance from a float64 evaluation, the host-side functions of the package (dsec_image_mapping,
dsec_datasamples' window rule, the weight table) against the witness, and the argument refusals of every new Python function, all of
which are made before a GPU context is asked for."""
import importlib

import numpy as np
import pytest

import _dsec_witness as DW

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
staging = importlib.import_module(pkg + '.staging')
ev = importlib.import_module(pkg + '.evaluation')


# -- rectification --------------------------------------------------------------------------------------------------------------
def test_rectify_known_answers():
    """A 4 x 6 map (H = 4, W = 6).  Entries at exactly .5 round to the even neighbour both ways (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4);
    -0.5 -> -0 = 0 stays inside; W - 0.5 = 5.5 -> 6 leaves; an event that leaves between two that stay keeps their order."""
    m = np.zeros((4, 6, 2), dtype=np.float32)
    m[..., 0], m[..., 1] = np.arange(6)[None, :], np.arange(4)[:, None]          # identity
    m[0, 0] = (0.5, 0.5)          # -> (0, 0)
    m[0, 1] = (1.5, 1.5)          # -> (2, 2)
    m[0, 2] = (2.5, 2.5)          # -> (2, 2)
    m[0, 3] = (3.5, 0.0)          # -> (4, 0)
    m[1, 0] = (-0.5, 1.0)         # -> (0, 1): kept
    m[1, 1] = (5.5, 1.0)          # -> (6, 1): x == W leaves
    m[1, 2] = (2.0, 3.5)          # -> (2, 4): y == H leaves
    m[1, 3] = (-0.51, 1.0)        # -> (-1, 1): leaves
    m[2, 2] = (4.49, 2.51)        # -> (4, 3)
    x = np.array([0, 1, 2, 3, 0, 1, 2, 3, 2, 5], dtype=np.int16)
    y = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 3], dtype=np.int16)
    rx, ry, keep = DW.rectify_events(x, y, m)
    assert keep.tolist() == [True, True, True, True, True, False, False, False, True, True]
    assert rx.tolist() == [0, 2, 2, 4, 0, 4, 5] and ry.tolist() == [0, 2, 2, 0, 1, 3, 3]
    assert rx.dtype == np.int16 and ry.dtype == np.int16
    # one that leaves between two that stay: the survivors are neighbours, in stream order
    rx, ry, keep = DW.rectify_events(np.array([2, 1, 5]), np.array([2, 1, 3]), m)
    assert keep.tolist() == [True, False, True] and rx.tolist() == [4, 5] and ry.tolist() == [3, 3]


def test_rectify_refusals():
    m = DW.distortion_map(8, 10)
    events = {'x': np.zeros(3, np.int16), 'y': np.zeros(3, np.int16), 't': np.arange(3), 'p': np.zeros(3, np.int8)}
    with pytest.raises(ValueError, match='rectify_map'):
        staging.rectify_events(events, m[..., :1])
    with pytest.raises(ValueError, match='rectify_map'):
        staging.rectify_events(events, m[0])
    with pytest.raises(ValueError, match='float32'):
        staging.rectify_events(events, m.astype(np.float64))
    with pytest.raises(ValueError, match='lack'):
        staging.rectify_events({k: events[k] for k in 'xyt'}, m)
    with pytest.raises(ValueError, match='integer'):
        staging.rectify_events(dict(events, x=np.zeros(3)), m)
    with pytest.raises(ValueError, match='length'):
        staging.rectify_events(dict(events, y=np.zeros(4, np.int16)), m)
    with pytest.raises(ValueError, match='length of x'):
        staging.rectify_events(dict(events, t=np.arange(4)), m)
    with pytest.raises(ValueError, match='chunk'):
        staging.rectify_events(events, m, chunk=0)
    with pytest.raises(ValueError, match='int16 range'):
        staging.rectify_events(dict(events, x=np.array([0, 1, 70000])), m)
    with pytest.raises(ValueError, match=r'\(4, 6, 2\)'):
        E.check_rectify_map(m, (4, 6))


# -- cubic remap ----------------------------------------------------------------------------------------------------------------
def test_table_sums_and_package_table():
    t = DW.cubic_table()
    assert t.shape == (32, 32, 4, 4) and np.all(t.sum(axis=(2, 3)) == 32768)
    assert t[0, 0, 1, 1] == 32768 and np.count_nonzero(t[0, 0]) == 1
    raw = np.array([[np.rint((DW.keys_weights_f32(a / 32)[:, None] * DW.keys_weights_f32(b / 32)[None, :]).astype(np.float32)
                             * np.float32(32768)) for b in range(32)] for a in range(32)]).astype(np.int64)
    fix = np.abs(raw.sum(axis=(2, 3)) - 32768)
    assert fix.max() <= 16 and np.all(np.abs(t - raw).sum(axis=(2, 3)) == fix)         # one weight of the set carries the whole fix-up
    print('largest fix-up', fix.max(), 'sets fixed', np.count_nonzero(fix))
    got = E.remap_cubic_table()
    assert got.dtype == np.int32 and got.shape == (32, 32, 16) and np.array_equal(got.reshape(32, 32, 4, 4), t)


def test_identity_and_shift_maps():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, size=(2, 21, 33), dtype=np.uint8)
    ys, xs = np.mgrid[0:21, 0:33].astype(np.float32)
    ident = np.stack([xs, ys], axis=-1)
    assert np.array_equal(DW.remap_cubic(src, ident), src)
    for dx, dy in [(3, 0), (-2, 5), (0, -7), (40, 0)]:
        want = np.zeros_like(src)
        y0, y1, x0, x1 = max(0, -dy), min(21, 21 - dy), max(0, -dx), min(33, 33 - dx)
        if y0 < y1 and x0 < x1:
            want[:, y0:y1, x0:x1] = src[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        assert np.array_equal(DW.remap_cubic(src, ident + np.float32([dx, dy])), want), (dx, dy)
    nan_map = ident.copy()
    nan_map[3, 4, 0] = np.nan
    nan_map[5, 6] = (np.inf, -np.inf)
    out = DW.remap_cubic(src, nan_map)
    assert out[0, 3, 4] == 0 and out[0, 5, 6] == 0


def test_fixed_point_weights_within_one_level_of_float64():
    """Bound, derived from the table and not from a run.  A weight set is 16 products rounded to a multiple of 2^-15, each off by at
    most half a unit from its float32 product, which itself is off the exact Keys product by float32 rounding (below 2^-22 relative,
    nothing against a unit of 2^-15); then one fix-up of at most the sum of those 16 errors (8 units; the table test above allows 16
    to be safe).  Taking one unit per conversion and a fix-up as large as their sum: 32 units of 255 / 32768 grey levels = 0.249
    levels, under half a level.  So the exact sum S and the fixed-point sum S' differ by less than 0.5, and floor(S + 0.5) and
    (S' * 2^15 + 2^14) >> 15 = floor(S' + 0.5) can part by one level and no more.  The witness's reference here is the float64 Keys
    kernel at the same quantised coordinate, zero outside, rounded half up, saturated."""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=(60, 80), dtype=np.uint8)
    worst, share = 0, 0.0
    for seed in range(3):
        r = np.random.default_rng(seed)
        m = np.stack([r.uniform(-4, 84, size=(50, 70)), r.uniform(-4, 64, size=(50, 70))], axis=-1).astype(np.float32)
        a = DW.remap_cubic(src, m).astype(np.int64)
        b = DW.remap_cubic_f64(src, m).astype(np.int64)
        worst = max(worst, int(np.abs(a - b).max()))
        share = max(share, float(np.mean(a != b)))
    print('largest difference', worst, 'largest share of differing pixels', share)
    assert worst <= 1


def test_remap_refusals():
    m = np.zeros((4, 6, 2), dtype=np.float32)
    img = np.zeros((5, 7), dtype=np.uint8)
    with pytest.raises(ValueError, match='uint8'):
        staging.map_images_to_rect_event(img.astype(np.float32), m)
    with pytest.raises(ValueError, match='remap input'):
        staging.map_images_to_rect_event(img[0], m)
    with pytest.raises(ValueError, match='remap input'):
        staging.map_images_to_rect_event(np.zeros((0, 5, 7), np.uint8), m)
    with pytest.raises(ValueError, match=r'\(H, W, 2\)'):
        staging.map_images_to_rect_event(img, m[..., 0])
    with pytest.raises(ValueError, match='float32'):
        staging.map_images_to_rect_event(img, m.astype(np.float64))


# -- calibration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_image_mapping_against_quaternion_path(seed):
    """The package keeps rotations as matrices; the reference goes through quaternions.  The two float64 maps agree to their last
    bits, so the float32 maps may differ only where the float64 value sits at a float32 rounding boundary: counted, and capped at
    0.1 % of the entries so that a wrong matrix cannot pass."""
    cal = DW.dsec_like_calibration(seed)
    got = staging.dsec_image_mapping(cal, (480, 640))
    want32, want64 = DW.image_mapping_quat(cal, (480, 640))
    assert got.shape == (480, 640, 2) and got.dtype == np.float32
    diff = got != want32
    print('entries that differ', int(diff.sum()), 'of', diff.size)
    assert diff.sum() <= diff.size // 1000
    assert np.abs(got.astype(np.float64) - want64).max() <= np.spacing(np.float32(2048.0))       # never more than a float32 step
    assert 1.9 < got[0, 1, 0] - got[0, 0, 0] < 2.2            # about two frame pixels per event pixel


def test_image_mapping_refusals():
    cal = DW.dsec_like_calibration(0)
    bad = {'intrinsics': cal['intrinsics'], 'extrinsics': {k: v for k, v in cal['extrinsics'].items() if k != 'T_10'}}
    with pytest.raises(ValueError, match='T_10'):
        staging.dsec_image_mapping(bad)
    bad = {'intrinsics': {'camRect0': {'camera_matrix': [1, 2, 3]}, 'camRect1': cal['intrinsics']['camRect1']}, 'extrinsics': cal['extrinsics']}
    with pytest.raises(ValueError, match='four'):
        staging.dsec_image_mapping(bad)
    bad = {'intrinsics': cal['intrinsics'], 'extrinsics': dict(cal['extrinsics'], R_rect0=np.eye(4).tolist())}
    with pytest.raises(ValueError, match=r'\(3, 3\)'):
        staging.dsec_image_mapping(bad)
    bad = {'intrinsics': cal['intrinsics'], 'extrinsics': dict(cal['extrinsics'], R_rect1=(np.eye(3) * np.nan).tolist())}
    with pytest.raises(ValueError, match='non-finite'):
        staging.dsec_image_mapping(bad)
    with pytest.raises(ValueError, match='sensor_size'):
        staging.dsec_image_mapping(cal, (0, 640))


# -- flow codec -----------------------------------------------------------------------------------------------------------------
def test_flow_round_trip_every_code():
    """decode(encode(v)) = v for every v = k / 128 in range: all 65536 codes."""
    codes = np.arange(65536, dtype=np.int64)
    v = (codes - 32768) / 128.0
    flow = np.stack([v, v[::-1]], axis=-1).reshape(256, 256, 2)
    enc = DW.flow_code(flow, valid=np.ones((256, 256)))
    assert enc.dtype == np.uint16 and np.array_equal(enc[..., 0].ravel(), codes) and np.all(enc[..., 2] == 1)
    dec, valid = DW.flow_decode(enc)
    assert valid.all() and np.array_equal(dec, flow)
    # truncation, not rounding: just under the next code stays; an invalid pixel decodes to exactly 0
    assert DW.flow_code(np.array([[[1 / 128 - 1e-9, -1 / 128 + 1e-9]]]))[0, 0].tolist() == [32768, 32767, 0]
    dec, valid = DW.flow_decode(np.array([[[40000, 20000, 0], [40000, 20000, 1]]], dtype=np.uint16))
    assert dec[0, 0].tolist() == [0.0, 0.0] and dec[0, 1].tolist() == [(40000 - 32768) / 128, (20000 - 32768) / 128]
    assert valid.tolist() == [[False, True]]


def test_flow_refusals():
    f = np.zeros((4, 6, 3), dtype=np.uint16)
    with pytest.raises(ValueError, match='uint16'):
        ev.flow_16bit_to_float(f.astype(np.int32))
    with pytest.raises(ValueError, match='16-bit flow'):
        ev.flow_16bit_to_float(f[..., :2])
    with pytest.raises(ValueError, match='16-bit flow'):
        ev.flow_16bit_to_float(f[0])
    th = np.zeros((2, 2, 2))
    with pytest.raises(ValueError, match='theta'):
        ev.dsec_submission_flow(th[..., :1], (4, 6))
    with pytest.raises(ValueError, match='theta'):
        ev.dsec_submission_flow(th[0], (4, 6))
    with pytest.raises(ValueError, match='numeric'):
        ev.dsec_submission_flow(th.astype(complex), (4, 6))
    with pytest.raises(ValueError, match='valid'):
        ev.dsec_submission_flow(th, (4, 6), valid=np.ones((4, 5)))
    with pytest.raises(ValueError, match='valid'):
        ev.dsec_submission_flow(np.zeros((3, 2, 2, 2)), (4, 6), valid=np.ones((2, 4, 6)))


# -- the window rule ------------------------------------------------------------------------------------------------------------
def _stream():
    t = np.array([100, 110, 110, 120, 130, 140, 150, 160, 170, 180, 190, 200], dtype=np.int64)       # 12 events, one tie
    n = len(t)
    events = {'x': np.arange(n, dtype=np.int16), 'y': np.arange(n, dtype=np.int16) + 20, 't': t, 'p': (np.arange(n) % 2).astype(np.int8)}
    image_ts = np.array([1090, 1110, 1130, 1150, 1170, 1190, 1210], dtype=np.int64)
    images = np.arange(7, dtype=np.uint8)[:, None, None] * np.ones((1, 4, 6), dtype=np.uint8)
    t_offset = 1000
    eval_ts = np.array([[1130, 1170, 10],       # starts and ends exactly on an event time and an image time
                        [1105, 1195, 12],       # long
                        [1185, 1200, 14],       # short, at the end of the stream
                        [1100, 1112, 16]], dtype=np.int64)
    return events, images, image_ts, eval_ts, t_offset


def _same(a, b):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        if k == 'events':
            for c in 'xytp':
                assert np.array_equal(a[k][c], b[k][c]) and a[k][c].dtype == b[k][c].dtype, (k, c)
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_datasamples_by_hand():
    events, images, image_ts, eval_ts, off = _stream()
    # window 0, des 4: [130, 170) on the offset-free times is events 4..7 ('left' on both ends: the event at 170 is not in, the one
    # at 130 is); images 'left' of 1130 -> 2, of 1170 -> 4, slice 2:5
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0], des_n_events=4)[0]
    assert d['events']['x'].tolist() == [4, 5, 6, 7] and d['events']['t'].tolist() == [1130, 1140, 1150, 1160]
    assert d['events']['y'].tolist() == [24, 25, 26, 27] and d['events']['p'].tolist() == [0, 1, 0, 1]
    assert d['image_ts'].tolist() == [1130, 1150, 1170] and np.asarray(d['images'])[:, 0, 0].tolist() == [2, 3, 4]
    assert d['eval_ts_us'].tolist() == [1130, 1170] and d['file_idx'] == 10
    assert d['n_event_deficiency'] == 0 and d['orig_n_events'] == 4
    assert sorted(d) == ['eval_ts_us', 'events', 'file_idx', 'image_ts', 'images', 'n_event_deficiency', 'orig_n_events']
    # short: 4 events wanted 7 -> deficiency 3, two more in front (ceil), one behind (floor): events 2..8
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0], des_n_events=7)[0]
    assert d['events']['x'].tolist() == [2, 3, 4, 5, 6, 7, 8] and d['n_event_deficiency'] == 3 and d['orig_n_events'] == 4
    # short at the stream's end: [185, 200) -> events 9..10 (190; 200 is 'left' out): 10, 11); wanted 8: deficiency 7, 4 in front,
    # 3 behind clamped to the stream's 12
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [2], des_n_events=8)[0]
    assert d['orig_n_events'] == 1 and d['n_event_deficiency'] == 7 and d['events']['x'].tolist() == [6, 7, 8, 9, 10, 11]
    # short at the stream's start: [100, 112) -> events 0..2 (the tie at 110 both in); wanted 9: 6 short, 3 + 3, start clamped to 0
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [3], des_n_events=9)[0]
    assert d['orig_n_events'] == 3 and d['events']['x'].tolist() == [0, 1, 2, 3, 4, 5]
    assert d['image_ts'].tolist() == [1110, 1130]            # 'left' of 1100 -> 1, of 1112 -> 2, slice 1:3
    # long: [105, 195) -> events 1..10 (10 events), wanted 3: the latest three, or the earliest three
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [1], des_n_events=3, prefer_latest_events=True)[0]
    assert d['events']['x'].tolist() == [8, 9, 10] and d['n_event_deficiency'] == -7 and d['orig_n_events'] == 10
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [1], des_n_events=3, prefer_latest_events=False)[0]
    assert d['events']['x'].tolist() == [1, 2, 3]
    # no count rule: the deficiency is not defined
    d = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [1], des_n_events=None)[0]
    assert d['n_event_deficiency'] is None and d['events']['x'].tolist() == list(range(1, 11))


@pytest.mark.parametrize('des,latest', [(None, True), (1, True), (4, False), (5, True), (9, True), (30, False)])
def test_datasamples_against_witness(des, latest):
    events, images, image_ts, eval_ts, off = _stream()
    got = staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [3, 0, 1, 2], des_n_events=des, prefer_latest_events=latest)
    want = DW.dsec_datasamples(events, images, image_ts, eval_ts, off, [3, 0, 1, 2], des_n_events=des, prefer_latest_events=latest)
    assert len(got) == 4
    for a, b in zip(got, want):
        _same(a, b)


def test_datasamples_refusals():
    events, images, image_ts, eval_ts, off = _stream()
    with pytest.raises(ValueError, match='eval_ts_us'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts[:, :2], off, [0])          # no file index and no GT
    with pytest.raises(ValueError, match='eval_ts_us'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts[:, 0], off, [0])
    with pytest.raises(ValueError, match='images'):
        staging.dsec_datasamples(events, images[:3], image_ts, eval_ts, off, [0])
    with pytest.raises(ValueError, match='lack'):
        staging.dsec_datasamples({k: events[k] for k in 'xyt'}, images, image_ts, eval_ts, off, [0])
    with pytest.raises(ValueError, match='one length'):
        staging.dsec_datasamples(dict(events, p=events['p'][:3]), images, image_ts, eval_ts, off, [0])
    with pytest.raises(ValueError, match='eval index'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [4])
    with pytest.raises(ValueError, match='des_n_events'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0], des_n_events=0)
    with pytest.raises(ValueError, match='uint16'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0], flow_gt_16bit=np.zeros((1, 4, 6, 3)))
    with pytest.raises(ValueError, match='one .* per requested window'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0, 1], flow_gt_16bit=np.zeros((1, 4, 6, 3), np.uint16))
    with pytest.raises(ValueError, match='float32'):
        staging.dsec_datasamples(events, images, image_ts, eval_ts, off, [0], mapping=np.zeros((4, 6, 2)))


def test_engine_argument_checks():
    """The checks the Engine methods make before they touch the GPU."""
    with pytest.raises(ValueError, match='chunk'):
        E.check_chunk(True)
    with pytest.raises(ValueError, match='chunk'):
        E.check_chunk((1 << 30) + 1)
    with pytest.raises(ValueError, match='1-D'):
        E.check_event_coords(np.zeros((2, 2), np.int16), np.zeros((2, 2), np.int16))
    x, y = E.check_event_coords(np.array([1, 2], np.uint16), np.array([3, 4], np.int64))
    assert x.dtype == np.int16 and y.dtype == np.int16
    t, v, single = E.check_theta_batch(np.zeros((3, 4, 2), np.float32), np.ones((4, 6)), (4, 6))
    assert t.shape == (1, 3, 4, 2) and t.dtype == np.float64 and v.shape == (1, 4, 6) and v.dtype == np.uint8 and single
