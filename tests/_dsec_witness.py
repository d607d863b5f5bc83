"""numpy witness of the DSEC data path, written from the contracts and importing nothing from the package:

  rectify_events      DSECDataLoader.rectify_events (src/dataloaders/dsec_loader.py:145-171)
  cubic_table / remap_cubic   the written contract of cv.remap(INTER_CUBIC) on 8-bit images (dsec_loader.py:243-245); remap_cubic_f64
                      is the independent float64 evaluation of the same Keys kernel the contract's integer weights approximate
  flow_decode / flow_code     the 16-bit flow format (dsec_loader.py:247-266, src/dsec_npz_to_png.py:84-96; the up-sampling before the
                      code is the oracle's, oracle/eincm_oracle.py)
  dsec_datasamples    precompute_eval_event_indices / precompute_eval_image_indices / get_sample (dsec_loader.py:173-186, :285-350)
  image_mapping_quat  construct_mapping_for_image (dsec_loader.py:188-218) through scipy Rotation and quaternions, as the reference
"""
import numpy as np


# -- rectification --------------------------------------------------------------------------------------------------------------
def rectify_events(x, y, rectify_map):
    """(rec_x, rec_y, keep): kept events in stream order, int16; keep over the input."""
    H, W, two = rectify_map.shape
    assert two == 2 and rectify_map.dtype == np.float32
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    assert x.size == 0 or (x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H)
    moved = rectify_map[y, x]                                    # (n, 2) float32
    rx = np.round(moved[:, 0]).astype(np.int16)                  # np.round: half to even, in float32
    ry = np.round(moved[:, 1]).astype(np.int16)
    keep = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    return rx[keep], ry[keep], keep


def distortion_map(H, W, k=-0.25, shift=(1.5, -2.25)):
    """A smooth synthetic rectify map (radial term about the centre plus a shift) that sends about two per cent of the pixels past each
    border (k = -0.25).  float32 (H, W, 2), channel 0 = x."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u, v = (xs - cx) / cx, (ys - cy) / cy
    r2 = u * u + v * v
    s = 1.0 + k * (r2 - 1.3)
    return np.stack([cx + u * s * cx + shift[0], cy + v * s * cy + shift[1]], axis=-1).astype(np.float32)


# -- cubic remap ----------------------------------------------------------------------------------------------------------------
def keys_weights_f32(f):
    """The four taps of the Keys cubic (A = -0.75) at offset f in [0, 1), evaluated in float32 in the written order."""
    one, A = np.float32(1), np.float32(-0.75)
    f = np.float32(f)
    a = f + one
    b = one - f
    c0 = ((A * a - np.float32(5) * A) * a + np.float32(8) * A) * a - np.float32(4) * A
    c1 = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c2 = ((A + np.float32(2)) * b - (A + np.float32(3))) * b * b + one
    c3 = one - c0 - c1 - c2
    return np.array([c0, c1, c2, c3], dtype=np.float32)


def keys_weights_f64(f):
    """The same kernel in float64: w(d) for the taps at distances 1 + f, f, 1 - f, 2 - f."""
    A = -0.75

    def w(d):
        d = abs(d)
        if d <= 1:
            return ((A + 2) * d - (A + 3)) * d * d + 1
        if d < 2:
            return ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
        return 0.0
    return np.array([w(1 + f), w(f), w(1 - f), w(2 - f)])


_TABLE = None


def cubic_table():
    """(32, 32, 4, 4) int64: [fy, fx, ky, kx].  Each set: rint(wy * wx * 32768) with the float32 product, then its sum is brought to
    32768 on the largest (sum short) or smallest (sum over) of the four middle weights [1:3, 1:3], the first in row-major order."""
    global _TABLE
    if _TABLE is None:
        one_d = [keys_weights_f32(k / 32) for k in range(32)]
        t = np.zeros((32, 32, 4, 4), dtype=np.int64)
        for fy in range(32):
            for fx in range(32):
                prod = (one_d[fy][:, None] * one_d[fx][None, :]).astype(np.float32) * np.float32(32768)
                s = np.rint(prod).astype(np.int64)
                over = int(s.sum()) - 32768
                if over != 0:
                    best = None
                    for ky in (1, 2):
                        for kx in (1, 2):
                            if best is None or (over < 0 and s[ky, kx] > s[best]) or (over > 0 and s[ky, kx] < s[best]):
                                best = (ky, kx)
                    s[best] -= over
                t[fy, fx] = s
        _TABLE = t
    return _TABLE


def fixed_point_coords(mapping):
    """(sx, sy, nan): rint(map * 32) with the product in float32, clamped to +-2^30; nan where either component is NaN."""
    m = np.asarray(mapping)
    assert m.dtype == np.float32 and m.shape[-1] == 2
    with np.errstate(invalid='ignore', over='ignore'):
        p = m * np.float32(32)
        nan = np.isnan(p).any(axis=-1)
        p = np.clip(np.where(np.isnan(p), np.float32(0), p), np.float32(-2.0 ** 30), np.float32(2.0 ** 30))
        s = np.rint(p).astype(np.int64)
    return s[..., 0], s[..., 1], nan


def remap_cubic(src, mapping):
    """The contract on (n, Hs, Ws) or (Hs, Ws) uint8 -> (n, H, W) or (H, W) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    single = src.ndim == 2
    stack = src[None] if single else src
    n, Hs, Ws = stack.shape
    sx, sy, nan = fixed_point_coords(mapping)
    ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)
    w = cubic_table()[sy & 31, sx & 31]                          # (H, W, 4, 4)
    padded = np.zeros((n, Hs + 2, Ws + 2), dtype=np.int64)       # a zero frame: every tap outside lands on it
    padded[:, 1:-1, 1:-1] = stack
    acc = np.zeros((n,) + sx.shape, dtype=np.int64)
    for ky in range(4):
        for kx in range(4):
            ty, tx = iy - 1 + ky, ix - 1 + kx
            py = np.where((ty >= 0) & (ty < Hs), ty + 1, 0)
            px = np.where((tx >= 0) & (tx < Ws), tx + 1, 0)
            acc += padded[:, py, px] * w[None, :, :, ky, kx]
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255)
    out[:, nan] = 0
    out = out.astype(np.uint8)
    return out[0] if single else out


def remap_cubic_f64(src, mapping):
    """An independent float64 evaluation at the quantised coordinate (sx / 32, sy / 32): Keys weights in float64, zero outside the
    source, floor(v + 0.5), clamped to [0, 255].  One (Hs, Ws) image."""
    src = np.asarray(src)
    Hs, Ws = src.shape
    sx, sy, nan = fixed_point_coords(mapping)
    ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)
    wx = np.array([keys_weights_f64(k / 32) for k in range(32)])[sx & 31]       # (H, W, 4)
    wy = np.array([keys_weights_f64(k / 32) for k in range(32)])[sy & 31]
    padded = np.zeros((Hs + 2, Ws + 2))
    padded[1:-1, 1:-1] = src
    v = np.zeros(sx.shape)
    for ky in range(4):
        for kx in range(4):
            ty, tx = iy - 1 + ky, ix - 1 + kx
            inside = (ty >= 0) & (ty < Hs) & (tx >= 0) & (tx < Ws)
            v += padded[np.where(inside, ty + 1, 0), np.where(inside, tx + 1, 0)] * wy[..., ky] * wx[..., kx]
    out = np.clip(np.floor(v + 0.5), 0, 255)
    out[nan] = 0
    return out.astype(np.uint8)


# -- 16-bit flow ----------------------------------------------------------------------------------------------------------------
def flow_decode(flow_16bit):
    """(flow float64 (..., 2), valid bool): (c - 2^15) / 128 where channel 2 is 1, zero elsewhere.  Channel 2 must be 0 or 1."""
    f = np.asarray(flow_16bit)
    assert f.dtype == np.uint16 and f.shape[-1] == 3
    valid = f[..., 2] == 1
    assert np.all(f[..., 2][~valid] == 0)
    out = np.zeros(f.shape[:-1] + (2,), dtype=np.float64)
    out[valid] = (f[..., :2][valid].astype(np.float64) - 2 ** 15) / 128
    return out, valid


def flow_code(scaled_theta, valid=None):
    """The submission code of an already up-sampled (.., H, W, 2) float64 flow: uint16(trunc(v * 128 + 2^15)), channel 2 zero or valid."""
    v = np.asarray(scaled_theta, dtype=np.float64) * 128 + 2 ** 15
    assert np.all(np.isfinite(v)) and v.min() >= 0 and v.max() < 65536
    out = np.zeros(v.shape[:-1] + (3,), dtype=np.uint16)
    out[..., :2] = np.trunc(v).astype(np.uint16)
    if valid is not None:
        out[..., 2] = np.asarray(valid) != 0
    return out


# -- the window rule ------------------------------------------------------------------------------------------------------------
def dsec_datasamples(events, images, image_ts_us, eval_ts_us, t_offset, eval_indices, des_n_events=1_500_000, prefer_latest_events=True,
                     flow_gt_16bit=None, mapping=None):
    t = np.asarray(events['t'])
    n = len(t)
    eval_ts_us = np.asarray(eval_ts_us)
    out = []
    for b, k in enumerate(eval_indices):
        lo = int(np.searchsorted(t, eval_ts_us[k, 0] - t_offset, side='left'))
        hi = int(np.searchsorted(t, eval_ts_us[k, 1] - t_offset, side='left'))
        im_lo = int(np.searchsorted(image_ts_us, eval_ts_us[k, 0], side='left'))
        im_hi = int(np.searchsorted(image_ts_us, eval_ts_us[k, 1], side='left'))
        orig = hi - lo
        lack = None
        if des_n_events is not None:
            lack = des_n_events - orig
            if lack > 0:                         # grow on both sides, the odd event to the front, and stay inside the stream
                lo = max(0, lo - (lack + 1) // 2)
                hi = min(n, hi + lack // 2)
            elif lack < 0:
                if prefer_latest_events:
                    lo = hi - des_n_events
                else:
                    hi = lo + des_n_events
        imgs = images[im_lo:im_hi + 1]
        if mapping is not None:
            imgs = remap_cubic(imgs, mapping)
        d = {'events': {'x': events['x'][lo:hi], 'y': events['y'][lo:hi], 't': t[lo:hi] + t_offset, 'p': events['p'][lo:hi]},
             'images': imgs, 'image_ts': np.asarray(image_ts_us)[im_lo:im_hi + 1], 'eval_ts_us': eval_ts_us[k, :2],
             'n_event_deficiency': lack, 'orig_n_events': orig}
        if flow_gt_16bit is None:
            d['file_idx'] = eval_ts_us[k, 2]
        else:
            d['flow_gt'], d['valid2D'] = flow_decode(flow_gt_16bit[b])
        out.append(d)
    return out


# -- calibration ----------------------------------------------------------------------------------------------------------------
def small_rotation(rx, ry, rz):
    """A proper rotation matrix from three small angles (radians), composed as Rz Ry Rx."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def dsec_like_calibration(seed=0):
    """A cam_to_cam dict with DSEC-like numbers: a 640 x 480 event camera and a 1440 x 1080 frame camera, milliradian rotations."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-4e-3, 4e-3, size=(3, 3))
    T_10 = np.eye(4)
    T_10[:3, :3] = small_rotation(*a[2])
    T_10[:3, 3] = [-0.045, 0.0007, 0.0012]
    return {
        'intrinsics': {
            'camRect0': {'camera_matrix': [569.7632987 + rng.uniform(-2, 2), 569.7632987 + rng.uniform(-2, 2), 335.0999832, 221.2311783]},
            'camRect1': {'camera_matrix': [1164.6238115 + rng.uniform(-4, 4), 1164.6238115 + rng.uniform(-4, 4), 713.5791168, 570.9349365]},
        },
        'extrinsics': {'R_rect0': small_rotation(*a[0]).tolist(), 'R_rect1': small_rotation(*a[1]).tolist(), 'T_10': T_10.tolist()},
    }


def image_mapping_quat(cam_to_cam, sensor_size=(480, 640)):
    """construct_mapping_for_image with every rotation held as a scipy Rotation (a quaternion inside) and composed there."""
    from scipy.spatial.transform import Rotation
    H, W = sensor_size

    def K(name):
        fx, fy, cx, cy = cam_to_cam['intrinsics'][name]['camera_matrix']
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    ex = cam_to_cam['extrinsics']
    q_r0 = Rotation.from_matrix(np.array(ex['R_rect0']))
    q_r1 = Rotation.from_matrix(np.array(ex['R_rect1']))
    q_10 = Rotation.from_matrix(np.array(ex['T_10'])[:3, :3])
    R = (q_r1 * q_10 * q_r0.inv()).as_matrix()
    P = K('camRect1') @ R @ np.linalg.inv(K('camRect0'))
    grid = np.stack(list(np.meshgrid(np.arange(W), np.arange(H))) + [np.ones((H, W))], axis=-1).astype(np.float64)
    hom = np.einsum('ij,hwj->hwi', P, grid)
    return (hom[..., :2] / hom[..., 2:]).astype(np.float32), (hom[..., :2] / hom[..., 2:])
