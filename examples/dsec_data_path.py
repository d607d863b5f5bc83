"""The DSEC data path on a synthetic recording: raw events -> rectify_events -> dsec_datasamples (frames warped
into the rectified event camera) -> stage_datasample -> one loss and gradient -> the 16-bit submission image of a theta and back.
Everything is generated from a seed; with a real sequence the arrays come from the files INTEGRATION.md lists.
    python3 examples/dsec_data_path.py [--events N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, evaluation, staging, synth  # noqa: E402

H, W = 480, 640


def recording(seed, n_events):
    """Raw events (a mild radial distortion map rectifies them), 1080 x 1440 frames, timestamps in microseconds."""
    rng = np.random.default_rng(seed)
    win = synth.make_window(seed, (H, W), n_events, 3, flow='smooth', flow_mag=8.0)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u, v = (xs - cx) / cx, (ys - cy) / cy
    s = 1.0 - 0.05 * (u * u + v * v - 1.3)
    rectify_map = np.stack([cx + u * s * cx, cy + v * s * cy], axis=-1).astype(np.float32)
    t_offset = 40_000_000
    events = {'x': win['xs'], 'y': win['ys'], 't': (1_000_000 + np.round(win['ts'] * 200_000)).astype(np.int64),
              'p': rng.random(n_events) < 0.5}
    image_ts_us = t_offset + 1_000_000 + np.arange(5, dtype=np.int64) * 50_000
    frames = np.stack([np.kron(np.clip(np.rint(30 + 200 * win['edges'][k % 3]), 0, 255).astype(np.uint8), np.ones((3, 3), np.uint8))[:1080, :1440]
                       for k in range(5)])
    eval_ts_us = np.array([[image_ts_us[0], image_ts_us[2], 0], [image_ts_us[2], image_ts_us[4], 1]], dtype=np.int64)
    cam_to_cam = {'intrinsics': {'camRect0': {'camera_matrix': [569.8, 569.8, 335.1, 221.2]},
                                 'camRect1': {'camera_matrix': [1164.6, 1164.6, 713.6, 570.9]}},
                  'extrinsics': {'R_rect0': np.eye(3).tolist(), 'R_rect1': np.eye(3).tolist(), 'T_10': np.eye(4).tolist()}}
    return events, rectify_map, frames, image_ts_us, eval_ts_us, t_offset, cam_to_cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--events', type=int, default=300_000)
    a = ap.parse_args()
    events, rectify_map, frames, image_ts_us, eval_ts_us, t_offset, cam_to_cam = recording(0, a.events)
    rect = staging.rectify_events(events, rectify_map)
    print(f'rectified: {len(rect["x"])} of {len(events["x"])} events stay on the sensor')
    mapping = staging.dsec_image_mapping(cam_to_cam, (H, W))
    samples = staging.dsec_datasamples(rect, frames, image_ts_us, eval_ts_us, t_offset, [0, 1], des_n_events=100_000, mapping=mapping)
    for s in samples:
        xs, ys, ts, edges, edge_ts = staging.stage_datasample(s)
        theta = np.zeros((16, 16, 2))
        with E.Engine((H, W), len(xs), max_refs=len(edge_ts)) as eng:
            eng.set_window(xs, ys, ts, edges, edge_ts)
            v, g, _ = eng.loss_grad(theta, E.make_params(2000.0, 4000.0, 0.0, 0.0, 0))
        theta = theta - 1e-3 * g[0] / max(np.abs(g[0]).max(), 1e-30)            # one small step, to have a flow to encode
        code = evaluation.dsec_submission_flow(theta, (H, W))
        flow, _ = evaluation.flow_16bit_to_float(np.where(np.arange(3) == 2, np.uint16(1), code))
        print(f'window file_idx {int(s["file_idx"])}: {len(xs)} events ({s["orig_n_events"]} in the window, deficiency '
              f'{s["n_event_deficiency"]}), {len(edge_ts)} frames, loss {v[0]:.6f}, |grad| max {np.abs(g[0]).max():.3e}, '
              f'submission image {code.shape} {code.dtype}, decoded flow max {np.abs(flow).max():.5f} px')


if __name__ == '__main__':
    main()
