"""Scenes for the motion-model tests (tests/test_motion_interface.py, tests/test_gpu_motion.py): a synthetic window whose ground-truth
flow is the field of a model at coefficients c_true, and test coefficients c = c_true * U(0.5, 1.5) per coefficient - near the truth
(events land in frame) and away from the optimum, where the gradient would cancel and a max-norm relative error say nothing.  This is
synth.theta_near_truth's recipe in the coefficients.  Every scene is built once per session."""
import importlib

import numpy as np

synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
motion = importlib.import_module('edge-informed-contrast-maximization_amd.motion')

ZOOM = np.zeros((12, 1))
ZOOM[1, 0] = ZOOM[8, 0] = 1.0                      # the custom K = 1 model: Theta = c (u, v)

_SCENES = {}


def make_model(kind, shape):
    return motion.MotionModel('custom', shape, matrix=ZOOM) if kind == 'zoom' else motion.MotionModel(kind, shape)


def true_coeffs(model, rng):
    """Coefficients whose field stays within some 10 px: translation 6 px, linear terms 4 px at the border, quadratic ones 2 px; all
    of it scaled down on a sensor under 32 px, so that the events stay in frame."""
    return _true_coeffs(model, rng) * min(1.0, min(model.sensor_size) / 32.0)


def _true_coeffs(model, rng):
    K = model.n_coeffs
    if model.kind == 'rotation':
        return rng.uniform(-5.0, 5.0, 3) / model.scale                # rad per unit time: some 5 px at the principal point
    if model.kind == 'custom':
        return rng.uniform(2.0, 5.0, K) * rng.choice([-1.0, 1.0], K)
    if model.kind == 'polynomial2':
        mag = np.array([6.0, 4.0, 4.0, 2.0, 2.0, 2.0] * 2)
    else:
        mag = np.array([6.0, 6.0, 4.0, 4.0, 4.0, 4.0, 2.0, 2.0])[:K]
    return rng.uniform(0.3, 1.0, K) * rng.choice([-1.0, 1.0], K) * mag


def scene(kind, shape, n_events, R=3, seed=0):
    """(model, window dict, c (K,)) of one window."""
    key = (kind, tuple(shape), n_events, R, seed)
    if key not in _SCENES:
        model = make_model(kind, shape)
        rng = np.random.default_rng(1000 + seed)
        c_true = true_coeffs(model, rng)
        win = synth.make_window(seed, shape, n_events, R, flow=model.field(c_true))
        _SCENES[key] = (model, win, c_true * rng.uniform(0.5, 1.5, model.n_coeffs), c_true)
    return _SCENES[key][:3]


def true_of(kind, shape, n_events, R=3, seed=0):
    scene(kind, shape, n_events, R, seed)
    return _SCENES[(kind, tuple(shape), n_events, R, seed)][3]


def batch(kind, shape, n_events, R=3, seeds=(0, 1, 2)):
    """(model, [window dicts], c (B, K)) of len(seeds) windows of one model."""
    parts = [scene(kind, shape, n_events, R, s) for s in seeds]
    return parts[0][0], [p[1] for p in parts], np.stack([p[2] for p in parts])


def win_args(win):
    return (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])
