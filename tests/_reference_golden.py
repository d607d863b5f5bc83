"""Loader of the fixtures recorded from the reference's own code (tests/golden/ref_*.npz, made by
tests/golden/make_reference_golden.py)."""
import glob
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPECIAL = ('splat_window', 'objective_kinds', 'edge_maps')


def _load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, f'ref_{name}.npz'), allow_pickle=False))


def loss_case_names():
    names = (os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'ref_*.npz')))
    return sorted(n for n in names if n not in SPECIAL)


def load_loss_case(name):
    """One loss case: inputs, the recorded outputs, and conveniences (sensor_size, kw, window, objectives)."""
    d = _load(name)
    d['edges'] = d['edges'].astype(np.float64)               # recorded at fp32-representable values
    al, be, ga, de, lvl = d['params']
    d['kw'] = dict(alpha=float(al), beta=float(be), gamma=float(ga), delta=float(de), cur_pyr_lvl=int(lvl),
                   method=str(d['method']))
    d['sensor_size'] = tuple(int(v) for v in d['edges'].shape[1:])
    d['window'] = (d['xs'], d['ys'], d['ts'], d['edges'], d['edge_ts'])
    d['objectives'] = {k[4:]: d[k] for k in d if k.startswith('obj_')}
    for k in ('value', 'mean_rel_corr', 'mean_rel_contrast', 'mean_rel_iwe_divergence', 'theta_total_variation',
              'ho_value', 'ho_dalpha', 'alpha_handover'):
        if k in d:
            d[k] = float(d[k])
    d['order_sensitive'] = [str(s) for s in d['order_sensitive']]
    return d


def splat_window():
    return _load('splat_window')


def objective_kinds():
    d = _load('objective_kinds')
    d['edge'] = d['edge'].astype(np.float64)
    return d


def edge_maps():
    return _load('edge_maps')
