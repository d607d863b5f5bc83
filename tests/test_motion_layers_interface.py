"""The composition of a motion segmentation where no GPU is needed: the symbol in the binding table and in the
built library, the flag values against the header, every refusal of check_compose_args and of check_segmented_flow_args with its
message, the layout's shapes, and the witness's own functions on hand-made pixels."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import _motion_layers_witness as WIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')
M = importlib.import_module('edge-informed-contrast-maximization_amd.motion')
S = importlib.import_module('edge-informed-contrast-maximization_amd.segmentation')


def test_symbol_is_bound_and_exported(built_lib):
    sig = {n: (r, a) for n, r, a in L.SIGNATURES}
    assert 'eincm_compose_motions' in sig
    res, args = sig['eincm_compose_motions']
    assert res is C.c_int and len(args) == 8 and args[1] is C.c_int and args[3] is C.c_uint
    assert hasattr(built_lib, 'eincm_compose_motions') and built_lib.eincm_abi_version() == 6


def test_flag_values_are_the_headers():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    val = {n: int(v) for n, v in re.findall(r'#define\s+EINCM_ML_(\w+)\s+(\d+)u?\b', txt)}
    assert val == dict(HARD=L.ML_HARD, SOFT=L.ML_SOFT, FILL_ZERO=L.ML_FILL_ZERO, FILL_DOMINANT=L.ML_FILL_DOMINANT, NO_LABEL=L.ML_NO_LABEL)
    assert L.ML_MODES == {'hard': 0, 'soft': 1} and L.ML_FILLS == {'zero': 0, 'dominant': 2}
    assert WIT.NO_LABEL == L.ML_NO_LABEL and WIT.Q_ONE == L.ML_Q_ONE
    assert re.search(r'#define\s+EINCM_ABI_VERSION\s+6\b', txt)


def test_null_context_is_refused_without_a_gpu(built_lib):
    assert built_lib.eincm_compose_motions(None, 2, None, 0, None, None, None, None) == L.ERR_ARG


GOOD = dict(n_models=2, coeffs=np.zeros((4, 6)), n_windows=4, n_coeffs=6, mode='hard', fill='zero', want=('theta', 'labels'))


def _args(**kw):
    a = dict(GOOD)
    a.update(kw)
    return a


def test_good_arguments_come_back_normalised():
    K, c, flags, want = E.check_compose_args(**_args(coeffs=[[1, 2, 3, 4, 5, 6]] * 4, mode='soft', fill='dominant', want='mass'))
    assert K == 2 and c.dtype == np.float64 and c.flags.c_contiguous and c.shape == (4, 6) and flags == 3 and want == ('mass',)
    assert E.check_compose_args(**_args())[2] == 0 and E.check_compose_args(**_args(fill='dominant'))[2] == 2
    assert E.check_compose_args(**_args(mode='soft'))[2] == 1
    # what depends on the staged batch or the values is the library's to refuse: it passes here
    E.check_compose_args(**_args(coeffs=np.full((4, 6), np.nan)))
    E.check_compose_args(**_args(n_models=3))
    E.check_compose_args(**_args(coeffs=np.zeros((5, 9)), n_windows=0, n_coeffs=None))
    assert E.check_compose_args(**_args(want=E.ML_OUTPUTS))[3] == ('theta', 'labels', 'mass', 'total')


@pytest.mark.parametrize('kw,msg', [
    (dict(n_models=0), r'n_models must be an integer within 1 \.\. 8, got 0'),
    (dict(n_models=9), r'n_models must be an integer within 1 \.\. 8, got 9'),
    (dict(n_models=2.0), r'n_models must be an integer within 1 \.\. 8, got 2\.0'),
    (dict(n_models=True), r'n_models must be an integer within 1 \.\. 8, got True'),
    (dict(mode='blend'), r"mode 'blend' unknown; one of \('hard', 'soft'\)"),
    (dict(mode=1), r"mode 1 unknown"),
    (dict(fill='nearest'), r"fill 'nearest' unknown; one of \('zero', 'dominant'\)"),
    (dict(want=()), r'want must be a non-empty choice of .* without repeats, got \(\)'),
    (dict(want=('theta', 'flow')), r'want must be a non-empty choice'),
    (dict(want=('mass', 'mass')), r'without repeats'),
    (dict(coeffs=np.zeros((4, 6), dtype=bool)), r'coeffs must be numeric, got dtype bool'),
    (dict(coeffs=[['a'] * 6] * 4), r'coeffs must be numeric'),
    (dict(coeffs=np.zeros(6)), r'coeffs must be \(4, 6\): one row of model coefficients per staged window, got \(6,\)'),
    (dict(coeffs=np.zeros((3, 6))), r'coeffs must be \(4, 6\).* got \(3, 6\)'),
    (dict(coeffs=np.zeros((4, 2))), r'coeffs must be \(4, 6\).* got \(4, 2\)'),
    (dict(coeffs=np.zeros((2, 2, 6))), r'coeffs must be \(4, 6\)'),
    (dict(coeffs=np.zeros((4, 6, 1)), n_windows=0, n_coeffs=None), r'coeffs must be \(B, K_c\)'),
])
def test_every_refusal_and_its_message(kw, msg):
    with pytest.raises(ValueError, match=msg):
        E.check_compose_args(**_args(**kw))


def test_layout_shapes():
    lay = E.compose_motions_layout(3, 2, (40, 72))
    assert lay['theta'][0] == (3, 40, 72, 2) and lay['labels'][0] == (3, 40, 72) and lay['mass'][0] == (3, 2, 40, 72) and lay['total'][0] == (3, 2)
    assert lay['mass'][2].tolist() == [0, 2 * 40 * 72, 4 * 40 * 72] and lay['theta'][2].dtype == np.int64
    assert all(len(E.compose_motions_layout(0, 2, (40, 72))[n][2]) == 0 for n in E.ML_OUTPUTS)


# ---- segmented_flow's own check ----
def _windows(G=2, n=5):
    return [(np.zeros(n, np.int16), np.zeros(n, np.int16), np.zeros(n), np.zeros((1, 8, 9)), np.zeros(1)) for _ in range(G)]


def _record(G=2, K=2, n=5, Kc=2):
    return dict(coeffs=np.zeros((G, K, Kc)), weights=[[np.full(n, 0.5) for _ in range(K)] for _ in range(G)])


def test_segmented_flow_arguments():
    model = M.MotionModel('translation', (8, 9))
    c, w = S.check_segmented_flow_args(_windows(), model, _record())
    assert c.shape == (2, 2, 2) and w[1][1].dtype == np.float32 and w[1][1].shape == (5,)
    bad = [(dict(windows=[]), 'at least one'), (dict(windows=[w + (None,) for w in _windows()]), 'got 6 elements'),
           (dict(record=[1]), "a dict with 'coeffs' and 'weights'"), (dict(record=dict(coeffs=np.zeros((2, 2, 2)))), "a dict with 'coeffs'"),
           (dict(record=_record(Kc=3)), r"record\['coeffs'\] must be \(2, K, 2\)"), (dict(record=_record(G=3)), r"record\['coeffs'\] must be"),
           (dict(record=dict(_record(), weights=None)), 'record_weights=False'),
           (dict(record=dict(_record(), weights=_record(K=3)['weights'])), 'must be 2 lists of 2 weight arrays'),
           (dict(record=_record(n=4)), r'window 0: every array .* must be \(5,\)')]
    for kw, msg in bad:
        a = dict(windows=_windows(), model=model, record=_record())
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            S.check_segmented_flow_args(**a)


# ---- the witness on pixels a reader can follow ----
def test_witness_on_a_hand_made_group():
    model = M.MotionModel('affine', (3, 4))
    xs = np.array([0, 0, 3, 3, 1]); ys = np.array([0, 0, 2, 2, 1])
    w0 = np.array([1.0, 0.5, 0.25, 0.25, 0.00001], dtype=np.float32)
    w1 = np.array([0.0, 0.5, 0.25, 0.75, 0.00001], dtype=np.float32)
    c = np.array([[1.0, 2.0, 0.1, 0.2, 0.3, 0.4], [-3.0, 0.5, 0.0, 0.0, 0.0, 0.0]])
    r = WIT.compose(model, [(xs, ys, [w0, w1])], c, 'hard', 'zero')
    assert r['mass'].dtype == np.uint32 and r['total'].dtype == np.uint64 and r['labels'].dtype == np.uint8
    assert r['mass'][0, :, 0, 0].tolist() == [6144, 2048] and r['mass'][0, :, 2, 3].tolist() == [2048, 4096] and r['mass'][0, :, 1, 1].tolist() == [0, 0]
    assert r['total'].tolist() == [[8192, 6144]]
    assert r['labels'][0, 0, 0] == 0 and r['labels'][0, 2, 3] == 1 and r['labels'][0, 1, 1] == 255 and (r['labels'] == 255).sum() == 10
    f = model.field(c)
    assert np.array_equal(r['theta'][0, 0, 0], f[0, 0, 0]) and np.array_equal(r['theta'][0, 2, 3], f[1, 2, 3]) and not r['theta'][0, 1, 1].any()
    d = WIT.compose(model, [(xs, ys, [w0, w1])], c, 'hard', 'dominant')['theta']
    assert np.array_equal(d[0, 1, 1], f[0, 1, 1]) and np.array_equal(d[0, 0, 0], f[0, 0, 0])
    s = WIT.compose(model, [(xs, ys, [w0, w1])], c, 'soft', 'zero')['theta']
    assert np.array_equal(s[0, 0, 0], 0.75 * f[0, 0, 0] + 0.25 * f[1, 0, 0]) and not s[0, 1, 1].any()
    assert np.array_equal(s[0, 2, 3], (2048 / 6144) * f[0, 2, 3] + (4096 / 6144) * f[1, 2, 3])
    # an equal split goes to the lowest label; unweighted windows count 4096 per event
    t = WIT.compose(model, [(xs, ys, [None, None])], c)
    assert t['labels'][0, 0, 0] == 0 and t['mass'][0, :, 0, 0].tolist() == [8192, 8192] and t['total'].tolist() == [[5 * 4096] * 2]
