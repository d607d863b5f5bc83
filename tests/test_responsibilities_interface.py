"""The E-step operator and the EM driver without a GPU: the entry point in the header, the binding and the
library; where the kernel and the rules live; every refusal of the Python layer with a stub in the library's place; the Python
restatement of the layout against the header's; the float32 rule on hand-made inputs; and, from tests/_responsibilities_witness.py
alone, the conditions that keep tests/test_gpu_responsibilities.py honest - the generated cases' and the driver case's."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import _host_check as HC
import _responsibilities_witness as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'edge-informed-contrast-maximization_amd'
L = importlib.import_module(PKG + '._lib')
E = importlib.import_module(PKG + '.engine')
synth = importlib.import_module(PKG + '.synth')
motion = importlib.import_module(PKG + '.motion')
segmentation = importlib.import_module(PKG + '.segmentation')

NAME = 'eincm_event_responsibilities'
# the Python entry points: a tree without them has nothing that this module could test
responsibilities, layout, segment_motions = E.Engine.event_responsibilities, E.event_responsibilities_layout, segmentation.segment_motions


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_in_header_binding_and_library(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    m = re.search(r'int\s+' + NAME + r'\s*\(([^)]*)\)', hdr)
    assert m, 'not declared'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert args == ['eincm_ctx* ctx', 'int n_models', 'const float* images', 'const double* ref_weights', 'const float* const* weights_in',
                    'const double* prior', 'uint32_t flags', 'float* weights_out', 'uint8_t* labels', 'double* mass', 'int64_t* n_unsupported']
    defines = dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)u?\b', hdr))
    assert int(defines['EINCM_ABI_VERSION']) == 6
    assert int(defines['EINCM_RS_MAX_MODELS']) == L.RS_MAX_MODELS == RW.MAX_MODELS == 8
    assert int(defines['EINCM_RS_EXCLUDE_SELF']) == L.RS_EXCLUDE_SELF == 1
    assert NAME in hdr.split('#define EINCM_ABI_VERSION')[1].split('*/')[0], 'not in the name list after EINCM_ABI_VERSION'
    doc = hdr.split('int ' + NAME)[0].rsplit('/* The E-step', 1)[1]
    for words in ('the same bits', 'a NaN becomes +0', 'ascending l from +0', 'unsupported', 'correctly rounded', 'v_div_scale',
                  'no float atomics', 'in this order', 'writes nothing', 'lowest l'):
        assert words in doc, words
    assert [n for n, _, _ in L.SIGNATURES].count(NAME) == 1
    res, a = {n: (r, a) for n, r, a in L.SIGNATURES}[NAME]
    assert res is C.c_int and a == [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 4
    fn = getattr(built_lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == a
    assert built_lib.eincm_abi_version() == 6
    assert fn(None, 2, None, None, None, None, 0, None, None, None, None) == L.ERR_ARG      # no context: refused without a GPU


def test_kernel_lives_in_its_own_header_and_the_rules_in_a_hip_free_one():
    csrc = os.path.join(ROOT, PKG, 'csrc')
    rules = open(os.path.join(csrc, 'eincm_responsibilities.h')).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', rules)
    assert 'hip' not in ''.join(includes).lower() and 'eincm_event_scores.h' in includes
    for fn in ('rs_check', 'rs_code', 'rs_why', 'rs_weights_offset', 'rs_weights_total', 'rs_labels_offset', 'rs_labels_total', 'rs_group_events'):
        assert re.search(r'\b' + fn + r'\(', rules), fn
    kern = open(os.path.join(csrc, 'eincm_responsibilities.hip.h')).read()
    assert re.search(r'__global__[^;{]*\bk_responsibilities\(', kern) and re.search(r'__global__[^;{]*\bk_rs_mass\(', kern)
    assert 'v_div_scale' in kern                                              # the header says how the division must stay
    code = re.sub(r'//[^\n]*', '', kern)
    assert '#pragma clang fp contract(off)' in code and 'sc_event_ref(' in code and ' / T' in code
    assert 'atomicAdd(uns' in code and code.count('atomic') == 1              # the one atomic is the integer count
    for banned in ('__fdividef', '__frcp', 'rcp', 'fast'):
        assert banned not in code, banned
    scores = open(os.path.join(csrc, 'eincm_event_scores.hip.h')).read()
    assert re.search(r'__device__[^;{]*\bsc_event_ref\(', scores) and not re.search(r'__device__[^;{]*\bsc_event_ref\(', kern)
    assert re.sub(r'//[^\n]*', '', scores).count('sc_event_ref(') == 2         # defined once, used by k_event_scores
    api = open(os.path.join(csrc, 'eincm_api.hip')).read()
    body = api.split('int ' + NAME + '(')[1].split('\n}\n')[0]
    assert body.index('rs_check(') < body.index('ensure_theta_image(c)') < body.index('OneShot op(c);')
    assert body.count('op.sync()') == 1 and 'hipMalloc' not in body and 'op.launch(' in body
    assert 'rs_weights_total(' in body and 'rs_labels_total(' in body and 'rs_weights_offset(' in body
    assert 'd_w' not in re.sub(r'd_w(in|out)', '', body)                      # the staged weights are the caller's, never the context's


# ---- the Python layer with a stub in the library's place ------------------------------------------------------------------------------------
class NoGpu:
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


class Reached(Exception):
    pass


class Records:
    def __init__(self):
        self.calls = []

    def eincm_event_responsibilities(self, *a):
        self.calls.append(a)
        raise Reached()


def stub_engine(lib=None, B=4, R=3, H=5, W=7, n=(4, 4, 6, 6), weights='ones'):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, lib or NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = 'fp32', 3, B, R, H, W
    eng._io, eng.n_events = {}, np.array(n, dtype=np.int64)
    if weights == 'ones':
        eng._staged_weights = [None] * B
    elif weights is not None:
        eng._staged_weights = weights
    return eng


def test_a_good_call_reaches_the_library_with_its_arguments(built_lib):
    lib = Records()
    w = [None, np.full(4, 0.5, np.float32), None, None]
    for kw, eng in ((dict(), stub_engine(lib)), (dict(exclude_self=False, want='labels'), stub_engine(lib, weights=None)),
                    (dict(images=np.zeros((4, 3, 5, 7)), ref_weights=[1, 0, -1], prior=[1, 0, 0.5, 0.5], want=('mass', 'n_unsupported')),
                     stub_engine(lib, weights=w)), (dict(prior=np.ones(4), want=['weights']), stub_engine(lib))):
        with pytest.raises(Reached):
            eng.event_responsibilities(2, **kw)
        _, K, images, rw, w_in, prior, flags, w_out, labels, mass, n_uns = lib.calls[-1]
        want = kw.get('want', ('weights', 'labels', 'mass'))
        assert K == 2 and (images is None) == ('images' not in kw) and rw is not None and (prior is None) == ('prior' not in kw)
        assert flags == (L.RS_EXCLUDE_SELF if kw.get('exclude_self', True) else 0)
        assert (w_in is not None) == (getattr(eng, '_staged_weights', None) is w)
        assert [(o is not None) for o in (w_out, labels, mass, n_uns)] == [k in want for k in E.RS_OUTPUTS]


BAD = [('k-zero', (0,), {}, 'n_models'), ('k-nine', (9,), {}, 'n_models'), ('k-float', (2.0,), {}, 'n_models'), ('k-bool', (True,), {}, 'n_models'),
       ('k-does-not-divide', (3,), {}, 'whole number of groups'), ('unequal-in-a-group', (4,), {}, 'equal numbers of events'),
       ('want-empty', (2,), dict(want=()), 'want'), ('want-unknown', (2,), dict(want=('weights', 'scores')), 'want'),
       ('want-twice', (2,), dict(want=('mass', 'mass')), 'want'),
       ('prior-short', (2,), dict(prior=[1.0, 1.0]), r'prior must be \(4,\)'), ('prior-negative', (2,), dict(prior=[1, -0.5, 1, 1]), 'finite and >= 0'),
       ('prior-nan', (2,), dict(prior=[1, np.nan, 1, 1]), 'finite and >= 0'), ('prior-too-large-for-a-float', (2,), dict(prior=[1, 1e300, 1, 1]), 'finite and >= 0'),
       ('prior-group-of-zeros', (2,), dict(prior=[1, 1, 0, 0]), 'positive'), ('prior-underflows', (2,), dict(prior=[1, 1, 1e-300, 0]), 'positive'),
       ('prior-strings', (2,), dict(prior=['a', 'b', 'c', 'd']), 'prior must be'),
       ('images-shape', (2,), dict(images=np.zeros((2, 3, 5, 7))), 'images must be'), ('ref-weights-nan', (2,), dict(ref_weights=[1, np.nan, 1]), 'finite'),
       ('ref-weights-short', (2,), dict(ref_weights=[1, 1]), 'ref_weights must be')]


@pytest.mark.parametrize('name,args,kw,match', BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_value_errors_before_any_library_call(built_lib, name, args, kw, match):
    with pytest.raises(ValueError, match=match):
        stub_engine().event_responsibilities(*args, **kw)


def test_exclude_self_without_the_staged_weights_is_a_value_error(built_lib):
    for eng in (stub_engine(weights=None), stub_engine(weights=[None])):
        with pytest.raises(ValueError, match='does not hold them'):
            eng.event_responsibilities(2)


def test_signatures_of_the_python_layer():
    p = inspect.signature(E.Engine.event_responsibilities).parameters
    assert list(p) == ['self', 'n_models', 'images', 'ref_weights', 'prior', 'exclude_self', 'want']
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, True, ('weights', 'labels', 'mass')]
    p = inspect.signature(segment_motions).parameters
    assert list(p) == ['engine', 'windows', 'model', 'coeffs0', 'params', 'n_iters', 'maxiter', 'gtol', 'weights0', 'prior', 'min_mass', 'callback']
    assert (p['n_iters'].default, p['maxiter'].default, p['gtol'].default, p['weights0'].default, p['callback'].default) == (5, 25, 1e-6, None, None)
    assert p['prior'].default in segmentation.PRIORS and segmentation.PRIORS == ('mass', 'uniform')


def test_segment_motions_refuses_bad_arguments_before_it_touches_the_engine():
    model = motion.MotionModel('translation', (5, 7))
    win = (np.zeros(3, np.int16), np.zeros(3, np.int16), np.linspace(0, 1, 3), np.zeros((2, 5, 7)), np.array([0.0, 1.0]))
    good = np.array([[[1.0, 0.0], [0.0, 1.0]]])
    eng = NoGpu()
    for kw, match in ((dict(windows=[]), 'at least one'), (dict(windows=[win + (None,)]), '5|tuple'), (dict(coeffs0=good[0]), 'coeffs0 must be'),
                      (dict(coeffs0=np.zeros((1, 2, 3))), 'coeffs0 must be'), (dict(coeffs0=np.array([[[1.0, 2.0], [1.0, 2.0]]])), 'never separate'),
                      (dict(coeffs0=good * np.nan), 'finite'), (dict(n_iters=0), 'n_iters'), (dict(prior='flat'), 'prior'), (dict(min_mass=-1.0), 'min_mass'),
                      (dict(weights0=[[np.ones(3)]]), 'weights0'), (dict(weights0=[[np.ones(3), np.ones(2)]]), r'\(3,\)')):
        a = dict(windows=[win], coeffs0=good)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            segment_motions(eng, a.pop('windows'), model, a.pop('coeffs0'), None, **a)


# ---- the layout: the Python restatement against the header's ---------------------------------------------------------------------------
LAYOUTS = [(1, []), (3, []), (1, [7]), (2, [7, 7]), (3, [5, 5, 5, 0, 0, 0, 9, 9, 9]), (2, [0, 0, 0, 0]), (8, [3] * 16), (1, [1, 40, 0, 1000000, 1]),
           (2, [1500000000, 1500000000, 1, 1])]


def test_layout_in_python_is_the_header_s(tmp_path_factory):
    exe = HC.build(tmp_path_factory, 'responsibilities_check')
    cases = {}
    for i, (K, ne) in enumerate(LAYOUTS):
        HC.add_case(cases, i, 'layout', K, len(ne), *ne)
    out = HC.run(exe, cases, tmp_path_factory, 'responsibilities_layouts')
    for i, (totals, w_off, lab_off, lab_len) in out.items():
        K, ne = LAYOUTS[i]
        o, tot, lo, ll, ltot = layout(ne, K)
        assert (tot, ltot) == tuple(int(t) for t in totals) and o.dtype == lo.dtype == ll.dtype == np.int64
        assert np.array_equal(o, HC.i(w_off)) and np.array_equal(lo, HC.i(lab_off)) and np.array_equal(ll, HC.i(lab_len))
        assert len(o) == len(ne) and len(lo) == len(ne) // K


# ---- the float32 rule on hand-made inputs -------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_made_inputs():
    f = np.float32
    s = f([[3.0, 0.0, -1.0, np.nan, 2.0, np.inf], [1.0, 0.0, 4.0, 1.0, 2.0, 1.0]])
    q = f([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    r = RW.responsibilities_f32(s, q, None, None, False)
    assert np.array_equal(r['weights'], f([[0.75, 0.5, 0.0, 0.0, 0.5, 0.5], [0.25, 0.5, 1.0, 1.0, 0.5, 0.5]]))
    assert list(r['unsupported']) == [False, True, False, False, False, True] and list(r['labels']) == [0, 0, 1, 1, 0, 0]
    r = RW.responsibilities_f32(s, q, f([[1.0] * 6, [0.0] * 6]), [1.0, 3.0], True)           # a = (2, 0, 0, 0, 1, inf), (1, 0, 4, 1, 2, 1)
    assert np.array_equal(r['weights'], f([[0.4, 0.25, 0.0, 0.0, 0.14285715, 0.25], [0.6, 0.75, 1.0, 1.0, 0.85714287, 0.75]]))
    assert list(r['labels']) == [1, 1, 1, 1, 1, 1] and list(r['unsupported']) == [False, True, False, False, False, True]
    one = RW.responsibilities_f32(s[:1], q[:1], None, [0.3], True)                               # K = 1: all ones, whatever the score
    assert np.array_equal(one['weights'], np.ones((1, 6), f))
    m = RW.ordered_mass(np.random.default_rng(0).uniform(0, 1, (3, 700)).astype(f))
    assert np.allclose(m, np.random.default_rng(0).uniform(0, 1, (3, 700)).astype(f).astype(np.float64).sum(axis=1), rtol=1e-13, atol=0)


# ---- what keeps the GPU module honest -------------------------------------------------------------------------------------------------------
def _all(groups, key):
    return np.concatenate([g[key] for g in groups if g is not None], axis=-1)


@pytest.mark.parametrize('name', sorted(RW.GENERATED))
def test_every_generated_case_meets_the_conditions(name):
    c = RW.generated(name)
    K = c['K']
    assert all(len(w['xs']) == c['ns'][b // K] for b, w in enumerate(c['windows'])) and c['theta'].shape[0] == c['G'] * K
    assert np.all(c['theta'][-1] == RW.FAR) and np.abs(c['theta'][:-1]).max() <= 9.0 and (c['stack'] < 0).any() and (c['stack'] > 0).any()
    for exclude_self in (True, False):
        for use_prior in (True, False):
            st = RW.witness_case(name, 'stack', exclude_self, use_prior)
            frac = _all(st, 'unsupported').mean()
            assert 0.05 <= frac <= 0.50, (exclude_self, use_prior, frac)
            far = st[-1]                                                          # the far model scores exactly 0: it gets no share
            assert not far['a'][-1].any() and np.all(far['weights'][-1][~far['unsupported']] == 0)
    if K > 1:
        # with IWEs as the source most events have two models with a positive share (plain scores; leave-one-out where the case is dense)
        for exclude_self in ((False, True) if sum(c['ns']) >= 256 else (False,)):
            iw = RW.witness_case(name, 'iwe', exclude_self, True)
            two = ((_all(iw, 'weights') > 0) & ~_all(iw, 'unsupported')[None]).sum(axis=0) >= 2
            assert two.mean() >= 0.5, (exclude_self, two.mean())
        for source in ('iwe', 'stack'):
            a, b = (_all(RW.witness_case(name, source, ex, True), 'weights') for ex in (True, False))
            changed = (np.abs(a - b) > 1e-5).mean()
            if source == 'iwe':
                assert changed >= 0.5, changed


def test_generated_cases_cover_the_shapes_and_counts():
    specs = list(RW.GENERATED.values())
    assert {s[0] for s in specs} == {(33, 65), (60, 80)} and {s[1] for s in specs} == {None, (3, 5)}
    assert {n for s in specs for n in s[4]} >= {1, 63, 64, 65, 255, 256, 257, 700, 0}
    assert {s[3] for s in specs} == {1, 2, 3, 8} and {len(s[4]) for s in specs} == {1, 2, 3} and any(s[4][1:2] == [0] and len(s[4]) == 3 for s in specs)
    kern = open(os.path.join(ROOT, PKG, 'csrc', 'eincm_types.h')).read()
    assert int(re.search(r'constexpr int NT = (\d+);', kern).group(1)) == RW.NT


def test_the_driver_case_segments_under_the_witness_em(built_lib):
    """The input condition of the GPU driver test: the numpy EM reaches label accuracy >= 0.85 and velocities within 1 px on the
    two-layer scene.  The witness's accuracy per iteration is printed."""
    case = RW.driver_case(synth)
    d = RW.DRIVER
    assert len(case['truth']) == 2 * d['n_layer'] and np.all(np.diff(case['window'][2]) >= 0)
    assert np.allclose(case['coeffs0'][0], [[7.2, 1.8], [-8.4, -12.6]])
    out = RW.em_witness(case, E.multi_ref_weights(d['R']), d['n_iters'], prior='uniform')
    acc = [RW.accuracy(o['labels'], case['truth']) for o in out]
    err = np.abs(out[-1]['coeffs'] - case['flows']).max()
    print(f'witness EM: accuracy per iteration {[round(a, 4) for a in acc]}, final velocities {out[-1]["coeffs"].round(3).tolist()}, '
          f'largest velocity error {err:.3f} px')
    assert acc[-1] >= 0.85 and err <= 1.0
    assert abs(acc[-1] - RW.DRIVER_WITNESS_ACCURACY) <= 5e-4, 'the recorded accuracy is not the one the witness reaches'
    assert all(abs(o['mass'].sum() - len(case['truth'])) <= 1e-3 for o in out)
