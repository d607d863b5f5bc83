"""The per-pixel label prior and the E-step with a prior image where no GPU is needed: the three entry points in
the header, the binding table and the built library, prototype by prototype; the new Python signatures and their defaults, and the
pinned ones unchanged beside them; every refusal of the check_* functions; the Python layer with a stub in the library's place; the
EM driver's refusals before it touches the engine and the calls it makes of a scripted engine; and the witness on hand-made pixels."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import _label_prior_witness as WIT
import _responsibilities_witness as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'edge-informed-contrast-maximization_amd'
L = importlib.import_module(PKG + '._lib')
E = importlib.import_module(PKG + '.engine')
motion = importlib.import_module(PKG + '.motion')
segmentation = importlib.import_module(PKG + '.segmentation')
batch_solver = importlib.import_module(PKG + '.batch_solver')

# the Python entry points: a tree without them has nothing that this module could test
label_prior, staged_prior = E.Engine.label_prior, E.Engine.staged_prior
spatial, apply_spatial = E.Engine.event_responsibilities_spatial, E.Engine.apply_responsibilities_spatial
segment_motions_spatial = segmentation.segment_motions_spatial

C_TYPES = {'eincm_ctx*': C.c_void_p, 'int': C.c_int, 'unsigned': C.c_uint, 'uint32_t': C.c_uint32}      # any other pointer: a raw address
PROTOTYPES = {
    'eincm_label_prior': ['eincm_ctx* ctx', 'int n_models', 'int radius', 'uint32_t floor_mass', 'unsigned flags', 'float* prior',
                          'uint64_t* smoothed'],
    'eincm_get_staged_prior': ['eincm_ctx* ctx', 'float* prior'],
    'eincm_event_responsibilities_spatial': ['eincm_ctx* ctx', 'int n_models', 'const float* images', 'const double* ref_weights',
                                             'const float* const* weights_in', 'const double* prior', 'const float* prior_images',
                                             'uint32_t flags', 'float* weights_out', 'uint8_t* labels', 'double* mass', 'int64_t* n_unsupported'],
}


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(PROTOTYPES))
def test_entry_point_in_header_binding_and_library(built_lib, name):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
    assert m, 'not declared'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert args == PROTOTYPES[name]
    assert name in hdr.split('#define EINCM_ABI_VERSION')[1].split('*/')[0], 'not in the name list after EINCM_ABI_VERSION'
    assert [n for n, _, _ in L.SIGNATURES].count(name) == 1
    res, a = {n: (r, a) for n, r, a in L.SIGNATURES}[name]
    want = [C_TYPES.get(' '.join(arg.split()[:-1]), C.c_void_p) for arg in args]
    assert res is C.c_int and a == want
    fn = getattr(built_lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == a
    assert fn(*([None] + [0 if t in (C.c_int, C.c_uint, C.c_uint32) else None for t in a[1:]])) == L.ERR_ARG      # no context: refused without a GPU


def test_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    defines = dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)u?\b', hdr))
    assert int(defines['EINCM_ABI_VERSION']) == 6
    assert int(defines['EINCM_LP_MAX_RADIUS']) == L.LP_MAX_RADIUS == WIT.MAX_RADIUS == 8
    assert int(defines['EINCM_RS_PRIOR_STAGED']) == L.RS_PRIOR_STAGED == 8
    flags = [L.RS_EXCLUDE_SELF, L.RS_STAGED_WEIGHTS, L.RS_APPLY, L.RS_PRIOR_STAGED]
    assert sorted(flags) == [1, 2, 4, 8]                                           # one bit each
    doc = hdr.split('int eincm_label_prior')[0].rsplit('/* The per-pixel label prior', 1)[1]
    for words in ('as uint64', 'T == 0 ? 1.0f', 'T < 2^53', 'STAGED PRIOR', 'dropped by the next eincm_set_windows', 'the same bytes', 'in the order'):
        assert words in doc, words
    doc = hdr.split('int eincm_event_responsibilities_spatial')[0].rsplit('/* The E-step with a prior image', 1)[1]
    for words in ('c_l  = (float)prior[b] * P[b, y_e, x_e]', 'unsupported once', 'without contraction', 'the bytes of eincm_event_responsibilities',
                  'names window and pixel'):
        assert words in doc, words


def test_kernels_live_in_their_own_header_and_the_rules_in_a_hip_free_one():
    csrc = os.path.join(ROOT, PKG, 'csrc')
    rules = open(os.path.join(csrc, 'eincm_label_prior.h')).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', rules)
    assert 'hip' not in ''.join(includes).lower() and 'eincm_motion_layers.h' in includes
    for fn in ('lp_check', 'lp_code', 'lp_why', 'lp_prior_offset', 'lp_smoothed_offset', 'lp_prior'):
        assert re.search(r'\b' + fn + r'\(', rules), fn
    kern = open(os.path.join(csrc, 'eincm_label_prior.hip.h')).read()
    code = re.sub(r'//[^\n]*', '', kern)
    assert re.search(r'__global__[^;{]*\bk_label_prior\(', kern) and 'lp_prior(' in code and 'atomic' not in code
    assert 'k_ml_mass' not in code                                                 # the mass images are eincm_motion_layers.hip.h's, not restated
    api = open(os.path.join(csrc, 'eincm_api.hip')).read()
    body = api.split('int eincm_label_prior(')[1].split('\n}\n')[0]
    assert body.index('lp_check(') < body.index('OneShot op(c);') < body.index('k_ml_mass') < body.index('lp_kernel(')
    assert body.count('op.sync()') == 1 and 'hipMalloc' not in body
    body = api.split('int eincm_event_responsibilities_spatial(')[1].split('\n}\n')[0]
    assert body.index('rs_check(') < body.index('rs_spatial_check(') < body.index('ensure_theta_image(c)') < body.index('OneShot op(c);')
    resp = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, 'eincm_responsibilities.hip.h')).read())
    assert 'template <int K, int SP = 0' in resp and resp.count('__global__') == 2  # one kernel with a second template parameter, and k_rs_mass


# ---- the signatures: the new ones, and the pinned ones beside them unchanged ----------------------------------------------------------------
def test_signatures_of_the_python_layer():
    p = inspect.signature(label_prior).parameters
    assert list(p) == ['self', 'n_models', 'radius', 'floor_mass', 'want'] and (p['floor_mass'].default, p['want'].default) == (4096, ('prior',))
    assert list(inspect.signature(staged_prior).parameters) == ['self']
    p = inspect.signature(spatial).parameters
    assert list(p) == ['self', 'n_models', 'prior_images', 'images', 'ref_weights', 'prior', 'exclude_self', 'want']
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, None, True, ('weights', 'labels', 'mass')]
    q = inspect.signature(apply_spatial).parameters
    assert list(q) == list(p) and [q[k].default for k in list(q)[2:]] == [None, None, None, None, True, ('labels', 'mass')]
    p = inspect.signature(segment_motions_spatial).parameters
    assert list(p) == ['engine', 'windows', 'model', 'coeffs0', 'params', 'radius', 'floor_mass', 'n_iters', 'maxiter', 'gtol', 'weights0', 'prior',
                       'min_mass', 'callback', 'in_place', 'record_weights']
    assert [p[k].default for k in list(p)[5:]] == [2, 4096, 5, 25, 1e-6, None, 'mass', 1.0, None, True, True]
    assert E.LP_OUTPUTS == ('prior', 'smoothed')


def test_the_pinned_signatures_are_unchanged():
    p = inspect.signature(E.Engine.event_responsibilities).parameters
    assert list(p) == ['self', 'n_models', 'images', 'ref_weights', 'prior', 'exclude_self', 'want']
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, True, ('weights', 'labels', 'mass')]
    p = inspect.signature(E.Engine.apply_responsibilities).parameters
    assert list(p) == ['self', 'n_models', 'images', 'ref_weights', 'prior', 'exclude_self', 'want']
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, True, ('labels', 'mass')]
    p = inspect.signature(segmentation.segment_motions).parameters
    assert list(p) == ['engine', 'windows', 'model', 'coeffs0', 'params', 'n_iters', 'maxiter', 'gtol', 'weights0', 'prior', 'min_mass', 'callback']
    assert (p['n_iters'].default, p['maxiter'].default, p['gtol'].default, p['weights0'].default, p['callback'].default) == (5, 25, 1e-6, None, None)
    assert segmentation.PRIORS == ('mass', 'uniform')


# ---- the check_* functions ---------------------------------------------------------------------------------------------------------------------
def test_good_label_prior_arguments_come_back_normalised():
    assert E.check_label_prior_args(np.int64(3), np.int32(0), np.uint32(7), 'smoothed') == (3, 0, 7, ('smoothed',))
    assert E.check_label_prior_args(8, 8, 0xFFFFFFFF, ()) == (8, 8, 0xFFFFFFFF, ())
    assert E.check_label_prior_args(1, 2, 0, ['smoothed', 'prior'])[3] == ('smoothed', 'prior')
    lay = E.label_prior_layout(2, 3, (40, 72))
    assert lay['prior'][0] == (6, 40, 72) and lay['smoothed'][0] == (2, 3, 40, 72) and lay['prior'][2].tolist() == [0, 3 * 40 * 72]


BAD_LP = [(dict(n_models=0), 'n_models'), (dict(n_models=9), 'n_models'), (dict(n_models=2.0), 'n_models'), (dict(n_models=True), 'n_models'),
          (dict(radius=-1), 'radius'), (dict(radius=9), 'radius'), (dict(radius=1.0), 'radius'), (dict(radius=False), 'radius'),
          (dict(floor_mass=-1), 'floor_mass'), (dict(floor_mass=1 << 32), 'floor_mass'), (dict(floor_mass=4096.0), 'floor_mass'),
          (dict(want=('mass',)), 'want'), (dict(want=('prior', 'prior')), 'want'), (dict(want='labels'), 'want')]


@pytest.mark.parametrize('kw,match', BAD_LP, ids=[f'{list(k)[0]}-{i}' for i, (k, _) in enumerate(BAD_LP)])
def test_bad_label_prior_arguments(kw, match):
    a = dict(n_models=2, radius=2, floor_mass=4096, want=('prior',))
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        E.check_label_prior_args(**a)


def test_prior_images_come_back_as_float32_or_are_refused():
    assert E.check_prior_images(None, 4, (5, 7)) is None
    a = E.check_prior_images(np.arange(4 * 5 * 7).reshape(4, 5, 7), 4, (5, 7))
    assert a.dtype == np.float32 and a.flags['C_CONTIGUOUS'] and a.shape == (4, 5, 7)
    assert E.check_prior_images(np.ones((5, 7)), 1, (5, 7)).shape == (1, 5, 7)
    assert E.check_prior_images(np.ones((2, 7, 5)).transpose(0, 2, 1), 2, (5, 7)).flags['C_CONTIGUOUS']
    bad = np.ones((4, 5, 7))
    for shape_bad in (np.ones((3, 5, 7)), np.ones((5, 7)), np.ones((4, 7, 5)), np.ones((4, 1, 5, 7))):
        with pytest.raises(ValueError, match='prior_images must be'):
            E.check_prior_images(shape_bad, 4, (5, 7))
    with pytest.raises(ValueError, match='numbers'):
        E.check_prior_images(np.full((4, 5, 7), 'a'), 4, (5, 7))
    for value in (np.nan, np.inf, -1e-30, 1e39):                                  # (1e39 is not finite as the float the kernel takes)
        bad = np.ones((4, 5, 7))
        bad[2, 3, 6] = value
        with pytest.raises(ValueError, match=r'window 2, pixel \(x 6, y 3\)'):
            E.check_prior_images(bad, 4, (5, 7))


# ---- the Python layer with a stub in the library's place ------------------------------------------------------------------------------------
class NoGpu:
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


class Reached(Exception):
    pass


class Records:
    def __init__(self):
        self.calls = []

    def eincm_event_responsibilities_spatial(self, *a):
        self.calls.append(('spatial',) + a)
        raise Reached()

    def eincm_label_prior(self, *a):
        self.calls.append(('label_prior',) + a)
        raise Reached()


def stub_engine(lib=None, B=4, R=3, H=5, W=7, n=(4, 4, 6, 6), keep_order=False):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, lib or NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = 'fp32', 3, B, R, H, W
    eng._io, eng.n_events = {}, np.array(n, dtype=np.int64)
    eng._staged_weights, eng._keep_order = [None] * B, keep_order
    return eng


def test_good_calls_reach_the_library_with_their_arguments():
    lib = Records()
    with pytest.raises(Reached):
        stub_engine(lib).label_prior(2, 3, floor_mass=5, want='smoothed')
    _, _, K, r, floor, flags, prior, smoothed = lib.calls[-1]
    assert (K, r, floor, flags) == (2, 3, 5, 0) and prior is None and smoothed is not None
    with pytest.raises(Reached):
        stub_engine(lib).label_prior(2, 0, want=())
    assert lib.calls[-1][2:] == (2, 0, 4096, 0, None, None)
    for kw, keep, method in ((dict(), False, 'event_responsibilities_spatial'), (dict(prior_images=np.ones((4, 5, 7))), False, 'event_responsibilities_spatial'),
                             (dict(exclude_self=False, want='labels'), False, 'event_responsibilities_spatial'),
                             (dict(want=()), True, 'apply_responsibilities_spatial'),
                             (dict(prior_images=np.ones((4, 5, 7)), prior=[1, 0, 0.5, 0.5]), True, 'apply_responsibilities_spatial')):
        eng = stub_engine(lib, keep_order=keep)
        with pytest.raises(Reached):
            getattr(eng, method)(2, **kw)
        _, _, K, images, rw, w_in, prior, pimg, flags, w_out, labels, mass, n_uns = lib.calls[-1]
        apply = method.startswith('apply')
        want = kw.get('want', ('labels', 'mass') if apply else ('weights', 'labels', 'mass'))
        assert K == 2 and images is None and rw is not None and (prior is None) == ('prior' not in kw)
        assert (pimg is None) == ('prior_images' not in kw)
        expect = (L.RS_EXCLUDE_SELF if kw.get('exclude_self', True) else 0) | (L.RS_APPLY if apply else 0) | (0 if 'prior_images' in kw else L.RS_PRIOR_STAGED)
        if keep and kw.get('exclude_self', True):
            expect |= L.RS_STAGED_WEIGHTS
        assert flags == expect
        assert [(o is not None) for o in (w_out, labels, mass, n_uns)] == [k in want for k in E.RS_OUTPUTS]


BAD = [('label_prior', (0, 2), {}, 'n_models'), ('label_prior', (2, 9), {}, 'radius'), ('label_prior', (2, 2), dict(floor_mass=-3), 'floor_mass'),
       ('label_prior', (2, 2), dict(want=('theta',)), 'want'),
       ('event_responsibilities_spatial', (9,), {}, 'n_models'), ('event_responsibilities_spatial', (3,), {}, 'whole number of groups'),
       ('event_responsibilities_spatial', (4,), {}, 'equal numbers of events'), ('event_responsibilities_spatial', (2,), dict(want=()), 'want'),
       ('event_responsibilities_spatial', (2,), dict(prior=[1, 1, 0, 0]), 'positive'),
       ('event_responsibilities_spatial', (2,), dict(prior_images=np.ones((2, 5, 7))), 'prior_images must be'),
       ('event_responsibilities_spatial', (2,), dict(prior_images=-np.ones((4, 5, 7))), 'finite and >= 0'),
       ('event_responsibilities_spatial', (2,), dict(images=np.zeros((2, 3, 5, 7))), 'images must be'),
       ('event_responsibilities_spatial', (2,), dict(ref_weights=[1, np.nan, 1]), 'finite'),
       ('apply_responsibilities_spatial', (2,), {}, 'keep_order=True')]


@pytest.mark.parametrize('method,args,kw,match', BAD, ids=[f'{b[0]}-{i}' for i, b in enumerate(BAD)])
def test_bad_arguments_are_value_errors_before_any_library_call(method, args, kw, match):
    with pytest.raises(ValueError, match=match):
        getattr(stub_engine(), method)(*args, **kw)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------
MODEL = motion.MotionModel('translation', (5, 7))
WIN = (np.zeros(3, np.int16), np.zeros(3, np.int16), np.linspace(0, 1, 3), np.zeros((2, 5, 7)), np.array([0.0, 1.0]))
GOOD = np.array([[[1.0, 0.0], [0.0, 1.0]]])


def test_the_driver_refuses_bad_arguments_before_it_touches_the_engine():
    eng = NoGpu()
    for kw, match in ((dict(windows=[]), 'at least one'), (dict(coeffs0=np.array([[[1.0, 2.0], [1.0, 2.0]]])), 'never separate'), (dict(n_iters=0), 'n_iters'),
                      (dict(prior='flat'), 'prior'), (dict(weights0=[[np.ones(3), np.ones(2)]]), r'\(3,\)'), (dict(record_weights=0), 'True or False'),
                      (dict(in_place=False, record_weights=False), 'record_weights=False goes with in_place=True'),
                      (dict(radius=9), 'radius'), (dict(radius=-1), 'radius'), (dict(radius=1.5), 'radius'), (dict(floor_mass=-1), 'floor_mass'),
                      (dict(floor_mass=2.0 ** 32), 'floor_mass'), (dict(coeffs0=np.arange(18.0).reshape(1, 9, 2)), 'n_models')):
        a = dict(windows=[WIN], coeffs0=GOOD)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            segment_motions_spatial(eng, a.pop('windows'), MODEL, a.pop('coeffs0'), None, **a)


class _Script:
    """An engine that records what the EM driver asks of it and answers with fixed responsibilities."""
    def __init__(self, n, K):
        self.calls, self.n, self.K = [], n, K

    def set_motion_model(self, model): pass
    def set_motion_path(self, path): pass

    def set_windows(self, windows, keep_order=False):
        self.calls.append(('set_windows', keep_order))

    def set_weights(self, weights):
        self.calls.append(('set_weights',))

    def label_prior(self, K, radius, floor_mass=4096, want=('prior',)):
        self.calls.append(('label_prior', K, radius, floor_mass, tuple(want)))
        return {}

    def loss_grad_motion(self, coeffs, params, **kw):
        self.calls.append(('loss_grad_motion',))

    def _answer(self, want):
        w = [np.full(self.n, (l + 1) / 4.0, np.float32) for l in range(self.K)]
        full = dict(weights=w, labels=[np.zeros(self.n, np.uint8)], mass=np.array([[3.0, 2.0]]), n_unsupported=np.zeros(1, np.int64))
        self.device_weights = w
        return {k: full[k] for k in want}

    def event_responsibilities_spatial(self, K, prior_images=None, prior=None, exclude_self=True, want=()):
        self.calls.append(('event_responsibilities_spatial', prior_images, tuple(want)))
        return self._answer(want)

    def apply_responsibilities_spatial(self, K, prior_images=None, prior=None, exclude_self=True, want=()):
        self.calls.append(('apply_responsibilities_spatial', prior_images, tuple(want)))
        return self._answer(want)

    def staged_weights(self):
        self.calls.append(('staged_weights',))
        return self.device_weights


@pytest.mark.parametrize('in_place', [True, False])
def test_the_driver_forms_the_prior_after_every_stage_and_before_every_e_step(monkeypatch, in_place):
    monkeypatch.setattr(batch_solver, 'minimize_motion', lambda eng, model, c, *a, **kw: [None] * len(c))
    eng = _Script(3, 2)
    hist = segment_motions_spatial(eng, [WIN], MODEL, GOOD, None, radius=3, floor_mass=17, n_iters=2, in_place=in_place)
    names = [c[0] for c in eng.calls]
    e_step = 'apply_responsibilities_spatial' if in_place else 'event_responsibilities_spatial'
    assert len(hist) == 2 and names.count(e_step) == 3 and names.count('label_prior') == 3
    assert names.count('set_windows') == (1 if in_place else 3) and 'event_responsibilities' not in names and 'apply_responsibilities' not in names
    assert all(c[1:] == (2, 3, 17, ()) for c in eng.calls if c[0] == 'label_prior')          # staged only: nothing is downloaded
    assert all(c[1] is None for c in eng.calls if c[0] == e_step)                            # the staged prior, not a host stack
    # between two E-steps there is exactly one label_prior, and it comes before the M-step's evaluation of the same iteration
    marks = [n for n in names if n in ('label_prior', e_step)]
    assert marks == ['label_prior', e_step] * 3
    for i, n in enumerate(names):
        if n == e_step:
            assert 'label_prior' in names[:i] and names[i - 1] == 'loss_grad_motion'
    assert all(np.array_equal(r['mass'], [[3.0, 2.0]]) for r in hist)


# ---- the witness on hand-made pixels ----------------------------------------------------------------------------------------------------------
def test_witness_on_hand_made_pixels():
    xs, ys = np.array([0, 0, 4, 6]), np.array([0, 0, 2, 4])
    ws = [np.array([1.0, 0.5, 0.25, 0.0], np.float32), None]
    r = WIT.label_prior([(xs, ys, ws)], (5, 7), 1, 0)
    assert r['mass'][0, 0, 0, 0] == 6144 and r['mass'][0, 1, 0, 0] == 8192 and r['mass'][0, 0, 4, 6] == 0 and r['mass'][0, 1, 4, 6] == 4096
    assert r['smoothed'][0, :, 1, 1].tolist() == [6144, 8192] and r['smoothed'][0, :, 1, 2].tolist() == [0, 0]
    assert r['smoothed'][0, :, 3, 5].tolist() == [1024, 8192] and r['smoothed'][0, :, 2, 4].tolist() == [1024, 4096]
    assert r['prior'].shape == (2, 5, 7) and r['prior'].dtype == np.float32
    assert r['prior'][:, 1, 1].tolist() == [np.float32(6144 / 14336), np.float32(8192 / 14336)] and r['prior'][:, 1, 2].tolist() == [1.0, 1.0]
    assert r['prior'][:, 4, 6].tolist() == [0.0, 1.0]
    f = WIT.label_prior([(xs, ys, ws)], (5, 7), 1, 4096)['prior']
    assert f[:, 1, 2].tolist() == [0.5, 0.5] and f[:, 4, 6].tolist() == [np.float32(4096 / 12288), np.float32(8192 / 12288)]


def test_the_spatial_rule_on_hand_made_inputs():
    f = np.float32
    s = f([[3.0, 0.0, 2.0, 0.0, 5.0], [1.0, 0.0, 2.0, 0.0, 5.0]])
    q = np.zeros((2, 5), f)
    P = f([[0.5, 0.25, 0.5, 0.0, 0.0], [0.5, 0.75, 0.5, 0.0, 1.0]])
    r = WIT.responsibilities_spatial_f32(s, q, None, [1.0, 3.0], P, False)
    # p = (1.5, 0, 1, 0, 0), (1.5, 0, 3, 0, 15); event 1 falls back on c = (0.25, 2.25), event 3 on pi = (1, 3)
    assert np.array_equal(r['weights'], f([[0.5, 0.1, 0.25, 0.25, 0.0], [0.5, 0.9, 0.75, 0.75, 1.0]]))
    assert list(r['labels']) == [0, 1, 1, 1, 1] and list(r['unsupported']) == [False, True, False, True, False] and list(r['fallback']) == [0, 1, 0, 2, 0]
    ones = WIT.responsibilities_spatial_f32(s, q, None, [1.0, 3.0], np.ones((2, 5), f), False)
    plain = RW.responsibilities_f32(s, q, None, [1.0, 3.0], False)
    assert ones['weights'].tobytes() == plain['weights'].tobytes() and np.array_equal(ones['labels'], plain['labels'])
    assert np.array_equal(ones['unsupported'], plain['unsupported'])
    assert WIT.prior_at_events(np.arange(70.0).reshape(2, 5, 7), [([6, 0], [0, 4])] * 2).tolist() == [[6.0, 28.0], [41.0, 63.0]]
