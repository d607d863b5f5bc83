"""The fused motion-model evaluation at its interfaces, without a GPU: the header declares
eincm_loss_grad_motion_fused, the library exports it and _lib binds it with the signature of eincm_loss_grad_motion, the ABI version
stays 6; the evaluation path (Engine.set_motion_path, losses.motion_loss_funcs) is validated and every refusal Python can see is raised
before any GPU call, while the signatures of section 20's callables stay as tests/test_motion_interface.py pins them; the Python side of the support
predicate agrees, row by row, with the reasons csrc/eincm_motion.h gives (tests/test_host_motion_fused.py runs that one)."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

pkg = 'edge-informed-contrast-maximization_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
motion = importlib.import_module(pkg + '.motion')
losses = importlib.import_module(pkg + '.losses')
bs = importlib.import_module(pkg + '.batch_solver')

NAME = 'eincm_loss_grad_motion_fused'


# ---- the C-ABI ----
def test_header_exports_and_binding_table_agree(built_lib):
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    proto = lambda n: re.sub(r'\s+', ' ', re.search(r'\bint ' + n + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S).group(1))
    # the same arguments as eincm_loss_grad_motion, declared once
    assert proto(NAME) == proto('eincm_loss_grad_motion') and len(re.findall(r'\b' + NAME + r'\s*\(', code)) == 1
    table = {n: (res, args) for n, res, args in L.SIGNATURES}
    assert [n for n, _, _ in L.SIGNATURES].count(NAME) == 1
    assert table[NAME] == table['eincm_loss_grad_motion'] and len(table[NAME][1]) == len(proto(NAME).split(',')) == 7
    fn = getattr(built_lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    # the ABI version stays, and its comment names the entry point among those added without a new version
    assert built_lib.eincm_abi_version() == 6 and re.search(r'#define EINCM_ABI_VERSION 6\b', txt)
    assert NAME in txt[txt.index('#define EINCM_ABI_VERSION'):txt.index('#define EINCM_OK')]
    assert fn(None, None, None, None, None, None, None) == L.ERR_ARG          # a null context is refused before anything is read


# ---- the path ----
def test_path_is_a_setting_and_the_default_is_expanded():
    assert E.MOTION_PATHS == ('expanded', 'fused', 'auto')
    assert list(inspect.signature(E.Engine.set_motion_path).parameters) == ['self', 'path']
    assert inspect.signature(losses.motion_loss_funcs).parameters['path'].default == 'expanded'
    # section 20's callables keep their signatures: the path is no keyword of theirs
    for fn in (E.Engine.loss_grad_motion, bs.minimize_motion, losses.motion_loss_func, losses.value_and_grad_motion_loss_func):
        assert 'path' not in inspect.signature(fn).parameters, fn.__name__
    eng = stub_engine()
    assert eng.motion_path == 'expanded'
    for ok in E.MOTION_PATHS:
        assert E.check_motion_path(ok) == ok
        eng.set_motion_path(ok)
        assert eng.motion_path == ok
        f, vg = losses.motion_loss_funcs(ok)
        assert callable(f) and callable(vg)
    for bad in ('Fused', 'dense', '', None, 1, b'fused'):
        with pytest.raises(ValueError, match="one of 'expanded', 'fused', 'auto'"):
            E.check_motion_path(bad)
        with pytest.raises(ValueError, match="one of 'expanded', 'fused', 'auto'"):
            eng.set_motion_path(bad)
        with pytest.raises(ValueError, match="one of 'expanded', 'fused', 'auto'"):
            losses.motion_loss_funcs(bad)
    assert eng.motion_path == 'auto'                              # a refused value leaves the setting


class NoGpu:
    """Stands where the library is: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a GPU call')


def stub_engine(precision='fp32', splat_window=3, model=None, B=2, path='expanded'):
    eng = E.Engine.__new__(E.Engine)
    eng.motion_path = path
    eng._ctx, eng._lib = None, NoGpu()
    eng.precision, eng.splat_window, eng.motion_model, eng.B, eng.R = precision, splat_window, model, B, 3
    eng.H, eng.W = (model.sensor_size if model is not None else (20, 26))
    eng.n_events = np.array([100] * B)
    return eng


def params(gamma=0.0, lvl=1, full_aux=False, rk='mse'):
    return E.make_params(20.0, 35.0, gamma, 0.0, lvl, 'bilinear', full_aux=full_aux, correlation_kind=rk)


#            name -> (engine keywords, params keywords, a word of the reason or None)
REFUSALS = {
    'ok': ({}, {}, None),
    'ok-gamma-above-level-0': ({}, dict(gamma=2.5e-3, lvl=1), None),
    'ok-level-0-without-tv': ({}, dict(lvl=0), None),
    'ok-another-correlation-kind': ({}, dict(rk=2), None),
    'fp64': (dict(precision='fp64'), {}, 'fp64'),
    'splat-5': (dict(splat_window=5), {}, '3x3 splat window'),
    'full-aux': ({}, dict(full_aux=True), 'full_aux'),
    'tv-level-0': ({}, dict(gamma=2.5e-3, lvl=0), 'TV term'),
    'fp64-first': (dict(precision='fp64', splat_window=5), dict(full_aux=True), 'fp64'),
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_python_side_of_the_predicate(name):
    ekw, pkw, word = REFUSALS[name]
    why = E.motion_fused_refusal(ekw.get('precision', 'fp32'), ekw.get('splat_window', 3), params(**pkw))
    assert (why is None) if word is None else (word in why), (name, why)


def test_refusals_come_before_any_gpu_call():
    model = motion.MotionModel('affine', (20, 26))
    c = np.zeros((2, 6))
    # the coefficients are checked first, then the fused path's refusals - all without the library
    for path in E.MOTION_PATHS:
        with pytest.raises(ValueError, match='no motion model'):
            stub_engine(model=None, path=path).loss_grad_motion(c, params())
        with pytest.raises(ValueError, match=r'\(2,6\)'):
            stub_engine(model=model, path=path).loss_grad_motion(np.zeros((3, 6)), params())
    for name, (ekw, pkw, word) in REFUSALS.items():
        if word is None:
            continue
        with pytest.raises(ValueError, match=word):
            stub_engine(model=model, path='fused', **ekw).loss_grad_motion(c, params(**pkw))
        # 'auto' and 'expanded' do not refuse: they go on to the library (here: the stub)
        for path in ('auto', 'expanded'):
            with pytest.raises(AssertionError, match='eincm_loss_grad_motion was reached'):
                stub_engine(model=model, path=path, **ekw).loss_grad_motion(c, params(**pkw))
    # where the fused path applies, 'fused' reaches the fused entry point and 'expanded' the other
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion_fused was reached'):
        stub_engine(model=model, path='fused').loss_grad_motion(c, params())
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion was reached'):
        stub_engine(model=model).loss_grad_motion(c, params())
    # 'auto' follows the rule of profiles/motion_fused.md
    want = NAME if E.motion_auto_takes_fused(2, 200, 3) else 'eincm_loss_grad_motion'
    with pytest.raises(AssertionError, match=want + ' was reached'):
        stub_engine(model=model, path='auto').loss_grad_motion(c, params())
    # the solver evaluates by the engine's setting
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion_fused was reached'):
        bs.minimize_motion(stub_engine(model=model, path='fused'), model, np.zeros((2, 6)), params(), 5, 1e-5)
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion was reached'):
        bs.minimize_motion(stub_engine(model=model), model, np.zeros((2, 6)), params(), 5, 1e-5)


def test_the_example_takes_a_path_option():
    txt = open(os.path.join(ROOT, 'examples', 'motion_model.py')).read()
    assert re.search(r"add_argument\('--path', default='expanded', choices=\['expanded', 'fused', 'auto'\]", txt) and 'set_motion_path(a.path)' in txt
