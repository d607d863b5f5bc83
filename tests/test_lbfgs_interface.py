"""The limited-memory BFGS at its interfaces, without a GPU: header, exports and binding table agree and the ABI version is unchanged;
the solver's and minimize_thetas' keywords are validated before any GPU call."""
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bs = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
sol = importlib.import_module('edge-informed-contrast-maximization_amd.solver')
eng = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')

LBFGS_SYMBOLS = ['eincm_lbfgs_begin', 'eincm_lbfgs_history_ptrs']
LOSS = dict(alpha=20.0, beta=35.0, gamma=0.0, delta=0.0, scale_to_sensor_size_method='bilinear')


def header():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    return txt, re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


def test_header_exports_and_binding_table_agree(built_lib):
    txt, code = header()
    assert sorted(set(re.findall(r'\b(eincm_lbfgs_[a-z_0-9]+)\s*\(', code))) == LBFGS_SYMBOLS
    table = {n: (res, args) for n, res, args in L.SIGNATURES}
    for s in LBFGS_SYMBOLS:
        assert s in table and hasattr(built_lib, s)
        proto = re.search(r'\b' + s + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S).group(1)
        assert len(proto.split(',')) == len(table[s][1]), s
    assert built_lib.eincm_abi_version() == 6
    assert int(re.search(r'#define\s+EINCM_ABI_VERSION\s+(\d+)', txt).group(1)) == 6
    for name, val in (('EINCM_LBFGS_MAX_HISTORY', L.LBFGS_MAX_HISTORY), ('EINCM_LBFGS_SCALE_IDENTITY', L.LBFGS_SCALES['identity']),
                      ('EINCM_LBFGS_SCALE_LAST_PAIR', L.LBFGS_SCALES['last_pair']), ('EINCM_BFGS_MAX_N', L.BFGS_MAX_N)):
        assert int(re.search(r'#define\s+' + name + r'\s+(\d+)', txt).group(1)) == val, name
    assert L.LBFGS_MAX_HISTORY == 16


def make_solver(**kw):
    n_lvls = 4
    return bs.BatchedMultipleLevelEINCMSolver(
        kw.pop('B', 2), (96, 128), n_lvls, sol.growing_maxiters(n_lvls, 3, 16), dict(LOSS, **kw.pop('loss', {})),
        {'method': 'BFGS', 'options': {'gtol': 1e-7}}, **kw)


def test_solver_keywords_are_validated_before_any_gpu_call(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(bs, 'Engine', no_engine)
    s = make_solver()
    assert (s.hessian, s.history, s.initial_scale) == ('dense', 10, 'last_pair')      # the defaults: today's behaviour
    for h in ('dense', 'limited', 'auto'):
        assert make_solver(hessian=h, bfgs_state='device').hessian == h
    for bad in ('sparse', None, 'Dense', 1):
        with pytest.raises(ValueError, match='hessian'):
            make_solver(hessian=bad)
    for bad in (0, -1, 2.0, True, '10', None):
        with pytest.raises(ValueError, match='history'):
            make_solver(hessian='limited', history=bad)
    with pytest.raises(ValueError, match='history'):
        make_solver(hessian='limited', history=17, bfgs_state='device')                # EINCM_LBFGS_MAX_HISTORY binds the device state
    assert make_solver(hessian='limited', history=40).history == 40                    # ... not the host's
    assert make_solver(hessian='limited', history=16, bfgs_state='device').history == 16
    for bad in ('none', None, 'Identity', 1):
        with pytest.raises(ValueError, match='initial_scale'):
            make_solver(hessian='limited', initial_scale=bad)
    assert make_solver(hessian='limited', initial_scale='identity').initial_scale == 'identity'
    # the device form on one fp32 context only, as for the dense matrix
    with pytest.raises(ValueError, match='n_groups'):
        make_solver(hessian='limited', bfgs_state='device', n_groups=2)
    with pytest.raises(ValueError, match='fp32'):
        make_solver(hessian='auto', bfgs_state='device', loss={'precision': 'fp64'})
    assert make_solver(hessian='limited', bfgs_state='host', n_groups=2, loss={'precision': 'fp64'}).hessian == 'limited'


def test_minimize_thetas_validates_before_it_touches_the_engine():
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError('the engine was touched: ' + name)
    th = np.zeros((2, 3, 3, 2))
    p = eng.make_params(1.0, 1.0, 0.0, 0.0, 1)
    for kw, what in ((dict(hessian='full'), 'hessian'), (dict(history=0), 'history'), (dict(history=17), 'history'),
                     (dict(initial_scale='gamma'), 'initial_scale'), (dict(bfgs_state='gpu'), 'bfgs_state')):
        with pytest.raises(ValueError, match=what):
            bs.minimize_thetas(NoEngine(), th, p, 5, 1e-6, **kw)
    with pytest.raises(ValueError, match='theta0'):
        bs.minimize_thetas(NoEngine(), np.zeros((2, 3, 3)), p, 5, 1e-6)


def test_state_backends_share_one_interface():
    for cls in (bs.NumpyLBFGSState, bs.DeviceLBFGSState):
        for m in ('begin', 'eval', 'accept', 'fetch'):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert bs.HESSIANS == ('dense', 'limited', 'auto')
    with pytest.raises(ValueError, match='history'):
        bs.DeviceLBFGSState(None, (3, 3, 2), None, history=17)
    with pytest.raises(ValueError, match='initial_scale'):
        bs.NumpyLBFGSState(None, 5, 'newest')
    with pytest.raises(ValueError, match='history'):
        eng.check_history(np.float64(3))


def test_minimize_thetas_host_forms_on_a_plain_objective():
    """The host forms need no engine when the caller supplies fun_batch: 'limited' above 64 unknowns runs NumpyLBFGSState, 'dense' and
    anything up to 64 unknowns LockstepBFGS (SciPy's own update, hess_inv returned)."""
    import _bfgs_cases as CASES
    for shape, hessian, limited in (((5, 13, 2), 'limited', True), ((5, 13, 2), 'auto', False), ((3, 5, 2), 'limited', False)):
        n = int(np.prod(shape))
        funs = [CASES.quartic_bowl(s, n) for s in (0, 1)]
        x0 = np.random.default_rng(3).standard_normal((2,) + shape)
        stats = {}
        res = bs.minimize_thetas(None, x0, None, 200, 1e-6, hessian=hessian, bfgs_state='host', fun_batch=CASES.batch_of(funs), stats=stats)
        for r in res:
            assert r.status == 0 and (r.hess_inv is None) == limited
        assert stats['n_batch_evals'] >= 1 and stats['n_window_evals'] >= 2
