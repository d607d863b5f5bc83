"""The device-resident BFGS at its interfaces, without a GPU: the header declares the eincm_bfgs_* entry points and the binding table
matches it, the ABI version is unchanged, and the solver's ``bfgs_state`` keyword is validated before any GPU call."""
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bs = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
sol = importlib.import_module('edge-informed-contrast-maximization_amd.solver')
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')

BFGS_SYMBOLS = ['eincm_bfgs_accept', 'eincm_bfgs_begin', 'eincm_bfgs_eval', 'eincm_bfgs_fetch', 'eincm_bfgs_reduce',
                'eincm_bfgs_state_ptrs', 'eincm_bfgs_trial', 'eincm_bfgs_trial_ptrs']
LOSS = dict(alpha=20.0, beta=35.0, gamma=0.0, delta=0.0, scale_to_sensor_size_method='bilinear')


def header():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    return txt, re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


def test_header_declares_the_entry_points_and_the_binding_table_matches(built_lib):
    txt, code = header()
    declared = sorted(set(re.findall(r'\b(eincm_bfgs_[a-z_0-9]+)\s*\(', code)))
    assert declared == BFGS_SYMBOLS
    table = {n: (res, args) for n, res, args in L.SIGNATURES}
    for s in BFGS_SYMBOLS:
        assert s in table and hasattr(built_lib, s)
        # the number of parameters in the header's prototype equals the binding's
        proto = re.search(r'\b' + s + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S).group(1)
        assert len(proto.split(',')) == len(table[s][1]), s


def test_abi_version_and_constants(built_lib):
    txt, _ = header()
    assert built_lib.eincm_abi_version() == 6
    for name, val in (('EINCM_BFGS_MAX_N', L.BFGS_MAX_N), ('EINCM_BFGS_MAX_WINDOWS', L.BFGS_MAX_WINDOWS), ('EINCM_BFGS_NS', L.BFGS_NS),
                      ('EINCM_BFGS_SKIP', L.BFGS_SKIP), ('EINCM_BFGS_UPDATE', L.BFGS_UPDATE), ('EINCM_BFGS_MOVE', L.BFGS_MOVE),
                      ('EINCM_BFGS_INIT', L.BFGS_INIT), ('EINCM_BFGS_S_DPHI0', L.BFGS_S_DPHI0), ('EINCM_BFGS_S_GMAX', L.BFGS_S_GMAX),
                      ('EINCM_BFGS_S_PNORM', L.BFGS_S_PNORM), ('EINCM_BFGS_S_XMAX', L.BFGS_S_XMAX), ('EINCM_BFGS_S_PMAX', L.BFGS_S_PMAX),
                      ('EINCM_BFGS_S_GNORM', L.BFGS_S_GNORM), ('EINCM_BFGS_S_YS', L.BFGS_S_YS), ('EINCM_BFGS_S_YHY', L.BFGS_S_YHY)):
        assert int(re.search(r'#define\s+' + name + r'\s+(\d+)', txt).group(1)) == val, name
    assert L.BFGS_MAX_N >= 512                                 # the reference's finest theta grid: 2 * 16 * 16


def make_solver(**kw):
    n_lvls = 4
    return bs.BatchedMultipleLevelEINCMSolver(
        kw.pop('B', 2), (96, 128), n_lvls, sol.growing_maxiters(n_lvls, 3, 16), dict(LOSS, **kw.pop('loss', {})),
        {'method': 'BFGS', 'options': {'gtol': 1e-7}}, **kw)


def test_bfgs_state_is_validated_before_any_gpu_call(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(bs, 'Engine', no_engine)
    assert make_solver().bfgs_state == 'host'                  # the default: nothing changes for existing callers
    assert make_solver(bfgs_state='device').bfgs_state == 'device'
    assert make_solver(bfgs_state='host', n_groups=2).bfgs_state == 'host'
    for bad in ('gpu', None, 'Device', 1):
        with pytest.raises(ValueError, match='bfgs_state'):
            make_solver(bfgs_state=bad)
    with pytest.raises(ValueError, match='n_groups'):
        make_solver(bfgs_state='device', n_groups=2)
    with pytest.raises(ValueError, match='fp32'):
        make_solver(bfgs_state='device', loss={'precision': 'fp64'})
    assert make_solver(bfgs_state='host', loss={'precision': 'fp64'}).bfgs_state == 'host'


def test_state_backends_share_one_interface():
    for cls in (bs.NumpyBFGSState, bs.DeviceBFGSState):
        for m in ('begin', 'eval', 'accept', 'fetch'):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert bs.BFGS_STATES == ('host', 'device')


def test_numpy_state_accept_modes():
    """MOVE moves the point and keeps H and p; INIT also takes p = -H g; SKIP touches nothing."""
    n = 5
    rng = np.random.default_rng(0)
    g1 = rng.standard_normal((3, n))
    st = bs.NumpyBFGSState(lambda X, m: (np.zeros(3), g1))
    x0 = rng.standard_normal((3, n))
    st.begin(x0)
    st.eval(np.zeros(3), np.ones(3, bool))
    sc = st.accept(np.zeros(3), [L.BFGS_INIT, L.BFGS_MOVE, L.BFGS_SKIP])
    x, g, H = st.fetch(True)
    assert np.array_equal(x, x0) and np.array_equal(g[:2], g1[:2]) and not g[2].any()
    assert np.array_equal(st.p[0], -g1[0]) and not st.p[1].any() and not st.p[2].any()
    assert np.array_equal(H, np.stack([np.eye(n)] * 3))
    assert sc[0, L.BFGS_S_DPHI0] == -np.dot(g1[0], g1[0]) and sc[0, L.BFGS_S_GNORM] == np.linalg.norm(g1[0])
    assert sc[0, L.BFGS_S_GMAX] == np.abs(g1[0]).max() and sc[0, L.BFGS_S_XMAX] == np.abs(x0[0]).max()
    assert not sc[2].any()
