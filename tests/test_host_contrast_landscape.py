"""The HIP-free rules of the contrast landscape (csrc/eincm_contrast_landscape.h) on the CPU: the argument check
in its stated order, one refusal at a time and with every later fault present, and the band plan over H, W in {1, 33, 65, 260, 480,
32767} and the four cell sizes: the bands hold every cell exactly once, each band fits the LDS budget beside the table and the
reduction's partials, and an image that fits is one band.

tests/host/contrast_landscape_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_responsibilities.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import itertools

import numpy as np
import pytest

import _host_check as HC

(OK, IN_FLIGHT, NULL_OUTPUTS, NOT_STAGED, NO_MODEL, SHARDED, RANGE, NULL_INPUT, NONFINITE) = range(9)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NULL_OUTPUTS: ERR_ARG, NOT_STAGED: ERR_STATE, NO_MODEL: ERR_STATE, SHARDED: ERR_UNSUPPORTED,
        RANGE: ERR_ARG, NULL_INPUT: ERR_ARG, NONFINITE: ERR_ARG}
LDS_BYTES, NT, TABLE_MAX = 65536, 1024, 2048                 # CL_LDS_BYTES, CL_NT, CL_TABLE_MAX
RED_BYTES = 2 * (NT // 64) * 8


@pytest.fixture(scope='session')
def contrast_landscape_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'contrast_landscape_check')


CASES, EXPECT = {}, {}
GOOD_C = np.arange(12, dtype=np.float64).reshape(2, 3, 2) - 5.0          # B = 2, V = 3, K = 2


def _check(name, fault, where=(-7, -7), in_flight=0, has_outputs=1, staged=1, model_set=1, sharded=0, B=2, K=2, V=3, cell=1, coeffs=GOOD_C,
           t_ref=(0.5, 0.25)):
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, has_outputs, staged, model_set, sharded, B, K, V, cell, int(coeffs is not None),
                int(t_ref is not None), *([] if coeffs is None else [float(v) for v in np.asarray(coeffs).reshape(-1)]),
                *([] if t_ref is None else [float(v) for v in t_ref]))
    EXPECT['check-' + name] = (fault, where)
    return 'check-' + name


def _with(i, v):
    c = GOOD_C.copy()
    c.reshape(-1)[i] = v
    return c


# every fault at once: each of the order's eight, the later ones still present when the earlier ones are mended
ALL_BAD = dict(in_flight=1, has_outputs=0, staged=0, model_set=0, sharded=1, V=0, cell=3, coeffs=None, t_ref=None)
_order = ['in_flight', 'has_outputs', 'staged', 'model_set', 'sharded', 'range', 'null', 'nonfinite']
_mend = {'in_flight': dict(in_flight=0), 'has_outputs': dict(has_outputs=1), 'staged': dict(staged=1), 'model_set': dict(model_set=1),
         'sharded': dict(sharded=0), 'range': dict(V=3, cell=2), 'null': dict(coeffs=_with(7, np.inf), t_ref=(np.nan, 0.5)),
         'nonfinite': dict(coeffs=GOOD_C, t_ref=(0.5, 0.5))}


def _from(i):
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw.update(_mend[k])
    return kw


CHECKS = [_check('ok', OK), _check('ok-v1-k12-cell8', OK, B=1, K=12, V=1, cell=8, coeffs=np.ones((1, 1, 12)), t_ref=(0.0,)),
          _check('ok-v-max', OK, B=1, K=1, V=4096, cell=4, coeffs=np.zeros((1, 4096, 1)), t_ref=(1.0,)),
          _check('ok-huge-finite', OK, coeffs=_with(3, 1e300), t_ref=(-1e300, 1e300)),
          _check('in-flight', IN_FLIGHT, in_flight=1), _check('null-outputs', NULL_OUTPUTS, has_outputs=0),
          _check('not-staged', NOT_STAGED, staged=0), _check('no-model', NO_MODEL, model_set=0), _check('sharded', SHARDED, sharded=1),
          _check('v0', RANGE, V=0, coeffs=None), _check('v-negative', RANGE, V=-1, coeffs=None), _check('v-4097', RANGE, V=4097, coeffs=None),
          _check('cell0', RANGE, cell=0), _check('cell3', RANGE, cell=3), _check('cell16', RANGE, cell=16), _check('cell-negative', RANGE, cell=-2),
          _check('coeffs-null', NULL_INPUT, coeffs=None), _check('t-ref-null', NULL_INPUT, t_ref=None),
          _check('nan-first', NONFINITE, (0, 0), coeffs=_with(0, np.nan)), _check('inf-last', NONFINITE, (1, 5), coeffs=_with(11, -np.inf)),
          _check('nan-second-window', NONFINITE, (1, 0), coeffs=_with(6, np.nan)),
          _check('t-ref-nan', NONFINITE, (0, -1), t_ref=(np.nan, 0.5)), _check('t-ref-inf-last', NONFINITE, (1, -1), t_ref=(0.5, np.inf)),
          _check('coeff-before-t-ref-of-its-window', NONFINITE, (0, 4), coeffs=_with(4, np.nan), t_ref=(np.nan, 0.5)),
          _check('t-ref-before-the-next-window', NONFINITE, (0, -1), coeffs=_with(6, np.nan), t_ref=(np.nan, 0.5))]
_where = {7: (0, -1)}                                                     # 'from-08': t_ref[0] is NaN, the inf sits in window 1
CHECKS += [_check(f'from-{i + 1:02d}-{k}', i + 1, _where.get(i, (-7, -7)), **_from(i)) for i, k in enumerate(_order)]
CHECKS += [_check('all-mended', OK, **_from(len(_order)))]

SIZES, CELLS = (1, 33, 65, 260, 480, 32767), (1, 2, 4, 8)
BANDS = [HC.add_case(CASES, f'bands-{H}x{W}-cell{c}', 'bands', H, W, c) for H, W, c in itertools.product(SIZES, SIZES, CELLS)]


@pytest.fixture(scope='module')
def out(contrast_landscape_check, tmp_path_factory):
    return HC.run(contrast_landscape_check, CASES, tmp_path_factory, 'contrast_landscape_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code, wb, wi = (int(v) for v in out[name][0])
    assert (fault, (wb, wi)) == EXPECT[name] and code == CODE[fault]


@pytest.mark.parametrize('name', BANDS)
def test_band_plan(out, name):
    H, W, cell = (int(t) for t in CASES[name].split()[1:])
    (Hc, Wc, rows, nrb, cols, ncb, table, n_bands, lds), (lo, hi, cells_max) = ([int(v) for v in part] for part in out[name][:2])
    assert (Hc, Wc) == (-(-H // cell), -(-W // cell)) and n_bands == nrb * ncb
    assert lo == 1 and hi == 1                                            # every cell (so every cell row) in exactly one band
    assert table == (W + H if W + H <= TABLE_MAX else 0)
    assert cells_max <= rows * cols and lds == table * 8 + (rows * cols + 1) // 2 * 8 + RED_BYTES and lds <= LDS_BYTES
    if table * 8 + Hc * Wc * 4 + RED_BYTES <= LDS_BYTES:
        assert n_bands == 1 and (rows, cols) == (Hc, Wc)                   # one band where the image fits
    else:
        assert n_bands > 1
    assert nrb == -(-Hc // rows) and ncb == -(-Wc // cols)
    if ncb > 1:
        assert rows == 1                                                  # the rows are cut only where one cell row does not fit
    else:
        assert cols == Wc and (rows == Hc or (rows + 1) * cols * 4 + table * 8 + RED_BYTES > LDS_BYTES)    # as many rows as fit


def test_the_constants_are_the_headers():
    import os
    import re
    txt = open(os.path.join(HC.CSRC, 'eincm_contrast_landscape.h')).read()
    assert int(re.search(r'constexpr int CL_NT = (\d+);', txt).group(1)) == NT
    assert int(re.search(r'constexpr int CL_LDS_BYTES = (\d+);', txt).group(1)) == LDS_BYTES
    assert int(re.search(r'constexpr int CL_TABLE_MAX = (\d+);', txt).group(1)) == TABLE_MAX
    assert 'hip' not in ''.join(re.findall(r'#include\s+[<"]([^>"]+)[>"]', txt)).lower()
    assert 'DROPPED' in txt and 'wrap' in txt                            # the header says that nothing wraps
