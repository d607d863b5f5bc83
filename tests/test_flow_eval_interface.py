"""The batched flow-error evaluation without a GPU: the header declares the struct and both functions, _lib binds
them with the C compiler's layout, the ABI version stays 6, the Python entry points have the documented signatures, and every shape
and dtype refusal of the Python side is made before a GPU context is asked for."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

pkg = 'edge-informed-contrast-maximization_amd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
ev = importlib.import_module(pkg + '.evaluation')


def test_header_declares_struct_and_functions():
    txt = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    assert re.search(r'typedef struct eincm_flow_error_out \{[^}]*\} eincm_flow_error_out;', txt)
    assert re.search(r'int eincm_flow_eval_stage\(eincm_ctx\* ctx, int n_windows, const double\* gt_flow, const int64_t\* n_events, '
                     r'const int16_t\* xs,\s+const int16_t\* ys, const uint8_t\* eval_mask\);', txt)
    assert re.search(r'int eincm_flow_errors\(eincm_ctx\* ctx, const double\* theta, int h, int w, int method, '
                     r'eincm_flow_error_out\* out, double\* ee_map\);', txt)
    assert re.search(r'#define EINCM_ABI_VERSION 6\b', txt)
    line = txt[txt.index('#define EINCM_ABI_VERSION'):txt.index('#define EINCM_OK')]
    assert 'eincm_flow_eval_stage' in line and 'eincm_flow_errors' in line


def test_binding_and_abi_version(built_lib):
    names = [n for n, _, _ in L.SIGNATURES]
    assert names.count('eincm_flow_eval_stage') == 1 and names.count('eincm_flow_errors') == 1
    assert built_lib.eincm_abi_version() == 6
    assert built_lib.eincm_flow_eval_stage.restype is C.c_int and len(built_lib.eincm_flow_eval_stage.argtypes) == 7
    assert built_lib.eincm_flow_errors.restype is C.c_int and len(built_lib.eincm_flow_errors.argtypes) == 7
    assert L.FLOW_ERROR_THRESHOLDS == (1, 2, 3, 5, 10, 20)
    # a null context is refused by both, before anything else is looked at
    assert built_lib.eincm_flow_eval_stage(None, 1, None, None, None, None, None) == L.ERR_ARG
    assert built_lib.eincm_flow_errors(None, None, 1, 1, 0, None, None) == L.ERR_ARG


def test_struct_layout_matches_the_c_compiler(tmp_path):
    fields = [f for f, _ in L.FlowErrorOut._fields_]
    assert fields == ['n_ee', 'n_pred', 'n_gt', 'n_over', 'sum_ee', 'sum_ree', 'aee', 'aree', 'anpe']
    src = tmp_path / 'fe.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eincm.h"\nint main(void){'
                   'printf("%zu", sizeof(eincm_flow_error_out));'
                   + ''.join(f'printf(" %zu", offsetof(eincm_flow_error_out, {f}));' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'fe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.FlowErrorOut) == 9 * 8 + 10 * 8
    assert vals[1:] == [getattr(L.FlowErrorOut, f).offset for f in fields]


def test_python_signatures():
    p = inspect.signature(E.Engine.flow_eval_stage).parameters
    assert list(p) == ['self', 'gt_flows', 'events', 'eval_masks'] and p['eval_masks'].default is None
    p = inspect.signature(E.Engine.flow_errors).parameters
    assert list(p) == ['self', 'thetas', 'method', 'ee_map'] and p['method'].default == 'bilinear' and p['ee_map'].default is False
    p = inspect.signature(ev.BatchThetaEvaluator.__init__).parameters
    assert list(p) == ['self', 'sensor_size', 'windows', 'gt_flows', 'alpha', 'beta', 'gamma', 'delta', 'err_eval_event_masks', 'method',
                       'window_size', 'precision', 'engine']
    assert (p['err_eval_event_masks'].default, p['method'].default, p['window_size'].default, p['precision'].default,
            p['engine'].default) == (None, 'bilinear', 3, 'fp32', None)
    for name in ('flow_errors', 'evaluate', 'close', '__enter__', '__exit__'):
        assert callable(getattr(ev.BatchThetaEvaluator, name))
    assert 'BatchThetaEvaluator' in ev.__doc__ and 'stay on the host' in ev.__doc__


def test_stage_argument_checks_need_no_device():
    H, W = 6, 8
    gt = np.zeros((2, H, W, 2))
    events = [(np.array([0, 1]), np.array([2, 3])), (np.zeros(0, np.int16), np.zeros(0, np.int16))]
    g, n, xs, ys, m = E.check_flow_eval_batch(gt.astype(np.float32), events, None, (H, W))
    assert g.dtype == np.float64 and n.tolist() == [2, 0] and xs.dtype == np.int16 and xs.tolist() == [0, 1] and ys.tolist() == [2, 3]
    assert m is None
    *_, m = E.check_flow_eval_batch(gt, events, np.ones((2, H, W), bool), (H, W))
    assert m.dtype == np.uint8 and m.flags.c_contiguous and m.min() == 1
    # float32 widens exactly
    f = np.random.default_rng(0).normal(size=(2, H, W, 2)).astype(np.float32)
    assert np.array_equal(E.check_flow_eval_batch(f, events, None, (H, W))[0], f.astype(np.float64))
    with pytest.raises(ValueError, match='float32 or float64'):
        E.check_flow_eval_batch(gt.astype(np.int32), events, None, (H, W))
    with pytest.raises(ValueError, match='gt_flows must be'):
        E.check_flow_eval_batch(gt[0], events, None, (H, W))
    with pytest.raises(ValueError, match='gt_flows must be'):
        E.check_flow_eval_batch(gt, events, None, (H, W + 1))
    with pytest.raises(ValueError, match='gt_flows must be'):
        E.check_flow_eval_batch(gt[:0], [], None, (H, W))
    with pytest.raises(ValueError, match='event lists'):
        E.check_flow_eval_batch(gt, events[:1], None, (H, W))
    with pytest.raises(ValueError, match=r'\(xs, ys\)'):
        E.check_flow_eval_batch(gt, [events[0], (np.zeros(1),)], None, (H, W))
    with pytest.raises(ValueError, match='one length'):
        E.check_flow_eval_batch(gt, [events[0], (np.zeros(2), np.zeros(3))], None, (H, W))
    with pytest.raises(ValueError, match='int16 range'):
        E.check_flow_eval_batch(gt, [events[0], (np.array([70000]), np.array([0]))], None, (H, W))
    with pytest.raises(ValueError, match='eval_masks must be'):
        E.check_flow_eval_batch(gt, events, np.ones((H, W), bool), (H, W))
    with pytest.raises(ValueError, match='eval_masks must be'):
        E.check_flow_eval_batch(gt, events, np.ones((2, H, W), dtype=object), (H, W))


def test_theta_argument_checks_need_no_device():
    H, W = 6, 8
    t, code = E.check_flow_eval_thetas(np.zeros((3, 2, 2, 2), np.float32), 3, (H, W), 'cubic')
    assert t.dtype == np.float64 and code == L.METHODS['cubic']
    assert E.check_flow_eval_thetas(np.zeros((H, W, 2)), 1, (H, W), 'bilinear')[0].shape == (1, H, W, 2)
    with pytest.raises(ValueError, match='method'):
        E.check_flow_eval_thetas(np.zeros((1, 2, 2, 2)), 1, (H, W), 'nearest')
    with pytest.raises(ValueError, match='method'):
        E.check_flow_eval_thetas(np.zeros((1, 2, 2, 2)), 1, (H, W), 0)
    with pytest.raises(ValueError, match='thetas must be'):
        E.check_flow_eval_thetas(np.zeros((2, 2, 2, 2)), 3, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='thetas must be'):
        E.check_flow_eval_thetas(np.zeros((2, 2, 2)), 2, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='thetas must be'):
        E.check_flow_eval_thetas(np.zeros((1, 2, 2, 3)), 1, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='thetas must be'):
        E.check_flow_eval_thetas(np.zeros((1, 0, 2, 2)), 1, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='numeric'):
        E.check_flow_eval_thetas(np.zeros((1, 2, 2, 2), dtype=complex), 1, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='finer'):
        E.check_flow_eval_thetas(np.zeros((1, H + 1, 2, 2)), 1, (H, W), 'bilinear')
    with pytest.raises(ValueError, match='finer'):
        E.check_flow_eval_thetas(np.zeros((1, 2, W + 1, 2)), 1, (H, W), 'bilinear')


def test_evaluator_refuses_before_an_engine_exists(monkeypatch):
    """Every refusal below comes from the constructor's own checks: a stand-in Engine records any attempt to create a context."""
    made = []
    monkeypatch.setattr(ev, 'Engine', lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError('context asked for')))
    H, W = 6, 8
    win = (np.array([1, 2]), np.array([3, 4]), np.array([0.0, 1.0]), np.zeros((2, H, W)), np.array([0.0, 1.0]))
    gt = np.zeros((1, H, W, 2))
    args = (1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match='no windows'):
        ev.BatchThetaEvaluator((H, W), [], gt, *args)
    with pytest.raises(ValueError, match='must be'):
        ev.BatchThetaEvaluator((H, W), [win[:4]], gt, *args)
    with pytest.raises(ValueError, match='method'):
        ev.BatchThetaEvaluator((H, W), [win], gt, *args, method='nearest')
    with pytest.raises(ValueError, match='precision'):
        ev.BatchThetaEvaluator((H, W), [win], gt, *args, precision='fp16')
    with pytest.raises(ValueError):
        ev.BatchThetaEvaluator((H, W), [win], gt, *args, window_size=9)
    with pytest.raises(ValueError, match='ground-truth flows for'):
        ev.BatchThetaEvaluator((H, W), [win, win], gt, *args)
    with pytest.raises(ValueError, match='gt_flows must be'):
        ev.BatchThetaEvaluator((H, W), [win], np.zeros((1, H, W + 1, 2)), *args)
    with pytest.raises(ValueError, match='eval_masks must be'):
        ev.BatchThetaEvaluator((H, W), [win], gt, *args, err_eval_event_masks=np.ones((H, W)))
    with pytest.raises(ValueError, match='without gt_flows'):
        ev.BatchThetaEvaluator((H, W), [win], None, *args, err_eval_event_masks=np.ones((1, H, W)))
    assert made == []
