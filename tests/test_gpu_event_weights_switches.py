"""The environment switches of DESIGN.md 5.1 with a weighted batch: tests/test_gpu_switches.py with per-event weights.

tests/_weighted_switch_probe.py evaluates two weighted three-window batches (narrow and wide: window 0 with n * R above and below
4096) at the four theta shapes of tests/_switch_probe.py, one fresh process per switch and one at a time (the evaluation knobs are
read once per process).  Every run - the default one and every switched one - is held to the fp64 witness of
tests/_event_weights_witness.py at 1e-5 (value and gradient of every window, the IWE stack of window 0; the witness is computed
once, in the parent), and every switched run to the default run at the bars of tests/test_gpu_switches.py between two configurations
of the library: 2e-6 for the value, 2e-5 for the gradient and dL/dIWE, 1e-6 for the IWE stack.

Which weighted code each run reaches is asserted, not derived by eye: the launch form of an evaluation (the instantiation of k_splat and
k_gather with its threads, LDS bytes and lists) is a value of the plan (plan_forms in csrc/eincm_plan.h), and
tests/test_host_plan.py::test_named_cells_take_their_forms asserts on the CPU which form each run of this module plans - the cases
forms-2dof-, forms-grid*-, forms-noproj- and forms-allr- at -w1-wide0 (narrow batch) and -w1-wide1 (wide batch); DESIGN.md section 22
has the table, staging kernels included.  This module asserts the inputs those cases assume: n * R on either side of 4096 (plan_staging:
wide), the cells a tile touches (plan_eval: proj), and the environment each child saw.

The all-reference-times gather also runs without a switch, on the 16-window batches of
tests/test_gpu_event_weights_cells.py (1500 segments and more; WIDE = 0: forms-cell-*-w1), and the weighted k_mask in its
test_weight_zero_is_absence_on_host_binning, where pixels that hold nothing but weight-0 events decide the TV term.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _event_weights_witness as EW
from oracle import eincm_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location('_weighted_switch_probe', os.path.join(HERE, '_weighted_switch_probe.py'))
probe = importlib.util.module_from_spec(spec)
spec.loader.exec_module(probe)

TOL = 1e-5                                                  # against the witness (tests/test_gpu_parity.py)
TOL_SAME_V, TOL_SAME_G, TOL_SAME_I = 2e-6, 2e-5, 1e-6       # between two configurations (tests/test_gpu_switches.py)
PG_MAXC, TS = 6, 32                                         # csrc/eincm_types.h

RUNS = [
    ('default', {}),
    ('no-host-asm', {'EINCM_NO_HOST_ASM': '1'}),
    ('no-big-theta-arg', {'EINCM_NO_BIG_THETA_ARG': '1'}),
    ('no-proj-in-gather', {'EINCM_NO_PROJ_IN_GATHER': '1'}),
    ('plain-copies', {'EINCM_NO_SEGSORT': '1', 'EINCM_NO_SPREAD': '1'}),
    ('segment-lengths', {'EINCM_SEG': '4096', 'EINCM_SEG_SPLAT': '2048', 'EINCM_SEG_2DOF': '8192'}),
    ('host-binning', {'EINCM_HOST_BINNING': '1'}),
    ('gather-all-r', {'EINCM_GATHER_ALL_R': '1'}),
    ('pitch-aligned-2', {'EINCM_PITCH_ALIGNED': '2'}),
]


def rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def run_probe(tmp, tag, env_extra):
    out = os.path.join(tmp, f'{tag}.npz')
    env = {k: v for k, v in os.environ.items() if not k.startswith('EINCM_') or k == 'EINCM_LIB'}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, '_weighted_switch_probe.py'), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
    got = dict(np.load(out))
    assert json.loads(str(got.pop('env'))) == env_extra, tag          # the child saw this switch and no other
    return got


def cells_under_a_tile(n_in, n_out):
    """The most coarse cells a 32-pixel tile's rows of the resampling matrix touch (build_resample in csrc/eincm_plan.h)."""
    A = O.resample_matrix(n_in, n_out, n_out / n_in, 'bilinear')
    most = 0
    for t0 in range(0, n_out, TS):
        nz = np.nonzero(np.abs(A[t0:t0 + TS]).sum(axis=0))[0]
        most = max(most, int(nz.max()) + 1 - int(nz.min()))
    return most


def test_the_coverage_tables_inputs():
    """What the docstring's table rests on, as far as it can be seen from outside the library."""
    R = probe.R
    assert all(n * R >= probe.WIDE_BELOW for n in probe.BATCHES['narrow'])
    assert probe.BATCHES['wide'][0] * R < probe.WIDE_BELOW and all(n * R >= probe.WIDE_BELOW for n in probe.BATCHES['wide'][1:])
    shapes = [hw for hw, _, _ in probe.CASES]
    assert shapes[0] == (1, 1) and len(shapes) == 4
    for h, w in shapes[1:]:                   # every grid projects inside the gather unless the switch forbids it
        assert cells_under_a_tile(h, probe.H) <= PG_MAXC and cells_under_a_tile(w, probe.W) <= PG_MAXC
    assert sum(1 for _, g, lvl in probe.CASES[1:] if g != 0.0 and lvl == 0) == 2      # the mask is read by two of the grids
    assert probe.WEIGHTED == (True, True, False)
    # (the environment of each run: run_probe compares what the child saw with the run's switch)


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp('weighted_switches'))


@pytest.fixture(scope='module')
def witness():
    """{(batch, case, window): (value, gradient, IWE stack)} in fp64, once; windows 1 and 2 are shared by the two batches."""
    out, shared = {}, {}
    for batch in probe.BATCHES:
        wins, weights, thetas = probe.inputs(batch)
        for i, (th, (hw, gamma, lvl)) in enumerate(zip(thetas, probe.CASES)):
            A = (O.resample_matrix(hw[0], probe.H, probe.H / hw[0], 'bilinear'), O.resample_matrix(hw[1], probe.W, probe.W / hw[1], 'bilinear'))
            for b, (w, wt) in enumerate(zip(wins, weights)):
                k = (i, b) if b > 0 else (batch, i, b)
                if k not in shared:
                    v, g, _, I, _ = EW.loss_and_grad(th[b], w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts'], probe.ALPHA, probe.BETA,
                                                     gamma, 0.0, lvl, *A, weights=wt)
                    shared[k] = (v, g, I if b == 0 else None)
                out[batch, i, b] = shared[k]
    return out


@pytest.fixture(scope='module')
def default_run(built_lib, tmp):
    return run_probe(tmp, 'default', {})


def against_witness(tag, got, witness):
    worst = np.zeros(3)
    for batch in probe.BATCHES:
        for i, (hw, _, _) in enumerate(probe.CASES):
            for b in range(probe.B):
                v_w, g_w, I_w = witness[batch, i, b]
                e = [abs(got[f'{batch}_v{i}'][b] - v_w) / abs(v_w), rel(got[f'{batch}_g{i}'][b], g_w),
                     rel(got[f'{batch}_iwe{i}'][b], I_w) if I_w is not None else 0.0]
                worst = np.maximum(worst, e)
                assert max(e) <= TOL, (tag, batch, hw, b, e)
    print(f'WSWITCH {tag} against the witness: value={worst[0]:.2e} grad={worst[1]:.2e} iwe={worst[2]:.2e}')


@pytest.mark.timeout(900)
@pytest.mark.parametrize('tag,env', RUNS, ids=[t for t, _ in RUNS])
def test_weighted_switch(tmp, witness, default_run, tag, env):
    got = default_run if not env else run_probe(tmp, tag, env)
    against_witness(tag, got, witness)
    if not env:
        return
    worst = np.zeros(4)
    for batch in probe.BATCHES:
        for i, (hw, _, _) in enumerate(probe.CASES):
            e = [rel(got[f'{batch}_{q}{i}'], default_run[f'{batch}_{q}{i}']) for q in ('v', 'g', 'iwe', 'G')]
            worst = np.maximum(worst, e)
            assert e[0] <= TOL_SAME_V and e[1] <= TOL_SAME_G and e[2] <= TOL_SAME_I and e[3] <= TOL_SAME_G, (tag, batch, hw, e)
    print(f'WSWITCH {tag} against the default run: value={worst[0]:.2e} grad={worst[1]:.2e} iwe={worst[2]:.2e} G={worst[3]:.2e}')
