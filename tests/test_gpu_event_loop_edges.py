"""The event kernels' loops at every trip boundary, and their window walks at the image borders (tests/_event_loop_edge_cases.py).

k_splat walks a segment in trips of 256 or 512 events through a pipeline unrolled x3 whose full trips carry no bound test and
whose one partial trip is peeled; k_gather walks the two halves of a segment in trips of 256.  The counts sit on both sides of
every multiple of 256, 512, 768 and 1536, with all events of a window in one source tile so that the count is the segment length;
three counts are also cut into segments of 512 (a last segment of one event).  Every count runs at a small theta (every tap
inside the LDS window), at a theta that carries the windows across the image borders (wrap / drop forms of the splat's flush
and of the gather's G-window load), both again with the capacity pinned to 1024 words (every window clamped: the out-of-window
taps and the flush of a clamped window), each as 2-DoF theta and as a 4x4 grid.

Three checks per evaluation:
  * value, gradient and IWE stack against the C port of the oracle at the bars of tests/test_gpu_parity.py: 1e-5, and 5e-5 for the
    gradient where taps leave the windows (the pinned capacity), the bar of test_huge_displacement_takes_the_direct_path;
  * the IWE stack of the pinned context array_equal to the automatic one's (the stack is an exact integer sum; the idiom of
    tests/test_gpu_launch_policy_parity.py::test_pinned_capacity_gives_the_same_accumulators);
  * value, gradient and IWE stack array_equal to tests/golden/event_loop_edges/parent.npz, recorded on an MI355X from the commit before
    the loops were reshaped (tools/record_event_loop_edges.py): the IWE is an integer sum and the 2-DoF gradient's per-thread fp32
    sums keep their order, so any differing bit is a lost, doubled or reordered event.
"""
import os

import numpy as np
import pytest

import _event_loop_edge_cases as E
from oracle import eincm_c_port as CP

pytestmark = pytest.mark.gpu

TOL = 1e-5                     # tests/test_gpu_parity.py
TOL_GRAD_DIRECT = 5e-5         # its bar for a gradient whose taps leave the LDS windows
PINNED = 1024
NTHREADS = min(os.cpu_count() or 1, 16)
RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'event_loop_edges', 'parent.npz')     # (a directory of its own: the loaders of tests/golden/*.npz take every file there for one of theirs)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope='module')
def parent():
    return dict(np.load(RECORDING, allow_pickle=False))


_PORT = {}


def port(n, setting, mode):
    """The C port's (value, gradient, IWE stack) per window; computed once per (n, theta) - segment lengths do not change it."""
    k = (n, setting, mode)
    if k not in _PORT:
        th = E.theta(setting, mode)
        out = []
        for b, win in enumerate(E.windows(n)):
            v, g, im = CP.loss_and_grad(th[b], *win, E.ALPHA, E.BETA, (E.H, E.W), nthreads=NTHREADS, return_images=True)
            out.append((v, g, im['iwes']))
        _PORT[k] = out
    return _PORT[k]


def check_port(tag, n, setting, mode, v, g, iw, tol_g):
    for b, (v_ref, g_ref, iw_ref) in enumerate(port(n, setting, mode)):
        e = (abs(v[b] - v_ref) / abs(v_ref), rel(g[b], g_ref), rel(iw[b], iw_ref))
        print(f'EDGE {tag} window {b} value={e[0]:.2e} grad={e[1]:.2e} iwe={e[2]:.2e}')
        assert e[0] <= TOL, (tag, b, 'value', e[0])
        assert e[1] <= tol_g, (tag, b, 'grad', e[1])
        assert e[2] <= TOL, (tag, b, 'iwes', e[2])


RUNS = E.runs()


@pytest.mark.parametrize('n,seg', RUNS, ids=[f'n{n}' + (f'-seg{seg}' if seg else '') for n, seg in RUNS])
def test_event_count_at_a_trip_boundary(built_lib, parent, n, seg):
    auto, pinned = E.stage(n, seg=seg), E.stage(n, wincap=PINNED, seg=seg)
    try:
        pol = pinned.launch_policy
        for setting in E.SETTINGS:
            for mode in E.MODES:
                tag = f'n{n} seg{seg or 0} {setting} {mode}'
                v, g, iw = E.evaluate(auto, setting, mode)
                check_port(tag + ' auto', n, setting, mode, v, g, iw, TOL)
                vp, gp, iwp = E.evaluate(pinned, setting, mode)
                p = pol()
                assert p['cap_splat'] == PINNED and p['cap_gather'] == PINNED and p['cap_gather_2dof'] == PINNED
                check_port(tag + ' pinned', n, setting, mode, vp, gp, iwp, TOL_GRAD_DIRECT)
                assert np.array_equal(iwp, iw), (tag, 'pinned IWE', rel(iwp, iw))
                # the parent commit's bits
                assert np.array_equal(v, parent[E.key(n, seg, setting, mode, 'value')]), (tag, 'value')
                assert np.array_equal(g, parent[E.key(n, seg, setting, mode, 'grad')]), (tag, 'grad')
                assert np.array_equal(E.digest(iw), parent[E.key(n, seg, setting, mode, 'iwe_sha256')]), (tag, 'IWE')
                if E.key(n, seg, setting, mode, 'iwe_nz_index') in parent:
                    full = np.zeros(iw.size, dtype=np.float32)
                    full[parent[E.key(n, seg, setting, mode, 'iwe_nz_index')]] = parent[E.key(n, seg, setting, mode, 'iwe_nz_value')]
                    assert np.array_equal(iw.reshape(-1), full), (tag, 'IWE in full')
    finally:
        auto.close()
        pinned.close()
