"""Re-weighting a staged batch in place without a GPU: the new entry points and flags in header, binding table
and cross-compiled library, the refusals that Python reaches before a library call (set_weights' arguments, keep_order on engines
that have no weighted form, the calls that need a keep-order batch), the flags the applying E-step hands over, the in-place EM
driver's arguments, and where the kernels carry the index.

The existing interface tests pin the parameter lists of Engine.event_responsibilities and segmentation.segment_motions, so the
applying E-step and the in-place driver are entry points of their own beside them: Engine.apply_responsibilities and
segmentation.segment_motions_in_place."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'edge-informed-contrast-maximization_amd'
L = importlib.import_module(PKG + '._lib')
E = importlib.import_module(PKG + '.engine')
motion = importlib.import_module(PKG + '.motion')
segmentation = importlib.import_module(PKG + '.segmentation')
sharding = importlib.import_module(PKG + '.sharding')
batch_solver = importlib.import_module(PKG + '.batch_solver')

# the Python entry points: a tree without them has nothing that this module could test
set_weights, staged_weights, staged_order, apply_responsibilities = (E.Engine.set_weights, E.Engine.staged_weights, E.Engine.staged_order,
                                                                     E.Engine.apply_responsibilities)
segment_motions_in_place, keep_order_refusal = segmentation.segment_motions_in_place, E.keep_order_refusal

NEW = {'eincm_set_weights': ['eincm_ctx* ctx', 'const float* const* weights'],
       'eincm_get_stage_order': ['eincm_ctx* ctx', 'uint32_t* order_splat', 'uint32_t* order_gather'],
       'eincm_get_staged_weights': ['eincm_ctx* ctx', 'float* weights']}


# ---- header, binding table, library ---------------------------------------------------------------------------------------------
def test_entry_points_and_flags_in_header_binding_and_library(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    defines = dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)u?\b', hdr))
    assert int(defines['EINCM_ABI_VERSION']) == 6 and built_lib.eincm_abi_version() == 6
    assert int(defines['EINCM_SW_KEEP_ORDER']) == L.SW_KEEP_ORDER == 2 and int(defines['EINCM_SW_DEFER_CONSTANTS']) == L.SW_DEFER_CONSTANTS == 1
    assert int(defines['EINCM_RS_EXCLUDE_SELF']) == L.RS_EXCLUDE_SELF == 1
    assert int(defines['EINCM_RS_STAGED_WEIGHTS']) == L.RS_STAGED_WEIGHTS == 2 and int(defines['EINCM_RS_APPLY']) == L.RS_APPLY == 4
    names_after_version = hdr.split('#define EINCM_ABI_VERSION')[1].split('*/')[0]
    table = {n: (res, a) for n, res, a in L.SIGNATURES}
    for name, args in NEW.items():
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', hdr)
        assert m, name + ' is not declared'
        assert [' '.join(a.split()) for a in m.group(1).split(',')] == args
        assert name in names_after_version, name + ' is not in the name list after EINCM_ABI_VERSION'
        assert [n for n, _, _ in L.SIGNATURES].count(name) == 1
        res, a = table[name]
        assert res is C.c_int and a == [C.c_void_p] * len(args)
        fn = getattr(built_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == a
        assert fn(*([None] * len(args))) == L.ERR_ARG                              # no context: refused without a GPU
    # no struct changed: the structures of the binding table are the header's as before (tests/test_abi.py compares them in full)
    assert 'struct' not in hdr.split('int eincm_set_weights')[0].rsplit('int eincm_set_windows_weighted', 1)[1]


def test_the_index_rides_through_the_three_permutation_kernels_and_the_host_sort():
    csrc = os.path.join(ROOT, PKG, 'csrc')
    code = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, 'eincm_binning.hip.h')).read())
    for kernel in ('k_bin_scatter', 'k_spread', 'k_segsort'):
        assert re.search(r'template <int WT, int IX = 0>\s*__global__[^;{]*\b' + kernel + r'\(', code), kernel
    assert re.search(r'__global__[^;{]*\bk_reweight\(', code)
    body = code.split('void k_reweight(')[1].split('\n}\n')[0]
    assert 'ev_w[i] = w_raw[idx[i]];' in body and 'ev_w_g[i] = w_raw[idx_g[i]];' in body and 'atomic' not in body
    # pure moves: every statement under IX is a load or a store of the index, nothing is computed from it
    ix = [s.strip() for s in re.findall(r'if \(IX\) ([^;]*;)', code)]
    assert len(ix) == 6 and all(re.fullmatch(r'(ev_i|dst_i)\[[^\]]*\] = (src|\(uint32_t\)\(bb\.start \+ i\));|(src|ni) = (ev_i|src_i)\[[^\]]*\];', s) for s in ix), ix
    plan = open(os.path.join(csrc, 'eincm_plan.h')).read()
    assert 'std::vector<uint32_t>* sidx = nullptr' in plan and '(*sidx)[d] = (uint32_t)(base + i);' in plan
    assert 'P.weighted = P.keep_order || batch_weighted(n_windows, n_events, weights);' in plan
    api = open(os.path.join(csrc, 'eincm_api.hip')).read()
    for launch in ('k_bin_scatter<1, 1>', 'k_spread<1, 1>', 'k_segsort<1, 1>', 'k_bin_scatter<0>', 'k_spread<0>', 'k_segsort<0>'):
        assert launch in api, launch
    body = api.split('int eincm_set_weights(')[1].split('\n}\n')[0]
    assert body.index('keep_order_ready(') < body.index('check_weights(') < body.index('OneShot op(c);') < body.index('upload_raw_weights(')
    assert 'hipMalloc' not in body and 'alloc_dev' not in body
    # reweight_staged and the two functions it shares with a staging - what depends on the weights, what a new batch drops - hold the steps
    fn = {name: api.split(f'static {ret} {name}(')[1].split('\n}\n')[0]
          for ret, name in (('int', 'reweight_staged'), ('int', 'weight_state'), ('void', 'drop_batch_state'))}
    assert fn['reweight_staged'].index('k_reweight') < fn['reweight_staged'].index('weight_state(c') \
        < fn['reweight_staged'].index('drop_batch_state(c)') < fn['reweight_staged'].index('window_constants(c)')
    body = '\n'.join(fn.values())
    for step in ('k_reweight', 'k_tile_counts', 'k_mask', 'most_on_one_pixel', 'window_constants(c)', 'have_eval = false', 'objc_valid = false',
                 'bfgs.begun = false', 'last_q.clear()', 'seg0.clear()', 'policy_evaluated = false'):
        assert step in body, step
    for untouched in ('k_edges', 'build_list', 'k_segsort', 'k_spread', 'k_bin_', 'upload_raw_events', 'alloc_dev'):
        assert untouched not in body, untouched
    # one owner each: a staging calls the same two and states neither list itself
    staging = api.split('static int finish_lists(')[1].split('\nint eincm_set_windows_ex(')[0]
    assert 'weight_state(c' in staging and 'drop_batch_state(c)' in staging
    for once in ('k_tile_counts', 'k_mask', 'objc_valid = false', 'bfgs.begun = false', 'have_eval = false', 'policy_evaluated = false'):
        assert once not in staging, once


def test_c_side_states_the_refusals_in_their_own_words():
    api = open(os.path.join(ROOT, PKG, 'csrc', 'eincm_api.hip')).read()
    for phrase in ('EINCM_SW_KEEP_ORDER is not supported in fp64 mode', 'EINCM_SW_KEEP_ORDER has the 3x3 splat window only',
                   'EINCM_SW_KEEP_ORDER is not supported in an event-sharded staging', 'the batch was staged without EINCM_SW_KEEP_ORDER',
                   'weights_in must be NULL with EINCM_RS_STAGED_WEIGHTS'):
        assert phrase in api, phrase


# ---- the Python layer with a stub in the library's place ------------------------------------------------------------------------
class NoGpu:
    """Stands where the library is: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


class Reached(Exception):
    pass


class Records:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name,) + a)
            raise Reached()
        return call


def stub_engine(lib=None, precision='fp32', splat_window=3, B=2, R=2, H=20, W=26, n=(5, 3), keep_order=True):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, lib or NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = precision, splat_window, B, R, H, W
    eng._io, eng.n_events = {}, np.array(n, dtype=np.int64)
    eng._keep_order, eng._weighted, eng._staged_weights = keep_order, keep_order, [None] * B
    return eng


def _tiny_window(n=5, H=20, W=26):
    return (np.arange(n, dtype=np.int16), np.arange(n, dtype=np.int16), np.linspace(0.0, 1.0, n), np.zeros((2, H, W)), np.array([0.0, 1.0]))


BAD_WEIGHTS = [('wrong-list-length', [np.ones(5)], 'list of 2 entries'), ('list-too-long', [None, None, None], 'list of 2 entries'),
               ('not-a-list', None, 'list of 2 entries'), ('one-array-for-the-batch', np.ones(8), 'list of 2 entries'),
               ('wrong-array-length', [np.ones(5), np.ones(4)], r'weights must be \(3,\)'), ('value-above-one', [np.ones(5), [0.5, 1.5, 0.5]], r'within \[0, 1\]'),
               ('value-below-zero', [np.array([0.5, 0.5, -1e-9, 0.5, 0.5]), None], r'within \[0, 1\]'), ('nan', [None, [0.5, np.nan, 0.5]], 'finite'),
               ('inf', [None, [0.5, np.inf, 0.5]], 'finite'), ('strings', [['a'] * 5, None], 'numbers')]


@pytest.mark.parametrize('name,weights,match', BAD_WEIGHTS, ids=[b[0] for b in BAD_WEIGHTS])
def test_set_weights_refuses_bad_arguments_before_any_library_call(name, weights, match):
    with pytest.raises(ValueError, match=match):
        stub_engine().set_weights(weights)
    with pytest.raises(ValueError, match=match):
        E.check_weight_list(weights, [5, 3])


def test_a_good_set_weights_reaches_the_library_with_one_pointer_per_window():
    lib = Records()
    w = np.array([0.0, 0.25, 1.0], dtype=np.float64)
    with pytest.raises(Reached):
        stub_engine(lib).set_weights([None, w])
    name, _, wp = lib.calls[-1]
    assert name == 'eincm_set_weights' and len(wp) == 2 and wp[0] is None and wp[1] is not None
    assert np.array_equal(np.ctypeslib.as_array(C.cast(wp[1], C.POINTER(C.c_float)), (3,)), w.astype(np.float32))
    with pytest.raises(Reached):
        stub_engine(lib).set_weights([None, None])                                 # all ones: a NULL array
    assert lib.calls[-1][2] is None
    got = E.check_weight_list([None, w], [5, 3])
    assert got[0] is None and got[1].dtype == np.float32 and np.array_equal(got[1], w.astype(np.float32))


def test_calls_that_need_a_keep_order_batch_name_the_flag():
    eng = stub_engine(keep_order=False)
    for call in (lambda: eng.set_weights([None, None]), eng.staged_weights, eng.staged_order, lambda: eng.apply_responsibilities(2)):
        with pytest.raises(ValueError, match='keep_order=True'):
            call()
    assert E.Engine.__new__(E.Engine).keep_order is False and isinstance(E.Engine.keep_order, property)


def test_keep_order_is_refused_where_weights_are_with_messages_of_its_own():
    assert keep_order_refusal('fp32', 3) is None
    whys = [keep_order_refusal('fp64', 3), keep_order_refusal('fp32', 5), keep_order_refusal('fp32', 3, sharded=True)]
    assert 'fp64' in whys[0] and '3x3 splat window' in whys[1] and 'sharded' in whys[2]
    assert len(set(whys)) == 3 and all('keep_order' in w for w in whys)
    assert not set(whys) & {E.event_weights_refusal('fp64', 3), E.event_weights_refusal('fp32', 5), E.event_weights_refusal('fp32', 3, sharded=True)}
    win = _tiny_window()
    with pytest.raises(ValueError, match='keep_order is not supported in fp64'):
        stub_engine(precision='fp64').set_windows([win], keep_order=True)
    with pytest.raises(ValueError, match='keep_order has the 3x3'):
        stub_engine(splat_window=5).set_windows([win], keep_order=True)
    with pytest.raises(ValueError, match='keep_order is not supported by the event-sharded'):
        stub_engine().set_windows([win], defer_constants=True, keep_order=True)
    with pytest.raises(ValueError, match='keep_order is not supported in fp64'):
        stub_engine(precision='fp64').set_window(*win, keep_order=True)
    # the sharded engine and the engine group do not take the keyword
    assert 'keep_order' not in inspect.signature(sharding.ShardedEngine.set_windows).parameters
    assert 'keep_order' not in inspect.signature(E.EngineGroup.set_windows).parameters
    assert inspect.signature(E.Engine.set_windows).parameters['keep_order'].default is False
    assert inspect.signature(E.Engine.set_window).parameters['keep_order'].default is False


def test_a_keep_order_staging_takes_the_weighted_entry_point_with_the_flag():
    lib = Records()
    win = _tiny_window()
    with pytest.raises(Reached):
        stub_engine(lib).set_windows([win, win], keep_order=True)
    assert lib.calls[-1][0] == 'eincm_set_windows_weighted' and lib.calls[-1][-1] == L.SW_KEEP_ORDER and lib.calls[-1][-2] is None
    with pytest.raises(Reached):
        stub_engine(lib).set_windows([win + (np.full(5, 0.5),), win], keep_order=True)
    assert lib.calls[-1][0] == 'eincm_set_windows_weighted' and lib.calls[-1][-1] == L.SW_KEEP_ORDER and lib.calls[-1][-2] is not None
    with pytest.raises(Reached):
        stub_engine(lib).set_windows([win, win])                                   # without the keyword: the entry point and flags of before
    assert lib.calls[-1][0] == 'eincm_set_windows_ptrs' and lib.calls[-1][-1] == 0


def test_the_applying_e_step_hands_over_its_flags_and_downloads_nothing_per_event():
    lib = Records()
    for kw, eng in ((dict(), stub_engine(lib, n=(4, 4))), (dict(want=()), stub_engine(lib, n=(4, 4))),
                    (dict(want=('weights', 'labels', 'mass', 'n_unsupported'), exclude_self=False), stub_engine(lib, n=(4, 4)))):
        with pytest.raises(Reached):
            eng.apply_responsibilities(2, **kw)
        name, _, K, images, rw, w_in, prior, flags, w_out, labels, mass, n_uns = lib.calls[-1]
        want = kw.get('want', ('labels', 'mass'))
        assert name == 'eincm_event_responsibilities' and K == 2 and w_in is None
        assert flags == (L.RS_APPLY | ((L.RS_EXCLUDE_SELF | L.RS_STAGED_WEIGHTS) if kw.get('exclude_self', True) else 0))
        assert [(o is not None) for o in (w_out, labels, mass, n_uns)] == [k in want for k in E.RS_OUTPUTS]
    # the plain E-step on a keep-order batch reads the staged weights on the device; on any other batch it is the call of before
    with pytest.raises(Reached):
        stub_engine(lib, n=(4, 4)).event_responsibilities(2)
    assert lib.calls[-1][7] == L.RS_EXCLUDE_SELF | L.RS_STAGED_WEIGHTS and lib.calls[-1][5] is None
    with pytest.raises(Reached):
        stub_engine(lib, n=(4, 4), keep_order=False).event_responsibilities(2)
    assert lib.calls[-1][7] == L.RS_EXCLUDE_SELF
    p = inspect.signature(apply_responsibilities).parameters
    assert list(p) == ['self', 'n_models', 'images', 'ref_weights', 'prior', 'exclude_self', 'want']
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, True, ('labels', 'mass')]
    with pytest.raises(ValueError, match='want'):
        stub_engine(n=(4, 4)).event_responsibilities(2, want=())                   # only the applying form may fetch nothing


# ---- the in-place EM driver ---------------------------------------------------------------------------------------------------------
def test_check_segment_args_accepts_in_place():
    model = motion.MotionModel('translation', (5, 7))
    win = (np.zeros(3, np.int16), np.zeros(3, np.int16), np.linspace(0, 1, 3), np.zeros((2, 5, 7)), np.array([0.0, 1.0]))
    good = np.array([[[1.0, 0.0], [0.0, 1.0]]])
    for kw in (dict(), dict(in_place=False), dict(in_place=True), dict(in_place=True, record_weights=False)):
        c, w0 = segmentation.check_segment_args([win], model, good, 3, None, 'mass', 1.0, **kw)
        assert np.array_equal(c, good) and w0 is None
    p = inspect.signature(segmentation.check_segment_args).parameters
    assert p['in_place'].default is False and p['record_weights'].default is True
    for kw, match in ((dict(in_place=1), 'True or False'), (dict(in_place='yes'), 'True or False'), (dict(in_place=True, record_weights=None), 'True or False'),
                      (dict(in_place=False, record_weights=False), 'in_place=True')):
        with pytest.raises(ValueError, match=match):
            segmentation.check_segment_args([win], model, good, 3, None, 'mass', 1.0, **kw)


def test_the_in_place_driver_has_segment_motions_arguments_and_refuses_the_same():
    ref = inspect.signature(segmentation.segment_motions).parameters
    p = inspect.signature(segment_motions_in_place).parameters
    assert list(p) == list(ref) + ['record_weights'] and p['record_weights'].default is True
    assert [p[k].default for k in ref] == [ref[k].default for k in ref]
    model = motion.MotionModel('translation', (5, 7))
    win = (np.zeros(3, np.int16), np.zeros(3, np.int16), np.linspace(0, 1, 3), np.zeros((2, 5, 7)), np.array([0.0, 1.0]))
    good = np.array([[[1.0, 0.0], [0.0, 1.0]]])
    for kw, match in ((dict(windows=[]), 'at least one'), (dict(coeffs0=np.array([[[1.0, 2.0], [1.0, 2.0]]])), 'never separate'), (dict(n_iters=0), 'n_iters'),
                      (dict(weights0=[[np.ones(3), np.ones(2)]]), r'\(3,\)'), (dict(record_weights=0), 'True or False')):
        a = dict(windows=[win], coeffs0=good)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            segment_motions_in_place(NoGpu(), a.pop('windows'), model, a.pop('coeffs0'), None, **a)


class _Script:
    """An engine that records what the EM drivers ask of it and answers with fixed responsibilities."""
    def __init__(self, n, K):
        self.calls, self.n, self.K, self.keep_order = [], n, K, False

    def set_motion_model(self, model): pass
    def set_motion_path(self, path): pass

    def set_windows(self, windows, keep_order=False):
        self.keep_order = keep_order
        self.calls.append(('set_windows', keep_order, [None if len(w) == 5 or w[5] is None else np.array(w[5]) for w in windows]))

    def set_weights(self, weights):
        self.calls.append(('set_weights', [np.array(w) for w in weights]))

    def loss_grad_motion(self, coeffs, params, **kw):
        self.calls.append(('loss_grad_motion',))

    def _answer(self, want):
        w = [np.full(self.n, (l + 1) / 4.0, np.float32) for l in range(self.K)]
        full = dict(weights=w, labels=[np.zeros(self.n, np.uint8)], mass=np.array([[3.0, 2.0]]), n_unsupported=np.zeros(1, np.int64))
        self.device_weights = w
        return {k: full[k] for k in want}

    def event_responsibilities(self, K, prior=None, exclude_self=True, want=()):
        self.calls.append(('event_responsibilities', tuple(want)))
        return self._answer(want)

    def apply_responsibilities(self, K, prior=None, exclude_self=True, want=()):
        self.calls.append(('apply_responsibilities', tuple(want)))
        return self._answer(want)

    def staged_weights(self):
        self.calls.append(('staged_weights',))
        return self.device_weights


@pytest.mark.parametrize('with_weights0', [False, True])
def test_the_in_place_driver_stages_once_and_lets_the_e_step_apply(monkeypatch, with_weights0):
    model = motion.MotionModel('translation', (5, 7))
    win = (np.zeros(3, np.int16), np.zeros(3, np.int16), np.linspace(0, 1, 3), np.zeros((2, 5, 7)), np.array([0.0, 1.0]))
    good = np.array([[[1.0, 0.0], [0.0, 1.0]]])
    monkeypatch.setattr(batch_solver, 'minimize_motion', lambda eng, model, c, *a, **kw: [None] * len(c))
    w0 = [[np.full(3, 0.25, np.float32), np.full(3, 0.75, np.float32)]] if with_weights0 else None
    runs = {}
    for name, drive, kw in (('restage', segmentation.segment_motions, {}), ('in_place', segment_motions_in_place, {}),
                            ('unrecorded', segment_motions_in_place, dict(record_weights=False))):
        eng = _Script(3, 2)
        runs[name] = (drive(eng, [win], model, good, None, n_iters=2, weights0=w0, **kw), [c[0] for c in eng.calls], eng.calls)
    hist, names, calls = runs['in_place']
    assert names.count('set_windows') == 1 and calls[names.index('set_windows')][1] is True and names.count('event_responsibilities') == 0
    assert all(w is None for w in calls[names.index('set_windows')][2])            # the windows as they are: weights0 goes in through set_weights
    assert names.count('set_weights') == (1 if with_weights0 else 0)
    assert names.count('apply_responsibilities') == (2 if with_weights0 else 3)
    assert all('weights' not in c[1] for c in calls if c[0] == 'apply_responsibilities')      # nothing per-event but the labels comes down
    assert names.count('staged_weights') == 2 and runs['unrecorded'][1].count('staged_weights') == 0
    assert [r['weights'] for r in runs['unrecorded'][0]] == [None, None]
    ref, ref_names, ref_calls = runs['restage']
    assert ref_names.count('set_windows') == (2 if with_weights0 else 3) and not any(c[1] for c in ref_calls if c[0] == 'set_windows')
    assert 'set_weights' not in ref_names and 'apply_responsibilities' not in ref_names
    for a, b in zip(hist, ref):
        assert sorted(a) == sorted(b)
        for k in ('coeffs', 'mass', 'n_unsupported', 'active'):
            assert np.array_equal(a[k], b[k])
        assert all(np.array_equal(x, y) for x, y in zip(a['weights'][0], b['weights'][0]))
