"""The case table of test_gpu_transport.py crosses every transport limit of the sources: theta in the kernel arguments (THETA_ARG_MAX /
_MID / _BIG), zero-copy theta and results (ZERO_COPY_MAX), the gradient copied back in pieces (1 << 17 doubles) and Engine.loss_grad's
cached staging buffers.  The limits are read from the sources, so that moving one without moving the table fails here (no GPU needed)."""
import os
import re

from _transport_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'edge-informed-contrast-maximization_amd')


def _read(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def _const(src, name):
    m = re.search(r'constexpr\s+(?:int|size_t)\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'{name} not found'
    return int(m.group(1))


def limits():
    types = _read('csrc', 'eincm_types.h')           # the argument blocks' sizes, shared by the kernels and the planning
    plan = _read('csrc', 'eincm_plan.h')             # plan_eval decides where theta rides
    api = _read('csrc', 'eincm_api.hip')
    lim = {n: _const(types, n) for n in ('THETA_ARG_MAX', 'THETA_ARG_MID', 'THETA_ARG_BIG')}
    lim['ZERO_COPY_MAX'] = _const(plan, 'ZERO_COPY_MAX')
    # enqueue_result_copies: the gradient comes back in pieces from nd >= 1 << k, so the last nd of one copy is (1 << k) - 1
    pieces = set(re.findall(r'want_grad && \(size_t\)g\.B \* nth >= \(\(size_t\)1 << (\d+)\)', api))
    assert len(pieces) == 1, f'the piece threshold of enqueue_result_copies not found (or ambiguous): {pieces}'
    lim['GRAD_PIECES'] = (1 << int(pieces.pop())) - 1
    m = re.search(r'small = th\.size <= (\d+)', _read('engine.py'))
    assert m, "Engine.loss_grad's staging-buffer limit not found"
    lim['ENGINE_SMALL'] = int(m.group(1))
    return lim


def test_the_limits_are_where_the_table_was_made_for():
    """A sanity check of the parsing: every limit is found and they are ordered as the transport code assumes."""
    lim = limits()
    assert lim['THETA_ARG_MAX'] < lim['THETA_ARG_MID'] < lim['THETA_ARG_BIG'] < lim['ZERO_COPY_MAX'] < lim['GRAD_PIECES']


def test_every_limit_is_crossed_by_one_theta_shape():
    for name, lim in limits().items():
        shapes = [hw for hw in {c.hw for c in CASES}
                  if any(c.hw == hw and c.nd <= lim for c in CASES) and any(c.hw == hw and c.nd > lim for c in CASES)]
        assert shapes, f'no theta shape of the table has a case at nd <= {name} ({lim}) and one above it'


def test_the_two_assembly_and_copy_regimes_are_reached():
    """Every theta shape has cases; the dense shape reaches one copy (B == capacity), two copies (B < capacity) and pieces; a mask is
    tried with more than 64 windows (windows from 64 on are always evaluated) and in the piece regime; async in both regimes of the
    findings (2-DoF between THETA_ARG_MAX and THETA_ARG_BIG, gradient pieces)."""
    lim = limits()
    dense = [c for c in CASES if c.hw == (48, 64)]
    one_copy = [c for c in dense if lim['ZERO_COPY_MAX'] < c.nd <= lim['GRAD_PIECES'] and c.cap == c.B]
    two_copies = [c for c in dense if lim['ZERO_COPY_MAX'] < c.nd <= lim['GRAD_PIECES'] and c.cap > c.B]
    pieces = [c for c in CASES if c.nd > lim['GRAD_PIECES']]
    assert one_copy and two_copies and pieces
    assert any(c.mask for c in pieces) and any(c.run_async for c in pieces)
    bug1 = [c for c in CASES if c.hw == (1, 1) and lim['THETA_ARG_MAX'] < c.nd <= lim['THETA_ARG_BIG']]
    assert any(c.mask for c in bug1) and any(c.run_async for c in bug1) and any(c.tv for c in bug1)
    assert any(c.mask and c.B > 64 for c in CASES)
    assert any(c.tiny and c.B > 64 for c in CASES)
    assert len({c.id for c in CASES}) == len(CASES)
