"""Every path of the loss's scalar assembly computes the bits it computed before the formula moved into csrc/eincm_loss.h.

tests/golden/loss_assembly/parent.npz was recorded on an MI355X from the commit before (tools/record_loss_assembly.py) on the cases of
tests/_loss_assembly_cases.py: value, gradient and every aux field of host assembly, k_final, k_final_dense, the float64 engine, the
objective kinds, the handover blend, objectives() and the device-resident entry point, with forward-only, masked and NaN-theta forms.
The assembly is plain fp64 arithmetic on sums whose order is fixed, so the comparison is array_equal (NaN equal to NaN).
"""
import os

import numpy as np
import pytest

import _loss_assembly_cases as A

pytestmark = pytest.mark.gpu

RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loss_assembly', 'parent.npz')
PARENT = dict(np.load(RECORDING, allow_pickle=False))
CASES = sorted({k.split('/')[0] for k in PARENT})


@pytest.fixture(scope='module')
def now(built_lib):
    return A.record()


def test_the_recording_holds_every_case(now):
    assert len(CASES) == 21
    assert sorted(now) == sorted(PARENT)


@pytest.mark.parametrize('case', CASES)
def test_bits_of_the_parent(now, case):
    keys = [k for k in PARENT if k.split('/')[0] == case]
    assert keys
    for k in keys:
        assert now[k].dtype == PARENT[k].dtype and now[k].shape == PARENT[k].shape, k
        assert np.array_equal(now[k], PARENT[k], equal_nan=True), (k, now[k], PARENT[k])
