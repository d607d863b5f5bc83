"""Staging's payload states against the commit before they got one owner: byte equality with a recording.

tests/test_gpu_reweight.py compares the engine with itself (set_weights against a fresh staging); a change to both sides needs an
outside reference.  tests/golden/staging_payload/parent.json holds what the build of the commit it names answered on the batch of
tests/_reweight_scene.py (64 x 96, 2 x 3 tiles, R = 2, B = 4 with 3000 / 300 / 0 / 700 events) in the four payload situations - plain;
weighted with w1; keep-order with w1; keep-order with w1, then set_weights(w2) - under the four launch settings - default,
EINCM_HOST_BINNING=1, EINCM_NO_SEGSORT=1, EINCM_NO_SPREAD=1: everything RS.answers() collects and, for the keep-order situations,
staged_order() and staged_weights().  The engine is bit-reproducible, so nothing here has a tolerance.  Each setting runs once, in a
child process (tests/_staging_payload.py); tools/record_staging_payload.py writes the recording."""
import json
import os

import pytest

import _staging_payload as SP

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'staging_payload', 'parent.json')
_computed = {}


def _recording():
    assert os.path.exists(GOLDEN), f'{GOLDEN} is missing: tools/record_staging_payload.py writes it, on a build of the parent commit'
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert len(rec['recorded_by']) >= 7 and rec['settings'] == dict(SP.SETTINGS)
    return rec


def _compute(tag, tmp_path_factory):
    if tag not in _computed:
        _computed[tag] = SP.run_setting(dict(SP.SETTINGS)[tag], str(tmp_path_factory.mktemp('payload') / f'{tag}.json'))
    return _computed[tag]


def test_the_recording_names_its_commit_and_holds_every_case():
    rec = _recording()
    assert sorted(rec['cases']) == sorted(t for t, _ in SP.SETTINGS)
    for tag, cases in rec['cases'].items():
        assert sorted(cases) == sorted(SP.SITUATIONS), tag
        for name, case in cases.items():
            assert ('staged_order' in case) == ('staged_weights' in case) == name.startswith('keep_order'), (tag, name)
            assert len(case['answers']) == 16, (tag, name)
    d = rec['cases']['default']
    assert d['weighted']['answers'] != d['plain']['answers']                       # the weights are seen,
    assert d['keep_order']['answers'] == d['weighted']['answers']                  # keeping the order changes no answer,
    assert d['keep_order_reweighted']['answers'] != d['keep_order']['answers']     # and the second set is another one


@pytest.mark.parametrize('situation', SP.SITUATIONS)
@pytest.mark.parametrize('tag', [t for t, _ in SP.SETTINGS])
def test_staging_answers_with_the_recorded_bytes(built_lib, tmp_path_factory, tag, situation):
    want = _recording()['cases'][tag][situation]
    got = _compute(tag, tmp_path_factory)[situation]
    diff = list(SP.differences(got, want))
    assert not diff, f'{tag} / {situation}: {len(diff)} entries differ from the recording:\n' + '\n'.join(diff[:20])
    assert got == want
