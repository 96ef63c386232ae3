"""The callers of the decode step -- ContinuousEngine and api.greedy_loop -- make the calls on the model they made before the
eight step kinds were stated in one table: every combination of sampling, penalties, guide and logprobs, in six engine situations
and in the loop, against the recording in tests/golden/step_calls.json (written by tests/golden/gen_golden_step_calls.py from the
code as it stood before steps.py; no model, no GPU)."""
import json

import pytest

import gen_golden_step_calls as gen


@pytest.fixture(scope="module")
def golden():
    out = {}
    with open(gen.PATH) as f:
        for part, group, case, value in json.load(f):
            out.setdefault(part, {}).setdefault(group, {})[case] = value
    return out


@pytest.fixture(scope="module")
def got():
    """Recorded once from the code under test, shared by the tests below and left unchanged."""
    return gen.record_all()


def test_the_matrix_covers_every_combination_and_situation(got):
    assert len(gen.COMBOS) == 16 and len(set(gen.COMBOS)) == 16
    assert len(got["engine"]) == 16 and all(sorted(v) == sorted(gen.SITUATIONS) for v in got["engine"].values())
    assert len(got["loop"]["cpu"]) == 16
    # every step method is taken somewhere, and a plain request is driven by the greedy step alone
    assert {s for v in got["engine"].values() for c in v.values() for s in c["steps"]} == set(gen.STEPS)
    assert {s for c in got["loop"]["cpu"].values() for s in c["steps"]} == set(gen.STEPS)
    assert set(got["engine"]["plain"]["alone"]["steps"]) == {"greedy_step"}


@pytest.mark.parametrize("part", ["engine", "loop"])
def test_calls_on_the_model(got, golden, part):
    have = json.loads(json.dumps(got[part], sort_keys=True))
    assert sorted(have) == sorted(golden[part])
    for group in golden[part]:
        assert sorted(have[group]) == sorted(golden[part][group]), group
        for case, want in golden[part][group].items():
            assert have[group][case] == want, (group, case)


def test_the_recording_is_byte_for_byte_what_the_generator_writes(got):
    with open(gen.PATH) as f:
        assert gen.dumps(got) == f.read()
