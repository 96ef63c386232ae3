"""The callers of the decode step -- ContinuousEngine, api.greedy_loop and api._generate around it -- make the calls on the model
that tests/golden/step_calls.json records: every combination of sampling, penalties, guide and logprobs, in six engine situations,
in the loop, and in _generate for one prompt, two prompts and n = 3 (written by tests/golden/gen_golden_step_calls.py; no model,
no GPU).  The engine and loop parts are as recorded before steps.py; since row_options.py the family's setters come in the group's
order, and _generate makes the engine's calls for the first token (set_sampling + sample_logits, set_logprobs + logprobs_of)."""
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
    assert len(got["generate"]) == 16 and all(sorted(v) == ["n3", "one", "two"] for v in got["generate"].values())
    # every step method is taken somewhere, and a plain request is driven by the greedy step alone
    assert {s for v in got["engine"].values() for c in v.values() for s in c["steps"]} == set(gen.STEPS)
    assert {s for c in got["loop"]["cpu"].values() for s in c["steps"]} == set(gen.STEPS)
    assert {s for v in got["generate"].values() for c in v.values() for s in c["steps"]} == set(gen.STEPS)
    assert set(got["engine"]["plain"]["alone"]["steps"]) == {"greedy_step"}


@pytest.mark.parametrize("part", ["engine", "loop", "generate"])
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
