"""The serving stack's host path hands on what it handed on before it was folded into one options record: the handler in five
server configurations, server.run()'s generate_fn and the engine's text front, for every request option and every pair, against
the recording in tests/golden/serving_calls.json (written by tests/golden/gen_golden_serving_calls.py; no model, no GPU)."""
import json

import pytest

import gen_golden_serving_calls as gen


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
    with pytest.MonkeyPatch.context() as mp:
        return gen.record_all(mp.setattr)


def same(got, want):
    got = json.loads(json.dumps(got, sort_keys=True))               # (tuples -> lists, as the file has them)
    assert sorted(got) == sorted(want)
    for group in want:
        assert sorted(got[group]) == sorted(want[group]), group
        for case in want[group]:
            assert got[group][case] == want[group][case], (group, case)


def test_the_matrix_covers_every_option_and_pair():
    names = set(gen.bodies())
    n = len(gen.OPTIONS)
    assert len([c for c in names if not c.startswith("bad:") and "+" in c]) == n * (n - 1) // 2
    assert set(gen.OPTIONS) | {"plain"} <= names and sum(c.startswith("bad:") for c in names) == sum(map(len, gen.BAD.values()))


def test_handler_calls_in_five_configurations(got, golden):
    assert sorted(got["http"]) == ["continuous", "continuous_store", "merge", "queue", "sharded_spec"]
    same(got["http"], golden["http"])
    # the first rule the ladders encode, read off the recording: a plain request reaches a stub with no keyword at all
    for group, pos in (("queue", 2), ("merge", 2), ("continuous", 4)):
        call = got["http"][group]["plain"][2][0]
        assert call["pos"] == pos and call["kw"] == []


def test_run_generate_fn_calls(got, golden):
    same(got["run"], golden["run"])
    assert got["run"]["run"]["plain"][2][0]["kw"] == ["max_tokens", "verbose"]


def test_engine_level_calls(got, golden):
    same(got["engine"], golden["engine"])
    for group in ("text", "router", "text_store", "router_store"):
        call = got["engine"][group]["plain"]["calls"][0]
        assert call["same_object"] and call["keys"] == [] and call["kw"] == {}
    assert all(got["engine"]["router_submit"][c][0]["same_object"] for c in ("plain", "sampling", "adapter", "carriers"))


def test_the_recording_is_byte_for_byte_what_the_generator_writes(got):
    with open(gen.PATH) as f:
        assert gen.dumps(got) == f.read()
