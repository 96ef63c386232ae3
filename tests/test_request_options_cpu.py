"""request.RequestOptions: one record of a request's options, one reader and one writer of what rides beside its inputs."""
import dataclasses
import itertools
import pickle

import numpy as np
import pytest

from phi_3_vision_mlx_amd import engine
from phi_3_vision_mlx_amd.request import RequestOptions

INF = float("inf")

# one value of every option (fields of the record); a pair is the union of two
OPTIONS = {
    "sampling": dict(sampling={"temperature": 0.7, "top_k": 5, "seed": 11}),
    "adapter": dict(adapter="a1"),
    "logprobs": dict(logprobs=2),
    "logprobs0": dict(logprobs=0),
    "penalties": dict(penalties={"repetition_penalty": 1.3, "logit_bias": {"5": -2.0}}),
    "n": dict(n=3),
    "best_of": dict(n=2, best_of=4),
    "best_of_alone": dict(best_of=4),
    "image_digests": dict(image_digests=["d1"]),
    "no_cache": dict(cache_prompt=False),
    "prefix_len": dict(prefix_len=7),
}


class Recorder:
    def submit(self, *args, **kw):
        self.args, self.kw = args, kw
        return "handle"


def inputs():
    return {"input_ids": np.zeros((1, 4), dtype=np.int64), "image_sizes": np.asarray([[336, 336]])}


def records():
    yield "plain", RequestOptions()
    for a in OPTIONS:
        yield a, RequestOptions(**OPTIONS[a])
    for a, b in itertools.combinations(OPTIONS, 2):
        yield f"{a}+{b}", RequestOptions(**{**OPTIONS[a], **OPTIONS[b]})


@pytest.mark.parametrize("name,opts", list(records()), ids=[n for n, _ in records()])
def test_what_send_writes_read_reads_back(name, opts):
    stub, x = Recorder(), inputs()
    assert opts.send(stub, x, 9) == "handle"
    written, max_tokens = stub.args
    assert max_tokens == 9 and set(stub.kw) == {k for k in ("sampling", "adapter") if getattr(opts, k) is not None}
    assert RequestOptions.read(written, **stub.kw) == opts
    assert set(x) == {"input_ids", "image_sizes"}                # the processor's own result is never touched
    assert pickle.loads(pickle.dumps(opts)) == opts
    if name != "plain":
        assert opts != RequestOptions()


def test_a_plain_record_sends_the_callers_own_inputs_and_nothing_else():
    stub, x = Recorder(), inputs()
    RequestOptions().send(stub, x, 5)
    assert stub.args[0] is x and stub.args[1:] == (5,) and stub.kw == {}
    # sampling and adapter are keywords: the inputs stay the caller's object
    RequestOptions(sampling={"seed": 1}, adapter="a1").send(stub, x, 5)
    assert stub.args[0] is x and stub.kw == {"sampling": {"seed": 1}, "adapter": "a1"}
    # what counts as "not asked": n = 1, cache_prompt True
    RequestOptions(n=1, cache_prompt=True).send(stub, x, 5)
    assert stub.args[0] is x


def test_the_four_public_helpers_return_what_they_returned():
    x = {"input_ids": 1}
    assert engine.cache_args(x) == {"input_ids": 1, "prefix_cache_args": {"image_digests": None, "cache_prompt": True, "prefix_len": None}}
    assert engine.cache_args(x, ["d"], False, 7) == {"input_ids": 1, "prefix_cache_args": {"image_digests": ["d"], "cache_prompt": False, "prefix_len": 7}}
    assert engine.cache_args(x, cache_prompt="no")["prefix_cache_args"]["cache_prompt"] == "no"      # (unchecked: `submit` checks)
    assert engine.logprob_args(x, 3) == {"input_ids": 1, "logprobs": 3}
    assert engine.logprob_args(x, None) == {"input_ids": 1, "logprobs": None}
    assert engine.penalty_args(x) == {"input_ids": 1, "penalties": {"repetition_penalty": 1.0, "presence_penalty": 0.0,
                                                                    "frequency_penalty": 0.0, "logit_bias": None}}
    assert engine.penalty_args(x, 1.2, 0.1, 0.2, {"5": -1.0}) == {"input_ids": 1, "penalties": {
        "repetition_penalty": 1.2, "presence_penalty": 0.1, "frequency_penalty": 0.2, "logit_bias": {"5": -1.0}}}
    assert engine.n_args(x, 3) == {"input_ids": 1, "n_completions": {"n": 3, "best_of": None}}
    assert engine.n_args(x, 2, 5) == {"input_ids": 1, "n_completions": {"n": 2, "best_of": 5}}
    assert x == {"input_ids": 1}
    assert (engine.PREFIX_ARGS, engine.LOGPROB_ARGS, engine.PENALTY_ARGS, engine.N_ARGS) == \
        ("prefix_cache_args", "logprobs", "penalties", "n_completions")
    tagged = engine.n_args(engine.penalty_args(engine.logprob_args(x, 1), presence_penalty=0.5), 2)
    assert engine.requested_logprobs(tagged) == 1 and engine.requested_n(tagged) == {"n": 2, "best_of": None}
    assert engine.requested_penalties(tagged)["presence_penalty"] == 0.5 and engine.requested_n(x) is None


def test_checked_normalises():
    got = RequestOptions.read(engine.n_args(engine.logprob_args(engine.penalty_args(inputs(), frequency_penalty=0.5), 2), 2, 4),
                              {"temperature": 0.7, "seed": 3}, "a1").checked(["a1"], 100, inputs())
    assert got == RequestOptions(sampling=(0.7, 0, 1.0, 3), adapter="a1", logprobs=2, penalties=(1.0, 0.5, 0.0, None), n=2, best_of=4)
    assert got.m == 4 and RequestOptions().checked([]) == RequestOptions() and RequestOptions().m == 1
    # all defaults: a plain request; a tuple passes as the record it is
    assert RequestOptions.read(engine.penalty_args(inputs())).checked([]).penalties is None
    assert RequestOptions(sampling=(0.5, 3, 0.9, 7)).checked([]).sampling == (0.5, 3, 0.9, 7)
    assert RequestOptions(n=3).checked([]).m == 3 and RequestOptions(n=2, best_of=2).checked([]).m == 2
    # the Request keeps the checked values as plain attributes
    r = engine.Request(inputs(), 4, dataclasses.replace(got, image_digests=["d"], cache_prompt=False, prefix_len=3))
    assert (r.sampling, r.adapter, r.logprobs, r.asked_logprobs, r.penalties) == ((0.7, 0, 1.0, 3), "a1", 2, 2, (1.0, 0.5, 0.0, None))
    assert (r.image_digests, r.cache_prompt, r.prefix_len, r.n, r.family) == (["d"], False, 3, 1, None)


# every value that fails a handle at `submit` (tests/test_logprobs_cpu.py, test_penalties_cpu.py, test_prefix_cache_cpu.py,
# test_parallel_sampling_cpu.py), with a word of the message it fails with
IMG = dict(inputs())
TEXT = {"input_ids": np.zeros((1, 4), dtype=np.int64)}
RAISING = [(engine.logprob_args(TEXT, bad), "0..8") for bad in (True, False, 1.0, "3", -1, 9, [1, 2, 3], [1, "a"], [True], [1])] + [
    (engine.penalty_args(TEXT, repetition_penalty=0.0), "repetition_penalty must be finite and > 0"),
    (engine.penalty_args(TEXT, frequency_penalty=INF), "frequency_penalty must be finite"),
    (engine.penalty_args(TEXT, logit_bias={"1000": 1.0}), "logit_bias key 1000 lies outside the vocabulary [0, 100)"),
    (engine.penalty_args(TEXT, logit_bias={"a": 1}), "logit_bias keys must be token ids"),
    (engine.cache_args(TEXT, image_digests="abc"), "image_digests must be a list of non-empty strings"),
    (engine.cache_args(TEXT, image_digests=["a"]), "1 digests for 0 images"),
    (engine.cache_args(TEXT, image_digests=[1]), "image_digests must be a list of non-empty strings"),
    (engine.cache_args(TEXT, prefix_len=0), "prefix_len must be a positive integer"),
    (engine.cache_args(TEXT, prefix_len=-3), "prefix_len must be a positive integer"),
    (engine.cache_args(TEXT, prefix_len=2.5), "prefix_len must be a positive integer"),
    (engine.cache_args(TEXT, prefix_len=True), "prefix_len must be a positive integer"),
    (engine.cache_args(TEXT, cache_prompt="no"), "cache_prompt must be True or False"),
    (engine.cache_args(IMG, image_digests=["a", "b"]), "2 digests for 1 images"),
    (dict(TEXT, prefix_cache_args={"extra": 1}), "prefix_cache_args must be what engine.cache_args makes"),
    (dict(TEXT, prefix_cache_args="x"), "prefix_cache_args must be what engine.cache_args makes"),
    (dict(TEXT, n_completions={"n": 0}), "1..16"),
    (dict(TEXT, n_completions={"n": 2, "best_of": 1}), "n..16"),
    (dict(TEXT, n_completions={"n": 2, "extra": 1}), "n_completions must be what engine.n_args makes"),
    (dict(TEXT, n_completions="3"), "n_completions must be what engine.n_args makes"),
]


@pytest.mark.parametrize("carried,word", RAISING, ids=[f"{i}:{w[:24]}" for i, (_, w) in enumerate(RAISING)])
def test_bad_values_raise_with_the_same_words(carried, word):
    with pytest.raises(ValueError) as e:
        RequestOptions.read(carried).checked(["a1"], 100, carried)
    assert word in str(e.value)


def test_bad_sampling_and_adapter_raise_with_the_same_words():
    for kw, word in ((dict(sampling={"temperature": -1}), "temperature must be finite and >= 0"),
                     (dict(sampling={"heat": 1}), "unknown sampling settings ['heat']"),
                     (dict(sampling={"top_p": 0}), "top_p must lie in (0, 1]"),
                     (dict(adapter=7), "adapter must be a name (string) or None, got int; known adapters: ['a1']"),
                     (dict(adapter="zz"), "unknown adapter 'zz'; known adapters: ['a1']")):
        with pytest.raises(ValueError) as e:
            RequestOptions.read(TEXT, **kw).checked(["a1"])
        assert word in str(e.value), kw


def test_options_per_prompt_keeps_the_normalisers_length_checks():
    from phi_3_vision_mlx_amd.request import options_per_prompt
    assert options_per_prompt(2) == [RequestOptions()] * 2
    got = options_per_prompt(2, [{"seed": 1}, {"seed": 2}], ["a1", None], [2, None], {"presence_penalty": 0.5}, False)
    assert got == [RequestOptions(sampling={"seed": 1}, adapter="a1", logprobs=2, penalties={"presence_penalty": 0.5}, cache_prompt=False),
                   RequestOptions(sampling={"seed": 2}, penalties={"presence_penalty": 0.5}, cache_prompt=False)]
    assert options_per_prompt(1, n=2, best_of=3) == [RequestOptions(n=2, best_of=3)]
    assert options_per_prompt(1, best_of=3) == [RequestOptions(n=1, best_of=3)]
    assert options_per_prompt(1, n=1) == options_per_prompt(1, n=1, best_of=1) == [RequestOptions()]    # a family of one: a plain request
    assert options_per_prompt(1, cache_prompt=True) == options_per_prompt(1, cache_prompt=None) == [RequestOptions()]
    for kw, word in ((dict(sampling=[{}]), "sampling: 1 records for 2 prompts"), (dict(adapter=["a"]), "adapter: 1 names for 2 prompts"),
                     (dict(adapter=7), "adapter must be a name, None, or a list of one per prompt, got int"),
                     (dict(logprobs=[1]), "logprobs: 1 values for 2 rows"), (dict(logprobs=True), "0..8"),
                     (dict(penalties=[None]), "penalties: 1 values for 2 prompts"), (dict(n=2), "one prompt (a string) per call"),
                     (dict(n=0), "1..16")):
        with pytest.raises(ValueError) as e:
            options_per_prompt(2, **kw)
        assert word in str(e.value), kw


def test_leaf_engines_walks_backend_fleet_router_engine():
    from types import SimpleNamespace as NS
    a, b = NS(name="a"), NS(name="b")
    router = NS(engines=[a, b])
    assert list(engine.leaf_engines(a)) == [a] and list(engine.leaf_engines(router)) == [a, b]
    assert list(engine.leaf_engines(NS(engine=NS(engine=router)))) == [a, b]          # a backend over a fleet over a router
    assert not engine.has_prefix_cache(router)
    b.prefix_cache = object()
    assert engine.has_prefix_cache(NS(engine=router)) and not engine.has_prefix_cache(a)
