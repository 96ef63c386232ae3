"""steps.py: the eight kinds of the captured decode step, their names, the selector and the methods made from the table (no GPU)."""
import itertools
import sys
import types

import pytest

from phi_3_vision_mlx_amd import steps

NAMES = {"greedy_step": "graph", "sample_step": "sample_graph", "logprob_step": "logprob_graph",
         "sample_logprob_step": "sample_logprob_graph", "penal_step": "penal_graph", "penal_logprob_step": "penal_logprob_graph",
         "guide_step": "guide_graph", "guide_logprob_step": "guide_logprob_graph"}
FLAGS16 = list(itertools.product([False, True], repeat=4))


def test_sixteen_flag_combinations_are_eight_kinds_with_the_sixteen_names():
    kinds = {steps.StepKind(*f) for f in FLAGS16}
    assert len(kinds) == 8 and kinds == set(steps.ALL) and len(steps.ALL) == 8
    for k in kinds:
        assert (not k.guided or k.penalized) and (not k.penalized or k.sampled)
        with pytest.raises(Exception):
            k.sampled = not k.sampled                                                 # immutable
    assert {k.method: k.capture for k in steps.ALL} == NAMES
    assert len({k.method for k in steps.ALL}) == 8 and len({k.capture for k in steps.ALL}) == 8
    assert steps.GREEDY.method == "greedy_step" and steps.StepKind() == steps.GREEDY
    # dropping by a flag: `penalized` takes the guided captures with it
    assert {k.capture for k in steps.with_flag("penalized")} == {"penal_graph", "penal_logprob_graph", "guide_graph", "guide_logprob_graph"}
    assert {k.capture for k in steps.with_flag("guided")} == {"guide_graph", "guide_logprob_graph"}


def test_steps_does_not_import_torch():
    import subprocess
    code = "import sys, importlib.util as u; s = u.spec_from_file_location('steps', sys.argv[1]); m = u.module_from_spec(s); " \
           "sys.modules['steps'] = m; s.loader.exec_module(m); assert 'torch' not in sys.modules and 'numpy' not in sys.modules"
    subprocess.run([sys.executable, "-c", code, steps.__file__], check=True)


def _if_chain(sampled, penalized, guided, scored):
    """ContinuousEngine.step's choice as it was written before the table: assign, then overwrite."""
    replay = "sample_step" if sampled else "greedy_step"
    if penalized:
        replay = "penal_step"
    if guided:
        replay = "guide_step"
    if scored:
        replay = "sample_logprob_step" if sampled else "logprob_step"
        if penalized:
            replay = "penal_logprob_step"
        if guided:
            replay = "guide_logprob_step"
    return replay


@pytest.mark.parametrize("flags", FLAGS16)
def test_selector_against_the_if_chain(flags):
    assert steps.kind_for(*flags).method == _if_chain(*flags)
    assert steps.kind_for(*(1 if f else 0 for f in flags)) == steps.kind_for(*flags)   # (truthy values: the same kind)


def _model_class():
    @steps.methods()
    class M:
        def __init__(self):
            self.seen = []

        def _replay(self, token, cache, kind):
            self.seen.append((token, kind))
            return "logits", "next"
    return M


def _cache(**attrs):
    st = types.SimpleNamespace(**{**dict(sample_rows=None, penalty=None, guide=None, logprob_want=None), **attrs})
    return [types.SimpleNamespace(state=st)]


def test_a_class_built_from_the_table_has_the_eight_methods_each_with_its_kind():
    M = _model_class()
    m = M()
    full = _cache(sample_rows=1, penalty=1, guide=1, logprob_want=1)
    for k in steps.ALL:
        assert getattr(M, k.method).__name__ == k.method and getattr(M, k.method).__doc__
        assert getattr(m, k.method)("tok", full) == ("logits", "next")
        assert m.seen[-1] == ("tok", k)
    assert [k for _, k in m.seen] == list(steps.ALL)
    wrapped = []

    @steps.methods(lambda fn: wrapped.append(fn.__name__) or fn)
    class W:
        pass
    assert wrapped == [k.method for k in steps.ALL]


ATTRS = {"sampled": "sample_rows", "penalized": "penalty", "guided": "guide", "logprobs": "logprob_want"}
SETTERS = {"sample_rows": "set_sampling", "penalty": "set_penalties", "guide": "set_guides", "logprob_want": "set_logprobs"}


@pytest.mark.parametrize("kind", steps.ALL, ids=lambda k: k.method)
def test_a_method_raises_when_the_state_lacks_what_its_kind_needs_and_only_then(kind):
    m = _model_class()()
    needed = {a for f, a in ATTRS.items() if getattr(kind, f)}
    for present in itertools.product([False, True], repeat=4):
        have = {a for a, p in zip(ATTRS.values(), present) if p}
        cache = _cache(**{a: object() for a in have})
        del m.seen[:]
        if needed <= have:
            getattr(m, kind.method)("tok", cache)
            assert len(m.seen) == 1
        else:
            with pytest.raises(RuntimeError) as e:
                getattr(m, kind.method)("tok", cache)
            assert not m.seen                                                         # nothing was replayed
            assert kind.method in str(e.value)
            assert {s for s in SETTERS.values() if s in str(e.value)} == {SETTERS[a] for a in needed - have}


@pytest.mark.parametrize("flag", steps.FLAGS)
def test_making_one_option_s_table_makes_exactly_what_needs_names_for_it(flag):
    """The model's one make-or-get helper and CacheState's properties follow steps.NEEDS: a state that had only one option's table
    made reports that attribute, and no other, as made -- an option added to the table alone (or to the model alone) fails here."""
    from phi_3_vision_mlx_amd.model import CacheState, Phi3VModel, _records
    assert [f for f, _, _ in steps.NEEDS] == list(steps.FLAGS)
    me = types.SimpleNamespace(cfg=types.SimpleNamespace(vocab_size=40), device="cpu", _drop_captures=Phi3VModel._drop_captures)
    st = object.__new__(CacheState)
    st.B, st.shared, st.graphs = 3, {}, {"greedy": {k.capture: object() for k in steps.ALL}}
    assert all(getattr(st, attr) is None for _, attr, _ in steps.NEEDS)
    made = Phi3VModel._option_table(me, st, flag)
    assert {attr for _, attr, _ in steps.NEEDS if getattr(st, attr) is not None} == {ATTRS[flag]}
    assert getattr(st, ATTRS[flag]) is made and _records(made).shape[0] == 3
    assert Phi3VModel._option_table(me, st, flag) is made                             # (the second call gets, it does not make)
    # what baked the old pointer (or its absence) in is gone: the captures of the kinds with that flag, and no others
    assert set(st.graphs["greedy"]) == {k.capture for k in steps.ALL if not getattr(k, flag)}
    for k in steps.ALL:
        assert (k.missing(st) == []) == (not any(getattr(k, f) for f in steps.FLAGS if f != flag)), k


def test_the_model_class_has_the_table_s_methods_and_each_reaches_replay_with_its_kind():
    from phi_3_vision_mlx_amd.model import Phi3VModel
    seen = []
    me = types.SimpleNamespace(_replay=lambda token, cache, kind: seen.append(kind) or ("logits", "next"))
    full = _cache(sample_rows=1, penalty=1, guide=1, logprob_want=1)
    for k in steps.ALL:
        fn = getattr(Phi3VModel, k.method)
        assert fn.__name__ == k.method and fn.__doc__
        inner = fn.__wrapped__                                                        # (under the model's device guard)
        assert inner(me, "tok", full) == ("logits", "next")
        if k != steps.GREEDY:
            with pytest.raises(RuntimeError, match=k.method):
                inner(me, "tok", _cache())
    assert seen == list(steps.ALL)
