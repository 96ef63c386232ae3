"""Guided decoding, host side (no GPU): the regex compiler against Python's `re`, the DFA's shape, the vocabulary table, a host
decode loop over the NumPy rule, and the plumbing of the new request field (RequestOptions, server parsing)."""
import itertools
import re

import numpy as np
import pytest

from phi_3_vision_mlx_amd import guide
from phi_3_vision_mlx_amd.processor import ByteTokenizer

EOS = 32007

# (pattern, alphabet): every supported construct; each alphabet holds a multi-byte character, and \n where it matters
PATTERNS = [
    ("abc", "abcé"),
    ("a|b|cé", "abcé"),
    ("a*", "abé"),
    ("a+b?", "abé"),
    ("(ab)*c", "abcé"),
    ("(?:a|b)+é", "abé"),
    ("a{2}", "abé"),
    ("a{1,}b", "abé"),
    ("a{1,3}", "abé"),
    ("(a|é){2,4}", "abé"),
    (".", "a\né"),
    ("a.b", "ab\né"),
    (".*", "a\né"),
    ("[ab]+", "abcé"),
    ("[a-c]x?", "acxé"),
    ("[^a]", "ab\né"),
    ("[^a\\n]*", "ab\né"),
    ("\\d+", "1a9é"),
    ("\\w\\s", "a_ é"),
    ("\\D", "1a\né"),
    ("\\W+", "a- é"),
    ("\\S\\s?", "a \né"),
    ("[\\d.]+", "1.aé"),
    ("[\\D]", "1aé"),
    ("\\n\\t?\\r?", "\n\t\ré"),
    ("\\x41\\.\\*", "A.*é"),
    ("é+|\\(a\\)", "é(a)"),
    ("(yes|no), [0-9]{1,3}\\.", "yeno, .19"),
    ("|a", "abé"),
    ("a{,2}b", "abé"),
    ("[]a]+", "]abé"),
    ("[a-]+", "a-bé"),
]


def _agree(pattern, dfa, s):
    want = re.fullmatch(pattern, s, re.ASCII) is not None
    assert dfa.matches(s) == want, f"{pattern!r} on {s!r}: re says {want}"


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=[p for p, _ in PATTERNS])
def test_compiler_agrees_with_re_exhaustively(pattern, alphabet):
    dfa = guide.compile_regex(pattern)
    chars = alphabet if len(alphabet) <= 4 else alphabet[:4]
    for n in range(6):
        for tup in itertools.product(chars, repeat=n):
            _agree(pattern, dfa, "".join(tup))
    rng = np.random.default_rng(len(pattern))
    for _ in range(300):
        n = int(rng.integers(0, 13))
        _agree(pattern, dfa, "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), n)))


def test_dot_and_negated_class_match_whole_code_points():
    dfa = guide.compile_regex(".")
    for ch in ("a", "é", "€", "\U0001F600"):
        assert dfa.matches(ch)
    for raw in (b"\xc3", b"\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82", b"\n"):
        assert not dfa.matches(raw), raw
    neg = guide.compile_regex("[^a]")
    assert neg.matches("€") and neg.matches("\n") and not neg.matches("a") and not neg.matches(b"\xe2\x82")


@pytest.mark.parametrize("pattern,word", [
    ("^a", "anchor"), ("a$", "anchor"), ("\\Aa", "anchor"), ("a\\Z", "anchor"), ("\\ba", "anchor"), ("a\\B", "anchor"),
    ("(a)\\1", "back-reference"), ("(?P<x>a)", "named group"), ("(?P=x)", "named group"),
    ("(?=a)", "look-around"), ("(?!a)", "look-around"), ("(?<=a)b", "look-around"), ("(?<!a)b", "look-around"),
    ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{1,2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
    ("[é]", "non-ASCII class member"), ("[a-é]", "non-ASCII class member"), ("[\\xe9]", "non-ASCII class member"),
    ("(?i)a", "group extension"), ("(a", "unbalanced"), ("a)", "unbalanced"), ("[a", "unterminated"), ("*a", "nothing to repeat"),
    ("a**", "multiple repeat"), ("a\\", "trailing backslash"), ("\\q", "escape"),
])
def test_unsupported_constructs_raise_naming_the_construct(pattern, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        guide.compile_regex(pattern)


def test_non_string_patterns_raise():
    for bad in (None, 3, b"a", ["a"]):
        with pytest.raises(ValueError):
            guide.compile_regex(bad)
    for bad in (None, [], "yes", [1], ["a", None]):
        with pytest.raises(ValueError):
            guide.compile_choice(bad)
    with pytest.raises(ValueError, match="exclude"):
        guide.compile_guide("a", ["a"])


def test_too_many_states_raises_with_the_count():
    assert guide.compile_regex("a{254}").n_states == 255
    with pytest.raises(ValueError, match="301 states"):
        guide.compile_regex("a{300}")
    with pytest.raises(ValueError, match="states"):
        guide.compile_regex("(a|b)*a(a|b){16}")


def _live(dfa):
    live = dfa.accept.astype(bool).copy()
    for _ in range(dfa.n_states + 1):
        live = live | live[dfa.delta].any(axis=1)
    return live


@pytest.mark.parametrize("pattern", [p for p, _ in PATTERNS])
def test_dfa_shape(pattern):
    dfa = guide.compile_regex(pattern)
    S = dfa.n_states
    assert 1 <= S <= 255 and dfa.delta.shape == (S + 1, 256) and dfa.accept.shape == (S + 1,)
    assert dfa.delta.dtype == np.uint16 and dfa.accept.dtype == np.uint8
    assert not dfa.delta[0].any() and dfa.accept[0] == 0                # state 0 is dead
    assert int(dfa.delta.max()) <= S
    live = _live(dfa)
    assert live[1:].all() and not live[0]                               # every state can reach an accepting one
    reach, todo = {1}, [1]                                              # ... and is reachable from the start, state 1
    while todo:
        for t in set(dfa.delta[todo.pop()].tolist()) - reach - {0}:
            reach.add(t)
            todo.append(t)
    assert reach == set(range(1, S + 1))


def test_minimisation_merges_equivalent_states():
    assert guide.compile_regex("(a|b)c|(b|a)c").n_states == guide.compile_regex("[ab]c").n_states == 3
    assert guide.compile_regex("a*").n_states == 1 and guide.compile_regex("(yes|no)").n_states == 5   # start, y, ye, n, end


def test_compile_choice_accepts_exactly_its_strings():
    choices = ["yes", "yes please", "no", "n", "a.b*", "é(1)", ""]
    dfa = guide.compile_choice(choices)
    for c in choices:
        assert dfa.matches(c)
    for s in ("ye", "yes ", "yes pleas", "nn", "aXb", "a.b**", "a.bb", "é", "é(1))", "no\n"):
        assert not dfa.matches(s), s
    assert guide.compile_choice(["a", "b"]) is guide.compile_choice(["a", "b"])       # the LRU cache of compiled guides


def test_lru_cache_is_bounded():
    first = guide.compile_regex("zz0")
    for i in range(guide.CACHE_SIZE + 3):
        guide.compile_regex(f"zz{i}")
    assert len(guide._cache) <= guide.CACHE_SIZE
    assert guide.compile_regex("zz0") is not first and guide.compile_regex("zz0").matches("zz0")


# ----------------------------------------------------------------------------- vocabulary tables
def test_token_bytes_byte_tokenizer():
    t = guide.token_bytes(ByteTokenizer(), 32064)
    assert t.n == 32064 and t.tok_off.dtype == np.uint32 and t.tok_off.shape == (32065,) and t.n_bytes == 256
    for i in (0, 1, 2, 259, 29871, 32000, EOS, 32063):
        assert t.bytes_of(i) == b""
    for i in range(3, 259):
        assert t.bytes_of(i) == bytes([i - 3])
    small = guide.token_bytes(ByteTokenizer(), 100)
    assert small.n == 100 and small.n_bytes == 97


class FakeSentencePiece:
    """A made-up sentencepiece-style vocabulary: specials, byte tokens, pieces with the space marker, multi-character pieces."""
    pieces = ["<unk>", "<s>", "</s>", "<0x00>", "<0xE2>", "<0x82>", "<0xAC>", "▁", "▁the", "ing", "é", "▁▁", "<|end|>", "a<0x41>"]
    all_special_ids = [0, 1, 2, 12]
    all_special_tokens = ["<unk>", "<s>", "</s>", "<|end|>"]

    def __len__(self):
        return len(self.pieces)

    def convert_ids_to_tokens(self, ids):
        return [self.pieces[i] for i in ids]


def test_token_bytes_sentencepiece_style():
    t = guide.token_bytes(FakeSentencePiece(), 20)
    want = [b"", b"", b"", b"\x00", b"\xe2", b"\x82", b"\xac", b" ", b" the", b"ing", "é".encode(), b"  ", b"", b"a<0x41>"]
    assert [t.bytes_of(i) for i in range(14)] == want
    assert all(t.bytes_of(i) == b"" for i in range(14, 20))             # ids beyond the tokenizer's own vocabulary
    lens, mat = t.padded()
    assert lens.tolist() == [len(w) for w in want] + [0] * 6 and mat.shape == (20, 7)
    # the euro sign is spelt by its three byte tokens
    dfa = guide.compile_regex("€+")
    guide.check(dfa, t, 12)
    with pytest.raises(ValueError, match="no token"):
        guide.check(guide.compile_regex("x"), t, 12)
    with pytest.raises(ValueError, match="eos"):
        guide.check(dfa, t, 99)
    with pytest.raises(ValueError):
        guide.token_bytes(object(), 10)


# ----------------------------------------------------------------------------- the rule in NumPy, and a host decode loop
def _bits(rng, n):
    return rng.integers(0, 1 << 16, n, dtype=np.uint16)


def test_reference_mask_rule_by_hand():
    table = guide.token_bytes(ByteTokenizer(), 301)
    eos = 300
    dfa = guide.compile_regex("ab?")
    delta, accept = guide.region(dfa)
    rng = np.random.default_rng(0)
    bits = _bits(rng, 301)
    tok = lambda ch: 3 + ord(ch)
    # inactive: untouched, state untouched
    out, st = guide.reference_mask(bits, [0, 7, 9, 0], delta, accept, table, tok("a"), eos)
    assert (out == bits).all() and st == 9
    # start state, nothing fed: only 'a'
    out, st = guide.reference_mask(bits, guide.record(dfa), delta, accept, table, None, eos)
    assert st == 1 and out[tok("a")] == bits[tok("a")] and (np.delete(out, tok("a")) == guide.NEG_INF).all()
    # fed 'a': 'b' and EOS
    out, st = guide.reference_mask(bits, guide.record(dfa), delta, accept, table, tok("a"), eos)
    keep = [tok("b"), eos]
    assert st == 2 and (out[keep] == bits[keep]).all() and (np.delete(out, keep) == guide.NEG_INF).all()
    # fed -1 or a token without bytes: the state stays
    for f in (-1, 0, 299, 10 ** 6):
        assert guide.reference_mask(bits, guide.record(dfa), delta, accept, table, f, eos)[1] == 1
    # fed EOS: DONE, only EOS
    out, st = guide.reference_mask(bits, guide.record(dfa, 2), delta, accept, table, eos, eos)
    assert st == guide.DONE and out[eos] == bits[eos] and (np.delete(out, eos) == guide.NEG_INF).all()
    # a banned token fed: state 0, masked as DONE
    out, st = guide.reference_mask(bits, guide.record(dfa), delta, accept, table, tok("z"), eos)
    assert st == 0 and out[eos] == bits[eos] and (np.delete(out, eos) == guide.NEG_INF).all()
    # records out of range: DONE, not written
    for rec in ([1, 0, 1, 0], [1, 256, 1, 0], [1, 2, 3, 0], [1, 2, 0, 0], [1, 2, -2, 0]):
        out, st = guide.reference_mask(bits, rec, delta, accept, table, tok("a"), eos)
        assert st == rec[2] and out[eos] == bits[eos] and (np.delete(out, eos) == guide.NEG_INF).all()


BOUNDED = ["(yes|no), [0-9]{1,3}\\.", "[0-9]{4}-[0-9]{2}-[0-9]{2}", "(é|ab){1,3}x?"]


@pytest.mark.parametrize("pattern", BOUNDED)
@pytest.mark.parametrize("seed", [None, 0, 1])
def test_host_loop_completes_bounded_patterns(pattern, seed):
    """reference_mask + arg-max (seed None) or a seeded draw over random logits: a bounded pattern's longest match is shorter
    than the budget, so every run ends with EOS and its bytes full-match; after EOS only EOS comes."""
    n, budget = 32064, 16
    table = guide.token_bytes(ByteTokenizer(), n)
    dfa = guide.compile_regex(pattern)
    guide.check(dfa, table, EOS)
    delta, accept = guide.region(dfa)
    rng = np.random.default_rng(1234 if seed is None else seed)
    rec, fed, out = guide.record(dfa), None, []
    for _ in range(budget):
        logits = rng.standard_normal(n).astype(np.float32)
        bits = (logits.view(np.uint32) >> 16).astype(np.uint16)
        masked, rec[2] = guide.reference_mask(bits, rec, delta, accept, table, fed, EOS)
        vals = (masked.astype(np.uint32) << 16).view(np.float32)
        if seed is None:
            fed = int(np.argmax(vals))
        else:
            p = np.exp(vals.astype(np.float64) - vals.max())
            fed = int(rng.choice(n, p=p / p.sum()))
        out.append(fed)
    assert EOS in out
    k = out.index(EOS)
    assert all(t == EOS for t in out[k:])
    data = b"".join(table.bytes_of(t) for t in out[:k])
    assert re.fullmatch(pattern, data.decode("utf-8"), re.ASCII), data
    assert guide.replay_state(dfa, table, out[:k], EOS) >= 1 and guide.replay_state(dfa, table, out, EOS) == guide.DONE


def test_per_prompt_arguments():
    assert guide.per_prompt(2) is None
    g = guide.per_prompt(2, regex="a+")
    assert g[0] is g[1] and g[0].matches("aa")
    g = guide.per_prompt(2, regex=["a", None], choice=[None, ["x", "y"]])
    assert g[0].matches("a") and g[1].matches("y")
    g = guide.per_prompt(2, choice=["x", "y"])
    assert g[0] is g[1] and g[0].matches("x")
    with pytest.raises(ValueError, match="exclude"):
        guide.per_prompt(1, regex="a", choice=["b"])
    with pytest.raises(ValueError, match="exclude"):
        guide.per_prompt(2, regex=["a", "b"], choice=[None, ["b"]])
    with pytest.raises(ValueError, match="2 prompts"):
        guide.per_prompt(2, regex=["a"])
    with pytest.raises(ValueError, match="speculate"):
        guide.refuse_speculation(guide.per_prompt(1, regex="a"), 2)
    guide.refuse_speculation(None, 2)
    guide.refuse_speculation(guide.per_prompt(1, regex="a"), 0)


# ----------------------------------------------------------------------------- plumbing: the request record, the server's fields
def test_request_options_round_trip_of_the_guide_carrier():
    from phi_3_vision_mlx_amd.engine import guide_args
    from phi_3_vision_mlx_amd.request import GUIDE_ARGS, RequestOptions
    inputs = {"input_ids": np.arange(5)[None]}
    assert guide_args(inputs) is inputs and GUIDE_ARGS not in inputs
    sent = guide_args(inputs, regex="a+")
    assert sent is not inputs and sent[GUIDE_ARGS] == {"regex": "a+"} and GUIDE_ARGS not in inputs
    opts = RequestOptions.read(sent)
    assert opts.guide == {"regex": "a+"} and RequestOptions.read(inputs).guide is None
    checked = opts.checked([])
    assert isinstance(checked.guide, guide.Dfa) and checked.guide.matches("aaa") and checked.checked([]).guide is checked.guide
    assert RequestOptions.read(guide_args(inputs, choice=("x", "y"))).checked([]).guide.matches("y")
    assert RequestOptions().checked([]).guide is None

    class Eng:                                                       # `send` writes the carrier back, and nothing for a plain request
        def submit(self, inputs, max_tokens, **kw):
            return inputs, kw
    got, kw = opts.send(Eng(), inputs, 4)
    assert got[GUIDE_ARGS] == {"regex": "a+"} and kw == {} and RequestOptions.read(got) == opts
    got, kw = RequestOptions().send(Eng(), inputs, 4)
    assert got is inputs and kw == {}
    with pytest.raises(ValueError, match="exclude"):
        guide_args(inputs, regex="a", choice=["b"])
    for bad in ({"regex": "a$"}, {"regex": 3}, {"choice": []}, {"choice": "ab"}, {"regex": "a", "choice": ["a"]}, {"json": "{}"}, "a+"):
        with pytest.raises(ValueError):
            RequestOptions(guide=bad).checked([])


def test_parse_guide_and_in_use():
    from phi_3_vision_mlx_amd.server import generate_kwargs, in_use, parse_guide
    assert parse_guide({}, 2) is None and parse_guide({"guided_regex": None, "guided_choice": None}, 1) is None
    assert parse_guide({"guided_regex": "a+"}, 2) == [{"regex": "a+"}] * 2
    assert parse_guide({"guided_choice": ["yes", "no"]}, 1) == [{"choice": ["yes", "no"]}]
    for bad, word in (({"guided_regex": 3}, "string"), ({"guided_regex": ["a"]}, "string"), ({"guided_choice": "yes"}, "non-empty list"),
                      ({"guided_choice": []}, "non-empty list"), ({"guided_choice": ["a", 1]}, "non-empty list"),
                      ({"guided_regex": "a", "guided_choice": ["a"]}, "exclude"), ({"guided_regex": "^a"}, "anchor"),
                      ({"guided_regex": "(?=a)"}, "look-around"), ({"guided_regex": "a{300}"}, "301 states")):
        with pytest.raises(ValueError, match=word):
            parse_guide(bad, 1)
    assert in_use() == {} and in_use(guide=None) == {}                  # a plain request passes nothing
    assert in_use(guide=[{"regex": "a"}]) == {"guide": [{"regex": "a"}]}
    assert generate_kwargs(None, None, None, None, None, None, 0, 1) == {}
    assert generate_kwargs(None, None, None, None, None, None, 0, 2, [{"regex": "a"}, None]) == {"guided_regex": ["a", None]}
    assert generate_kwargs(None, None, None, None, None, None, 0, 2, [{"choice": ["x"]}, {"regex": "b"}]) == \
        {"guided_regex": [None, "b"], "guided_choice": [["x"], None]}
    assert generate_kwargs(None, None, None, None, 2, None, 0, 1, [{"choice": ["x", "y"]}]) == {"guided_choice": ["x", "y"], "n": 2, "best_of": None}
    assert guide.per_prompt(2, regex=[None, "b"], choice=[["x"], None])[0].matches("x")


def _post(port, payload):
    import json
    import urllib.request
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


@pytest.mark.parametrize("merge", [True, False], ids=["merge", "solo"])
def test_server_carries_the_guide_and_answers_400(merge):
    import json
    import threading
    import urllib.error
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, **kw):
        calls.append(kw)
        out = [f"{p}|{max_tokens}" for p in prompts]
        return out[0] if len(out) == 1 else out

    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", merge=merge, max_tokens_cap=1000, vocab_size=64, speculate=True,
                          speculate_default=4)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    try:
        status, body = _post(port, {"prompt": ["a", "b"], "max_tokens": 5, "guided_regex": "[0-9]+"})
        assert status == 200 and body["responses"] == ["a|5", "b|5"]
        assert calls[-1] == {"guide": [{"regex": "[0-9]+"}] * 2}          # (the server-wide speculate default steps aside)
        assert _post(port, {"prompt": "c", "max_tokens": 5, "guided_choice": ["yes", "no"]})[0] == 200
        assert calls[-1] == {"guide": [{"choice": ["yes", "no"]}]}
        assert _post(port, {"prompt": "c", "max_tokens": 5, "temperature": 0})[0] == 200
        assert "guide" not in calls[-1]                                   # a plain request: nothing of the feature is passed
        for bad, word in (({"guided_regex": 5}, "string"), ({"guided_choice": []}, "non-empty"), ({"guided_choice": "x"}, "non-empty"),
                          ({"guided_regex": "a", "guided_choice": ["a"]}, "exclude"), ({"guided_regex": "a*?"}, "lazy"),
                          ({"guided_regex": "(a)\\1"}, "back-reference"), ({"guided_regex": "[é]"}, "non-ASCII"),
                          ({"guided_regex": "a{300}"}, "301 states"), ({"guided_regex": "a", "speculate": 4}, "speculative")):
            n = len(calls)
            with pytest.raises(urllib.error.HTTPError) as e:
                _post(port, dict({"prompt": "x", "max_tokens": 3}, **bad))
            assert e.value.code == 400 and word in json.loads(e.value.read())["error"], bad
            assert len(calls) == n                                        # nothing reached the engine
    finally:
        httpd.shutdown()
        engine.close()


def test_server_refuses_a_guide_on_the_sharded_path_and_the_continuous_backend_hands_it_on():
    import json
    import threading
    import urllib.error
    from phi_3_vision_mlx_amd.server import ContinuousBackend, serve
    httpd, engine = serve(lambda prompts, max_tokens, *a, **k: [f"{p}" for p in prompts], port=0, host="127.0.0.1",
                          sharded_fn=lambda prompts, images: True)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(httpd.server_address[1], {"prompt": "x", "guided_regex": "a"})
        assert e.value.code == 400 and "batch-sharded" in json.loads(e.value.read())["error"]
    finally:
        httpd.shutdown()
        engine.close()
    seen = {}

    class Eng:
        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def generate(self, prompts, images, max_tokens, timeout, **kw):
            seen.update(kw)
            return ["t"] * len(prompts)
    b = ContinuousBackend(Eng())
    try:
        assert b.submit(["p"], 4, guide=[{"regex": "a"}]) == ["t"] and seen == {"guide": [{"regex": "a"}]}
        seen.clear()
        b.submit(["p"], 4)
        assert seen == {}
    finally:
        b.close()


def test_generate_refuses_before_loading_a_model_and_keeps_the_package_signature():
    import inspect
    import phi_3_vision_mlx_amd as pkg
    from phi_3_vision_mlx_amd import api
    with pytest.raises(ValueError, match="speculate"):
        api.generate("hi", preload=(None, None), speculate=4, guided_regex="a", verbose=False)
    with pytest.raises(ValueError, match="anchor"):
        api.generate("hi", preload=(None, None), guided_regex="^a", verbose=False)
    with pytest.raises(ValueError, match="exclude"):
        api.generate("hi", preload=(None, None), guided_regex="a", guided_choice=["a"], verbose=False)
    sig = inspect.signature(api.generate).parameters
    assert sig["guided_regex"].default is None and sig["guided_choice"].default is None
    assert "guided_regex" not in inspect.signature(pkg.generate).parameters          # the package-level call keeps the reference's


# ----------------------------------------------------------------------------- engine bookkeeping on a stub model
def _guide_stub():
    from test_penalties_cpu import PenaltyStub

    class GuideStub(PenaltyStub):
        """PenaltyStub plus the guide calls, recorded: guided steps answer 300 + row."""
        cfg = type("Cfg", (), {"vocab_size": 32064})()

        def set_guide_vocab(self, table, eos):
            self.log.append(("vocab", table.n, eos))

        def set_guides(self, st, guides, row0=0, states=None):
            st.guide = True
            self.log.append(("guides", row0, [None if g is None else g.pattern for g in guides]))

        def clear_guides(self, st, row0=0, n=None):
            self.log.append(("clear_guides", row0, n))

        def guided_logits(self, st, logits, row0=0):
            self.log.append(("mask", row0))
            return logits

        def guide_step(self, token, cache):
            return self._step(cache, 300, "guide_step")
    return GuideStub()


def test_engine_sets_the_guide_before_the_first_token_and_clears_a_released_row():
    from test_penalties_cpu import _req
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, guide_args
    m = _guide_stub()
    proc = type("Proc", (), {"tokenizer": ByteTokenizer()})()
    e = ContinuousEngine(m, proc, slots=1, window=4096)
    a = e.submit(guide_args(_req(12, 1), regex="[0-9]+"), 3)
    b = e.submit(_req(12, 2), 3)                                      # takes over the one slot afterwards
    bad = e.submit(guide_args(_req(12, 3), regex="a$"), 3)
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and "anchor" in str(bad.error) and len(e.waiting) == 2
    e.run_until_idle()
    assert a.error is None and b.error is None
    assert isinstance(a.guide, guide.Dfa) and a.guide.matches("42") and b.guide is None
    assert a.tokens == [200, 300, 300] and b.tokens == [100, 100, 100]   # masked prefill pick, guided replays; b: plain ones
    names = [x[0] for x in m.log]
    assert names.index("vocab") < names.index("guides") < names.index("mask") < names.index("guide_step")
    assert m.log[names.index("guides")] == ("guides", 0, ["[0-9]+"]) and m.log[names.index("vocab")] == ("vocab", 32064, EOS)
    first_plain = names.index("greedy_step")
    assert "clear_guides" in names[:first_plain] and "guide_step" not in names[first_plain:]
    # world = 1: the fleet's own engine serves everything; a pattern that does not compile never reaches it
    front = fleet.EngineFleet(e, (None, None), 1)
    h = front.submit(guide_args(_req(8), regex="(?=a)"), 3)
    assert h.done.is_set() and isinstance(h.error, ValueError) and not e.waiting
    h = front.submit(guide_args(_req(8), choice=["yes", "no"]), 2)
    e.run_until_idle()
    assert h.error is None and h.tokens == [200, 300] and h.guide.matches("no")
