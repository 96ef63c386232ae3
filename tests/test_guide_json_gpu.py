"""guided_json on the MI355X: the WIDE form of a guide row in p3v_guide_mask against guide.reference_mask BIT FOR BIT (logits and
records; wide, narrow, inactive and DONE rows in one launch, records out of range), the captured guided step with a wide and a
narrow row against eager launches, api.generate(guided_json=...) end to end under a schema of more than 255 states, the engine
with refilled rows and the server's fields."""
import json
import string
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import guide, penalties
from test_guide_gpu import (BATCH, CANARY16, EOS, KW, NEG_INF, PROMPT, _bf16_dev, _bits_of, _dev_table, _gen, _i32, _table, _text_of,  # noqa: F401
                            _vocab, _Watch, tiny)
from test_guide_json_cpu import validate

pytestmark = pytest.mark.gpu
N = 8192 + 309                                                   # off a multiple of 8,192: a full pass of 1024 x 8 and a ragged one
W, ACT = guide.WIDE | guide.ACTIVE, guide.ACTIVE


# ---------------------------------------------------------------------------------------------------- p3v_guide_mask
def _hand_built():
    """Wide guides no compiler gives: one exactly at the entry bound (S = 1023, C = 63: 1024 x 64 entries, even pitch), one of a
    single class (C = 1) and one where every byte is a class of its own (C = 256, forced wide at S = 254)."""
    S = 1023
    d = np.zeros((S + 1, 256), dtype=np.uint16)
    for s in range(1, S + 1):
        d[s, ord("a")] = d[s, ord("b")] = s + 1 if s < S else 0                 # a counter: a / b step by one,
        d[s, ord("c")] = s + 2 if s + 2 <= S else 0                               # c by two
    for k, b in enumerate([ord(","), 0xC3, 0xA9] + list(range(1, 44)) + list(range(200, 214))):           # 60 bytes with a column of their own
        d[k + 1, b] = 1 + (k % 3)
    acc = np.zeros(S + 1, dtype=np.uint8)
    acc[S] = acc[702] = 1
    bound = guide.Dfa(d, acc, "hand-built at the bound")
    assert bound.n_classes == 63 and (S + 1) * 64 == guide.WIDE_MAX_ENTRIES and guide.wide_pitch(S, 63) == 64
    S = 300
    d = np.zeros((S + 1, 256), dtype=np.uint16)
    d[1:S] = np.arange(2, S + 1, dtype=np.uint16)[:, None]                       # every byte steps by one
    acc = np.zeros(S + 1, dtype=np.uint8)
    acc[S] = 1
    one = guide.Dfa(d, acc, "one class")
    assert one.n_classes == 1 and guide.wide_pitch(S, 1) == 3
    S = 254
    d = np.zeros((S + 1, 256), dtype=np.uint16)
    for b in range(256):
        d[1 + b % S, b] = 1 + b // S
    d[:, ord("a")] = np.r_[0, np.arange(2, S + 1), 0]                            # ... and 'a' steps by one, a column of its own still
    d[1 + ord("a") % S, ord("a")] = 7
    acc = np.ones(S + 1, dtype=np.uint8)
    acc[0] = 0
    every = guide.Dfa(d, acc, "256 classes")
    assert every.n_classes == 256 and guide.wide_pitch(S, 256) == 257
    return bound, one, every


STRINGS = {"type": "object", "properties": {"s": {"type": "string", "maxLength": 60}}, "required": ["s"]}


def _configs(n, eos):
    """(guide, forced wide, record, fed, what the record's state must be afterwards or None) per row, two launches of 16"""
    bound, one, every = _hand_built()
    w256 = guide.compile_wide("[ab]{255}")
    js = guide.compile_json(STRINGS)
    n1, n255 = guide.compile_regex("[ab]*"), guide.compile_regex("[ab]{254}")
    assert w256.n_states == 256 and js.n_states > 255 and n1.n_states == 1 and n255.n_states == 255
    A, C_, LONG, EMPTY = 1, 4, 5, 7                              # ids of 'a', 'c', a 40-byte token of a / b, a token without bytes
    inside, closed = js.walk(b'{"s":"ab'), js.walk(b'{"s": "ab"}')
    assert not js.accept[inside] and js.accept[closed] and inside > 0
    Cw, Cb, Cj = w256.n_classes, bound.n_classes, js.n_classes
    first = [
        (w256, None, [W, 256, 1, Cw], A, 2),                     # S = 256: the smallest wide guide
        (bound, None, [W, 1023, 1, Cb], LONG, 41),               # at the entry bound, from the start, 40 bytes
        (n1, None, [ACT, 1, 1, 0], LONG, 1),                     # a narrow row between the wide ones
        (bound, None, [W, 1023, 700, Cb], C_, 702),              # a state above 255; 'c' steps by two, into an accepting state
        (js, None, [0, 999, 77, 5], A, 77),                      # inactive: nothing read, nothing written
        (bound, None, [W, 1023, 1023, Cb], EMPTY, 1023),         # its last state (accepting), a token without bytes
        (one, None, [W, 300, 250, 1], LONG, 290),                # C = 1
        (every, True, [W, 254, 3, 256], A, 4),                   # C = 256
        (n255, None, [ACT, 255, 200, 0], LONG, 240),             # narrow, 255 states
        (js, None, [W, js.n_states, inside, Cj], -1, inside),    # a compiled JSON guide inside a string, fed -1
        (js, None, [W, js.n_states, closed, Cj], eos, guide.DONE),   # ... in its accepting state, fed EOS
        (js, None, [W, js.n_states, 1, Cj], A, 0),               # fed a token the guide bans: state 0
        (js, None, [W, js.n_states, guide.DONE, Cj], A, guide.DONE),  # a DONE wide row
        (w256, None, [W, 256, 5, Cw], n + 5, 5),                 # an id beyond the vocabulary
        (w256, None, [W | 2, 256, 256, Cw], A, 0),               # other flag bits; the last state, one byte too many
        (one, None, [W, 300, 299, 1], 2 ** 31 - 1, 299),
    ]
    second = [
        (w256, None, [W, 0, 1, Cw], A, 1),                       # records out of range: S = 0,
        (bound, None, [W, 1023, 1, 64], A, 1),                   # (S + 1) * (C + 1) over the bound,
        (w256, None, [W, 256, 1, 0], A, 1),                      # C = 0,
        (n255, None, [ACT, 255, 1, 0], A, 2),
        (w256, None, [W, 256, 257, Cw], A, 257),                 # state S + 1,
        (w256, None, [W, 256, 0, Cw], A, 0),
        (w256, None, [W, 256, -2, Cw], A, -2),
        (w256, None, [W, 256, 1, 257], A, 1),                    # C = 257,
        (js, None, [0, 0, 0, 0], A, 0),
        (w256, None, [W, 65535, 1, Cw], A, 1),                   # S far beyond the region
        (w256, None, [W, 2 ** 31 - 1, 1, 2 ** 31 - 1], A, 1),
        (w256, "entry", [W, 256, 1, Cw], A, 0),                  # a table entry above S on the walked path: dead, as a banned token
        (w256, "cls", [W, 256, 1, Cw], A, 0),                    # a cls value of C: dead as well
        (w256, "entry", [W, 256, 2, Cw], EMPTY, 2),              # (nothing walked: the patched entry only bans 'a' in the mask)
        (bound, None, [W, 1023, 1022, Cb], C_, 0),
        (js, None, [W, js.n_states, inside, Cj], EMPTY, inside),
    ]
    return first, second


def _regions(cfgs):
    delta = np.zeros((len(cfgs), 256, 256), dtype=np.uint16)
    accept = np.zeros((len(cfgs), 256), dtype=np.uint8)
    for r, (g, how, rec, _, _) in enumerate(cfgs):
        delta[r], accept[r] = guide.region(g, wide=True if how else None)
        if how == "entry":                                       # state 1 on 'a' and state 2 on 'a' lead above S
            pitch, col = guide.wide_pitch(g.n_states, g.n_classes), 1 + int(accept[r][ord("a")])
            delta[r].reshape(-1)[1 * pitch + col] = g.n_states + 1
            delta[r].reshape(-1)[2 * pitch + col] = 65535
        if how == "cls":
            accept[r][ord("a")] = g.n_classes
    return delta, accept


@pytest.mark.parametrize("with_fed", [False, True], ids=["fed=NULL", "fed"])
@pytest.mark.parametrize("which, rows", [(0, 16), (1, 16), (0, 1)], ids=["valid-16", "out-of-range-16", "1-row"])
def test_wide_rows_equal_the_restatement_bit_for_bit(which, rows, with_fed):
    from phi_3_vision_mlx_amd import ops
    n = N
    table, eos = _table(n)
    cfgs = _configs(n, eos)[which]
    cfgs = cfgs[3:4] if rows == 1 else cfgs                      # one row: the bound guide at state 700
    rng = np.random.default_rng(17 + which)
    bits = penalties.f32_to_bf16_bits(rng.normal(0, 4.0, (rows, n)).astype(np.float32))
    for r in range(rows):
        for k, s in enumerate((0x7FA5, 0xFFC1, 0x8000, 0x7F80, 0xFF80, 0x7FC0)):
            for j in range(6):
                bits[r, (k * 6 + j) * 5 % n] = s
    delta, accept = _regions(cfgs)
    recs = np.array([c[2] for c in cfgs], dtype=np.int64).astype(np.int32)
    fed = np.array([c[3] for c in cfgs], dtype=np.int64).astype(np.int32)
    guard, pad = 11, 3
    stride = guard + n + pad + guard                             # row_stride > n, rows start at odd elements
    wide = np.full((rows, stride), CANARY16, dtype=np.uint16)
    wide[:, guard:guard + n] = bits
    d_off, d_bytes = _dev_table(table)
    outs = []
    for _ in range(2):                                           # a second launch from the same inputs: the same bits
        d_wide = _bf16_dev(wide)
        d_recs, d_delta, d_accept = _i32(recs), torch.as_tensor(delta.view(np.int16)).cuda(), torch.as_tensor(accept).cuda()
        ops.guide_mask(d_wide[:, guard:guard + n], d_recs, d_delta, d_accept, d_off, d_bytes, eos, fed=_i32(fed) if with_fed else None,
                       n_bytes=table.n_bytes)
        torch.cuda.synchronize()
        outs.append((_bits_of(d_wide).reshape(rows, stride), d_recs.cpu().numpy()))
        assert np.array_equal(d_delta.cpu().numpy().view(np.uint16), delta) and np.array_equal(d_accept.cpu().numpy(), accept)
    full, after = outs[0]
    assert np.array_equal(full, outs[1][0]) and np.array_equal(after, outs[1][1])
    assert (full[:, :guard] == CANARY16).all() and (full[:, guard + n:] == CANARY16).all()      # the guard bands
    for r, (g, how, rec, f, want_state) in enumerate(cfgs):
        want, state = guide.reference_mask(bits[r], recs[r], delta[r], accept[r], table, int(fed[r]) if with_fed else None, eos)
        got = full[r, guard:guard + n]
        assert np.array_equal(got, want), (r, np.nonzero(got != want)[0][:8])
        assert after[r].tolist() == [recs[r][0], recs[r][1], state, recs[r][3]], (r, after[r], state)
        if with_fed:
            assert state == want_state, (r, state, want_state)  # the cases do what their comments say
        else:
            assert state == recs[r][2]
        if not recs[r][0] & 1:
            assert np.array_equal(got, bits[r])
    if which == 1:                                               # records out of range: unwritten, and only EOS is left
        for r in (0, 1, 2, 4, 5, 6, 7, 9, 10):
            assert after[r].tolist() == recs[r].tolist()
            assert full[r, guard + eos] == bits[r, eos] and (np.delete(full[r, guard:guard + n], eos) == NEG_INF).all(), r
    if which == 0 and rows == 16:
        allowed = [(full[r, guard:guard + n] != NEG_INF) | (bits[r] == NEG_INF) for r in range(rows)]
        assert allowed[9].sum() > 100 and not allowed[9][eos] and allowed[10].sum() <= 1 + (bits[10] == NEG_INF).sum()
        assert allowed[1].sum() > 100 and allowed[7].sum() > 100 and allowed[6].sum() > 100      # (the masks are not trivial)


# ---------------------------------------------------------------------------------------------------- the model
ITEM = {"type": "object", "properties": {"tag": {"enum": ["alpha", "beta", "gamma", "delta", "omega", "zeta"]}, "ok": {"type": "boolean"}},
        "required": ["tag", "ok"]}
SCHEMA = {"type": "object", "properties": {"items": {"type": "array", "items": ITEM, "maxItems": 3}, "note": {"type": "string", "maxLength": 10}},
          "required": ["items", "note"]}


def _longest(dfa):
    """the length in bytes of the longest string the guide accepts (the automaton of a bounded schema has no cycle)"""
    succ = [sorted(set(row.tolist()) - {0}) for row in dfa.delta]
    best, on_path = {}, set()

    def depth(s):
        if s in best:
            return best[s]
        assert s not in on_path, "the guide has a cycle: its instances are unbounded"
        on_path.add(s)
        best[s] = max([1 + depth(t) for t in succ[s]], default=0)
        on_path.discard(s)
        return best[s]
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * dfa.n_states + 100))
    return depth(1)


@pytest.fixture(scope="module")
def schema_guide():
    dfa = guide.compile_json(SCHEMA)
    longest = _longest(dfa)
    assert dfa.n_states > 255 and guide.record(dfa)[0] & guide.WIDE, dfa.n_states
    assert longest + 2 <= MAX_TOKENS, longest                   # every run ends in EOS
    return dfa


MAX_TOKENS = 200


def _assert_json(table, toks, what=""):
    out, ended = _text_of(table, toks)
    assert ended, (what, out)
    assert validate(SCHEMA, json.loads(out)), (what, out)
    assert all(t == EOS for t in toks[toks.index(EOS):]), (what, toks)
    return out


def test_captured_step_equals_eager_launches_with_a_wide_a_narrow_and_a_plain_row(tiny, schema_guide):
    from phi_3_vision_mlx_amd import ops, sampling
    model, proc = tiny
    table = _vocab(model, proc)
    model.set_guide_vocab(table, EOS)
    dfas = [schema_guide, guide.compile_regex("[a-z ]{20,30}"), None]
    prompts = [BATCH[1], BATCH[3], BATCH[0]]
    inputs = proc(prompts, None)
    srows = [(0.9, 50, 0.95, 11), (0.0, 0, 1.0, 0), (0.8, 40, 1.0, 5)]
    V = model.cfg.vocab_size
    logits, cache = model(**inputs, max_tokens=16)
    st = cache[0].state
    model.set_guides(st, dfas)
    assert st.guide["rows"].cpu().numpy().tolist() == [guide.record(d) for d in dfas]
    first = model.guided_logits(st, logits)
    tok = ops.sample(first, sampling.pack(srows, 0).cuda())[:, None]
    model.set_sampling(st, sampling.pack(srows, 1))
    graph = [(tok.reshape(-1).cpu().tolist(), _bits_of(first).reshape(3, V).copy(), st.guide["rows"].cpu().numpy().copy())]
    for _ in range(12):
        _, tok = model.guide_step(tok, cache)
        torch.cuda.synchronize()
        graph.append((tok.reshape(-1).cpu().tolist(), _bits_of(st.penalty["adj"]).reshape(3, V).copy(), st.guide["rows"].cpu().numpy().copy()))
    assert "guide_graph" in st.graphs["greedy"]
    logits, cache = model(**inputs, max_tokens=16)
    recs = _i32([guide.record(d) for d in dfas])
    regions = [guide.region(d) if d is not None else (np.zeros((256, 256), np.uint16), np.zeros(256, np.uint8)) for d in dfas]
    d_delta = torch.as_tensor(np.stack([r[0] for r in regions]).view(np.int16)).cuda()
    d_accept = torch.as_tensor(np.stack([r[1] for r in regions])).cuda()
    d_off, d_bytes = _dev_table(table)
    srec = sampling.pack(srows, 0).cuda()
    adj = ops.guide_mask(logits[:, -1, :].clone(), recs, d_delta, d_accept, d_off, d_bytes, EOS, n_bytes=table.n_bytes)
    tok = ops.sample(adj, srec)[:, None]
    eager = [(tok.reshape(-1).cpu().tolist(), _bits_of(adj).reshape(3, V).copy(), recs.cpu().numpy().copy())]
    for _ in range(12):
        logits, cache = model(input_ids=tok, cache=cache)
        adj = ops.guide_mask(logits[:, -1, :].clone(), recs, d_delta, d_accept, d_off, d_bytes, EOS, fed=tok.reshape(-1).contiguous(),
                             n_bytes=table.n_bytes)
        tok = ops.sample(adj, srec)[:, None]
        eager.append((tok.reshape(-1).cpu().tolist(), _bits_of(adj).reshape(3, V).copy(), recs.cpu().numpy().copy()))
    for k, (g, e) in enumerate(zip(graph, eager)):
        assert g[0] == e[0], (k, g[0], e[0])
        assert np.array_equal(g[2], e[2]), (k, g[2], e[2])
        assert np.array_equal(g[1], e[1]), k
    assert len({g[2][0, 2] for g in graph}) > 6 and len({g[2][1, 2] for g in graph}) > 6      # both guided rows moved
    assert all(g[2][2].tolist() == [0, 0, 0, 0] for g in graph)                                # the plain row: an inactive record


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_generate_guided_json_every_step_follows_the_host_rule(tiny, schema_guide, mode):
    model, proc = tiny
    table = _vocab(model, proc)
    dfa = schema_guide
    delta, accept = guide.region(dfa)
    kw = dict(temperature=1.0, seed=4) if mode == "sampled" else {}
    with _Watch(model) as w:
        toks, text = _gen(model, proc, PROMPT, max_tokens=MAX_TOKENS, guided_json=SCHEMA, **kw)
    toks = toks[0]
    out = _assert_json(table, toks, mode)
    assert text[0].replace("<|end|>", "") == out
    rec = guide.record(dfa)
    assert rec[0] == W
    for k, t in enumerate(toks):
        if k and k - 1 >= len(w.logits):
            break                                                # (the step enqueued behind the EOS step)
        raw = w.prefill[0][0] if k == 0 else w.logits[k - 1][0]
        want, rec[2] = guide.reference_mask(raw, rec, delta, accept, table, None if k == 0 else toks[k - 1], EOS)
        got = w.first[0][0] if k == 0 else w.adj[k - 1][0]
        assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:8])
        if k:
            assert w.state[k - 1][0] == rec[2]
        if mode == "greedy":
            assert t == int(np.argmax(penalties.bf16_bits_to_f32(want))), (k, t)
    assert len(toks) - 1 <= len(w.logits) <= len(toks)


def test_generate_guided_json_with_n_penalties_and_logprobs(tiny, schema_guide):
    model, proc = tiny
    table = _vocab(model, proc)
    toks, texts = _gen(model, proc, PROMPT, max_tokens=MAX_TOKENS, guided_json=json.dumps(SCHEMA), n=4, temperature=1.0, seed=5)
    outs = [_assert_json(table, row, j) for j, row in enumerate(toks)]
    assert len(texts) == 4 and len(set(outs)) > 1
    toks, _ = _gen(model, proc, PROMPT, max_tokens=MAX_TOKENS, guided_json=SCHEMA, repetition_penalty=1.3, frequency_penalty=0.5,
                   logit_bias={3 + ord("f"): -float("inf")})
    assert "f" not in _assert_json(table, toks[0])                               # the bias bans 'f': the guide leaves "ok": true
    info = {}
    with _Watch(model) as w:
        toks, _ = _gen(model, proc, PROMPT, max_tokens=MAX_TOKENS, guided_json=SCHEMA, logprobs=2, logprob_info=info)
    _assert_json(table, toks[0])
    assert set(w.names) == {"guide_logprob_step"} and info["token_ids"][0] == toks[0]
    from test_logprobs_cpu import assert_record, logprobs_ref
    for k, t in enumerate(toks[0][:40]):                                          # the records describe the RAW logits
        raw = w.prefill[0][0] if k == 0 else w.logits[k - 1][0]
        rec = dict(token=t, logprob=info["token_logprobs"][0][k], rank=info["ranks"][0][k], top=info["top_logprobs"][0][k])
        assert_record(rec, logprobs_ref(raw, t, 2), k)
    assert max(info["ranks"][0]) > 1


def test_generate_two_prompts_one_schema_one_none_and_no_guide_means_no_change(tiny, schema_guide):
    model, proc = tiny
    table = _vocab(model, proc)
    prompts = [BATCH[1], BATCH[3]]
    plain, _ = _gen(model, proc, prompts, max_tokens=12)
    toks, _ = _gen(model, proc, prompts, max_tokens=MAX_TOKENS, guided_json=[SCHEMA, None])
    _assert_json(table, toks[0])
    cut = lambda row: row[:row.index(EOS) + 1] if EOS in row else row            # noqa: E731
    assert cut(toks[1])[:12] == cut(plain[1]) and toks[0][:12] != plain[0]        # the row without a schema: the unguided call's tokens
    states, real = [], model._new_state

    def spy(*a, **k):
        states.append(real(*a, **k))
        return states[-1]
    model._new_state = spy
    try:
        none, _ = _gen(model, proc, prompts, max_tokens=12, guided_json=None)
        lst, _ = _gen(model, proc, prompts, max_tokens=12, guided_json=[None, None])
    finally:
        del model._new_state
    assert none == plain and lst == plain
    for st in states:
        assert st.guide is None and st.penalty is None and not {"guide_graph", "guide_logprob_graph", "penal_graph"} & set(st.graphs["greedy"])
    with pytest.raises(ValueError, match="exclude each other"):
        _gen(model, proc, prompts, max_tokens=4, guided_regex=["a", None], guided_json=[SCHEMA, None])
    with pytest.raises(ValueError, match="speculate"):
        _gen(model, proc, PROMPT, max_tokens=4, guided_json=SCHEMA, speculate=2)
    with pytest.raises(ValueError, match="minimum"):
        _gen(model, proc, PROMPT, max_tokens=4, guided_json={"type": "integer", "minimum": 0})


def test_engine_wide_narrow_and_plain_requests_through_refilled_rows(tiny, schema_guide):
    import re
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, guide_args
    model, proc = tiny
    table = _vocab(model, proc)
    bounded = "(yes|no), [0-9]{1,3}\\."
    texts = [BATCH[1], BATCH[0], BATCH[3], BATCH[2], BATCH[0]]
    guides = [dict(schema=SCHEMA), None, dict(regex=bounded), dict(schema=json.dumps(SCHEMA)), dict(regex=bounded)]
    budget = [MAX_TOKENS, 6, 14, MAX_TOKENS, 14]
    eng = ContinuousEngine(model, proc, slots=2, window=256)
    hs = [eng.submit(proc(t) if g is None else guide_args(proc(t), **g), b) for t, g, b in zip(texts, guides, budget)]
    bad = eng.submit(guide_args(proc(texts[0]), schema={"type": "string", "format": "date"}), 4)
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and "format" in str(bad.error)       # at submit, before admission
    eng.run_until_idle()
    assert all(h.error is None for h in hs), [h.error for h in hs]
    assert eng.failures == 0 and len({h.row for h in hs}) == 2                   # five requests through two slots: refilled
    for i, h in enumerate(hs):
        if guides[i] is None:
            solo, _ = _gen(model, proc, texts[i], max_tokens=budget[i])
            want = solo[0][:solo[0].index(EOS) + 1] if EOS in solo[0] else solo[0]
            assert h.tokens == want, (i, h.tokens, want)
        elif "schema" in guides[i]:
            _assert_json(table, h.tokens, i)
        else:
            out, ended = _text_of(table, h.tokens)
            assert ended and re.fullmatch(bounded, out, re.ASCII), (i, out)
    assert not eng.st.guide["rows"][:, 0].any()                                 # every row released: inactive records


def test_server_guided_json_response_format_and_400s(tiny, schema_guide):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = tiny
    eng = ContinuousEngine(model, proc, slots=2, window=256)
    httpd, backend = serve_continuous(eng, port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]

    def post(body):
        req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=300) as r:
            return r.status, json.loads(r.read())
    try:
        status, body = post({"prompt": "Give me items", "max_tokens": MAX_TOKENS, "guided_json": SCHEMA})
        assert status == 200 and validate(SCHEMA, json.loads(body["responses"][0].replace("<|end|>", ""))), body
        status, body = post({"prompt": ["One", "And two"], "max_tokens": MAX_TOKENS, "temperature": 1.0, "seed": 4,
                             "response_format": {"type": "json_schema", "json_schema": {"name": "items", "schema": SCHEMA}}})
        assert status == 200 and all(validate(SCHEMA, json.loads(r.replace("<|end|>", ""))) for r in body["responses"]), body
        huge = {"enum": [c + ("%02d" % i) * 6 for i, c in enumerate(string.ascii_letters + string.digits + "!#$%&()*+-.:;<=>?@^_~")]}
        for bad, word in (({"guided_json": "{"}, "not valid JSON"), ({"guided_json": {"type": "integer", "multipleOf": 2}}, "multipleOf"),
                          ({"guided_json": huge}, "at most 65536"), ({"response_format": {"type": "json_object"}}, "not a regular language"),
                          ({"guided_json": SCHEMA, "speculate": 3}, "speculat")):
            with pytest.raises(urllib.error.HTTPError) as e:
                post(dict({"prompt": "x", "max_tokens": 3}, **bad))
            assert e.value.code == 400 and word in json.loads(e.value.read())["error"], bad
    finally:
        httpd.shutdown()
        backend.close()
