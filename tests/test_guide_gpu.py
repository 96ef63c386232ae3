"""Guided decoding on the MI355X: p3v_guide_mask against the NumPy restatement of the rule (guide.reference_mask) BIT FOR BIT --
the rule only overwrites banned positions with one constant and moves an integer state, so there is no tolerance --, then the
guided captures of the model: captured against eager launches, every step of a guided run against the host rule (teacher-forced
against itself), api.generate end to end on bounded patterns, "no guide means no change", the continuous engine with refilled
rows, and one server round trip."""
import json
import re
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import guide, penalties

pytestmark = pytest.mark.gpu
N = 32064
EOS = 32007
CANARY16 = 0x7FD5                                   # a NaN payload no computation produces: "never written"
NEG_INF = 0xFF80


def _bf16_dev(bits):
    return torch.as_tensor(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _i32(v):
    return torch.as_tensor(np.ascontiguousarray(v).astype(np.int32)).cuda()


# ---------------------------------------------------------------------------------------------------- p3v_guide_mask
_TABLES = {}


def _table(n):
    """A vocabulary of tokens with 0, 1, 2, 3 and 40 bytes over a small alphabet (and pieces of a multi-byte character), so that
    walks die at the first byte, in the middle and not at all.  The last id of the small vocabulary and 32007 of the full one
    are the EOS: no bytes."""
    if n not in _TABLES:
        rng = np.random.default_rng(n)
        eos = EOS if n > EOS else n - 1
        strings = []
        for i in range(n):
            k = i % 7
            if i == eos or k == 0:
                s = b""
            elif k in (1, 2, 4):
                s = {1: b"a", 2: b"b", 4: b"c"}[k]
            elif k == 3:
                s = b"ab"
            elif k == 5:
                s = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 40).tolist())
            else:
                s = bytes(rng.choice(np.frombuffer("abc,é".encode(), dtype=np.uint8), int(rng.integers(1, 4))).tolist())
            strings.append(s)
        t = guide.VocabTable(strings)
        lens = t.padded()[0]
        assert {0, 1, 40} <= set(lens.tolist())
        _TABLES[n] = (t, eos)
    return _TABLES[n]


def _guides():
    one = guide.compile_regex("[ab]*")
    full = guide.compile_regex("[ab]{254}")
    mid = guide.compile_regex("(ab|ba)+c?")
    utf = guide.compile_regex(".*")
    assert one.n_states == 1 and full.n_states == 255
    return one, full, mid, utf


def _configs(n, eos):
    """(guide, record, fed) per row: every kind of state and of fed token the rule names."""
    one, full, mid, utf = _guides()
    A, LONG, EMPTY = 1, 5, 7                                     # ids of 'a', of a 40-byte token, of a token without bytes
    mid_acc = mid.walk(b"ab")
    assert mid.accept[mid_acc] and not mid.accept[mid.walk(b"a")]
    return [
        (full, [1, 255, 1, 0], A),                               # 255 states, the start, an ordinary token
        (mid, [0, 999, 77, 0], A),                               # inactive: nothing read, nothing written
        (one, [1, 1, 1, 0], LONG),                               # 1 state (accepting), a 40-byte token
        (mid, [1, mid.n_states, mid.walk(b"a"), 0], -1),         # a non-accepting state, fed -1
        (full, [1, 255, 200, 0], LONG),                          # 200 -> 240
        (full, [1, 255, 230, 0], LONG),                          # 230 + 40 bytes: a dead end -> state 0
        (utf, [1, utf.n_states, guide.DONE, 0], A),              # DONE stays DONE
        (mid, [1, mid.n_states, mid_acc, 0], eos),               # an accepting state, fed EOS -> DONE
        (one, [1, 0, 1, 0], A),                                  # n_states out of range
        (one, [1, 256, 1, 0], A),
        (mid, [1, mid.n_states, mid.n_states + 1, 0], A),        # state out of range
        (mid, [1, mid.n_states, 0, 0], A),
        (mid, [1, mid.n_states, -2, 0], A),
        (utf, [1, utf.n_states, 1, 0], n + 5),                   # an image-slot id: outside the vocabulary
        (full, [1, 255, 255, 0], EMPTY),                         # the last state (accepting), a token without bytes
        (mid, [3, mid.n_states, 1, 0], 2 ** 31 - 1),             # other flag bits set, a huge id
    ]


def _case(n, rows, seed):
    table, eos = _table(n)
    cfgs = _configs(n, eos)
    off = 4 if rows == 1 else 0
    cfgs = [cfgs[(r + off) % len(cfgs)] for r in range(rows)]
    rng = np.random.default_rng(seed)
    bits = penalties.f32_to_bf16_bits(rng.normal(0, 4.0, (rows, n)).astype(np.float32))
    for r in range(rows):                                        # NaN payloads, -0 and infinities in every row, wherever they fall
        for k, s in enumerate((0x7FA5, 0xFFC1, 0x8000, 0x7F80, 0xFF80, 0x7FC0)):
            for j in range(6):
                bits[r, (k * 6 + j) * 5 % n] = s                 # ids 0 .. ~175: tokens of every length class
        bits[r, eos] = 0x7FA7 if r % 2 else bits[r, eos]
    delta = np.zeros((rows, 256, 256), dtype=np.uint16)
    accept = np.zeros((rows, 256), dtype=np.uint8)
    for r, (g, _, _) in enumerate(cfgs):
        delta[r], accept[r] = guide.region(g)
    recs = np.array([c[1] for c in cfgs], dtype=np.int32)
    fed = np.array([c[2] for c in cfgs], dtype=np.int64).astype(np.int32)
    return table, eos, bits, delta, accept, recs, fed


def _dev_table(table):
    return torch.as_tensor(table.tok_off.view(np.int32).copy()).cuda(), torch.as_tensor(table.tok_bytes.copy()).cuda()


@pytest.mark.parametrize("with_fed", [False, True], ids=["fed=NULL", "fed"])
@pytest.mark.parametrize("pad", [0, 3], ids=["aligned", "stride+3"])
@pytest.mark.parametrize("rows", [1, 3, 16])
@pytest.mark.parametrize("n", [301, N])
def test_guide_mask_equals_the_restatement_bit_for_bit(n, rows, pad, with_fed):
    from phi_3_vision_mlx_amd import ops
    table, eos, bits, delta, accept, recs, fed = _case(n, rows, 1000 * rows + n + pad)
    guard = 8 + pad                                              # poison on both sides of every row; pad 3: rows start at odd elements
    stride = guard + n + pad + guard
    wide = np.full((rows, stride), CANARY16, dtype=np.uint16)
    wide[:, guard:guard + n] = bits
    d_wide = _bf16_dev(wide)
    d_recs, d_delta, d_accept = _i32(recs), torch.as_tensor(delta.view(np.int16)).cuda(), torch.as_tensor(accept).cuda()
    d_off, d_bytes = _dev_table(table)
    d_fed = _i32(fed) if with_fed else None
    got = ops.guide_mask(d_wide[:, guard:guard + n], d_recs, d_delta, d_accept, d_off, d_bytes, eos, fed=d_fed, n_bytes=table.n_bytes)
    torch.cuda.synchronize()
    assert got.data_ptr() == d_wide[:, guard:].data_ptr()
    full = _bits_of(d_wide).reshape(rows, stride)
    assert (full[:, :guard] == CANARY16).all() and (full[:, guard + n:] == CANARY16).all()      # nothing outside a row
    after = d_recs.cpu().numpy()
    banned_nan = kept_nan = 0
    for r in range(rows):
        want, state = guide.reference_mask(bits[r], recs[r], delta[r], accept[r], table, int(fed[r]) if with_fed else None, eos)
        assert np.array_equal(full[r, guard:guard + n], want), (r, np.nonzero(full[r, guard:guard + n] != want)[0][:8])
        assert after[r].tolist() == [recs[r][0], recs[r][1], state, recs[r][3]], (r, after[r], state)
        nan = (bits[r] & 0x7FFF) > 0x7F80
        banned_nan += int((nan & (want == NEG_INF)).sum())
        kept_nan += int((nan & (want == bits[r])).sum())
        if not recs[r][0] & 1:
            assert np.array_equal(want, bits[r]) and nan.any()                                    # an inactive row: payloads and -0 kept
    if rows > 1:
        assert banned_nan and kept_nan                           # a NaN in a banned position became -inf, one in an allowed one stayed
    # the tables are only read
    assert np.array_equal(d_delta.cpu().numpy().view(np.uint16), delta) and np.array_equal(d_accept.cpu().numpy(), accept)
    assert np.array_equal(d_off.cpu().numpy().view(np.uint32), table.tok_off) and np.array_equal(d_bytes.cpu().numpy(), table.tok_bytes)
    if with_fed and rows == 16:                                  # the cases do what their comments say
        assert after[:, 2].tolist() == [2, 77, 1, recs[3][2], 240, 0, -1, -1, 1, 1, recs[10][2], 0, -2, 1, 255, after[15, 2]]


def test_guide_mask_refuses_bad_arguments():
    from phi_3_vision_mlx_amd import _lib, ops
    lib = _lib.lib()
    n, rows = 301, 2
    table, eos, bits, delta, accept, recs, fed = _case(n, rows, 5)
    x = _bf16_dev(np.full((rows, n), CANARY16, dtype=np.uint16))
    d_recs, d_delta, d_accept = _i32(recs), torch.as_tensor(delta.view(np.int16)).cuda(), torch.as_tensor(accept).cuda()
    d_off, d_bytes = _dev_table(table)
    p = lambda a: a.data_ptr()                                                    # noqa: E731
    ok = (p(x), n, p(d_recs), p(d_delta), p(d_accept), p(d_off), p(d_bytes), table.n_bytes, None, eos, rows, n, None)
    for i, bad in ((0, None), (2, None), (3, None), (4, None), (5, None), (6, None), (1, n - 1), (10, 0), (10, 65536), (11, 0),
                   (7, -1), (3, p(d_delta) + 2)):
        args = list(ok)
        args[i] = bad
        assert lib.p3v_guide_mask(*args) == -22, (i, bad)
    torch.cuda.synchronize()
    assert (_bits_of(x) == CANARY16).all() and np.array_equal(d_recs.cpu().numpy(), recs)     # nothing was launched
    with pytest.raises((TypeError, ValueError)):
        ops.guide_mask(x, d_recs.to(torch.int64), d_delta, d_accept, d_off, d_bytes, eos)
    with pytest.raises(ValueError):
        ops.guide_mask(x, d_recs[:1], d_delta, d_accept, d_off, d_bytes, eos)
    with pytest.raises(ValueError):
        ops.guide_mask(x, d_recs, d_delta, d_accept, d_off[:n], d_bytes, eos)


# ---------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def tiny():
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    yield model, proc
    del model
    torch.cuda.empty_cache()


PROMPT = "<|user|>\nTell me a story<|end|>\n<|assistant|>\n"
BATCH = ["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nA longer question here, padded left<|end|>\n<|assistant|>\n",
         "<|user|>\nWhy?<|end|>\n<|assistant|>\n", "<|user|>\nOne two three four<|end|>\n<|assistant|>\n"]
KW = dict(verbose=False, stream=False, mute=True)
BOUNDED = "(yes|no), [0-9]{1,3}\\."                               # longest match: 9 bytes = 9 tokens of the byte vocabulary
CHOICES = ["red", "green", "blue", "greenish"]
LONGISH = "[a-z ]{20,30}"                                        # no EOS before 20 tokens: twelve steps stay inside the pattern


def _gen(model, proc, prompt, **kw):
    """api._generate -> (per-row token lists as the streamer got them, the returned text)"""
    from phi_3_vision_mlx_amd import api
    steps = []

    class Rec(api.Streamer):
        def __call__(self, token):
            steps.append(api._rows(token))
            return super().__call__(token)
    orig, api.Streamer = api.Streamer, Rec
    try:
        text = api._generate(model, proc, prompt, **KW, **kw)
    finally:
        api.Streamer = orig
    return [list(col) for col in zip(*steps)], text


def _text_of(table, toks):
    """the bytes a row generated up to its first EOS, and whether it got there"""
    k = toks.index(EOS) if EOS in toks else len(toks)
    return b"".join(table.bytes_of(t) for t in toks[:k]).decode("utf-8"), EOS in toks


def _vocab(model, proc):
    return guide.vocab_for(proc.tokenizer, model.cfg.vocab_size)


def test_captured_step_equals_eager_launches(tiny):
    """twelve steps of two rows under different guides: the captured guided step against eager model calls + p3v_guide_mask +
    p3v_sample on buffers of this test -- masked rows, states and tokens"""
    from phi_3_vision_mlx_amd import ops, sampling
    model, proc = tiny
    table = _vocab(model, proc)
    model.set_guide_vocab(table, EOS)
    dfas = [guide.compile_regex(LONGISH), guide.compile_regex("(ab|ba)+c?")]
    prompts = [BATCH[1], BATCH[3]]
    inputs = proc(prompts, None)
    srows = [(0.0, 0, 1.0, 0), (0.9, 50, 0.95, 11)]
    V = model.cfg.vocab_size
    # captured
    logits, cache = model(**inputs, max_tokens=16)
    st = cache[0].state
    model.set_guides(st, dfas)
    first = model.guided_logits(st, logits)
    raw0 = _bits_of(logits[:, -1, :]).reshape(2, V)
    assert np.array_equal(_bits_of(logits[:, -1, :]).reshape(2, V), raw0)          # the prefill logits stay raw
    tok = ops.sample(first, sampling.pack(srows, 0).cuda())[:, None]
    model.set_sampling(st, sampling.pack(srows, 1))
    graph = [(tok.reshape(-1).cpu().tolist(), _bits_of(first).reshape(2, V).copy(), st.guide["rows"].cpu().numpy().copy())]
    for _ in range(12):
        _, tok = model.guide_step(tok, cache)
        torch.cuda.synchronize()
        graph.append((tok.reshape(-1).cpu().tolist(), _bits_of(st.penalty["adj"]).reshape(2, V).copy(), st.guide["rows"].cpu().numpy().copy()))
    assert "guide_graph" in st.graphs["greedy"] and "penal_graph" not in st.graphs["greedy"]
    # eager
    logits, cache = model(**inputs, max_tokens=16)
    recs = _i32([guide.record(d) for d in dfas])
    regions = [guide.region(d) for d in dfas]
    d_delta = torch.as_tensor(np.stack([r[0] for r in regions]).view(np.int16)).cuda()
    d_accept = torch.as_tensor(np.stack([r[1] for r in regions])).cuda()
    d_off, d_bytes = _dev_table(table)
    srec = sampling.pack(srows, 0).cuda()
    adj = ops.guide_mask(logits[:, -1, :].clone(), recs, d_delta, d_accept, d_off, d_bytes, EOS, n_bytes=table.n_bytes)
    tok = ops.sample(adj, srec)[:, None]
    eager = [(tok.reshape(-1).cpu().tolist(), _bits_of(adj).reshape(2, V).copy(), recs.cpu().numpy().copy())]
    for _ in range(12):
        logits, cache = model(input_ids=tok, cache=cache)
        adj = ops.guide_mask(logits[:, -1, :].clone(), recs, d_delta, d_accept, d_off, d_bytes, EOS, fed=tok.reshape(-1).contiguous(),
                             n_bytes=table.n_bytes)
        tok = ops.sample(adj, srec)[:, None]
        eager.append((tok.reshape(-1).cpu().tolist(), _bits_of(adj).reshape(2, V).copy(), recs.cpu().numpy().copy()))
    for k, (g, e) in enumerate(zip(graph, eager)):
        assert g[0] == e[0], (k, g[0], e[0])
        assert np.array_equal(g[2], e[2]), (k, g[2], e[2])
        assert np.array_equal(g[1], e[1]), k
    assert len({tuple(g[2][:, 2]) for g in graph}) > 6                              # (the states did move)


class _Watch:
    """the model's guided entry points, with every call's raw logits, masked rows, states and tokens kept"""

    def __init__(self, model):
        self.model, self.prefill, self.first, self.fed, self.logits, self.adj, self.state, self.out, self.names = model, [], [], [], [], [], [], [], []
        self.orig = {k: getattr(model, k) for k in ("guide_step", "guide_logprob_step", "guided_logits")}
        self.st = None

    def __enter__(self):
        def step(name):
            def f(token, cache):
                self.fed.append(token.reshape(-1).cpu().tolist())
                lg, tok = self.orig[name](token, cache)
                torch.cuda.synchronize()
                st = cache[0].state
                self.logits.append(_bits_of(lg).reshape(st.B, -1).copy())
                self.adj.append(_bits_of(st.penalty["adj"]).reshape(st.B, -1).copy())
                self.state.append(st.guide["rows"].cpu().numpy()[:, 2].tolist())
                self.out.append(tok.reshape(-1).cpu().tolist())
                self.names.append(name)
                return lg, tok
            return f

        def first(st, logits, row0=0):
            self.st = st
            last = logits[:, -1, :] if logits.dim() == 3 else logits
            self.prefill.append(_bits_of(last).reshape(last.shape[0], -1).copy())
            out = self.orig["guided_logits"](st, logits, row0)
            self.first.append(_bits_of(out).reshape(last.shape[0], -1).copy())
            return out
        self.model.guide_step, self.model.guide_logprob_step, self.model.guided_logits = step("guide_step"), step("guide_logprob_step"), first
        return self

    def __exit__(self, *a):
        for k in self.orig:
            self.model.__dict__.pop(k, None)


def _prompt_row(proc, prompt):
    return np.asarray(proc(prompt, None)["input_ids"]).reshape(-1)


@pytest.mark.parametrize("mode", ["greedy+penalties", "sampled"])
def test_every_step_follows_the_host_rule(tiny, mode):
    """teacher-forced against itself: at every step the adjusted buffer is reference_mask of that step's penalised logits, the
    state is the walked one, and the next token is the sampler's rule on the masked row"""
    from test_sampling_cpu import sample_ref
    model, proc = tiny
    table = _vocab(model, proc)
    dfa = guide.compile_regex(BOUNDED)
    delta, accept = guide.region(dfa)
    if mode == "sampled":
        kw = dict(temperature=0.9, top_k=50, seed=3)              # top_k 50 > the allowed set (at most 10 digits + '.')
        pen_row, srow = None, (0.9, 50, 1.0, 3)
    else:
        kw = dict(repetition_penalty=1.3, presence_penalty=0.5)
        pen_row, srow = penalties.rows(1, 1.3, 0.5, 0.0, None)[0], None
    with _Watch(model) as w:
        toks, text = _gen(model, proc, PROMPT, max_tokens=14, guided_regex=BOUNDED, **kw)
    toks = toks[0]
    # (the loop runs one step ahead of the host: a step enqueued behind the EOS step is dropped, its call is still watched)
    assert set(w.names) == {"guide_step"} and len(w.prefill) == 1 and len(toks) - 1 <= len(w.logits) <= len(toks)
    prow, V = _prompt_row(proc, PROMPT), model.cfg.vocab_size
    rec = guide.record(dfa)
    for k, t in enumerate(toks):
        raw = w.prefill[0][0] if k == 0 else w.logits[k - 1][0]
        if pen_row is not None and k == 0:
            raw = w.prefill[0][0]                                # (what guided_logits was handed: the penalised prefill row)
        elif pen_row is not None:
            raw = penalties.reference_adjust(raw, (*pen_row[:3], penalties.flags(pen_row)), penalties.seen_table(prow, toks[:k], V))
        want, rec[2] = guide.reference_mask(raw, rec, delta, accept, table, None if k == 0 else toks[k - 1], EOS)
        got = w.first[0][0] if k == 0 else w.adj[k - 1][0]
        assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:8])
        if k:
            assert w.state[k - 1][0] == rec[2] and w.fed[k - 1][0] == toks[k - 1]
        vals = penalties.bf16_bits_to_f32(want)
        assert not np.isnan(vals).any() and int((want != NEG_INF).sum()) <= 11
        if srow is None:
            assert t == int(np.argmax(vals)), (k, t)
        else:
            assert t == sample_ref(want, srow[0], srow[1], srow[2], srow[3], k), (k, t)
    out, ended = _text_of(table, toks)
    assert ended and re.fullmatch(BOUNDED, out, re.ASCII), out
    assert all(t == EOS for t in toks[toks.index(EOS):])


def _assert_guided(table, toks, pattern, what=""):
    out, ended = _text_of(table, toks)
    assert ended, (what, toks)
    assert re.fullmatch(pattern, out, re.ASCII), (what, out)
    assert all(t == EOS for t in toks[toks.index(EOS):]), (what, toks)        # after EOS a row emits only EOS
    return out


@pytest.mark.parametrize("seed", [None, 1, 2, 3], ids=["greedy", "seed1", "seed2", "seed3"])
def test_generate_bounded_regex_and_choice(tiny, seed):
    """random weights do not say `(yes|no), [0-9]{1,3}\\.` on their own: without the feature these fail"""
    model, proc = tiny
    table = _vocab(model, proc)
    kw = {} if seed is None else dict(temperature=1.0, seed=seed)
    toks, text = _gen(model, proc, PROMPT, max_tokens=14, guided_regex=BOUNDED, **kw)
    out = _assert_guided(table, toks[0], BOUNDED, seed)
    assert text[0].replace("<|end|>", "") == out
    toks, text = _gen(model, proc, PROMPT, max_tokens=14, guided_choice=CHOICES, **kw)
    assert _assert_guided(table, toks[0], "red|green|blue|greenish", seed) in CHOICES


def test_generate_with_penalties_logprobs_and_n(tiny):
    model, proc = tiny
    table = _vocab(model, proc)
    toks, _ = _gen(model, proc, PROMPT, max_tokens=14, guided_regex=BOUNDED, repetition_penalty=1.3, frequency_penalty=0.5,
                   logit_bias={3 + ord("y"): -float("inf")})
    assert _assert_guided(table, toks[0], BOUNDED).startswith("no, ")         # the bias bans 'y': the guide leaves "no"
    info = {}
    with _Watch(model) as w:
        toks, _ = _gen(model, proc, PROMPT, max_tokens=14, guided_regex=BOUNDED, logprobs=2, logprob_info=info)
    _assert_guided(table, toks[0], BOUNDED)
    assert set(w.names) == {"guide_logprob_step"} and info["token_ids"][0] == toks[0]
    from test_logprobs_cpu import assert_record, logprobs_ref
    for k, t in enumerate(toks[0]):                                             # the records describe the RAW logits
        raw = w.prefill[0][0] if k == 0 else w.logits[k - 1][0]
        rec = dict(token=t, logprob=info["token_logprobs"][0][k], rank=info["ranks"][0][k], top=info["top_logprobs"][0][k])
        assert_record(rec, logprobs_ref(raw, t, 2), k)
    assert max(info["ranks"][0]) > 1                                            # (the guide did overrule the model somewhere)
    toks, texts = _gen(model, proc, PROMPT, max_tokens=14, guided_regex=BOUNDED, n=4, temperature=1.0, seed=5)
    outs = [_assert_guided(table, row, BOUNDED, j) for j, row in enumerate(toks)]
    assert len(texts) == 4 and len(set(outs)) > 1                               # every completion walked its own state


def test_generate_two_prompts_one_guide_one_none(tiny):
    model, proc = tiny
    table = _vocab(model, proc)
    prompts = [BATCH[1], BATCH[3]]
    plain, _ = _gen(model, proc, prompts, max_tokens=12)
    toks, _ = _gen(model, proc, prompts, max_tokens=12, guided_regex=[BOUNDED, None])
    _assert_guided(table, toks[0], BOUNDED)
    assert toks[1] == plain[1] and toks[0] != plain[0]                           # the row without a guide: the unguided call's tokens
    toks, _ = _gen(model, proc, prompts, max_tokens=12, guided_choice=[None, CHOICES])
    assert toks[0] == plain[0] and _text_of(table, toks[1])[0] in CHOICES
    with pytest.raises(ValueError, match="exclude"):
        _gen(model, proc, prompts, max_tokens=4, guided_regex=["a", None], guided_choice=[["b"], None])
    with pytest.raises(ValueError, match="speculate"):
        _gen(model, proc, PROMPT, max_tokens=4, guided_regex="a", speculate=2)


class _Count:
    """Counts the library's launches by name (everything but the graph / event helpers and the queries)."""

    def __init__(self):
        from phi_3_vision_mlx_amd import _lib
        self._lib, self.real, self.n = _lib, _lib.lib(), {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("p3v_") or name.startswith(("p3v_graph", "p3v_event", "p3v_device", "p3v_get", "p3v_set", "p3v_str",
                                                            "p3v_version")) or name.endswith(("_bytes", "_slices", "_role", "_can_fuse_oproj")):
            return fn

        def counted(*a):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a)
        return counted

    def __enter__(self):
        self._lib._lib = self
        return self

    def __exit__(self, *a):
        self._lib._lib = self.real


def test_no_guide_means_no_change(tiny, monkeypatch):
    """without the keywords (or with None): the launches of the model-level plain loop by name and count, one graph, no state"""
    from phi_3_vision_mlx_amd import api, ops
    model, proc = tiny
    n_tok = 10
    monkeypatch.setenv("P3V_PREFILL_GRAPH", "0")                 # (every run below prefills eagerly: comparable launch counts)

    def plain():
        logits, cache = model(**proc(PROMPT, None), max_tokens=n_tok)
        tok = ops.argmax(logits[:, -1, :].contiguous())[:, None]
        toks = [int(tok[0, 0])]
        for _ in range(n_tok - 1):
            _, tok = model.greedy_step(tok, cache)
            toks.append(int(tok[0, 0]))
        return toks, cache[0].state

    def via_generate(**kw):
        states, real = [], model._new_state

        def spy(*a, **k):
            states.append(real(*a, **k))
            return states[-1]
        model._new_state = spy
        try:
            toks, _ = _gen(model, proc, PROMPT, max_tokens=n_tok, **kw)
        finally:
            del model._new_state
        return toks[0], states[-1]
    plain()
    with _Count() as c_plain:
        toks_p, st_p = plain()
    with _Count() as c_default:
        toks_d, st_d = via_generate()
    with _Count() as c_none:
        toks_n, st_n = via_generate(guided_regex=None, guided_choice=None)
    if EOS in toks_p:
        toks_p = toks_p[:toks_p.index(EOS) + 1]
    drop = lambda d: {k: v for k, v in d.items() if k not in ("p3v_argmax",)}    # noqa: E731 (the host loop's own token plumbing)
    assert c_none.n == c_default.n and (EOS in toks_p or drop(c_default.n) == drop(c_plain.n)), (c_none.n, c_default.n, c_plain.n)
    assert "p3v_guide_mask" not in c_default.n and "p3v_penalize" not in c_default.n
    assert toks_d[:len(toks_p)] == toks_p and toks_n == toks_d
    for st in (st_d, st_n):
        assert st.guide is None and st.penalty is None and st.sample_rows is None
        assert sorted(st.graphs) == sorted(st_p.graphs) == ["greedy"]
        assert not {"guide_graph", "guide_logprob_graph", "penal_graph"} & set(st.graphs["greedy"])


def test_replan_after_a_failed_step_rebuilds_the_states(monkeypatch, capsys):
    """the loop's recovery drops the captures and rewinds: the rows' states are rebuilt by walking the tokens fed so far"""
    from phi_3_vision_mlx_amd import api, ops
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.processor import ByteTokenizer
    model, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=2)
    ids = torch.randint(3, 32000, (1, 1700), dtype=torch.int64, generator=torch.Generator().manual_seed(6)).numpy()
    table = guide.token_bytes(ByteTokenizer(), model.cfg.vocab_size)
    dfa = guide.compile_regex(LONGISH)
    model.set_guide_vocab(table, EOS)

    def run(fail):
        if fail is None:
            monkeypatch.delenv("P3V_DEBUG_FAIL_STEP", raising=False)
        else:
            monkeypatch.setenv("P3V_DEBUG_FAIL_STEP", str(fail))
        model.serving = False
        logits, cache = model(input_ids=torch.as_tensor(ids), max_tokens=40)
        st = cache[0].state
        model.set_guides(st, [dfa])
        token = ops.argmax(model.guided_logits(st, logits))[:, None]
        seen = []
        api.greedy_loop(model, token, cache, 10, lambda r: seen.append(list(r)), lambda r: False, guides=dict(dfas=[dfa], table=table, eos=EOS))
        fed = token.reshape(-1).cpu().tolist() + [r[0] for r in seen[:-1]]
        assert int(st.guide["rows"][0, 2]) == guide.replay_state(dfa, table, fed, EOS) == len(fed) + 1
        out = b"".join(table.bytes_of(t) for t in fed + seen[-1]).decode()
        assert re.fullmatch("[a-z ]{11}", out), out
        return seen, st.graphs["greedy"]["bufs"]["plan"].fuse_o

    good, fused = run(None)
    assert fused and len(good) == 10
    for fail in (0, 4):
        got, fused2 = run(fail)
        assert got == good and not fused2
        assert "continuing with separate launches" in capsys.readouterr().err
    del model
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- engine, server
def test_engine_mixed_guided_and_plain_requests_through_refilled_rows(tiny):
    """six requests through two slots, guided and plain: every guided text full-matches its own guide (a refilled row starts
    from its own start state, whatever its last occupant left), every plain request returns its solo run's tokens"""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, guide_args
    model, proc = tiny
    table = _vocab(model, proc)
    texts = [BATCH[1], BATCH[0], BATCH[3], BATCH[2], BATCH[0], BATCH[3]]
    guides = [dict(regex=BOUNDED), None, dict(choice=CHOICES), dict(regex="[0-9]{4}-[0-9]{2}"), None, dict(regex=BOUNDED)]
    wants = [BOUNDED, None, "red|green|blue|greenish", "[0-9]{4}-[0-9]{2}", None, BOUNDED]
    budget = [14, 5, 12, 12, 8, 14]
    eng = ContinuousEngine(model, proc, slots=2, window=96)
    hs = [eng.submit(proc(t) if g is None else guide_args(proc(t), **g), b) for t, g, b in zip(texts, guides, budget)]
    bad = eng.submit(guide_args(proc(texts[0]), regex="a$"), 4)
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and "anchor" in str(bad.error)      # at submit, before admission
    eng.run_until_idle()
    assert all(h.error is None for h in hs), [h.error for h in hs]
    assert eng.failures == 0 and len({h.row for h in hs}) == 2                   # six requests through two slots: refilled
    for i, h in enumerate(hs):
        if wants[i] is None:
            solo, _ = _gen(model, proc, texts[i], max_tokens=budget[i])
            want = solo[0][:solo[0].index(EOS) + 1] if EOS in solo[0] else solo[0]
            assert h.tokens == want, (i, h.tokens, want)
        else:
            assert h.tokens[-1] == EOS
            _assert_guided(table, h.tokens, wants[i], i)
    guided_rows = {hs[i].row for i in (0, 2, 3, 5)}
    assert any(hs[i].row in guided_rows for i in (1, 4))                         # a plain request took over a guided row's slot
    assert not eng.st.guide["rows"][:, 0].any()                                 # every row released: inactive records
    assert "guide_graph" in eng.st.graphs["greedy"]


def test_engine_family_members_walk_their_own_states(tiny):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, guide_args, n_args
    model, proc = tiny
    table = _vocab(model, proc)
    eng = ContinuousEngine(model, proc, slots=4, window=96)
    h = eng.submit(n_args(guide_args(proc(BATCH[1]), regex=BOUNDED), 3), 14, sampling={"temperature": 1.0, "seed": 9})
    eng.run_until_idle()
    assert h.error is None and h.family_done.is_set() and len(h.completions) == 3
    outs = [_assert_guided(table, r.tokens, BOUNDED, j) for j, r in enumerate(h.completions)]
    assert len(set(outs)) > 1


def test_server_round_trip_and_400s(tiny):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = tiny
    eng = ContinuousEngine(model, proc, slots=2, window=96)
    httpd, backend = serve_continuous(eng, port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]

    def post(body):
        req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=300) as r:
            return r.status, json.loads(r.read())
    try:
        status, body = post({"prompt": "Is it?", "max_tokens": 14, "guided_regex": BOUNDED})
        assert status == 200 and re.fullmatch(BOUNDED, body["responses"][0].replace("<|end|>", ""), re.ASCII), body
        status, body = post({"prompt": ["Colour?", "And this one?"], "max_tokens": 12, "guided_choice": CHOICES, "temperature": 1.0, "seed": 4})
        assert status == 200 and all(r.replace("<|end|>", "") in CHOICES for r in body["responses"]), body
        for bad, word in (({"guided_regex": "(?=a)b"}, "look-around"), ({"guided_regex": "a{300}"}, "301 states"),
                          ({"guided_choice": []}, "non-empty"), ({"guided_regex": "a", "speculate": 3}, "speculat")):
            with pytest.raises(urllib.error.HTTPError) as e:
                post(dict({"prompt": "x", "max_tokens": 3}, **bad))
            assert e.value.code == 400 and word in json.loads(e.value.read())["error"], bad
    finally:
        httpd.shutdown()
        backend.close()
