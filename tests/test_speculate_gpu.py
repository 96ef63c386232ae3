"""Speculative greedy decoding on the GPU: the kernels against the rule (speculate.py, exact), the verify step against the
oracle fixture tests/golden/tiny_spec_oracle.npz (tests/golden/gen_golden_spec.py), the captured step against the eager one,
the hand-over to the plain path, the public surface, one full-width run against the plain path, one server round trip."""
import json
import math
import os
import threading
import urllib.request

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
I32 = torch.int32
V_FULL = 32064


# ----------------------------------------------------------------------------- 1. kernels vs the rule
def _state(ctx, K, n_limit, forced=False, cap=None, hist_cap=256, rec_cap=32, n_max=3, n_min=1, tok0=None, d_past=None):
    from phi_3_vision_mlx_amd import _lib, ops
    Lq, n = K + 1, len(ctx)
    cap = cap or n + 64
    g = dict(K=K, tok=torch.zeros(Lq, dtype=I32, device=DEV), ctx=torch.zeros(cap, dtype=I32, device=DEV),
             ctl=torch.zeros(_lib.SPEC_CTL_INTS, dtype=I32, device=DEV), amax=torch.zeros(Lq, dtype=I32, device=DEV),
             ticket=torch.zeros(1, dtype=I32, device=DEV), d_past=torch.zeros(1, dtype=I32, device=DEV),
             d_step=torch.zeros(1, dtype=I32, device=DEV), history=torch.full((hist_cap,), -7, dtype=I32).pin_memory(),
             rec=torch.full((rec_cap, _lib.SPEC_REC_INTS), -7, dtype=I32).pin_memory())
    g["ctx"][:n] = torch.tensor(ctx, dtype=I32)
    g["ctl"].copy_(torch.tensor([n, 0, int(forced), 0, n_limit, 0, 0, 0], dtype=I32))
    g["tok"].fill_(ctx[-1] if tok0 is None else tok0)
    g["d_past"].fill_(n - 1 if d_past is None else d_past)
    g["state"] = ops.spec_state(g, n_max, n_min)
    return g


class PyState:
    """The rule of include/p3v.h applied by speculate.py to the same loop state."""

    def __init__(self, ctx, K, n_limit, forced=False, n_max=3, n_min=1, vocab=V_FULL):
        self.ctx, self.K, self.n_limit, self.forced, self.n_max, self.n_min, self.vocab = list(ctx), K, n_limit, forced, n_max, n_min, vocab
        self.drafts, self.tok0, self.d_past, self.d_step, self.hist, self.recs = [], ctx[-1], len(ctx) - 1, 0, [], []

    def propose(self):
        from phi_3_vision_mlx_amd import speculate
        return speculate.propose(self.ctx, self.K, self.n_max, self.n_min, self.vocab)

    def step(self, amax):
        from phi_3_vision_mlx_amd import speculate
        out = speculate.step(self.ctx, self.drafts, amax, self.n_limit)
        self.recs.append((len(out), len(self.drafts), list(self.drafts)))
        self.hist += out
        self.d_step += len(out)
        if out and out[-1] < 0:
            self.tok0, self.drafts = -1, []
            return
        self.ctx += out
        self.d_past += len(out)
        if out:
            self.tok0 = out[-1]
        if self.forced:
            self.drafts = []
        elif out:
            self.drafts = self.propose()


def _check(g, py, what):
    from phi_3_vision_mlx_amd import _lib
    torch.cuda.synchronize()
    ctl = g["ctl"].tolist()
    n = ctl[_lib.SPEC_CTL_N]
    assert int(g["ticket"][0]) == 0, f"{what}: arrival counter left at {int(g['ticket'][0])}"
    assert n == len(py.ctx), f"{what}: n {n} != {len(py.ctx)}"
    assert g["ctx"][:n].tolist() == py.ctx, what
    assert ctl[_lib.SPEC_CTL_NDRAFT] == len(py.drafts), f"{what}: n_draft {ctl[_lib.SPEC_CTL_NDRAFT]} != {py.drafts}"
    tok = g["tok"].tolist()
    assert tok[0] == py.tok0 and tok[1:1 + len(py.drafts)] == py.drafts, f"{what}: tok {tok} != {py.tok0} + {py.drafts}"
    if py.tok0 >= 0:
        assert all(0 <= t < py.vocab for t in tok), f"{what}: padding rows must be valid ids: {tok}"
    assert int(g["d_past"][0]) == py.d_past and int(g["d_step"][0]) == py.d_step, what
    assert ctl[_lib.SPEC_CTL_REPLAY] == len(py.recs), what
    assert g["history"][:len(py.hist)].tolist() == py.hist, f"{what}: history {g['history'][:len(py.hist) + 2].tolist()} != {py.hist}"
    assert int(g["history"][len(py.hist)]) == -7, f"{what}: a store behind the emitted run"
    for r, (c, k, d) in enumerate(py.recs):
        row = g["rec"][r].tolist()
        assert row[:2] == [c, k] and row[2:2 + k] == d, f"{what}: record {r} {row} != {(c, k, d)}"


def _logits(rng, amax, V=V_FULL, tie_rows=()):
    """[L, V] bf16 noise with the maximum planted at amax[j] (-1: a NaN row; tie_rows: a second equal maximum BEHIND it)."""
    lg = torch.from_numpy(rng.standard_normal((len(amax), V)).astype(np.float32) * 0.5)
    for j, a in enumerate(amax):
        if a < 0:
            lg[j, int(rng.integers(0, V))] = float("nan")
        else:
            lg[j, a] = 9.0
            if j in tie_rows and a + 1 < V:
                lg[j, int(rng.integers(a + 1, V))] = 9.0
    return lg.to(torch.bfloat16).to(DEV)


def _set_drafts(g, py, drafts):
    from phi_3_vision_mlx_amd import _lib
    py.drafts = list(drafts)
    if drafts:
        g["tok"][1:1 + len(drafts)] = torch.tensor(drafts, dtype=I32)
    g["ctl"][_lib.SPEC_CTL_NDRAFT] = len(drafts)


@pytest.mark.parametrize("K", [1, 4, 7, 15])
def test_spec_end_acceptance_every_prefix_ties_and_nan_rows(K):
    """Planted arg-maxes that match the first i drafts for every i and every n_draft 0..K; ties (first maximum); a NaN row inside
    and behind the accepted run; the budget cut.  The state after the launch is the rule's, exactly; the ticket is left zero."""
    from phi_3_vision_mlx_amd import ops
    rng = np.random.default_rng(K)
    base = rng.integers(0, 3, 40).tolist()                       # low entropy: the next proposal has several candidates
    for k in range(K + 1):
        for i in range(k + 1):
            for variant in ("plain", "tie", "nan_inside", "nan_behind", "budget"):
                drafts = rng.integers(0, 3, k).tolist()
                amax = drafts[:i] + [int((drafts[i] + 1) % 3) if i < k else int(rng.integers(0, 3))]
                amax += rng.integers(0, V_FULL, K + 1 - len(amax)).tolist()
                if variant == "nan_inside":
                    amax[int(rng.integers(0, i + 1))] = -1
                if variant == "nan_behind":
                    if i + 1 > K:
                        continue
                    amax[int(rng.integers(i + 1, K + 1))] = -1
                n_limit = len(base) + (max(0, i - 1) if variant == "budget" else 1000)
                g, py = _state(base, K, n_limit), PyState(base, K, n_limit)
                _set_drafts(g, py, drafts)
                ops.spec_end(_logits(rng, amax, tie_rows=range(K + 1) if variant == "tie" else ()), g["state"])
                py.step(amax)
                _check(g, py, f"K={K} k={k} i={i} {variant}")


def _lookup_cases():
    rng = np.random.default_rng(7)
    BIG = 1 << 30                                                  # (a vocabulary that holds every id of the distinct-id contexts)
    cases = [([5], "n=1", BIG), ([5, 5], "n=2", BIG), ([5, 6], "n=2 no match", BIG), ([5, 6, 5], "n=3", BIG), ([5, 5, 5], "n=3 same", BIG)]
    for n in (2500, 131072):
        uniq = (np.arange(n) + 100).tolist()
        cases.append((uniq, f"n={n} absent", BIG))
        a = list(uniq)
        a[-3:] = a[0:3]                                            # match at the very start
        cases.append((a, f"n={n} match at the start", BIG))
        a = list(uniq)
        a[-3:] = a[-7:-4]                                          # match at the very end (continuation runs into the suffix)
        cases.append((a, f"n={n} match at the end", BIG))
        a = list(uniq)
        a[-1] = a[-2]                                              # 1-gram, p = n - 2: a one-token draft
        cases.append((a, f"n={n} last two equal", BIG))
        cases.append((rng.integers(0, 3, n).tolist(), f"n={n} 3-symbol alphabet", V_FULL))
        a = rng.integers(0, 3, n)
        a[rng.integers(0, n, n // 50)] = -2                        # image-slot ids in between: drafts are cut in front of them
        a[rng.integers(0, n, n // 50)] = V_FULL + 3
        cases.append((a.tolist(), f"n={n} with ids outside the vocabulary", V_FULL))
    return cases


def test_ngram_propose_equals_the_python_rule():
    from phi_3_vision_mlx_amd import ops, speculate
    draft, nd = torch.zeros(16, dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    n_checked = 0
    for ctx, what, vocab in _lookup_cases():
        d_ctx = torch.tensor(ctx, dtype=I32, device=DEV)
        for K in (1, 4, 7, 15):
            for n_max, n_min in ((3, 1), (2, 2), (1, 1), (8, 1)):
                if len(ctx) > 10000 and (K, n_max) not in ((4, 3), (15, 8), (7, 1)):
                    continue
                draft.fill_(-9)
                ops.ngram_propose(d_ctx, len(ctx), K, n_max, n_min, vocab, draft, nd)
                want = speculate.propose(ctx, K, n_max, n_min, vocab)
                got = draft[:int(nd[0])].tolist()
                assert got == want, f"{what} K={K} n_max={n_max} n_min={n_min}: {got} != {want}"
                assert draft[int(nd[0]):].eq(-9).all(), f"{what}: stores behind the draft"
                n_checked += 1
    # a prefix of a longer buffer: ids behind n are never looked at
    buf = torch.tensor([1, 2, 3, 1, 2, 3, 1, 2], dtype=I32, device=DEV)
    ops.ngram_propose(buf, 5, 4, 3, 1, V_FULL, draft, nd)
    assert draft[:int(nd[0])].tolist() == speculate.propose([1, 2, 3, 1, 2], 4) == [3, 1, 2]
    assert n_checked > 60
    with pytest.raises(RuntimeError):
        ops.ngram_propose(buf, 5, 16, 3, 1, V_FULL, torch.zeros(16, dtype=I32, device=DEV), nd)     # K > P3V_DECODE_MAX_L - 1
    with pytest.raises(RuntimeError):
        ops.ngram_propose(buf, 5, 4, 9, 1, V_FULL, draft, nd)                                       # n_max > P3V_SPEC_NGRAM_CAP


@pytest.mark.parametrize("K,n,budget", [(4, 2500, None), (7, 131072, None), (15, 3, 9), (1, 1, 9), (4, 2, 9)])
def test_ten_launches_in_a_row_follow_the_rule(K, n, budget):
    """Ten spec_end launches on ONE state with the device's own proposals in between: a scripted "model" that continues the
    period-5 pattern of the context most of the time; every state equals the Python rule's, the counter is zero after each."""
    from phi_3_vision_mlx_amd import ops
    rng = np.random.default_rng(n + K)
    pattern = [11, 12, 13, 11, 14]
    ctx = [pattern[i % 5] for i in range(n)]
    n_limit = n + (budget or 1000)                               # budget 9: every launch emits at least one token, so the tenth
                                                                 # is a launch AT the budget: nothing emitted, nothing moved
    g, py = _state(ctx, K, n_limit, cap=n + 10 * (K + 1) + 8), PyState(ctx, K, n_limit)
    d, nd = torch.zeros(16, dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    ops.ngram_propose(g["ctx"], n, K, 3, 1, V_FULL, d, nd)
    _set_drafts(g, py, d[:int(nd[0])].tolist())
    assert py.drafts == py.propose()
    for launch in range(10):
        # the model's answer for every row: the pattern's continuation, with a deviation at a random row of most launches
        rows = [py.tok0] + py.drafts
        amax, c = [], list(py.ctx[:-1])
        for j in range(K + 1):
            c.append(rows[j] if j < len(rows) else 0)
            amax.append(pattern[len(c) % 5])
        if launch % 3 != 2:
            amax[int(rng.integers(0, K + 1))] = int(rng.integers(20, 30))
        ops.spec_end(_logits(rng, amax), g["state"])
        py.step(amax)
        _check(g, py, f"launch {launch}")
    if budget is None:
        assert sum(c - 1 for c, _, _ in py.recs) > 0 and any(k > 0 and c - 1 < k for c, k, _ in py.recs), py.recs
    else:
        assert len(py.ctx) == n_limit and py.recs[-1][0] == 0, py.recs


def test_spec_begin_rows_and_rotation():
    from phi_3_vision_mlx_amd import ops
    torch.manual_seed(0)
    V, H, T, half = 300, 64, 40, 16
    table = torch.randn(V, H, device=DEV).to(torch.bfloat16)
    cos_t, sin_t = torch.randn(1, T, half, device=DEV), torch.randn(1, T, half, device=DEV)
    for Lq, past in ((1, 0), (5, 17), (16, 24), (16, 30)):          # the last one runs over the table's end: clamped rows
        tok = torch.randint(0, V, (Lq,), dtype=I32, device=DEV)
        tok[0] = -4                                               # out-of-range ids are clamped, as p3v_embed_gather does
        x = torch.zeros(Lq, H, dtype=torch.bfloat16, device=DEV)
        co, so = torch.zeros(1, Lq, half, device=DEV), torch.zeros(1, Lq, half, device=DEV)
        ops.spec_begin(tok, table, x, cos_t, sin_t, torch.tensor([past], dtype=I32, device=DEV), co, so)
        pos = torch.clamp(torch.arange(Lq, device=DEV) + past, max=T - 1)
        assert torch.equal(x, table[tok.clamp(0, V - 1).long()])
        assert torch.equal(co[0], cos_t[0, pos]) and torch.equal(so[0], sin_t[0, pos])


# ----------------------------------------------------------------------------- the tiny model under the fixture's head
def _fixture():
    g = np.load(os.path.join(GOLDEN, "tiny_spec_oracle.npz"))
    return g, g["tokens"].reshape(-1).tolist(), int(g["first_unclear"][0])


def _tiny(**kw):
    from gen_golden_spec import chat_text
    from phi_3_vision_mlx_amd.api import load_synthetic
    g, fix, n_cmp = _fixture()
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device=DEV,
                                 lm_head_spread=float(g["spread"][0]), lm_head_seed=int(g["head_seed"][0]), **kw)
    inputs = proc(chat_text())
    assert np.array_equal(np.asarray(inputs["input_ids"]).reshape(-1), g["ids"])
    return model, proc, inputs, fix, n_cmp


def _prefill(model, inputs, max_tokens, K):
    from phi_3_vision_mlx_amd import ops
    logits, cache = model(**inputs, max_tokens=max_tokens, extra_tokens=K)
    return ops.argmax(logits[:, -1, :].contiguous())[:, None], cache


def _run(model, cache, ids, token, K, n_tokens, forced=None, eager=False, trace=None):
    """Verify steps, one sync per step, until n_tokens tokens exist (the prefill token included).  forced(out) -> the drafts of
    the next step.  Returns (tokens, records [(emitted, drafted, drafts)])."""
    from phi_3_vision_mlx_amd import speculate
    st = cache[0].state
    S = st.offset
    g = model.spec_start(cache, ids, token, K, n_limit=S + n_tokens, forced=forced is not None)
    out, recs = [int(token.reshape(-1)[0])], []
    while len(out) < n_tokens:
        if forced is not None:
            model.spec_force(cache, forced(out))
        elif trace is not None:
            trace.append(speculate.propose(list(ids) + out, K, vocab=model.cfg.vocab_size))
        model.spec_step(cache, K, eager=eager)
        toks = model.spec_sync(cache)
        r = g["rec"][g["n_replays"] - 1].tolist()
        recs.append((r[0], r[1], r[2:2 + r[1]]))
        assert len(toks) == len(out) - 1 + r[0] and r[0] >= 1
        out = out[:1] + toks
        assert st.offset == S + len(out) - 1
    return out, recs


@pytest.mark.parametrize("K", [4, 7])
def test_tokens_equal_the_oracle_fixture_with_the_device_drafter(K):
    model, proc, inputs, fix, n_cmp = _tiny()
    ids = np.asarray(inputs["input_ids"]).reshape(-1).tolist()
    token, cache = _prefill(model, inputs, len(fix), K)
    trace = []
    out, recs = _run(model, cache, ids, token, K, len(fix), trace=trace)
    assert out[:n_cmp] == fix[:n_cmp], f"{out} != oracle {fix} (compared up to its first unclear step {n_cmp})"
    assert len(out) == len(fix)
    for i, (rec, want) in enumerate(zip(recs, trace)):           # every step's draft is speculate.propose of its context
        assert rec[2] == want, f"step {i}: drafts {rec[2]} != {want}"
    steps, accepted = len(recs), sum(c - 1 for c, _, _ in recs)
    assert sum(c for c, _, _ in recs) == steps + accepted == len(out) - 1
    assert accepted > 0 and any(k > 0 and c - 1 < k for c, k, _ in recs), recs
    print(f"K={K}: {steps} steps, {sum(k for _, k, _ in recs)} drafted, {accepted} accepted, {len(out) - 1} tokens")


@pytest.mark.parametrize("K", [4, 7])
def test_forced_drafts_all_accepted_and_all_rejected(K):
    model, proc, inputs, fix, n_cmp = _tiny()
    ids = np.asarray(inputs["input_ids"]).reshape(-1).tolist()
    # (a) drafts taken from the fixture: everything is accepted, K + 1 tokens per step
    token, cache = _prefill(model, inputs, n_cmp, K)
    out, recs = _run(model, cache, ids, token, K, n_cmp, forced=lambda o: fix[len(o):min(len(o) + K, n_cmp - 1)])
    assert out == fix[:n_cmp]
    assert all(c - 1 == k for c, k, _ in recs), recs
    assert len(recs) == math.ceil((n_cmp - 1) / (K + 1))
    # (b) drafts that are the fixture's token + 1: nothing is accepted, one token per step
    token, cache = _prefill(model, inputs, n_cmp, K)
    out, recs = _run(model, cache, ids, token, K, n_cmp, forced=lambda o: [t + 1 for t in fix[len(o):len(o) + K]])
    assert out == fix[:n_cmp]
    assert all(c == 1 and k == min(K, len(fix) - i - 1) for i, (c, k, _) in enumerate(recs)), recs
    assert len(recs) == n_cmp - 1


def test_captured_step_equals_eager_step_bit_for_bit_and_rebuild_after_rewind():
    K = 4
    model, proc, inputs, fix, n_cmp = _tiny()
    ids = np.asarray(inputs["input_ids"]).reshape(-1).tolist()

    def drafts(o):                                                # right, wrong at the second place, wrong at once, in turn
        d = fix[len(o):len(o) + K]
        turn = drafts.n % 3
        drafts.n += 1
        return d if turn == 0 else (d[:1] + [t + 1 for t in d[1:]] if turn == 1 else [t + 1 for t in d])
    runs = []
    for eager in (False, True):
        drafts.n = 0
        token, cache = _prefill(model, inputs, len(fix), K)
        st = cache[0].state
        g = model.spec_start(cache, ids, token, K, forced=True)
        out, snaps = [int(token[0, 0])], []
        for _ in range(12):
            model.spec_force(cache, drafts(out))
            model.spec_step(cache, K, eager=eager)
            out = out[:1] + model.spec_sync(cache)
            snaps.append((g["logits"].clone(), g["tok"].clone(), int(g["d_past"][0]), list(out)))
        runs.append((snaps, g["rec"][:12].clone(), st, cache))
    (a, rec_a, st, cache), (b, rec_b, _, _) = runs
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0].view(torch.int16), y[0].view(torch.int16)), f"step {i}: logits differ between replay and eager"
        assert torch.equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3], f"step {i}"
    assert torch.equal(rec_a, rec_b)
    counts = rec_a[:, 0].tolist()
    assert 1 in counts and 2 in counts and K + 1 in counts, counts  # a rejection at once, a partial run, a full run
    assert a[-1][3][:n_cmp] == fix[:n_cmp][:len(a[-1][3])]
    # rewind below the captured lower bound: the capture is rebuilt (as greedy_step rebuilds), and the run goes on correctly
    S = len(ids)
    g_old = st.graphs["spec"]
    assert g_old["bufs"]["plan"].past_lb == S
    token, cache = _prefill(model, inputs, len(fix), K)
    st = cache[0].state
    tok = token
    for _ in range(6):
        _, tok = model.greedy_step(tok, cache)
    torch.cuda.synchronize()
    g1 = model.spec_start(cache, ids + fix[:6], tok, K)
    assert g1["bufs"]["plan"].past_lb == S + 6
    model.spec_step(cache, K)
    model.spec_sync(cache)
    st.offset = S + 2
    g2 = model.spec_start(cache, ids + fix[:2], torch.tensor([[fix[2]]], dtype=I32), K)
    assert g2 is not g1 and g2["bufs"]["plan"].past_lb == S + 2
    out = fix[:3]
    while len(out) < n_cmp:
        model.spec_step(cache, K)
        out = fix[:3] + model.spec_sync(cache)
    assert out[:n_cmp] == fix[:n_cmp]


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


def test_hand_over_to_the_plain_path_and_speculate_0_is_the_plain_path():
    from phi_3_vision_mlx_amd import api
    K = 4
    model, proc, inputs, fix, n_cmp = _tiny()
    ids = np.asarray(inputs["input_ids"]).reshape(-1).tolist()
    S = len(ids)
    # 10 tokens speculatively through the public loop, then plain greedy steps on the same cache
    token, cache = _prefill(model, inputs, len(fix), K)
    st = cache[0].state
    seen = []
    stop = type("Never", (), {"__call__": lambda self, rows: False})()
    info = {}
    last = api.speculative_loop(model, ids, token, cache, 9, K, lambda rows: seen.append(rows[0]), stop, info)
    out = [int(token[0, 0])] + seen
    assert len(out) == 10 and out == fix[:10] and int(last.reshape(-1)[0]) == fix[9]
    assert st.offset == S + 10 - 1                               # prompt + emitted tokens - 1: what the plain loop leaves
    assert info["emitted"] == info["steps"] + info["accepted"] >= 9
    tok = last
    for _ in range(n_cmp - 10):
        _, tok = model.greedy_step(tok, cache)
        out.append(int(tok.reshape(-1)[0]))
    assert out == fix[:n_cmp] and st.offset == S + n_cmp - 1
    # speculate=0: launch for launch the plain path -- the same launches by name and count as the model-level plain loop, the
    # same history and replay count
    proc.tokenizer = _IdTokenizer(proc.tokenizer)
    from gen_golden_spec import chat_text
    n_tok = 12

    def plain():
        logits, cache = model(**proc(chat_text()), max_tokens=n_tok)
        from phi_3_vision_mlx_amd import ops
        tok = ops.argmax(logits[:, -1, :].contiguous())[:, None]
        first = int(tok[0, 0])
        for _ in range(n_tok - 1):
            _, tok = model.greedy_step(tok, cache)
        torch.cuda.synchronize()
        g = cache[0].state.graphs["greedy"]
        return [first] + g["history"][0, :n_tok - 1].tolist(), g["n_replays"], sorted(cache[0].state.graphs)

    def via_generate(**kw):
        states = []
        real = model._new_state

        def spy(*a, **k):
            states.append(real(*a, **k))
            return states[-1]
        model._new_state = spy
        try:
            txt = api._generate(model, proc, chat_text(), max_tokens=n_tok, verbose=False, stream=False, mute=True, **kw)
        finally:
            del model._new_state
        g = states[-1].graphs["greedy"]
        return [int(t) for t in txt[0].split()], g["history"][0, :n_tok - 1].tolist(), g["n_replays"], sorted(states[-1].graphs)
    os.environ["P3V_PREFILL_GRAPH"] = "0"                         # (every run below prefills eagerly: comparable launch counts)
    try:
        plain()                                                  # (uncounted: builds what a model builds once, e.g. the rotation table)
        with _Count() as c_plain:
            toks_p, n_p, graphs_p = plain()
        with _Count() as c_default:
            txt_d, hist_d, n_d, graphs_d = via_generate()
        with _Count() as c_zero:
            txt_0, hist_0, n_0, graphs_0 = via_generate(speculate=0)
    finally:
        del os.environ["P3V_PREFILL_GRAPH"]
    assert c_zero.n == c_default.n, (c_zero.n, c_default.n)
    drop = lambda d: {k: v for k, v in d.items() if k not in ("p3v_argmax",)}    # (the host loop's own token plumbing)
    assert drop(c_zero.n) == drop(c_plain.n), (c_zero.n, c_plain.n)
    assert not any("spec" in k or "ngram" in k for k in c_zero.n)
    assert txt_0 == txt_d == toks_p and hist_0 == hist_d == toks_p[1:] and n_0 == n_d == n_p == n_tok - 1
    assert graphs_0 == graphs_d == graphs_p == ["greedy"]


class _IdTokenizer:
    """Delegates encoding to the real tokenizer; decodes to the ids themselves, so texts compare as tokens."""

    def __init__(self, real):
        self.real = real

    def __call__(self, *a, **kw):
        return self.real(*a, **kw)

    def encode(self, *a, **kw):
        return self.real.encode(*a, **kw)

    def decode(self, ids, **kw):
        return " ".join(str(int(i)) for i in ids)

    def batch_decode(self, seqs, **kw):
        return [self.decode(s) for s in seqs]


def test_generate_speculate_returns_exactly_max_tokens_and_the_plain_text():
    from gen_golden_spec import chat_text
    from phi_3_vision_mlx_amd import api
    model, proc, inputs, fix, n_cmp = _tiny()
    proc.tokenizer = _IdTokenizer(proc.tokenizer)
    kw = dict(verbose=False, stream=False, mute=True)
    for m in (1, 2, 3, 6, 13):
        info = {}
        spec = api._generate(model, proc, chat_text(), max_tokens=m, speculate=4, spec_info=info, **kw)[0].split()
        plain = api._generate(model, proc, chat_text(), max_tokens=m, **kw)[0].split()
        assert len(spec) == m == len(plain)
        assert [int(t) for t in spec] == fix[:m] == [int(t) for t in plain], (m, spec, plain)
        assert info["emitted"] == info["steps"] + info["accepted"] and (m > 1) == (info["steps"] > 0)
    # the public generate (chat template applied by it) takes the same keyword
    kw_pub = dict(verbose=False, stream=False)
    txt = api.generate("Repeat: a b a b a b", preload=(model, proc), max_tokens=6, speculate=4, **kw_pub)
    assert txt == api.generate("Repeat: a b a b a b", preload=(model, proc), max_tokens=6, **kw_pub)
    # refusals: a ValueError that names the limit
    with pytest.raises(ValueError, match="B = 1"):
        api._generate(model, proc, [chat_text(), chat_text()], max_tokens=4, speculate=4, **kw)
    with pytest.raises(ValueError, match="temperature"):
        api._generate(model, proc, chat_text(), max_tokens=4, speculate=4, temperature=0.8, seed=1, **kw)
    with pytest.raises(ValueError, match="early_stop"):
        api._generate(model, proc, chat_text(), max_tokens=4, speculate=4, early_stop=True, **kw)
    with pytest.raises(ValueError, match="15"):
        api._generate(model, proc, chat_text(), max_tokens=4, speculate=16, **kw)
    for cfg_kw, word in ((dict(tiny=True, use_quantized_cache=True, cache_format="mlx4"), "mlx4"),
                         (dict(tiny=True, use_quantized_cache=True), "int8"),
                         (dict(tiny=False, num_hidden_layers=2, quantized_fp8=True), "bf16 weights"),
                         (dict(tiny=False, num_hidden_layers=2, quantized_int4=True), "bf16 weights")):
        m2, p2 = api.load_synthetic(blind_model=True, seed=0, device=DEV, **cfg_kw)
        with pytest.raises(ValueError, match=word):
            api._generate(m2, p2, chat_text(), max_tokens=4, speculate=4, **kw)


# ----------------------------------------------------------------------------- 7. full width, 2 layers, against the plain path
HEAD_SEED_FULL = 9                 # head seeds 0 .. 24 give 15 .. 31 clear steps of 32 on the plain path; 9 gives 31


def _full_width(head_seed):
    """No fixture: speculate=4 on a 300-token prompt (a 50-token block repeated), 32 tokens; then the plain captured step,
    teacher-forced on those tokens.  Wherever the plain path's own top-2 clearance (the fixtures' rule, rel_tol 0.03) exceeds 1
    the speculative token must be the plain path's arg-max.  At least 24 of the 32 steps must be clear on the plain path:
    otherwise HEAD_SEED_FULL is changed, not the bar.  Returns (clear steps, statistics)."""
    from phi_3_vision_mlx_amd import api
    K, n_tok, rel_tol = 4, 33, 0.03
    model, proc = api.load_synthetic(blind_model=True, tiny=False, seed=0, device=DEV, num_hidden_layers=2, lm_head_spread=4.0,
                                     lm_head_seed=head_seed)
    rng = np.random.default_rng(0)
    ids = np.tile(rng.integers(1000, 30000, 50), 6).astype(np.int32)[None]
    inputs = {"input_ids": ids}
    token, cache = _prefill(model, inputs, n_tok, K)
    seen, info = [], {}
    stop = type("Never", (), {"__call__": lambda self, rows: False})()
    api.speculative_loop(model, ids.reshape(-1), token, cache, n_tok - 1, K, lambda rows: seen.append(rows[0]), stop, info)
    spec = [int(token[0, 0])] + seen
    assert len(spec) == n_tok
    # the plain path, teacher-forced on the speculative run's tokens
    logits, cache = model(**inputs, max_tokens=n_tok)
    norms = model.w["lm_head.weight"].float().norm(dim=-1).clamp_min(1e-30)
    n_clear, rows = 0, [logits[0, -1].float()]
    for t in spec[:-1]:
        lg, _ = model.greedy_step(torch.tensor([[t]], dtype=I32, device=DEV), cache)
        rows.append(lg[0, 0].float().clone())
    for i, lf in enumerate(rows[1:], start=1):                    # rows[i]: the plain path's logits for token i
        v, ix = lf.topk(2)
        E = rel_tol * (lf / norms).abs().max()
        clear = float((v[0] - v[1]) / (E * (norms[ix[0]] + norms[ix[1]])))
        if clear > 1.0:
            n_clear += 1
            assert spec[i] == int(ix[0]), f"token {i}: speculative {spec[i]} != plain arg-max {int(ix[0])} (clearance {clear:.2f})"
    print(f"full width, head seed {head_seed}: {n_clear} of {n_tok - 1} steps clear on the plain path; {info}")
    assert info["emitted"] == info["steps"] + info["accepted"]
    return n_clear, info


def test_full_width_two_layers_every_clear_token_is_the_plain_paths_argmax():
    n_clear, info = _full_width(HEAD_SEED_FULL)
    assert n_clear >= 24, f"only {n_clear} clear steps: pick another HEAD_SEED_FULL"


# ----------------------------------------------------------------------------- 8. server round trip
def test_server_round_trip_with_speculate():
    from gen_golden_spec import PROMPT
    from phi_3_vision_mlx_amd import api
    from phi_3_vision_mlx_amd.server import serve
    model, proc, inputs, fix, n_cmp = _tiny()
    proc.tokenizer = _IdTokenizer(proc.tokenizer)

    def generate_fn(prompts, max_tokens, images=None, sampling=None, adapter=None, speculate=0, spec_info=None):
        return api.generate(prompts[0], preload=(model, proc), max_tokens=max_tokens, verbose=False, speculate=speculate, spec_info=spec_info)
    httpd, engine = serve(generate_fn, port=0, host="127.0.0.1", device=model.device, speculate=True)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()

    def post(body):
        req = urllib.request.Request(f"http://127.0.0.1:{httpd.server_address[1]}/v1/completions", data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=300) as r:
            return json.loads(r.read())
    try:
        plain = post({"prompt": PROMPT, "max_tokens": n_cmp})
        spec = post({"prompt": PROMPT, "max_tokens": n_cmp, "speculate": 4})
    finally:
        httpd.shutdown()
        engine.close()
    assert "speculation" not in plain and set(spec["speculation"]) == {"steps", "drafted", "accepted"}
    assert spec["responses"] == plain["responses"]
    assert [int(t) for t in spec["responses"][0].split()] == fix[:n_cmp]
    assert spec["speculation"]["accepted"] > 0 and spec["speculation"]["steps"] < n_cmp - 1
