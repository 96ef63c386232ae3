"""share_prefix at the model level, on the tiny model of tests/golden/tiny_serve_oracle.npz with the bf16 cache: the rows of a
family read their prompt's K/V once (model.set_families -> ops.attention_decode_family).  The family here is the fixture's image
request (2,5xx prompt tokens: nine 256-key splits below share_end), so the shared splits carry nearly all of the keys.

Two kinds of comparison:
  * a state whose table names the family against the SAME state with the table cleared (set_families(st, [])): the same launch,
    the same split plan -- tokens, logits and records must be equal bit for bit, whatever else the request asks for;
  * share_prefix=True against share_prefix=False: two split plans -- logits within the tolerance tests/test_model_gpu.py applies
    between two split plans of this model (assert_logits(..., rel_atol=1e-2), "merge in launch vs merge launch"), tokens equal
    wherever the top-two gap exceeds twice that tolerance."""
import json
import threading
import urllib.request

import numpy as np
import pytest
import torch

from attn_probe import POISON
from test_kv_fork_gpu import EOS, SEED, _cache_of, _Count, _cut, _hand_family, _serve, _spy_forks
from test_model_gpu import assert_logits

pytestmark = pytest.mark.gpu
N, STEPS = 4, 23                                                  # rows of the family; decode steps after the first token
_RUNS = {}


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _dead_end(model, st):
    """Columns [0, dead_end) of a follower are not read: the whole family-plan splits below share_end."""
    from phi_3_vision_mlx_amd import ops
    plan = model._plan(st, st.B, 1, fuse_o=False)["plan"]
    assert plan.family
    chunk = ops.attention_family_chunk(st.Tp, plan.n_split)
    (rows, share_end), = st.families
    return share_end // chunk * chunk, chunk


def _run(share, table="family", temperature=0.8, force=None, after_fork=None, steps=STEPS, which=0):
    """The image request prefilled once, forked into N rows, first tokens from the one logits row, `steps` captured steps.
    share: fork_state(share=True); table "cleared": set_families(st, []) after the fork (the launch stays, the table names
    nobody).  force: the tokens to feed instead of the run's own (teacher forcing).  -> dict(toks [steps + 1][N], lgs, st)."""
    from phi_3_vision_mlx_amd import sampling
    g, model, proc, reqs = _serve()
    logits, cache = model(**reqs[which], max_tokens=STEPS + 1)      # (one capacity, so one split plan, whatever `steps`)
    cache = model.fork_state(cache[0].state, N, **({"share": True} if share else {}))
    st = cache[0].state
    if table == "cleared":
        model.set_families(st, [])
    if after_fork is not None:
        after_fork(model, st)
    recs = sampling.rows(N, temperature, 0, 1.0, 3)
    model.set_sampling(st, sampling.pack(recs, 0))
    token = model.sample_logits(st, logits[:, -1].expand(N, -1).contiguous())
    toks, lgs = [token.reshape(-1).tolist()], []
    for i in range(steps):
        if force is not None:
            token = torch.tensor(force[i], dtype=torch.int32, device=token.device).view(-1, 1)
        lg, token = model.sample_step(token, cache)
        torch.cuda.synchronize()
        lgs.append(lg.reshape(N, -1).clone())
        toks.append(token.reshape(-1).tolist())
    return dict(toks=toks, lgs=lgs, st=st)


def _memo(key, **kw):
    if key not in _RUNS:
        _RUNS[key] = _run(**kw)
    return _RUNS[key]


@pytest.mark.parametrize("temperature", [0.8, 0.0])
def test_a_family_equals_the_cleared_table_bit_for_bit(temperature):
    from golden_inputs import SERVE_TEXTS, make_image
    from phi_3_vision_mlx_amd import api
    g, model, proc, _ = _serve()
    a = _memo(("family", temperature), share=True, temperature=temperature)
    b = _memo(("cleared", temperature), share=True, table="cleared", temperature=temperature)
    st = a["st"]
    assert st.family is not None and len(st.families) == 1 and b["st"].family is not None and b["st"].families == []
    assert st.graphs["greedy"]["bufs"]["plan"].family and b["st"].graphs["greedy"]["bufs"]["plan"].family
    dead_end, chunk = _dead_end(model, st)
    assert dead_end >= 2048 and dead_end >= 8 * chunk, (dead_end, chunk)   # the comparison is about many shared splits
    assert a["toks"] == b["toks"]
    for step, (x, y) in enumerate(zip(a["lgs"], b["lgs"])):
        assert torch.equal(_bits(x), _bits(y)), f"logits of step {step}"
    rows = list(zip(*a["toks"]))
    if temperature:
        assert len(set(rows)) > 1, "four seeds gave four equal rows: nothing was sampled"
    else:
        assert len(set(rows)) == 1                                 # greedy: the completions are equal to each other
    out = api._generate(model, proc, SERVE_TEXTS[0], [make_image(336, 336, "noise", 0)], max_tokens=STEPS + 1, verbose=False,
                        stream=False, mute=True, n=N, temperature=temperature, seed=3, share_prefix=True)
    for j, text in enumerate(out):                                 # api.generate runs the same steps (its text ends at the row's EOS)
        got = [int(t) for t in text.split()]
        assert len(got) >= min(4, len(_cut(list(rows[j]), STEPS + 1)) - 1) and got == list(rows[j])[:len(got)], j


def test_share_prefix_against_the_unshared_plan():
    """The prompt is the fixture's image request and the rows are greedy (the same tokens in every row); the shared run is fed
    the unshared run's tokens.  At most a quarter of the steps may be too close to call: the unshared run alone decides which."""
    g, model, proc, _ = _serve()
    ref = _memo(("unshared", 0.0), share=False, temperature=0.0)
    assert ref["st"].family is None and not ref["st"].graphs["greedy"]["bufs"]["plan"].family
    got = _run(share=True, temperature=0.0, force=ref["toks"][:-1])
    unclear = 0
    for step, (x, y) in enumerate(zip(got["lgs"], ref["lgs"])):
        atol = assert_logits(x, y, f"shared vs unshared, step {step}", rel_atol=1e-2)
        top2 = y.float().topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 2 * atol
        unclear += int(not bool(clear.all()))
        for r in range(N):
            if clear[r]:
                assert got["toks"][step + 1][r] == ref["toks"][step + 1][r], (step, r)
    print(f"steps too close to call: {unclear} of {STEPS}")
    assert unclear <= STEPS // 4


def test_the_followers_prefix_is_not_read():
    def poison(model, st):
        dead_end, _ = _dead_end(model, st)
        assert dead_end > 2000
        for r in range(1, N):
            st.k[:, r, :, :dead_end] = POISON
            st.v[:, r, :, :, :dead_end] = POISON
    clean = _memo(("family", 0.8), share=True, temperature=0.8)
    dirty = _run(share=True, after_fork=poison, steps=16)
    assert dirty["toks"] == clean["toks"][:17]
    for step, (x, y) in enumerate(zip(dirty["lgs"], clean["lgs"])):
        assert torch.equal(_bits(x), _bits(y)), f"logits of step {step}"
    dead_end, _ = _dead_end(_serve()[1], dirty["st"])
    assert bool((dirty["st"].k[:, 1:, :, :dead_end] == POISON).all())


def test_the_captured_step_follows_the_table():
    """Eight replays, then row 2 becomes the leader and the old leader's shared columns are poisoned, then eight more: the logits
    are those of a twin state nobody touched, and the graph object is the one captured before."""
    g, model, proc, _ = _serve()
    twin = _memo(("family", 0.8), share=True, temperature=0.8)
    state = {}

    def run_half(model_, st):
        state["st"] = st
    a = _run(share=True, after_fork=run_half, steps=8)
    st = state["st"]
    graph = st.graphs["greedy"]["sample_graph"]
    (rows, share_end), = st.families
    assert rows[0] == 0
    model.set_families(st, [((2, 0, 1, 3), share_end)])
    dead_end, _ = _dead_end(model, st)
    st.k[:, 0, :, :dead_end] = POISON
    st.v[:, 0, :, :, :dead_end] = POISON
    token = torch.tensor(a["toks"][-1], dtype=torch.int32, device="cuda:0").view(-1, 1)
    cache = _cache_of(st)
    for step in range(8, 16):
        lg, token = model.sample_step(token, cache)
        torch.cuda.synchronize()
        assert torch.equal(_bits(lg.reshape(N, -1)), _bits(twin["lgs"][step])), f"logits of step {step}"
        assert token.reshape(-1).tolist() == twin["toks"][step + 1]
    assert st.graphs["greedy"]["sample_graph"] is graph and a["toks"] == twin["toks"][:9]


def _with_table(model):
    """model.new_slot_state that makes the family table at once (all single rows): the plan of a share_prefix engine."""
    real = model.new_slot_state

    def make(*a, **kw):
        st = real(*a, **kw)
        model.set_families(st, [], create=True)
        return st
    model.new_slot_state = make


def test_engine_family_shares_its_prefix_and_members_leave_one_by_one():
    """A sampled family of 3 of the image request joins a share_prefix engine beside a running request; a logit_bias lets its
    rows end at different steps, and a newcomer is refilled into the first row that leaves while the others still run.  The
    family's tokens are those of the same rows driven by hand on a state with a table of single rows (the same launch and plan;
    a family changes no bit), the newcomer's are those of its run alone, and no row is ever prefilled while a table entry names it."""
    from phi_3_vision_mlx_amd import penalties as pm
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, n_args, penalty_args
    g, model, proc, reqs = _serve()
    T, budget = 1.0, 14
    lg = model(**reqs[0], max_tokens=1)[0][0, -1].float()
    others = torch.logsumexp(torch.cat([lg[:EOS], lg[EOS + 1:]]) / T, 0)
    bias = {EOS: float(T * (np.log(0.2 / 0.8) + others) - lg[EOS])}
    settings = dict(temperature=T, top_k=0, top_p=1.0, seed=SEED)
    refills, real_prefill = [], model.prefill_slot

    def run(with_family):
        eng = ContinuousEngine(model, proc, slots=4, window=4096, share_prefix=True)

        def spy(st, row, inputs, **kw):
            n_rows = np.asarray(inputs["input_ids"]).reshape(-1, np.asarray(inputs["input_ids"]).shape[-1]).shape[0]
            named = {int(x) for x in st.family_host[:, 0].tolist()} | {r for rows, _ in eng.families for r in rows}
            refills.append((row, int(st.offset), with_family))
            lead_of_others = [b for b in range(st.B) if b not in range(row, row + n_rows) and int(st.family_host[b, 0]) in range(row, row + n_rows)]
            assert not lead_of_others, (row, lead_of_others)
            assert all(r not in range(row, row + n_rows) for rows, _ in eng.families for r in rows)
            return real_prefill(st, row, inputs, **kw)
        model.prefill_slot = spy
        try:
            a = eng.submit(reqs[0], 30)                              # (the image request: the family below fits its column)
            eng.step(), eng.step()
            head, late = None, None
            if with_family:
                head = eng.submit(n_args(penalty_args(reqs[0], logit_bias=bias), 3), budget, sampling=settings)
                eng.step()
                assert eng.families and len(eng.families[0][0]) >= 2 and eng.st.family is not None   # (a member may end on its first token)
                for _ in range(60):
                    if any(c.done.is_set() for c in head.members) or not eng._active():
                        break
                    eng.step()
            late = eng.submit(reqs[3], 6)
            eng.run_until_idle()
            assert eng.failures == 0 and a.error is None and late.error is None and eng.families == []
            assert eng.st.family_host[:, 0].tolist() == list(range(4))
            return eng, a, head, late
        finally:
            del model.prefill_slot
    from test_serving_gpu import tokens_vs_fixture
    _, alone, _, late_alone = run(False)
    forks = _spy_forks(model)
    try:
        eng, a, head, late = run(True)
    finally:
        del model.fork_rows
    assert a.tokens == alone.tokens and len(late.tokens) >= 1
    # the newcomer, refilled into a departed member's row, against the same request alone in that row at that column of a fresh
    # state with the same plan (a table of single rows): the same tokens, all of them
    (late_col,) = [col_ for row_, col_, fam_ in refills if fam_ and row_ == late.row][-1:]
    _with_table(model)
    try:
        solo, _ = _hand_family(model, 4, late_col, [late.row], reqs[3], [(0.0, 0, 1.0, 0)], 5)
    finally:
        del model.new_slot_state
    assert late.tokens == _cut(solo[late.row], 6), (late.row, late_col, late.tokens, solo[late.row])
    assert tokens_vs_fixture([late.tokens], g, "a row refilled after a member left", rows=[3], min_first=1, budgets=[6]) >= 1
    assert tokens_vs_fixture([late_alone.tokens], g, "the same request without a family around", rows=[3], min_first=1, budgets=[6]) >= 1
    lens = [len(c.tokens) for c in head.members]
    print("family lengths:", lens, "rows", [c.row for c in head.members], "newcomer row", late.row)
    assert len(set(lens)) > 1 and late.row in [c.row for c in head.members]      # a member left early and its row was refilled
    rows = [c.row for c in head.members]
    (col, src, dst), = forks
    assert [src] + dst == rows
    recs = [(T, 0, 1.0, SEED + j) for j in range(3)]
    _with_table(model)
    try:
        toks, _ = _hand_family(model, 4, col, rows, reqs[0], recs, budget - 1, pen=pm.request_row(dict(logit_bias=bias), model.cfg.vocab_size))
    finally:
        del model.new_slot_state
    for c in head.members:
        assert c.tokens == _cut(toks[c.row], budget), (c.row, c.tokens, toks[c.row])


def _generate(share, clear=False, on=None, **kw):
    """api._generate of the image request as a family (on = (model, processor, text): of that text prompt on that model); clear:
    the table is emptied right after the fork."""
    from golden_inputs import SERVE_TEXTS, make_image
    from phi_3_vision_mlx_amd import api
    if on is None:
        g, model, proc, _ = _serve()
        text, images = SERVE_TEXTS[0], [make_image(336, 336, "noise", 0)]
    else:
        (model, proc, text), images = on, None
    real = model.fork_state

    def fork(st1, n, **k):
        cache = real(st1, n, **k)
        assert (cache[0].state.family is not None) == bool(share)
        if clear:
            model.set_families(cache[0].state, [])
        return cache
    model.fork_state = fork
    try:
        return api._generate(model, proc, text, images, max_tokens=10, verbose=False,
                             stream=False, mute=True, **({"share_prefix": True} if share else {}), **kw)
    finally:
        del model.fork_state


def test_best_of_with_sharing():
    kw = dict(n=2, best_of=4, temperature=1.0, seed=11, logprobs=2)
    ia, ib, fa, fb = {}, {}, {}, {}
    a = _generate(True, logprob_info=ia, family_info=fa, **kw)
    b = _generate(True, clear=True, logprob_info=ib, family_info=fb, **kw)
    assert a == b and len(a) == 2 and fa == fb and ia == ib and len(ia["token_logprobs"]) == 2


def test_penalties_and_logprobs_with_sharing():
    kw = dict(n=3, temperature=0.9, seed=5, logprobs=1, repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2,
              logit_bias={100: 2.0, 101: -3.0})
    ia, ib = {}, {}
    a = _generate(True, logprob_info=ia, **kw)
    b = _generate(True, clear=True, logprob_info=ib, **kw)
    assert a == b and len(a) == 3 and ia == ib and len(set(a)) > 1


def test_an_adapter_on_the_family_with_sharing():
    """A family of 4 under adapter "A" of a bank (a 1,5xx-token text prompt on the blind tiny model: above the break-even):
    the registered family against the cleared table, bit for bit in tokens and records; and the adapter is part of it."""
    from gen_golden_adapters import fixture_adapter
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    from test_kv_fork_gpu import IdTokenizer
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    model.set_adapter_bank({n: resolve_adapter(model.cfg, *fixture_adapter(model.cfg, n)) for n in ("A", "B")})
    prompt = lambda reps: "<|user|>\n" + "Tell me a story about a story. " * reps + "<|end|>\n<|assistant|>\n"
    n_ids = lambda reps: int(np.asarray(proc(prompt(reps))["input_ids"]).shape[-1])
    per = n_ids(2) - n_ids(1)
    text = prompt(1 + (1500 - n_ids(1)) // per)                     # about 1,500 tokens, whatever the tokenizer makes of a sentence
    S = int(np.asarray(proc(text)["input_ids"]).shape[-1])
    assert 3 * S >= 4096 and S + 10 <= 4096, S                      # (n - 1) x shared keys: registered
    proc.tokenizer = IdTokenizer(proc.tokenizer)
    kw = dict(n=4, temperature=0.9, seed=21, logprobs=1, adapter="A")
    ia, ib, ic = {}, {}, {}
    a = _generate(True, on=(model, proc, text), logprob_info=ia, **kw)
    b = _generate(True, clear=True, on=(model, proc, text), logprob_info=ib, **kw)
    assert a == b and len(a) == 4 and ia == ib and len(set(a)) > 1
    base = _generate(True, on=(model, proc, text), logprob_info=ic, **dict(kw, adapter=None))
    assert ic["token_logprobs"][0][0] != ia["token_logprobs"][0][0]


def test_an_image_family_through_the_prefix_store_with_sharing():
    """api._generate(prompt, images, n=3, prefix_cache=store, share_prefix=True): the cold call and the warm one (restored through
    the last image slot, no vision tower) register the family, and give the tokens and records of their cleared-table twins."""
    from test_kv_fork_gpu import IMG_P, _Spy
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc, _ = _serve()
    kw = dict(n=3, temperature=0.9, seed=8, logprobs=0)
    runs = {}
    for clear in (False, True):
        store = PrefixCache(1 << 30, min_tokens=64)
        for phase in ("cold", "warm"):
            info, spy = {}, _Spy(model)
            try:
                out = _generate(True, clear=clear, prefix_cache=store, logprob_info=info, **kw)
            finally:
                spy.close()
            runs[clear, phase] = (out, info, spy.clip, dict(store.counters()))
    for phase in ("cold", "warm"):
        assert runs[False, phase][:2] == runs[True, phase][:2], phase
    assert runs[False, "cold"][2] == 1 and runs[False, "warm"][2] == 0                # the warm family never ran the vision tower
    c = runs[False, "warm"][3]
    assert (c["hits"], c["misses"], c["entries"], c["tokens_reused"]) == (1, 1, 1, IMG_P), c
    assert len(runs[False, "warm"][0]) == 3 and len(set(runs[False, "warm"][0])) > 1


def test_refusals_name_the_limit():
    from golden_inputs import SERVE_TEXTS
    from phi_3_vision_mlx_amd import api
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    g, model8, proc8, _ = _serve("int8")
    for kw in (dict(n=3), dict()):
        with pytest.raises(ValueError, match="share_prefix needs the bf16 KV cache.*int8"):
            api._generate(model8, proc8, SERVE_TEXTS[2], max_tokens=4, verbose=False, stream=False, mute=True, share_prefix=True, **kw)
    with pytest.raises(ValueError, match="share_prefix needs the bf16 KV cache"):
        ContinuousEngine(model8, proc8, slots=4, window=4096, share_prefix=True)
    st = model8.new_slot_state(2, 4096)
    with pytest.raises(ValueError, match="bf16 KV cache"):
        model8.set_families(st, [((0, 1), 0)])
    model8.cfg.cache_format = "mlx4"
    try:
        with pytest.raises(ValueError, match="share_prefix needs the bf16 KV cache.*mlx4"):
            api._generate(model8, proc8, SERVE_TEXTS[2], max_tokens=4, verbose=False, stream=False, mute=True, share_prefix=True)
    finally:
        model8.cfg.cache_format = "int8"


def test_defaults_launch_what_the_parent_launched(monkeypatch):
    """share_prefix left at its default: an n = 3 call launches what it launched before the feature existed -- no family launch,
    no table -- and share_prefix=False is the same call; with sharing on, the family launch replaces the plain one, one for one."""
    from golden_inputs import SERVE_TEXTS, make_image
    from phi_3_vision_mlx_amd import api
    g, model, proc, _ = _serve()
    monkeypatch.setenv("P3V_PREFILL_GRAPH", "0")

    def go(which=0, **kw):
        states, real = [], model.fork_state

        def spy(*a, **k):
            cache = real(*a, **k)
            states.append(cache[0].state)
            return cache
        model.fork_state = spy
        try:
            with _Count() as c:
                out = api._generate(model, proc, SERVE_TEXTS[which], [make_image(336, 336, "noise", 0)] if which == 0 else None,
                                    max_tokens=8, verbose=False, stream=False, mute=True, n=3, **kw)
        finally:
            del model.fork_state
        return out, c.n, states[0]
    go()                                                           # (uncounted: builds what a model builds once)
    out_d, n_d, st_d = go()
    out_f, n_f, st_f = go(share_prefix=False)
    out_s, n_s, st_s = go(share_prefix=True)
    assert n_d == n_f and out_d == out_f and "p3v_attention_decode_family" not in n_d and n_d["p3v_kv_fork"] == 1
    assert st_d.family is None and st_d.family_host is None and st_d.families == [] and not st_d.graphs["greedy"]["bufs"]["plan"].family
    assert st_s.family is not None and n_s["p3v_attention_decode_family"] == n_d["p3v_attention_decode"] - n_s.get("p3v_attention_decode", 0)
    assert {k: v for k, v in n_s.items() if not k.startswith("p3v_attention_decode")} == \
        {k: v for k, v in n_d.items() if not k.startswith("p3v_attention_decode")}
    # a family below the break-even (3 rows x a 30-token prompt): share_prefix=True leaves the plain state and the plain launches
    go(which=2)                                                    # (uncounted, as above)
    out_t, n_t, st_t = go(which=2)
    out_ts, n_ts, st_ts = go(which=2, share_prefix=True)
    assert st_ts.family is None and n_ts == n_t and out_ts == out_t


def test_http_n_3_with_share_prefix_answers_as_without():
    """serve_continuous over a share_prefix engine, the fixture's image request with "n": 3 (2 x 2,5xx shared keys: registered):
    the same fields as without the flag, and the same tokens under the rule of test_share_prefix_against_the_unshared_plan read
    off the responses' own log-probabilities ("logprobs": 2; top_k = 1 makes every draw the arg-max): while a row's tokens agree,
    its token's log-probability is within twice the logit tolerance (a log-probability is a logit minus a sum over logits, each
    within atol + 2e-2 |logit|), and the next token is equal wherever the unshared server's top-two gap exceeds twice atol; a
    row is followed up to its first step that is too close to call, and at most a quarter of the steps may be lost that way."""
    from golden_inputs import SERVE_PROMPTS, make_image
    from test_serving_gpu import _png_uri
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    g, model, proc, reqs = _serve()
    top = float(model(**reqs[0], max_tokens=1)[0][0, -1].float().abs().max())
    atol, steps = 1e-2 * top, 12
    body = {"prompt": SERVE_PROMPTS[0], "images": [_png_uri(make_image(336, 336, "noise", 0))], "max_tokens": steps, "n": 3,
            "temperature": 1.0, "top_k": 1, "seed": 42, "logprobs": 2}

    def ask(share):
        eng = ContinuousEngine(model, proc, slots=4, window=4096, **({"share_prefix": True} if share else {}))
        seen, real = [], model.set_families

        def spy(st, families, **kw):
            real(st, families, **kw)
            seen.append(list(st.families))
        model.set_families = spy
        httpd, backend = serve_continuous(eng, port=0)
        threading.Thread(target=httpd.serve_forever, daemon=True).start()
        try:
            r = urllib.request.Request(f"http://127.0.0.1:{httpd.server_address[1]}/v1/completions", data=json.dumps(body).encode(),
                                       headers={"Content-Type": "application/json"})
            with urllib.request.urlopen(r, timeout=300) as resp:
                return json.loads(resp.read()), eng, seen
        finally:
            httpd.shutdown()
            backend.close()
            del model.set_families
    a, eng_a, seen_a = ask(True)
    b, eng_b, seen_b = ask(False)
    assert set(a) == set(b) and {"model", "responses", "seeds", "logprobs"} <= set(a) and a["seeds"] == b["seeds"] == [42, 43, 44]
    assert eng_a.st.family is not None and eng_b.st.family is None and seen_b == []
    assert any(len(f) == 1 and len(f[0][0]) == 3 and f[0][1] > 2500 for f in seen_a), seen_a     # the family WAS registered while it ran
    assert len(a["responses"]) == len(b["responses"]) == 3
    lost = total = 0
    for ra, rb in zip(a["logprobs"], b["logprobs"]):
        assert ra["token_ids"][0] == rb["token_ids"][0]                              # drawn from the one prefill row
        n = min(len(ra["token_ids"]), len(rb["token_ids"]))
        total += n
        for t in range(n):
            if ra["token_ids"][t] != rb["token_ids"][t]:
                gap = rb["top_logprobs"][t][0]["logprob"] - rb["top_logprobs"][t][1]["logprob"]
                assert gap <= 2 * atol, (t, gap, atol, ra["token_ids"], rb["token_ids"])
                lost += n - t
                break
            assert abs(ra["token_logprobs"][t] - rb["token_logprobs"][t]) <= 2 * (atol + 2e-2 * top), t
    print(f"HTTP: {lost} of {total} steps behind a step too close to call")
    assert total >= 6 and lost <= total // 4
