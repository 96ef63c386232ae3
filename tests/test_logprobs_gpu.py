"""Token log-probabilities on the MI355X: p3v_logprobs / p3v_logprobs_step against the restatement of the rule
(test_logprobs_cpu.py) -- ids, ranks and n_top exact, every float within 1 fp32 ulp (device log and NumPy log may differ by one
fp64 ulp) --, the two log-probability captures of the model against the plain and sampled replays from the same state, then
api.generate / api.score, the continuous engine and the HTTP surface: the feature changes no token."""
import json
import math
import threading
import urllib.request

import numpy as np
import pytest
import torch

from test_logprobs_cpu import EOS, assert_record, logprobs_ref, to_bits

pytestmark = pytest.mark.gpu
N = 32064
CANARY = 0x5A5A5A5A


def _rows_bits():
    """the rows of the sampling test, plus the undefined ones: sigma 1, sigma 4, 500 -inf entries + 45 tokens tied at the top,
    a NaN row, a +inf row, an all -inf row"""
    rng = np.random.default_rng(1)
    rows = [to_bits(rng.normal(0, s, N)) for s in (1.0, 4.0)]
    tie = to_bits(rng.normal(0, 1.0, N))
    tie[rng.choice(np.arange(50, N), 500, replace=False)] = 0xFF80
    tie[:45] = to_bits(np.full(45, 10.0))
    rows.append(tie)
    nan = rows[0].copy()
    nan[1234] = 0x7FC0
    pinf = rows[1].copy()
    pinf[N - 1] = 0x7F80
    rows += [nan, pinf, np.full(N, 0xFF80, dtype=np.uint16)]
    return np.stack(rows)


def _dev(bits):
    return torch.as_tensor(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _i32(v):
    return torch.as_tensor(np.asarray(v, dtype=np.int32)).cuda()


def _unpack(words):
    from phi_3_vision_mlx_amd import logprobs
    return logprobs.unpack(words)


def _bits_of(t):
    return t.detach().reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------- kernel
def test_kernel_equals_restatement_at_the_vocabulary_size():
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()
    x = (bits[2].astype(np.uint32) << 16).view(np.float32)
    ninf_tok = int(np.nonzero(np.isneginf(x))[0][3])
    cases = []
    for r in range(len(bits)):
        finite = not (r >= 3)
        amax = int(np.argmax((bits[r].astype(np.uint32) << 16).view(np.float32))) if finite else 17
        for t in (amax, 20, ninf_tok, -1, N):                                 # arg-max, a tied token (row 2), a -inf token (row 2)
            for want in (0, 1, 5, 8):
                cases.append((r, t, want))
    logits = _dev(bits)[[c[0] for c in cases]]
    got = _unpack(ops.logprobs(logits, _i32([c[1] for c in cases]), _i32([c[2] for c in cases])))
    for (r, t, want), rec in zip(cases, got):
        assert_record(rec, logprobs_ref(bits[r], t, want), (r, t, want))
    # what the rows are there for
    by = {c: rec for c, rec in zip(cases, got)}
    assert by[(2, 20, 8)]["rank"] == 21 and [i for i, _ in by[(2, 20, 8)]["top"]] == list(range(8))
    assert by[(2, ninf_tok, 0)]["logprob"] == -math.inf
    assert all(by[(r, 20, 8)]["rank"] == 0 and by[(r, 20, 8)]["top"] == [] and math.isnan(by[(r, 20, 8)]["logprob"]) for r in (3, 4, 5))
    assert all(rec["rank"] == 1 for (r, t, w), rec in by.items() if r < 3 and t not in (20, ninf_tok, -1, N))


@pytest.mark.parametrize("n,stride", [(5, 5), (1023, 1031), (1025, 1025), (32769, 32776), (65536, 65536)])
def test_kernel_sizes_and_strides(n, stride):
    """below one chunk, around the 1024-thread block, an unaligned row stride (the scalar loads), and both sides of the
    32768-value register layout"""
    from phi_3_vision_mlx_amd import ops
    rng = np.random.default_rng(n)
    bits = np.stack([to_bits(rng.normal(0, 3.0, stride)) for _ in range(3)])
    bits[1, :n:3] = 0xFF80
    bits[2, max(0, n - 4):n] = bits[2, 0]                                     # ties across the row's two ends
    bits[:, n:] = 0x7FC0                                                      # beyond n: never read as part of the row
    toks = [int(rng.integers(0, n)) for _ in range(3)] + [n - 1, 0, n]
    wants = [8, 5, 8, 1, 0, 8]
    wide = _dev(bits)
    logits = wide[[0, 1, 2, 2, 1, 0]][:, :n]
    assert logits.stride(0) == stride
    got = _unpack(ops.logprobs(logits, _i32(toks), _i32(wants)))
    for k, (r, t, w) in enumerate(zip([0, 1, 2, 2, 1, 0], toks, wants)):
        assert_record(got[k], logprobs_ref(bits[r, :n], t, w), (n, k))
        assert len(got[k]["top"]) == min(w, n)


@pytest.mark.parametrize("n", [5, N])
def test_kernel_one_row(n):
    """a launch of ONE row (a grid of one workgroup), a skipped one included"""
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()[2, :n].copy()                                         # 45 (n = 5: all) tokens tied at the top
    for t, want in ((0, 8), (n - 1, 0), (n, 3), (3, -1)):
        out = torch.full((1, 20), CANARY, dtype=torch.int32, device="cuda")
        ops.logprobs(_dev(bits[None]), _i32([t]), _i32([want]), out=out)
        if want < 0:
            assert (out.cpu() == CANARY).all()
        else:
            rec = _unpack(out.cpu())[0]
            assert_record(rec, logprobs_ref(bits, t, want), (n, t, want))
            assert len(rec["top"]) == min(want, n)


def test_kernel_more_rows_than_cus_skips_unwanted_rows():
    from phi_3_vision_mlx_amd import ops
    rng = np.random.default_rng(5)
    n, rows = 1025, 300
    bits = np.stack([to_bits(rng.normal(0, 2.0, n)) for _ in range(rows)])
    toks = rng.integers(-1, n + 1, rows)
    wants = rng.integers(-1, 9, rows)
    wants[[0, 7, 299]] = -1
    out = torch.full((rows, 20), CANARY, dtype=torch.int32, device="cuda")
    ops.logprobs(_dev(bits), _i32(toks), _i32(wants), out=out)
    raw = out.cpu()
    got = _unpack(raw)
    for r in range(rows):
        if wants[r] < 0:
            assert (raw[r] == CANARY).all(), r                               # nothing written
        else:
            assert_record(got[r], logprobs_ref(bits[r], toks[r], wants[r]), r)
            unused = raw[r, 4 + len(got[r]["top"]):12]
            assert (unused == -1).all() and np.isnan(raw[r, 12 + len(got[r]["top"]):].view(torch.float32).numpy()).all()


def test_entry_points_refuse_bad_arguments():
    from phi_3_vision_mlx_amd import _lib, ops
    lib = _lib.lib()
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    t, w = _i32([0, 1]), _i32([0, 0])
    out = torch.full((2, 20), CANARY, dtype=torch.int32, device="cuda")
    p = lambda a: a.data_ptr()                                                # noqa: E731
    assert lib.p3v_logprobs(p(x), 64, p(t), None, p(out), 2, 64, None) == -22      # a NULL want
    assert lib.p3v_logprobs(p(x), 64, p(t), p(w), p(out), 0, 64, None) == -22
    assert lib.p3v_logprobs(p(x), 63, p(t), p(w), p(out), 2, 64, None) == -22      # row_stride < n
    assert lib.p3v_logprobs(p(x), 65537, p(t), p(w), p(out), 2, 65537, None) == -22
    assert lib.p3v_logprobs_step(p(x), p(t), p(w), None, p(out), 2, 64, 1, None) == -22
    assert lib.p3v_logprobs_step(p(x), p(t), p(w), p(t), p(out), 2, 64, 0, None) == -22
    torch.cuda.synchronize()
    assert (out.cpu() == CANARY).all()
    with pytest.raises((TypeError, ValueError)):
        ops.logprobs(x, t, w.to(torch.int64))
    with pytest.raises(ValueError):
        ops.logprobs(x, t, _i32([0]))


@pytest.mark.parametrize("B", [1, 5])
def test_step_form_writes_one_slot(B):
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()[:3]
    rng = np.random.default_rng(10 + B)
    max_steps = 6
    records = torch.full((B, max_steps, 20), CANARY, dtype=torch.int32).pin_memory()
    which = rng.integers(0, len(bits), B)
    logits = _dev(bits[which])
    next_tok = _i32(rng.integers(0, N, B))
    wants = rng.integers(0, 9, B)
    if B > 1:
        wants[2] = -1
    want = _i32(wants)
    for step in (1, 4, max_steps, max_steps + 1, 0):
        records.fill_(CANARY)
        d_step = _i32([step])
        ops.logprobs_step(logits, next_tok, want, d_step, records)
        torch.cuda.synchronize()
        assert int(d_step.item()) == step                                     # read-only on the loop state
        for b in range(B):
            for s in range(max_steps):
                if s == step - 1 and wants[b] >= 0:
                    assert_record(_unpack(records[b, s])[0], logprobs_ref(bits[which[b]], int(next_tok[b]), wants[b]), (step, b))
                else:
                    assert (records[b, s] == CANARY).all(), (step, b, s)      # canaries around every slot


# ---------------------------------------------------------------------------------------------------- model wiring
@pytest.fixture(scope="module")
def tiny():
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    yield model, proc
    del model
    torch.cuda.empty_cache()


PROMPT = "<|user|>\nTell me a story<|end|>\n<|assistant|>\n"
BATCH = ["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nA longer question here, padded left<|end|>\n<|assistant|>\n",
         "<|user|>\nWhy?<|end|>\n<|assistant|>\n"]
STEP = {"g": "greedy_step", "s": "sample_step", "gl": "logprob_step", "sl": "sample_logprob_step"}


def _run_plan(model, inputs, plan, rows, wants):
    """One prefill, then the plan's replays; returns everything a replay may change.  Scored replays are held to the restatement."""
    from phi_3_vision_mlx_amd import ops, sampling
    logits, cache = model(**inputs, max_tokens=12)
    st = cache[0].state
    model.set_sampling(st, sampling.pack(rows, 1))
    if wants is not None:
        model.set_logprobs(st, wants)
    token = ops.argmax(logits[:, -1, :].contiguous())[:, None]
    seen = []
    for kind in plan:
        lg, token = getattr(model, STEP[kind])(token, cache)
        torch.cuda.synchronize()
        g = st.graphs["greedy"]
        toks = token.reshape(-1).cpu().tolist()
        seen.append((_bits_of(lg).copy(), toks))
        if kind.endswith("l"):
            recs = _unpack(g["records"][:, g["n_replays"] - 1])
            for b, w in enumerate(wants):
                if w >= 0:
                    assert_record(recs[b], logprobs_ref(_bits_of(lg[b]), toks[b], w), (kind, b))
    g = st.graphs["greedy"]
    state = dict(history=g["history"].clone(), d_step=int(g["d_step"].item()), d_past=int(g["d_past"].item()), offset=st.offset,
                 counters=[r["counter"] for r in sampling.unpack(st.sample_rows)], keys=set(g))
    return seen, state


@pytest.mark.parametrize("q4", [False, True], ids=["bf16", "mlx4"])
def test_model_logprob_captures_change_nothing_and_match_the_restatement(q4, tiny):
    from phi_3_vision_mlx_amd import sampling
    from phi_3_vision_mlx_amd.api import load_synthetic
    if q4:
        model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0", quantized_int4=True)
        assert model.w4
    else:
        model, proc = tiny
    for text, wants in ((PROMPT, [5]), (BATCH, [3, -1, 8])):
        inputs = proc(text, None)
        B = inputs["input_ids"].shape[0]
        rows = sampling.rows(B, [0.8, 0.0, 1.5][:B], [0, 5, 40][:B], [0.9, 1.0, 0.5][:B], 77)
        base, s0 = _run_plan(model, inputs, ["g", "g", "s", "s", "g", "s"], rows, None)
        assert not {"logprob_graph", "sample_logprob_graph", "records"} & s0["keys"]
        for plan in (["gl", "gl", "sl", "sl", "gl", "sl"], ["g", "gl", "s", "sl", "gl", "s"]):     # scored, and alternating
            got, s1 = _run_plan(model, inputs, plan, rows, wants)
            for k, ((lb, tb), (lg, tg)) in enumerate(zip(base, got)):
                assert tb == tg and np.array_equal(lb, lg), (text, plan, k)   # bit-identical logits, the same tokens
            assert torch.equal(s0["history"], s1["history"])
            assert {k: s0[k] for k in ("d_step", "d_past", "offset", "counters")} == {k: s1[k] for k in ("d_step", "d_past", "offset", "counters")}
            assert {"logprob_graph", "sample_logprob_graph", "records"} <= s1["keys"]
    if q4:
        del model
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- api.generate
def _check_info(info, texts, proc, wants, greedy):
    for b, w in enumerate(wants):
        if w is None:
            assert all(info[k][b] is None for k in ("token_ids", "token_logprobs", "ranks", "top_logprobs"))
            continue
        ids, lps, ranks, tops = (info[k][b] for k in ("token_ids", "token_logprobs", "ranks", "top_logprobs"))
        assert len(ids) == len(lps) == len(ranks) == len(tops) >= 1
        cut = ids[:ids.index(EOS) + 1] if EOS in ids else ids
        assert proc.tokenizer.decode(cut) == texts[b]                         # the records are the generated tokens', in order
        for t, lp, rank, top in zip(ids, lps, ranks, tops):
            assert len(top) == w and rank >= 1 and lp <= 0.0
            assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
            if greedy:
                assert rank == 1
            if rank <= w:
                assert top[rank - 1] == (t, lp)
            else:
                assert all(i != t for i, _ in top) and all(v >= lp for _, v in top)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_generate_with_logprobs_returns_the_same_text(sampled, tiny):
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    kw = dict(max_tokens=10, verbose=False, stream=False, mute=True)
    if sampled:
        kw.update(temperature=0.9, top_p=0.95, seed=3)
    for prompt, lp in ((PROMPT, 3), (BATCH, [2, None, 8])):
        ref = api._generate(model, proc, prompt, **kw)
        info = {}
        got = api._generate(model, proc, prompt, logprobs=lp, logprob_info=info, **kw)
        assert got == ref
        texts = [got] if isinstance(got, str) else got
        wants = [lp] if isinstance(lp, int) else lp
        n_steps = {len(info["token_ids"][b]) for b, w in enumerate(wants) if w is not None}
        assert len(n_steps) == 1 and 1 <= n_steps.pop() <= 10                 # one entry per token handed to the streamer
        _check_info(info, texts, proc, wants, greedy=not sampled)


def test_sampled_runs_of_one_prompt_geometry_share_their_records(tiny, monkeypatch):
    """the callers of a captured-prefill entry share its sampled capture, which bakes the address of the sampling records in:
    every one of them must write the records that capture reads -- same seed, same text; another seed, that seed's text"""
    from phi_3_vision_mlx_amd import api, ops
    model, proc = tiny
    prompt = "<|user|>\nPlease tell me a rather long story about a ship, its crew and the sea<|end|>\n<|assistant|>\n"
    S = proc(prompt, None)["input_ids"].shape[1]
    assert ops.L.DECODE_MAX_L < S <= model.PREFILL_GRAPH_MAX_S
    gen = lambda seed: api._generate(model, proc, prompt, max_tokens=11, verbose=False, stream=False, mute=True,   # noqa: E731
                                     temperature=0.9, top_p=0.95, seed=seed)
    monkeypatch.setenv("P3V_PREFILL_GRAPH", "0")
    eager = {seed: gen(seed) for seed in (3, 4)}
    assert eager[3] != eager[4]
    monkeypatch.delenv("P3V_PREFILL_GRAPH")
    hits, orig = [], model._prefill_captured

    def counted(*a):
        out = orig(*a)
        hits.append(out is not None)
        return out

    monkeypatch.setattr(model, "_prefill_captured", counted)
    seeds = [3, 3, 3, 4, 3]                                                   # eager (first sighting), then four leases of one entry
    assert [gen(seed) for seed in seeds] == [eager[seed] for seed in seeds]
    assert hits == [False, True, True, True, True]


def test_generate_without_logprobs_is_todays_path(tiny):
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    prompt = "<|user|>\nHello there, how are you today<|end|>\n<|assistant|>\n"
    before = list(model._states)
    ref = api._generate(model, proc, prompt, max_tokens=10, verbose=False, stream=False, mute=True)
    info = {}
    got = api._generate(model, proc, prompt, max_tokens=10, verbose=False, stream=False, mute=True, temperature=0.0, logprobs=None,
                        logprob_info=info)
    assert got == ref and info == {}
    new = [s for s in model._states if not any(s is o for o in before)]
    assert new
    for s in new:
        g = s.graphs.get("greedy", {})
        assert not {"logprob_graph", "sample_logprob_graph", "sample_graph", "records"} & set(g)
        assert s.logprob_want is None


# ---------------------------------------------------------------------------------------------------- api.score
class _Spy:
    """the model, with the logits of its last call kept"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, *a, **kw):
        out = self.model(*a, **kw)
        self.calls.append((kw, out[0].detach().clone()))
        return out

    def __getattr__(self, name):
        return getattr(self.model, name)


def test_score_equals_the_restatement_over_the_prefill_rows(tiny):
    from PIL import Image
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))
    for prompt, images in (("Tell me a story", None), ("What is this?", [img]), (["Hi", "A longer question here, padded left"], None)):
        spy = _Spy(model)
        out = api.score(prompt, images, preload=(spy, proc), top=2)
        assert len(spy.calls) == 1 and spy.calls[0][0].get("full_logits") is True       # ONE prefill with every row's logits
        logits = spy.calls[0][1]
        text, imgs = api._apply_chat_template(prompt, images, False)
        inputs = proc(text, imgs)
        ids = np.asarray(inputs["input_ids"])
        ids = ids[None] if ids.ndim == 1 else ids
        pads = (np.asarray(inputs["mask"]) == 0).sum(1) if "mask" in inputs else [0] * len(ids)
        out = out if isinstance(prompt, list) else [out]
        assert len(out) == len(ids) and tuple(logits.shape[:2]) == ids.shape
        n_none = 0
        for b, res in enumerate(out):
            assert res["token_ids"] == ids[b].tolist()
            for i in range(ids.shape[1]):
                entry = (res["token_logprobs"][i], res["ranks"][i], res["top_logprobs"][i])
                if i <= pads[b] or not 0 <= ids[b, i] < N:                    # padding, the first token, image slots
                    assert entry == (None, None, None), (b, i)
                    n_none += 1
                    continue
                want = logprobs_ref(_bits_of(logits[b, i - 1]), ids[b, i], 2)
                assert_record(dict(token=int(ids[b, i]), logprob=entry[0], rank=entry[1], top=entry[2]), want, (b, i))
        assert n_none >= len(ids) + (100 if images else 0) + int(sum(pads))


# ---------------------------------------------------------------------------------------------------- engine + HTTP
def _engine_run(model, proc, texts, settings, wants, watch):
    """four requests, two joining mid-flight; the logits of every scored step (and of the prefill that scores a first token)
    are snapshotted around the model's own methods"""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args
    eng = ContinuousEngine(model, proc, slots=4, window=4096)
    snaps, firsts = [], {}
    orig = {name: getattr(model, name) for name in ("logprob_step", "sample_logprob_step", "logprobs_of")}

    def spy_step(name):
        def f(token, cache):
            lg, tok = orig[name](token, cache)
            torch.cuda.synchronize()
            snaps.append(lg.detach().clone())
            return lg, tok
        return f

    def spy_first(st, logits, tokens, row0=0):
        for i in range(tokens.numel()):
            firsts[row0 + i] = logits.detach().clone()[i, -1]
        return orig["logprobs_of"](st, logits, tokens, row0)

    if any(w is not None for w in wants):
        model.logprob_step, model.sample_logprob_step, model.logprobs_of = spy_step("logprob_step"), spy_step("sample_logprob_step"), spy_first
    try:
        sub = lambda i: eng.submit(proc(texts[i]) if wants[i] is None else logprob_args(proc(texts[i]), wants[i]), 8,   # noqa: E731
                                   **({} if settings[i] is None else {"sampling": settings[i]}))
        hs = [sub(0), sub(1)]
        eng.step()
        eng.step()
        hs += [sub(2), sub(3)]
        eng.run_until_idle()
    finally:
        for name in orig:
            model.__dict__.pop(name, None)
    assert all(h.error is None for h in hs), [h.error for h in hs]
    for i in watch:
        h = hs[i]
        if wants[i] is None:
            continue
        assert len(h.logprob_records) == len(h.tokens) and [r["token"] for r in h.logprob_records] == h.tokens
        assert_record(h.logprob_records[0], logprobs_ref(_bits_of(firsts[h.row]), h.tokens[0], wants[i]), (i, "first"))
        # requests 0 and 1 decode from the first scored step on; 2 and 3 join later, and the last scored step is request 2's last
        tail = snaps[len(snaps) - (len(h.tokens) - 1):] if i >= 2 else snaps[:len(h.tokens) - 1]
        assert len(tail) == len(h.tokens) - 1
        for k, lg in enumerate(tail):
            assert_record(h.logprob_records[1 + k], logprobs_ref(_bits_of(lg[h.row]), h.tokens[1 + k], wants[i]), (i, k))
    return [h.tokens for h in hs], [h.logprob_records for h in hs]


def test_engine_scored_requests_change_no_token(tiny):
    model, proc = tiny
    texts = ["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nTell me a long story about the sea<|end|>\n<|assistant|>\n",
             "<|user|>\nWhy is the sky blue, do you think?<|end|>\n<|assistant|>\n", "<|user|>\nOne two three<|end|>\n<|assistant|>\n"]
    settings = [None, {"temperature": 0.8, "seed": 1}, None, None]
    plain, _ = _engine_run(model, proc, texts, settings, [None] * 4, ())
    wants = [0, None, 8, None]
    scored, recs = _engine_run(model, proc, texts, settings, wants, (0, 2))   # both scored requests: N = 0 and the N = 8 top lists
    assert scored == plain
    assert recs[1] == [] and recs[3] == [] and all(r["top"] == [] for r in recs[0]) and all(len(r["top"]) == 8 for r in recs[2])
    assert all(r["rank"] == 1 for r in recs[0] + recs[2])                     # greedy rows: the emitted token is the arg-max
    st = [s for s in model._states if getattr(s, "slots", False)]
    assert all((s.logprob_want is None) or bool((s.logprob_want == -1).all()) for s in st)   # every row released


def test_engine_scores_after_more_plain_steps_than_record_slots(tiny):
    """every replay advances the step counter that indexes the records, and a slot state has window + 1 slots: the first scored
    request of an engine that has replayed past them (no record buffer yet), and one that is in flight when they run out"""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args
    model, proc = tiny
    text = "<|user|>\nOne two three<|end|>\n<|assistant|>\n"
    eng = ContinuousEngine(model, proc, slots=2, window=64)
    g = model.decode_graph(eng.st)
    slots = g["history"].shape[1]
    assert slots == 65

    def run(want, max_tokens=8):
        h = eng.submit(proc(text) if want is None else logprob_args(proc(text), want), max_tokens)
        eng.run_until_idle()
        assert h.error is None and eng.failures == 0, h.error
        return h

    ref = run(None)
    assert len(ref.tokens) >= 4
    for phase in ("no record buffer yet", "in flight when the slots run out"):
        # plain traffic up to: past the slots / three steps short of them
        goal = slots + 1 if phase.startswith("no") else slots - 3
        for _ in range(slots):
            if g["n_replays"] >= goal:
                break
            h = run(None, min(8, goal - g["n_replays"] + 1))
            assert h.tokens == ref.tokens[:len(h.tokens)]
        assert g["n_replays"] == goal and model.decode_graph(eng.st) is g
        if phase.startswith("no"):
            assert "records" not in g
        h = run(5)
        assert h.tokens == ref.tokens and [r["token"] for r in h.logprob_records] == h.tokens, phase
        for r in h.logprob_records:
            assert r["rank"] == 1 and len(r["top"]) == 5 and tuple(r["top"][0]) == (r["token"], r["logprob"]), phase
        assert g["n_replays"] < len(ref.tokens)                               # the counter was started afresh


def test_http_on_the_engine_answers_with_aligned_lists(tiny):
    from test_serving_gpu import IdTokenizer
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = tiny
    real = proc.tokenizer
    proc.tokenizer = IdTokenizer(real)
    eng = ContinuousEngine(model, proc, slots=4, window=4096)
    httpd, backend = serve_continuous(eng, port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]

    def post(body):
        req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=300) as r:
            return json.loads(r.read())

    try:
        plain = post({"prompt": ["Once upon a time", "The weather"], "max_tokens": 9})
        out = post({"prompt": ["Once upon a time", "The weather"], "max_tokens": 9, "logprobs": 2})
        assert out["responses"] == plain["responses"] and "logprobs" not in plain
        for text, obj in zip(out["responses"], out["logprobs"]):
            ids = [int(t) for t in text.split()]
            assert obj["token_ids"] == ids and obj["tokens"] == [str(i) for i in ids]      # the ids re-encode the response text
            assert len(obj["token_logprobs"]) == len(obj["ranks"]) == len(obj["top_logprobs"]) == len(ids)
            for t, lp, rank, top in zip(ids, obj["token_logprobs"], obj["ranks"], obj["top_logprobs"]):
                assert rank == 1 and len(top) == 2 and top[0] == {"id": t, "token": str(t), "logprob": lp} and lp <= 0
    finally:
        httpd.shutdown()
        backend.close()
        proc.tokenizer = real
