"""Seeded sampling on the MI355X: p3v_sample / p3v_sample_step_end against the restatement of the rule (test_sampling_cpu.py) on
every draw, the Philox wiring, greedy equivalence, the distribution, the sampled decode graph of the model, the continuous engine,
the recovery of the one-step-ahead loop and the HTTP surface on the engine."""
import json
import threading
import urllib.request

import numpy as np
import pytest
import torch

from test_sampling_cpu import draw_word, sample_probs, sample_ref, to_bits

pytestmark = pytest.mark.gpu
N = 32064


def _records(rows, counter):
    from phi_3_vision_mlx_amd import sampling
    return sampling.pack(rows, counter).cuda()


def _rows_bits():
    rng = np.random.default_rng(1)
    rows = [to_bits(rng.normal(0, s, N)) for s in (1.0, 4.0)]
    tie = to_bits(rng.normal(0, 1.0, N))
    tie[rng.choice(N, 500, replace=False)] = 0xFF80                     # -inf entries
    tie[:45] = to_bits(np.full(45, 9.0))                                 # 45 tokens tied at the top: any k <= 45 cuts inside them
    tie[45:50] = to_bits(np.full(5, 10.0))
    rows.append(tie)
    nan = rows[0].copy()
    nan[1234] = 0x7FC0
    rows.append(nan)
    return np.stack(rows)


SETTINGS = [(T, k, p) for T in (0.05, 0.7, 1.0, 3.0) for k in (0, 1, 40, N) for p in (1.0, 0.9, 0.3, 1e-4)]


def test_kernel_equals_restatement_on_every_draw():
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()
    R = len(bits)
    logits = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16).cuda()
    rng = np.random.default_rng(2)
    mism = []
    for (T, k, p) in SETTINGS:
        seeds = [int(s) for s in rng.integers(0, 1 << 63, 256, dtype=np.int64)]
        c0 = int(rng.integers(0, 1 << 20))
        # eager entry point: the 256 (seed, c) pairs as 256 launches' worth of rows, R rows each (one launch of R * 32 rows)
        for chunk in range(8):
            sl = seeds[chunk * 32:(chunk + 1) * 32]
            rows = [(T, k, p, s) for s in sl for _ in range(R)]
            rec = _records(rows, c0 + chunk)
            big = logits.repeat(len(sl), 1)
            got = ops.sample(big, rec).cpu().tolist()
            for i, (s, g) in enumerate(zip([s for s in sl for _ in range(R)], got)):
                want = sample_ref(bits[i % R], T, k, p, s, c0 + chunk)
                if g != want:
                    mism.append(("eager", T, k, p, s, i % R, g, want))
            from phi_3_vision_mlx_amd import sampling
            assert all(r["counter"] == c0 + chunk + 1 for r in sampling.unpack(rec))
    assert not mism, mism[:10]


@pytest.mark.parametrize("B", [1, 5])
def test_step_end_equals_restatement_and_keeps_the_books(B):
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()
    rng = np.random.default_rng(3 + B)
    max_steps = 40
    history = torch.zeros((B, max_steps), dtype=torch.int32).pin_memory()
    d_step = torch.zeros((1,), dtype=torch.int32, device="cuda")
    d_past = torch.full((1,), 100, dtype=torch.int32, device="cuda")
    ticket = torch.zeros((1,), dtype=torch.int32, device="cuda")
    next_tok = torch.zeros((B,), dtype=torch.int32, device="cuda")
    tok = torch.zeros((B,), dtype=torch.int32, device="cuda")
    mism = []
    for step, (T, k, p) in enumerate(SETTINGS[::2][:max_steps]):
        which = rng.integers(0, len(bits), B)
        rb = bits[which]
        logits = torch.as_tensor(rb.view(np.int16)).view(torch.bfloat16).cuda()
        seeds = [int(s) for s in rng.integers(0, 1 << 63, B, dtype=np.int64)]
        rows = [(T if b % 2 == 0 else 0.0, k, p, s) for b, s in enumerate(seeds)]
        rec = _records(rows, 7 * step)
        ops.sample_step_end(logits, rec, next_tok, tok, history, d_step, d_past, ticket)
        torch.cuda.synchronize()
        want = [sample_ref(rb[b], *rows[b], 7 * step) for b in range(B)]
        got = tok.cpu().tolist()
        if got != want:
            mism.append((step, got, want))
        assert next_tok.cpu().tolist() == got and history[:, step].tolist() == got
        assert int(d_step.item()) == step + 1 and int(d_past.item()) == 101 + step and int(ticket.item()) == 0
        assert (rec[:, 5].cpu() == 7 * step + 1).all()
    assert not mism, mism[:5]


def test_philox_wiring_on_flat_rows():
    from phi_3_vision_mlx_amd import ops
    pairs = [(0, 0), (1, 0), (0, 1), (0x0123456789ABCDEF, 7)]
    rng = np.random.default_rng(4)
    hi, lo, cs = rng.integers(0, 1 << 32, 4092), rng.integers(0, 1 << 32, 4092), rng.integers(0, 1 << 31, 4092)
    pairs += [((int(h) << 32) | int(l), int(c)) for h, l, c in zip(hi, lo, cs)]
    flat = torch.zeros((1, N), dtype=torch.bfloat16, device="cuda")
    got = []
    for i in range(0, len(pairs), 1024):
        part = pairs[i:i + 1024]
        rec = torch.cat([_records([(1.0, 0, 1.0, s)], c) for s, c in part])
        got += ops.sample(flat.repeat(len(part), 1), rec).cpu().tolist()
    assert got[:4] == [12795, 28545, 31173, 17858]
    assert got == [(N * draw_word(s, c)) >> 32 for s, c in pairs]


def test_greedy_rows_equal_argmax_bit_for_bit():
    from phi_3_vision_mlx_amd import ops
    bits = _rows_bits()
    logits = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16).cuda()
    ref = ops.argmax(logits).cpu().tolist()
    assert ref[-1] == -1
    rec = _records([(0.0, 40, 0.9, 5)] * len(bits), 0)
    assert ops.sample(logits, rec).cpu().tolist() == ref
    B = len(bits)
    hist = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    z = [torch.zeros((k,), dtype=torch.int32, device="cuda") for k in (B, B, 1, 1, 1)]
    ops.sample_step_end(logits, rec, z[0], z[1], hist, z[2], z[3], z[4])
    assert z[1].cpu().tolist() == ref and hist[:, 0].cpu().tolist() == ref


def test_distribution_chi_square():
    from phi_3_vision_mlx_amd import ops
    from scipy.stats import chi2
    bits = _rows_bits()[0]
    w = sample_probs(bits, 1.0, 50, 0.9)
    support = np.nonzero(w)[0]
    probs = w[support].astype(np.float64) / float(w.sum())
    logits = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16).cuda()
    counts = np.zeros(N, dtype=np.int64)
    n_draw = 1 << 16
    big = logits.repeat(1024, 1)
    for c0 in range(0, n_draw, 1024):
        rec = torch.cat([_records([(1.0, 50, 0.9, 12345)], c) for c in range(c0, c0 + 1024)])
        counts += np.bincount(ops.sample(big, rec).cpu().numpy(), minlength=N)
    assert counts[np.setdiff1d(np.arange(N), support)].sum() == 0
    exp = probs * n_draw
    stat = float(((counts[support] - exp) ** 2 / exp).sum())
    crit = float(chi2.isf(1e-6, len(support) - 1))
    assert stat < crit, (stat, crit, len(support))


# ---------------------------------------------------------------------------------------------------- model wiring
def _tiny(q4=False):
    from phi_3_vision_mlx_amd.api import load_synthetic
    kw = dict(quantized_int4=True) if q4 else {}                          # MLX 4-bit group-64 weights (quantize_model=True)
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0", **kw)
    assert bool(model.w4) == q4
    return model, proc


def _logits_bits(t):
    return t.detach().reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("q4", [False, True], ids=["bf16", "mlx4"])
def test_model_sampled_graph_matches_restatement(q4):
    from PIL import Image
    from phi_3_vision_mlx_amd import api, ops, sampling
    model, proc = _tiny(q4)
    prompt = "<|user|>\nTell me a story<|end|>\n<|assistant|>\n"
    a = api._generate(model, proc, prompt, max_tokens=12, verbose=False, stream=False, mute=True, temperature=0.9, top_p=0.95, seed=3)
    b = api._generate(model, proc, prompt, max_tokens=12, verbose=False, stream=False, mute=True, temperature=0.9, top_p=0.95, seed=3)
    assert a == b
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))
    cases = [(prompt, None), ("<|user|>\n<|image_1|>\nWhat is this?<|end|>\n<|assistant|>\n", [img]),
             (["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nA longer question here, padded left<|end|>\n<|assistant|>\n",
               "<|user|>\nWhy?<|end|>\n<|assistant|>\n"], None)]
    for text, imgs in cases:
        inputs = proc(text, imgs)
        B = inputs["input_ids"].shape[0]
        rows = sampling.rows(B, [0.8, 0.0, 1.5][:B], [0, 5, 40][:B], [0.9, 1.0, 0.5][:B], 77)
        logits, cache = model(**inputs, max_tokens=10)
        first = ops.sample(logits[:, -1, :], sampling.pack(rows, 0).cuda())
        toks = [first.cpu().tolist()]
        assert toks[0] == [sample_ref(_logits_bits(logits[b, -1]), *rows[b], 0) for b in range(B)]
        st = cache[0].state
        model.set_sampling(st, sampling.pack(rows, 1))
        token = first[:, None]
        by_hand = []
        for step in range(6):
            lg, token = model.sample_step(token, cache)
            torch.cuda.synchronize()
            got = token.reshape(-1).cpu().tolist()
            want = [sample_ref(_logits_bits(lg[b]), *rows[b], step + 1) for b in range(B)]
            assert got == want, (text, step, got, want)
            by_hand.append(got)
        assert "sample_graph" in st.graphs["greedy"]
        # the one-step-ahead loop returns the same tokens
        logits, cache = model(**inputs, max_tokens=10)
        first = ops.sample(logits[:, -1, :], sampling.pack(rows, 0).cuda())
        seen = []
        api.greedy_loop(model, first[:, None], cache, 6, lambda r: seen.append(list(r)), lambda r: False, sampling=rows)
        assert seen == by_hand
    del model
    torch.cuda.empty_cache()


def test_generate_temperature_zero_is_todays_path():
    from phi_3_vision_mlx_amd import api
    model, proc = _tiny()
    prompt = "<|user|>\nHello there<|end|>\n<|assistant|>\n"
    ref = api._generate(model, proc, prompt, max_tokens=10, verbose=False, stream=False, mute=True)
    states = list(model._states)
    got = api._generate(model, proc, prompt, max_tokens=10, verbose=False, stream=False, mute=True, temperature=0.0, seed=9)
    assert got == ref
    assert not any("sample_graph" in s.graphs.get("greedy", {}) for s in model._states)
    assert not any(getattr(s, "sample_rows", None) is not None for s in model._states if s not in states)


def test_sampled_loop_survives_a_timed_out_fused_launch(monkeypatch, capsys):
    from phi_3_vision_mlx_amd import api, ops, sampling
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, processor = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=2)
    ids = torch.randint(3, 32000, (1, 1700), dtype=torch.int64, generator=torch.Generator().manual_seed(6))
    rows = sampling.rows(1, 1.0, 0, 0.95, 2024)

    def run(fail):
        if fail is None:
            monkeypatch.delenv("P3V_DEBUG_FAIL_STEP", raising=False)
        else:
            monkeypatch.setenv("P3V_DEBUG_FAIL_STEP", str(fail))
        logits, cache = model(input_ids=ids, max_tokens=40)
        token = ops.sample(logits[:, -1, :], sampling.pack(rows, 0).cuda())[:, None]
        seen = []
        out = api.greedy_loop(model, token, cache, 12, lambda r: seen.append(list(r)), lambda r: False, sampling=rows)
        return seen, out.reshape(-1).tolist(), cache[0].state.offset, cache[0].state.graphs["greedy"]["bufs"]["plan"].fuse_o

    model.serving = False
    good, last, off, fused = run(None)
    assert fused and len(good) == 12 and off == 1700 + 12
    for fail in (0, 5, 11):
        model.serving = False
        rows_, last2, off2, fused2 = run(fail)
        assert rows_ == good and last2 == last and off2 == off and not fused2 and model.serving
        assert "continuing with separate launches" in capsys.readouterr().err
    del model
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- engine + HTTP
def _engine_run(model, proc, reqs, settings):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    eng = ContinuousEngine(model, proc, slots=4, window=4096)
    records = {}
    orig = model.sample_step

    def spy(token, cache):
        st = cache[0].state
        before = st.sample_rows.clone()
        lg, tok = orig(token, cache)
        torch.cuda.synchronize()
        records[eng.steps] = (before.cpu(), lg.detach().clone(), tok.reshape(-1).cpu().tolist())
        return lg, tok

    model.sample_step = spy
    try:
        hs = [eng.submit(r, 8, sampling=s) if s else eng.submit(r, 8) for r, s in zip(reqs[:3], settings[:3])]
        eng.step()
        eng.step()
        hs += [eng.submit(r, 8, sampling=s) if s else eng.submit(r, 8) for r, s in zip(reqs[3:], settings[3:])]
        eng.run_until_idle()
    finally:
        del model.sample_step
    assert all(h.error is None for h in hs), [h.error for h in hs]
    from phi_3_vision_mlx_amd import sampling
    for _, (rec, lg, tok) in records.items():
        for b, r in enumerate(sampling.unpack(rec)):
            if r["temperature"] > 0:
                want = sample_ref(_logits_bits(lg[b]), r["temperature"], r["top_k"], r["top_p"], r["seed"], r["counter"])
                assert tok[b] == want
    return [h.tokens for h in hs], records


def test_engine_mixed_sampled_and_greedy_requests():
    from test_serving_gpu import _tiny_serve
    g, model, proc, reqs = _tiny_serve()
    reqs = [reqs[i] for i in (1, 2, 3, 4, 5, 6)]
    settings = [None, {"temperature": 0.8, "seed": 1}, {"temperature": 1.2, "top_k": 40, "seed": 2}, None,
                {"temperature": 0.6, "top_p": 0.9, "seed": 3}, {"temperature": 2.0, "top_k": 5, "top_p": 0.5, "seed": 4}]
    toks1, recs1 = _engine_run(model, proc, reqs, settings)
    toks2, _ = _engine_run(model, proc, reqs, settings)
    assert toks1 == toks2 and len(recs1) > 0
    # the greedy requests match the oracle, as test_engine_tiny_requests_join_mid_flight_and_match_the_oracle checks them
    from test_serving_gpu import tokens_vs_fixture
    n = tokens_vs_fixture([toks1[0], toks1[3]], g, "engine+sampling", rows=[1, 4], min_first=2, budgets=[8, 8])
    assert n >= 4


def test_http_on_the_engine_reproduces_with_the_returned_seeds():
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device="cuda:0")
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
        body = {"prompt": ["Once upon a time", "The weather"], "max_tokens": 12, "temperature": 1.0, "top_p": 0.9}
        a = post({**body, "seed": 42})
        b = post({**body, "seed": 42})
        assert a == b and a["seeds"] == [42, 43]
        c = post(body)
        d = post({**body, "seed": c["seeds"][0]})
        assert d["responses"] == c["responses"] and d["seeds"] == c["seeds"]
    finally:
        httpd.shutdown()
        backend.close()
