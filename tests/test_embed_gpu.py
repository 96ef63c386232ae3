"""Embeddings end to end on the tiny synthetic model: api.embed against the CPU oracle's final-normed hidden state
(tests/golden/tiny_embed_oracle.npz, from OraclePhi3V.backbone) under the rule tests/test_model_gpu.py applies to this model's logits
against this oracle; normalisation; batch invariance; the pooled state through lm_head against the plain prefill; no state leaking
into a following generate; retrieval.VDB on the device; ContinuousEngine.embed between the steps of two generations; the HTTP
surface on the one-request path and under --continuous."""
import base64
import json
import os
import sys
import threading
import urllib.request

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_golden_embed as gge  # noqa: E402
from test_model_gpu import assert_logits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    yield model, proc
    del model
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def golden():
    return np.load(gge.FIXTURE)


@pytest.fixture(scope="module")
def embedded(tiny):
    """api.embed of the fixture's three requests, un-normalised, both poolings: computed once, shared, left unchanged."""
    from phi_3_vision_mlx_amd import api
    return {(name, pooling): api.embed(prompt, images, preload=tiny, pooling=pooling, normalize=False)
            for name, (prompt, images) in gge.requests().items() for pooling in ("last", "mean")}


def _rule(got, ref, what):
    """assert_logits' rule, with the worst |got - ref| / (1.5e-2 max|ref| + 2e-2 |ref|) printed first."""
    got, ref = torch.as_tensor(np.asarray(got)).float(), torch.as_tensor(np.asarray(ref)).float()
    got, ref = (got[None] if got.dim() == 1 else got), (ref[None] if ref.dim() == 1 else ref)
    tol = 1.5e-2 * ref.abs().max() + 2e-2 * ref.abs()
    print(f"{what}: worst |got - ref| / tol {float(((got - ref).abs() / tol).max()):.3f} (|ref|max {float(ref.abs().max()):.3f})")
    assert_logits(got, ref, what)


@pytest.mark.parametrize("name", ["text", "batch", "image"])
@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_embed_matches_the_oracle_hidden_state(embedded, golden, name, pooling):
    got = embedded[(name, pooling)]
    assert got.dtype == np.float32 and got.shape == (golden[f"{name}_{pooling}"].shape if name == "batch" else golden[f"{name}_{pooling}"][0].shape)
    _rule(got, golden[f"{name}_{pooling}"], f"{name} {pooling}")


@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_normalize_divides_by_the_fp64_norm(tiny, embedded, pooling):
    from phi_3_vision_mlx_amd import api
    prompt, _ = gge.requests()["batch"]
    e = api.embed(prompt, preload=tiny, pooling=pooling).astype(np.float64)
    p = embedded[("batch", pooling)].astype(np.float64)
    want = p / np.sqrt((p * p).sum(-1, keepdims=True))
    rel = np.abs(e - want) / np.where(want == 0, 1.0, np.abs(want))
    print(f"normalize {pooling}: worst |e - p / |p|| / |e| {rel.max():.3e} (the bound: {2.0 ** -20:.3e})")
    assert np.all(np.abs(e - want) <= 2.0 ** -20 * np.abs(want))
    assert np.allclose(np.linalg.norm(e, axis=-1), 1.0, atol=1e-5)


@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_a_prompt_alone_and_inside_the_padded_batch_agree(tiny, embedded, pooling):
    from phi_3_vision_mlx_amd import api
    batch = embedded[("batch", pooling)]
    for b, prompt in enumerate(gge.BATCH):
        alone = api.embed(prompt, preload=tiny, pooling=pooling, normalize=False)
        assert alone.shape == batch[b].shape
        _rule(batch[b], alone, f"row {b} in the batch vs alone, {pooling}")


def test_pooled_state_through_lm_head_is_the_prefill_logits_row(tiny, embedded):
    from phi_3_vision_mlx_amd.api import _apply_chat_template
    model, proc = tiny
    text, _ = _apply_chat_template(gge.TEXT, None, False)
    inputs = proc(text)
    logits, _ = model(**inputs)
    x = torch.as_tensor(embedded[("text", "last")]).to("cuda:0")
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.float(), x)                                       # LAST, un-normalised: fp32 of bf16 values
    got = model._proj(xb[None].contiguous(), "lm_head.weight").view(1, -1)
    ref = logits[:, -1, :].view(1, -1)
    print(f"embed -> lm_head vs the prefill's last logits row: {'bit-exact' if torch.equal(got, ref) else 'not bit-exact'}, "
          f"max |diff| {float((got.float() - ref.float()).abs().max()):.4f}")
    assert_logits(got, ref, "embed -> lm_head")


def test_embed_leaves_a_following_generate_unchanged(tiny):
    from phi_3_vision_mlx_amd import api
    prompts = ["Tell me a story", gge.BATCH]
    run = lambda p: api.generate(p, preload=tiny, max_tokens=8, verbose=False, stream=False)   # noqa: E731
    before = [run(p) for p in prompts]
    for pooling in ("last", "mean"):
        api.embed(gge.BATCH, preload=tiny, pooling=pooling)
        api.embed(gge.TEXT, preload=tiny, pooling=pooling)
        assert [run(p) for p in prompts] == before, pooling


def test_embed_refuses_bad_arguments(tiny):
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    with pytest.raises(ValueError, match="'last' or 'mean'"):
        model.embed(proc("<|user|>\nHi<|end|>\n<|assistant|>\n")["input_ids"], pooling="first")
    with pytest.raises(ValueError, match="unknown adapter"):
        api.embed("hi", preload=tiny, adapter="law")


# ---------------------------------------------------------------------------------------------------- VDB
WORDS = ("river", "lantern", "copper", "violin", "harbour", "glacier", "saffron", "meadow", "anchor", "thunder")
TEXTS = [f"{a} {b}" for a in WORDS[:8] for b in WORDS[5:]]                  # 40 short texts, all different


def test_vdb_on_the_device(tiny):
    from phi_3_vision_mlx_amd import VDB
    assert len(TEXTS) == 40 and len(set(TEXTS)) == 40
    db = VDB(TEXTS, preload=tiny, batch=8)
    assert len(db) == 40 and db.capacity == 64 and db.index.is_cuda and db.index.dtype == torch.bfloat16
    emb = db._embed(TEXTS)
    idx, score = db.search(emb, n_topk=5)
    assert idx.shape == score.shape == (40, 5) and idx[:, 0].tolist() == list(range(40))     # every text finds itself first
    assert [row[0] for row in db(TEXTS[:3])] == TEXTS[:3] and db(TEXTS[7], 2)[0][0] == TEXTS[7]
    for q in range(40):                                                     # the k results ARE a stable sort of their own scores
        assert np.lexsort((idx[q], -score[q].astype(np.float64))).tolist() == list(range(5)), q
    rows = db.index[:40].double().cpu().numpy()
    qs = torch.as_tensor(db._rows(emb)).to(torch.bfloat16).double().numpy()
    s64 = qs @ rows.T
    E = rows.shape[1] * 2.0 ** -23 * (np.abs(qs) @ np.abs(rows).T)
    checked = 0
    for q in range(40):
        host = np.lexsort((np.arange(40), -s64[q]))
        for j in range(5):
            i = host[j]
            clear = all(abs(s64[q, i] - s64[q, host[o]]) > 4 * max(E[q, i], E[q, host[o]]) for o in (j - 1, j + 1) if 0 <= o < 40)
            if clear:
                checked += 1
                assert idx[q, j] == i and abs(score[q, j] - s64[q, i]) <= E[q, i], (q, j)
    print(f"VDB: {checked} of 200 ranks clear of their neighbours by 4 E, all equal to the fp64 ranking")
    assert checked >= 40
    with pytest.raises(ValueError, match="P3V_SIM_TOPK_MAX"):
        db.search(TEXTS[0], n_topk=33)


# ---------------------------------------------------------------------------------------------------- engine + HTTP
GEN = ["<|user|>\nTell me a long story about the sea<|end|>\n<|assistant|>\n", "<|user|>\nOne two three<|end|>\n<|assistant|>\n"]


def _engine_tokens(model, proc, embed_inputs=None):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    eng = ContinuousEngine(model, proc, slots=4, window=4096)
    hs = [eng.submit(proc(t), 12) for t in GEN]
    eng.step()
    eng.step()
    jobs = []
    if embed_inputs is not None:
        assert len(eng._active()) == 2                                      # two generations in flight
        jobs = [eng.embed(inp, pooling, normalize=False) for inp in embed_inputs for pooling in ("last", "mean")]
        eng.step()
        assert all(j.done.is_set() for j in jobs)                           # served between two steps
    eng.run_until_idle()
    assert all(h.error is None for h in hs) and eng.failures == 0
    return [h.tokens for h in hs], jobs


def test_engine_embed_between_the_steps_of_two_generations(tiny, embedded):
    from phi_3_vision_mlx_amd.api import _apply_chat_template
    model, proc = tiny
    plain, _ = _engine_tokens(model, proc)
    inputs = [proc(*_apply_chat_template(p, im, False)) for p, im in (gge.requests()["text"], gge.requests()["batch"])]
    tokens, jobs = _engine_tokens(model, proc, inputs)
    assert tokens == plain                                                  # the generations did not notice
    assert all(j.error is None for j in jobs), [j.error for j in jobs]
    for j, key in zip(jobs, (("text", "last"), ("text", "mean"), ("batch", "last"), ("batch", "mean"))):
        ref = embedded[key]
        assert j.result.dtype == np.float32 and j.result.shape == (np.atleast_2d(ref)).shape
        _rule(j.result, np.atleast_2d(ref), f"engine {key}")
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    small = ContinuousEngine(model, proc, slots=2, window=64)
    with pytest.raises(ValueError, match="window of 64"):
        small.embed(inputs[0] if np.asarray(inputs[0]["input_ids"]).shape[-1] > 64 else proc("x " * 80))


def _post(port, body):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/embeddings", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=300) as r:
        return json.loads(r.read())


def _check_http(port, tiny):
    from phi_3_vision_mlx_amd import api
    ref = api.embed(gge.BATCH, preload=tiny, pooling="mean")
    out = _post(port, {"input": gge.BATCH, "pooling": "mean"})
    got = np.asarray([d["embedding"] for d in out["data"]], dtype=np.float32)
    assert out["object"] == "list" and [d["index"] for d in out["data"]] == [0, 1, 2] and got.shape == ref.shape
    _rule(got, ref, "http float")
    assert out["usage"]["prompt_tokens"] == out["usage"]["total_tokens"] == int(np.load(gge.FIXTURE)["batch_live"].sum())
    one = _post(port, {"input": gge.TEXT, "encoding_format": "base64", "normalize": False})
    vec = np.frombuffer(base64.b64decode(one["data"][0]["embedding"]), dtype="<f4")
    _rule(vec, api.embed(gge.TEXT, preload=tiny, normalize=False), "http base64")
    assert len(one["data"]) == 1 and one["usage"]["prompt_tokens"] == int(np.load(gge.FIXTURE)["text_live"][0])


def test_http_round_trip_on_the_one_request_path(tiny):
    from phi_3_vision_mlx_amd import api
    from phi_3_vision_mlx_amd.server import serve

    def embed_fn(prompts, images=None, pooling="last", normalize=True, adapter=None):
        info = {}
        out = api.embed(prompts[0] if len(prompts) == 1 else prompts, preload=tiny, pooling=pooling, normalize=normalize, info=info)
        return out, info["prompt_tokens"]

    httpd, engine = serve(lambda prompts, max_tokens: ["x"] * len(prompts), port=0, embed_fn=embed_fn, device=tiny[0].device)
    threading.Thread(target=httpd.serve_forever, args=(0.02,), daemon=True).start()
    try:
        _check_http(httpd.server_address[1], tiny)
    finally:
        httpd.shutdown()
        engine.close()


def test_http_round_trip_under_continuous(tiny):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = tiny
    httpd, backend = serve_continuous(ContinuousEngine(model, proc, slots=2, window=4096), port=0)
    threading.Thread(target=httpd.serve_forever, args=(0.02,), daemon=True).start()
    try:
        _check_http(httpd.server_address[1], tiny)
    finally:
        httpd.shutdown()
        backend.close()
