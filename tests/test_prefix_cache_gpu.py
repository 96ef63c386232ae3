"""The prompt prefix cache on the GPU, against tests/golden/tiny_prefix_oracle.npz (tests/golden/gen_golden_prefix.py).

A warm request -- prefix K/V restored from the store, the rest of the prompt computed as a cached call -- is NOT compared with
the cold run of the code under test: its yardstick is the request's own B = 1 ORACLE run under the fixture tolerance model
(`logits_vs_fixture`: every first-step logit inside the tolerance; `tokens_vs_fixture`: tokens equal up to the request's first
unclear step).  Bit-equality is asked of the copy and of the plumbing only (the int8 test)."""
import json
import threading
import urllib.request

import numpy as np
import pytest
import torch

from gen_golden_prefix import NAMES, PROMPTS, STEPS, request, source_image
from test_model_gpu import GOLDEN, head_row_norms, logits_vs_fixture
from test_serving_gpu import IdTokenizer, _png_uri, _post, tokens_vs_fixture

pytestmark = pytest.mark.gpu

IMG_P = 2513                       # tokens of an image request's default entry: through its last image slot (index 2512)


def _tiny_prefix(**kw):
    from phi_3_vision_mlx_amd.api import load_synthetic
    g = np.load(GOLDEN + "/tiny_prefix_oracle.npz")
    assert g["names"].tolist() == NAMES
    model, proc = load_synthetic(blind_model=False, tiny=True, seed=0, std_scale=4.0, device="cuda:0",
                                 lm_head_spread=float(g["spread"][0]), lm_head_seed=int(g["head_seed"][0]), **kw)
    return g, model, proc


def _inputs(proc, g):
    from phi_3_vision_mlx_amd.prefix import image_digests
    reqs = {n: request(proc, n) for n in NAMES}
    assert [int(np.asarray(reqs[n]["input_ids"]).shape[-1]) for n in NAMES] == g["n_ids"].tolist()
    digests = {n: image_digests([source_image(n)]) if source_image(n) is not None else None for n in NAMES}
    assert np.array_equal(reqs["img0"]["input_ids"], reqs["img1"]["input_ids"]) and digests["img0"] != digests["img1"]
    assert digests["img0"] == digests["img0_q2"] == digests["img0_q3"]
    return reqs, digests


def _ids(inputs):
    return np.asarray(inputs["input_ids"]).reshape(-1)


def _key(store, model, st, adapter=None):
    return store.key(model.epoch, adapter, st.T > model.cfg.original_max_position_embeddings, "int8" if st.quantized else "bf16")


class Spy:
    """Counts vision-tower runs and records the number of ids every decoder-stack call saw."""

    def __init__(self, model):
        self.model, self.clip, self.L = model, 0, []
        self.real_layers, self.real_clip = model._layers, model.clip_forward

        def layers(x, st, B, L, *a, **kw):
            self.L.append(B * L)
            return self.real_layers(x, st, B, L, *a, **kw)

        def clip(pix):
            self.clip += 1
            return self.real_clip(pix)
        model._layers, model.clip_forward = layers, clip

    def close(self):
        del self.model._layers, self.model.clip_forward


def _decode(model, st, first, n_steps):
    """Free-running greedy steps for ALL rows of a slot state (the engine's own loop): first [rows] -> [rows][n_steps + 1]."""
    gph = model.decode_graph(st)
    gph["tok"].copy_(torch.as_tensor(first, dtype=torch.int32))
    cache = [type("L", (), {"state": st})()]
    out = [[int(t)] for t in first]
    for _ in range(n_steps):
        _, tok = model.greedy_step(gph["host_tok"] if gph["host_tok"] is not None else gph["tok"].view(-1, 1), cache)
        for r, t in enumerate(tok.reshape(-1).tolist()):
            out[r].append(t)
    return out


def test_model_level_warm_prefill_matches_each_requests_own_oracle():
    """One slot state, column 2560: img0 cold into row 0 and captured; img0_q2 / img0_q3 warm (pads 9 / 15 against the entry's
    26: capture and restore shift V^T by odd element counts); sys_q1 cold + captured, sys_q2 warm."""
    from phi_3_vision_mlx_amd.prefix import PrefixCache, capture_len
    g, model, proc = _tiny_prefix()
    reqs, digests = _inputs(proc, g)
    norms = head_row_norms(model)
    st = model.new_slot_state(5, 4096)
    st.offset = 2560
    store = PrefixCache(1 << 30, min_tokens=64)
    key = _key(store, model, st)
    spy = Spy(model)
    first, rows = [], ["img0", "img0_q2", "img0_q3", "sys_q1", "sys_q2"]
    try:
        for row, name in enumerate(rows):
            ids, S = _ids(reqs[name]), int(g["n_ids"][NAMES.index(name)])
            hit = store.lookup(ids, digests[name], key)
            spy.clip, spy.L = 0, []
            tok, logits = model.prefill_slot(st, row, reqs[name], return_logits=True, **({} if hit is None else {"prefix": hit}))
            _, clear, worst = logits_vs_fixture(logits[:, -1], g, 0, norms, f"{name} ({'warm' if hit else 'cold'})", prefix=name + "_")
            print(f"{name}: {'warm P=%d' % hit[1] if hit else 'cold'}, worst first-step logit error {worst:.2f} x the tolerance")
            first.append(int(tok.reshape(-1)[0]))
            if name in ("img0", "sys_q1"):
                assert hit is None and spy.L == [S] and spy.clip == (1 if name == "img0" else 0)
                P = capture_len(ids)
                assert P == (IMG_P if name == "img0" else S)
                assert store.wants(ids, digests[name], key, P)
                store.insert(ids[:P], digests[name], key, model.capture_prefix(st, row, st.offset - S, P))
                assert not store.wants(ids, digests[name], key, P)
            else:
                assert hit is not None, name
                P = hit[1]
                assert spy.L == [S - P], (name, spy.L, S, P)       # the model call saw the last S - P ids only
                if name.startswith("img0"):
                    assert P == IMG_P and spy.clip == 0            # through the last slot; the vision tower did not run
                else:
                    assert 64 <= P < S - 1
    finally:
        spy.close()
    assert store.hits == 3 and store.tokens_reused == 2 * IMG_P + store.lookup(_ids(reqs["sys_q2"]), None, key, count=False)[1]
    toks = _decode(model, st, first, STEPS - 1)
    n = tokens_vs_fixture(toks, g, "model level", rows=[NAMES.index(r) for r in rows], min_first=2)
    assert n >= 10, n
    print(f"model level: {n} free-running tokens of 5 rows (3 of them warm) equal the oracle's")


def test_wrong_image_must_miss_and_the_fixture_can_tell():
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc = _tiny_prefix()
    reqs, digests = _inputs(proc, g)
    norms = head_row_norms(model)
    st = model.new_slot_state(3, 4096)
    st.offset = 2560
    store = PrefixCache(1 << 30, min_tokens=64)
    key = _key(store, model, st)
    ids, S = _ids(reqs["img0"]), int(g["n_ids"][0])
    model.prefill_slot(st, 0, reqs["img0"])
    entry = store.insert(ids[:IMG_P], digests["img0"], key, model.capture_prefix(st, 0, st.offset - S, IMG_P))
    assert store.lookup(ids, digests["img0"], key, count=False)[1] == IMG_P
    assert store.lookup(_ids(reqs["img1"]), digests["img1"], key) is None and store.misses == 1        # equal ids, another picture
    _, logits = model.prefill_slot(st, 1, reqs["img1"], return_logits=True)
    _, clear, worst = logits_vs_fixture(logits[:, -1], g, 0, norms, "img1 after img0 was cached", prefix="img1_")
    if clear.all():
        assert int(logits[:, -1].float().argmax(-1)[0]) == int(g["img1_tokens"][0, 0])
    # the digest check bypassed (lookup by ids only): img1 computed on top of img0's picture must FAIL the same comparison
    _, logits_bad = model.prefill_slot(st, 2, reqs["img1"], return_logits=True, prefix=(entry, IMG_P))
    with pytest.raises(AssertionError, match="logit error"):
        logits_vs_fixture(logits_bad[:, -1], g, 0, norms, "img1 on img0's prefix", prefix="img1_")
    print(f"wrong image: miss; cold logits {worst:.2f} x the tolerance; with img0's prefix forced the comparison fails as it must")


def _run_engine(model, proc, reqs, digests, store):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, cache_args
    eng = ContinuousEngine(model, proc, slots=3, window=4096, **({} if store is None else {"prefix_cache": store}))

    def inp(n):                                                   # (without a store: the processor's result as it is)
        return cache_args(reqs[n], image_digests=digests[n]) if store is not None and digests[n] is not None else reqs[n]
    budgets = {n: STEPS for n in NAMES}
    budgets["short"] = 3
    order = ["img0_q2", "sys_q2", "short"]                        # the LONGEST of each family first: the others fit left of the column
    h = {n: eng.submit(inp(n), budgets[n]) for n in order}
    for _ in range(2):
        eng.step()
    late = ["img0", "img0_q3", "img1", "sys_q1"]
    h.update({n: eng.submit(inp(n), budgets[n]) for n in late})
    eng.run_until_idle()
    assert all(h[n].done.is_set() and h[n].error is None for n in NAMES), {n: h[n].error for n in NAMES}
    assert eng.failures == 0 and eng.joined_mid_flight >= 1
    return eng, h, budgets


def _compare(h, g, budgets, what):
    six = [n for n in NAMES if n != "img1"]
    n = tokens_vs_fixture([h[x].tokens for x in six], g, what, rows=[NAMES.index(x) for x in six], min_first=2, budgets=[budgets[x] for x in six])
    n += tokens_vs_fixture([h["img1"].tokens], g, what + " img1", rows=[NAMES.index("img1")], min_first=0)
    return n


def test_engine_with_a_store_matches_the_oracle_and_is_invisible_when_off():
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc = _tiny_prefix()
    reqs, digests = _inputs(proc, g)
    store = PrefixCache(1 << 30, min_tokens=64)
    eng, h, budgets = _run_engine(model, proc, reqs, digests, store)
    n = _compare(h, g, budgets, "engine + store")
    assert n >= 12, n
    assert store.hits >= 3 and h["img0"].cached_tokens == IMG_P and h["img0_q3"].cached_tokens == IMG_P
    assert 64 <= h["sys_q1"].cached_tokens < int(g["n_ids"][NAMES.index("sys_q1")])
    assert h["img1"].cached_tokens == 0 and h["short"].cached_tokens == 0 and h["img0_q2"].cached_tokens == 0
    c = store.counters()
    assert c["tokens_reused"] == sum(x.cached_tokens for x in h.values()) and c["entries"] >= 3 and c["evictions"] == 0
    eng2, h2, _ = _run_engine(model, proc, reqs, digests, None)
    assert _compare(h2, g, budgets, "engine without a store") == n
    assert all(x.cached_tokens == 0 for x in h2.values())
    print(f"engine: {n} tokens of 7 requests equal the oracle's with the store ({c['hits']} hits, {c['misses']} misses) and without it")


def test_eviction_under_a_budget_that_holds_one_image_entry():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, cache_args
    from phi_3_vision_mlx_amd.prefix import PrefixCache, image_digests, kv_bytes
    from golden_inputs import make_image
    g, model, proc = _tiny_prefix()
    reqs, digests = _inputs(proc, g)
    cfg = model.cfg
    one = kv_bytes(IMG_P, cfg.num_hidden_layers, cfg.num_key_value_heads, model.hd, "bf16")
    store = PrefixCache(one + one // 2, min_tokens=64)
    eng = ContinuousEngine(model, proc, slots=1, window=4096, prefix_cache=store)
    third = make_image(336, 336, "noise", 7)
    extra = (proc("<|user|>\n<|image_1|>\nWhat is shown?<|end|>\n<|assistant|>\n", [third]), image_digests([third]))

    def run(name):
        inp, dg = (reqs[name], digests[name]) if name in reqs else extra
        r = eng.submit(cache_args(inp, image_digests=dg), STEPS)
        eng.run_until_idle()
        assert r.error is None
        if name in reqs:
            tokens_vs_fixture([r.tokens], g, f"eviction {name}", rows=[NAMES.index(name)], min_first=0 if name == "img1" else 2)
        return r.cached_tokens
    assert run("img0") == 0 and (store.entries, store.evictions) == (1, 0)
    assert run("img0_q2") == IMG_P
    assert run("img1") == 0 and (store.entries, store.evictions) == (1, 1)       # img1's entry pushed img0's out
    assert run("third") == 0 and (store.entries, store.evictions) == (1, 2)      # a third picture: img1's goes
    assert run("img1") == 0 and store.evictions == 3                              # ... so img1 misses again
    assert run("img0_q3") == 0 and store.evictions == 4                           # img0 went first: a miss now, captured again
    assert run("img0") == IMG_P and run("img0_q2") == IMG_P
    assert store.bytes == one and store.hits == 3


def test_int8_cache_round_trip_and_warm_request_bit_equal_to_the_hand_driven_model():
    """quantize_cache=True: capture / restore move codes AND scales bit for bit, and a warm request equals, bit for bit, the same
    model driven by hand (cold prefill of the first P ids, then a cached call on the rest).  (No oracle comparison here: the oracle's
    quantised-cache prefill attends on exact keys, a warm suffix on dequantised ones -- DESIGN.md section 7.)"""
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc = _tiny_prefix(use_quantized_cache=True)
    reqs, _ = _inputs(proc, g)
    st = model.new_slot_state(3, 4096)
    assert st.quantized
    st.offset = 400
    ids = _ids(reqs["sys_q1"])
    S, P = ids.size, 301
    model.prefill_slot(st, 0, reqs["sys_q1"])
    kv = model.capture_prefix(st, 0, st.offset - S, P)
    assert [t.dtype for t in kv] == [torch.uint8, torch.uint8, torch.float32, torch.float32]
    store = PrefixCache(1 << 30)
    entry = store.insert(ids[:P], None, _key(store, model, st), kv)
    before = [t.clone() for t in (st.k8, st.v8, st.ks, st.vs)]
    model._restore_prefix(st, 2, 33, entry, P)                    # another row, another column phase
    pad = st.offset - S
    assert torch.equal(st.k8[:, 2, :, 33:33 + P], st.k8[:, 0, :, pad:pad + P]) and torch.equal(st.v8[:, 2, :, :, 33:33 + P], st.v8[:, 0, :, :, pad:pad + P])
    assert torch.equal(st.ks[:, 2, :, 33:33 + P], st.ks[:, 0, :, pad:pad + P]) and torch.equal(st.vs[:, 2, :, 33:33 + P], st.vs[:, 0, :, pad:pad + P])
    for t, b in zip((st.k8, st.v8, st.ks, st.vs), before):        # nothing else moved
        t2 = t.clone()
        sl = (slice(None), 2, slice(None), slice(33, 33 + P)) if t.dim() == 4 or t is st.k8 else (slice(None), 2, slice(None), slice(None), slice(33, 33 + P))
        t2[sl] = b[sl]
        assert torch.equal(t2, b)
    for name in ("sys_q1", "sys_q2"):
        ids = _ids(reqs[name])
        S = ids.size
        for P in (S - 40, S - 7):                                 # suffixes of 40 (prompt-shaped call) and 7 tokens (decode-shaped call)
            la, cache = model(input_ids=ids[None, :P], max_tokens=S - P + 4)
            entry = store.insert(ids[:P], None, _key(store, model, cache[0].state), model.capture_prefix(cache[0].state, 0, 0, P))
            # (full_logits=False: as a prefill call does, the last layer's o_proj / MLP and the head run on the last row alone -- with
            #  all rows they are other kernels, and the comparison would measure that instead of the copy and the plumbing)
            lh, cache = model(input_ids=ids[None, P:], cache=cache, full_logits=False)
            lw, cw = model(input_ids=ids[None], max_tokens=4, prefix=(entry, P))
            assert cw[0].state.offset == cache[0].state.offset == S
            assert torch.equal(lh[:, -1].view(torch.int16), lw[:, -1].view(torch.int16)), (name, P)
            t = torch.as_tensor([[int(lw[:, -1].float().argmax(-1)[0])]], dtype=torch.int32, device=model.device)
            (l1, _), (l2, _) = model.greedy_step(t, cache), model.greedy_step(t, cw)
            assert torch.equal(l1.clone().view(torch.int16), l2.view(torch.int16))            # and the caches behind them agree


def test_adapter_bank_entries_are_keyed_by_adapter():
    from gen_golden_adapters import fixture_adapter
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    g, model, proc = _tiny_prefix()
    reqs, _ = _inputs(proc, g)
    model.set_adapter_bank({"A": resolve_adapter(model.cfg, *fixture_adapter(model.cfg, "A"))})
    store = PrefixCache(1 << 30, min_tokens=64)
    eng = ContinuousEngine(model, proc, slots=1, window=4096, prefix_cache=store)

    def run(name, adapter):
        r = eng.submit(reqs[name], STEPS, adapter=adapter)
        eng.run_until_idle()
        assert r.error is None
        if adapter is None:                                       # the base-model rows still equal the oracle's
            tokens_vs_fixture([r.tokens], g, f"bank {name}", rows=[NAMES.index(name)], min_first=2)
        return r.cached_tokens, r.tokens
    assert run("sys_q2", None)[0] == 0
    assert run("sys_q1", "A")[0] == 0                             # an entry captured without an adapter is not for "A" ...
    hit_a, toks_a = run("sys_q2", "A")
    assert hit_a >= 64                                            # ... its own entry is
    assert run("sys_q1", None)[0] >= 64
    store.clear()
    cold_a = run("sys_q2", "A")
    assert cold_a[0] == 0 and run("sys_q1", None)[0] == 0         # and vice versa
    assert cold_a[1][:2] == toks_a[:2]                            # (the adapted row, warm and cold: the same first tokens)
    model.set_adapter_bank({})                                    # epoch bump: everything captured so far is stale
    assert run("sys_q1", None)[0] == 0 and store.entries == 1


def test_http_second_post_about_the_same_image_reports_cached_tokens():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    from phi_3_vision_mlx_amd.server import serve_continuous
    g, model, proc = _tiny_prefix()
    proc.tokenizer = IdTokenizer(proc.tokenizer)
    store = PrefixCache(1 << 30, min_tokens=64)
    httpd, backend = serve_continuous(ContinuousEngine(model, proc, slots=2, window=4096, prefix_cache=store), port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    uri = _png_uri(source_image("img0"))
    try:
        a = _post(port, {"prompt": PROMPTS["img0"], "images": [uri], "max_tokens": STEPS})
        b = _post(port, {"prompt": PROMPTS["img0_q2"], "images": [uri], "max_tokens": STEPS})
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/v1/prefix_cache", timeout=60) as r:
            c = json.loads(r.read())["prefix_cache"]
        n_entries = c["entries"]
        d = _post(port, {"prompt": PROMPTS["sys_q1"], "max_tokens": STEPS, "cache_prompt": False})
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/v1/prefix_cache", timeout=60) as r:
            c2 = json.loads(r.read())["prefix_cache"]
    finally:
        httpd.shutdown()
        backend.close()
    assert a["cached_tokens"] == [0] and b["cached_tokens"] == [IMG_P] and d["cached_tokens"] == [0]
    assert c["hits"] == 1 and c["tokens_reused"] == IMG_P and n_entries == 1
    assert c2["entries"] == 1                                     # "cache_prompt": false left no entry
    toks = [[int(t) for t in x["responses"][0].split()] for x in (a, b, d)]
    assert tokens_vs_fixture(toks, g, "HTTP", rows=[NAMES.index(n) for n in ("img0", "img0_q2", "sys_q1")], min_first=2) >= 6


def test_api_generate_with_a_store_hits_on_the_second_call():
    from phi_3_vision_mlx_amd import api
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc = _tiny_prefix()
    proc.tokenizer = IdTokenizer(proc.tokenizer)
    store = PrefixCache(1 << 30, min_tokens=64)
    out = []
    for name in ("img0", "img0_q3", "sys_q1", "sys_q2"):
        img = source_image(name)
        txt = api.generate(PROMPTS[name], images=None if img is None else [img], preload=(model, proc), max_tokens=STEPS, verbose=False,
                           stream=False, prefix_cache=store)
        out.append([int(t) for t in (txt[0] if isinstance(txt, list) else txt).split()])
    # entries: img0's, sys_q1's, sys_q2's -- img0_q3's default range (through the last slot) is covered by img0's entry already
    assert store.hits == 2 and store.misses == 2 and store.tokens_reused > IMG_P + 64 and store.entries == 3
    assert tokens_vs_fixture(out, g, "api.generate", rows=[NAMES.index(n) for n in ("img0", "img0_q3", "sys_q1", "sys_q2")], min_first=2) >= 8
    sampled = api.generate(PROMPTS["img0_q2"], images=[source_image("img0")], preload=(model, proc), max_tokens=3, verbose=False, stream=False,
                           temperature=0.8, seed=5, prefix_cache=store)
    assert store.hits == 3 and sampled
    api.generate([PROMPTS["short"], PROMPTS["short"]], preload=(model, proc), max_tokens=2, verbose=False, stream=False, prefix_cache=store)
    assert store.bypassed == 1                                    # a list of prompts ignores the store
