"""Records what the serving stack's host path hands on, layer by layer, for a matrix of request options -- the fixture of
tests/test_serving_calls_cpu.py (tests/golden/serving_calls.json).  No model, no GPU: every backend is a recording stub.

    python tests/golden/gen_golden_serving_calls.py        # rewrites tests/golden/serving_calls.json

Three recordings:
  "http"    the real handler over HTTP (port 0) in five server configurations; per case the status, the response JSON and what each
            stub saw (positional count, sorted keyword names, the values that are plain data; a dict passed for statistics is "dict")
  "run"     server.run()'s `generate_fn` behind the real queue and handler: what `api.generate` / `dist.generate_sharded` receive
  "engine"  engine._generate_text, RegimeRouter and a router's submit in front of a stub `submit(inputs, max_tokens, **kw)`: whether
            `inputs` is the caller's object, which carrier keys ride beside it and which keywords arrive
Sampling always carries a seed, so nothing is random.
"""
import itertools
import json
import os
import sys
import threading
import types
import urllib.error
import urllib.request
from http.server import ThreadingHTTPServer

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "serving_calls.json")
EOS = 32007
INFO_KEYS = ("info", "logprob_info", "family_info", "spec_info")


def png():
    import base64
    from io import BytesIO
    from PIL import Image
    buf = BytesIO()
    Image.fromarray(np.full((8, 8, 3), 200, dtype=np.uint8)).save(buf, format="PNG")
    return "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()


# one body fragment per option; a pair is the union of two
OPTIONS = {
    "sampling": {"temperature": 0.7, "top_k": 5, "seed": 11},
    "adapter": {"adapter": "a1"},
    "logprobs": {"logprobs": 2},
    "penalties": {"repetition_penalty": 1.3, "logit_bias": {"5": -2.0}},
    "n": {"n": 3},
    "best_of": {"n": 2, "best_of": 4},
    "speculate": {"speculate": 4},
    "no_cache": {"cache_prompt": False},
    "two": {"prompt": ["a", "bb"]},
    "image": {"images": "PNG"},
}

BAD = {
    "temperature": [-1, "x", [0.5]], "top_p": [0, 2], "top_k": [-1, 1.5], "seed": [-1, "s"],
    "adapter": [7, "nope", ["a1", "a1"], [3]],
    "logprobs": [True, "2", 9, -1, [1]],
    "repetition_penalty": [0, "x", [1.1]], "presence_penalty": ["x"], "frequency_penalty": [[0.1]],
    "logit_bias": [[1], {"x": 1}, {"5": "y"}, {"100": 1.0}, {"-1": 1.0}],
    "n": [0, 17, True, "2", 2.5], "best_of": [1, 17, "4"],
    "speculate": [-1, 16, True, "3"],
    "cache_prompt": ["no", 0],
    "prompt": [7, []], "images": [["x", "y"], 5, "data:image/png;base64,####"], "max_tokens": ["x"],
}


def bodies():
    """name -> request body: plain, every option, every pair, the bad values."""
    out = {"plain": {}}
    for k, v in OPTIONS.items():
        out[k] = dict(v)
    for a, b in itertools.combinations(OPTIONS, 2):
        out[f"{a}+{b}"] = {**OPTIONS[a], **OPTIONS[b]}
    for field, values in BAD.items():
        for i, v in enumerate(values):
            out[f"bad:{field}:{i}"] = {field: v, **({"n": 2} if field == "best_of" else {})}
    uri = png()
    for body in out.values():
        body.setdefault("prompt", "a")
        body.setdefault("max_tokens", 4)
        if body.get("images") == "PNG":
            body["images"] = [uri] + [None] * (len(body["prompt"]) - 1 if isinstance(body["prompt"], list) else 0)
    return out


def plain(key, v):
    """A recorded value: JSON data as it is, a statistics dict as "dict", a picture as "image"."""
    if key in INFO_KEYS:
        return "dict" if isinstance(v, dict) else repr(type(v).__name__)
    if isinstance(v, (list, tuple)):
        return [plain(None, x) for x in v]
    if isinstance(v, dict):
        return {str(k): plain(None, x) for k, x in v.items()}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return "image" if hasattr(v, "tobytes") and hasattr(v, "mode") else type(v).__name__


def seen(names, args, kw):
    """What a stub saw: positional count, sorted keyword names, plain values."""
    return {"pos": len(args), "kw": sorted(kw), "args": {n: plain(n, a) for n, a in zip(names, args)},
            "vals": {k: plain(k, kw[k]) for k in sorted(kw)}}


def fake_entry(w):
    return dict(token_ids=[7, EOS], token_logprobs=[-0.5, -0.25], ranks=[1, 2], top_logprobs=[[(7 + j, -0.5 - j) for j in range(w)]] * 2)


def fill(prompts, kw, logprobs_key="logprob_info"):
    """Answer as a backend does: the texts, and the statistics dicts filled the way the real ones fill them."""
    prompts = [prompts] if isinstance(prompts, str) else list(prompts)
    wants = kw.get("logprobs")
    n = kw.get("n")
    count = n if n is not None else len(prompts)
    if wants is not None and kw.get(logprobs_key) is not None:
        wants = list(wants) if isinstance(wants, (list, tuple)) else [wants] * len(prompts)
        wants = wants * count if n is not None else wants
        rows = [None if w is None else fake_entry(w) for w in wants]
        if logprobs_key == "info":
            kw["info"]["logprobs"] = rows
        else:
            for key in ("token_ids", "token_logprobs", "ranks", "top_logprobs"):
                kw[logprobs_key][key] = [None if r is None else r[key] for r in rows]
    if kw.get("family_info") is not None and kw.get("sampling") is not None:
        kw["family_info"]["seeds"] = [100 + j for j in range(count)]
    if n is not None and logprobs_key == "info" and kw.get("sampling") is not None:
        kw["info"]["seeds"] = [100 + j for j in range(count)]
    if kw.get("spec_info") is not None:
        kw["spec_info"].update(steps=2, drafted=8, accepted=5)
    if logprobs_key == "info" and kw.get("info") is not None:
        kw["info"]["cached_tokens"] = [3] * len(prompts)
    return [f"{prompts[0]}#{j}" for j in range(n)] if n is not None else [f"{p}|" for p in prompts]


def post(port, body):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(req, timeout=20) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read())


def drive(httpd, calls, cases=None):
    """Post every body, one at a time; -> {case: [status, response, calls]}."""
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    out = {}
    try:
        for name, body in bodies().items():
            if cases is not None and not cases(name):
                continue
            del calls[:]
            status, resp = post(httpd.server_address[1], body)
            out[name] = [status, resp, list(calls)]
    finally:
        httpd.shutdown()
        httpd.server_close()
    return out


# ---------------------------------------------------------------------------------------------------- 1. the handler
def record_http():
    from phi_3_vision_mlx_amd.server import ContinuousBackend, make_handler, serve
    out = {}
    common = dict(port=0, window_s=0.001, adapter_names=["a1", "a2"], decode_fn=lambda i: f"<{i}>", vocab_size=100)
    for name, extra in (("queue", {}), ("merge", {"merge": True}),
                        ("sharded_spec", dict(sharded_fn=lambda prompts, images: images is not None, speculate=True, speculate_default=3))):
        calls = []

        def fake_generate(*args, **kw):
            calls.append(seen(("prompts", "max_tokens", "images"), args, kw))
            return fill(args[0], kw)
        httpd, engine = serve(fake_generate, **common, **extra)
        try:
            out[name] = drive(httpd, calls)
        finally:
            engine.close()

    class Tok:
        def decode(self, ids):
            return "".join(f"[{i}]" for i in ids)

    class Store:
        def counters(self):
            return {"hits": 1, "min_tokens": 16}

    for name, store in (("continuous_store", Store()), ("continuous", None)):
        calls = []

        class Eng:
            processor = types.SimpleNamespace(tokenizer=Tok())
            model = types.SimpleNamespace(cfg=types.SimpleNamespace(vocab_size=100))
            adapter_names = ["a1", "a2"]

            def serve_forever(self, stop, idle_sleep=0.002):
                stop.wait()

            def generate(self, *args, **kw):
                calls.append(seen(("prompts", "images", "max_tokens", "timeout"), args, kw))
                return fill(args[0], kw, "info")
        eng = Eng()
        if store is not None:
            eng.prefix_cache = store
        backend = ContinuousBackend(eng)
        try:
            out[name] = drive(ThreadingHTTPServer(("127.0.0.1", 0), make_handler(backend)), calls)
        finally:
            backend.close()
    return out


# ---------------------------------------------------------------------------------------------------- 2. run()'s generate_fn
DIRECT = {   # generate_fn called as the queue calls it for a merged group: per-row lists with rows that did not ask
    "rows:logprobs": dict(logprobs=[2, None], logprob_info={}),
    "rows:penalties": dict(penalties=[{"repetition_penalty": 1.3}, None]),
    "rows:adapter": dict(adapter=["a1", None]),
    "rows:sampling": dict(sampling=[dict(temperature=0.7, top_k=5, top_p=1.0, seed=11), dict(temperature=0.7, top_k=5, top_p=1.0, seed=12)]),
    "rows:all": dict(sampling=[dict(temperature=0.7, top_k=5, top_p=1.0, seed=11), dict(temperature=0.7, top_k=5, top_p=1.0, seed=12)],
                     adapter=["a1", "a2"], logprobs=[None, 1], logprob_info={}, penalties=[None, {"logit_bias": {"5": -2.0}, "presence_penalty": 0.5}]),
}


def record_run(patch):
    """`patch(obj, name, value)` as pytest's monkeypatch.setattr (the generator restores by hand)."""
    from phi_3_vision_mlx_amd import api, dist, server
    calls, caught = [], {}
    model = types.SimpleNamespace(device=None, cfg=types.SimpleNamespace(vocab_size=100))
    processor = types.SimpleNamespace(tokenizer=types.SimpleNamespace(decode=lambda ids: "".join(f"[{i}]" for i in ids)))

    def fake_api_generate(*args, **kw):
        assert kw.pop("preload")[0] is model
        calls.append(dict(seen(("prompt",), args, kw), fn="generate"))
        return fill(args[0], kw)

    def fake_sharded(*args, **kw):
        assert kw.pop("preload")[0] is model
        calls.append(dict(seen(("prompts", "images"), args, kw), fn="generate_sharded"))
        return fill(args[0], kw)

    def fake_serve(generate_fn, **kw):
        caught.update(generate_fn=generate_fn, kw=kw)
        return types.SimpleNamespace(serve_forever=lambda: None), types.SimpleNamespace(close=lambda: None)
    patch(api, "load", lambda **kw: (model, processor))
    patch(api, "generate", fake_api_generate)
    patch(dist, "generate_sharded", fake_sharded)
    real_serve = server.serve
    patch(server, "serve", fake_serve)
    out = {}
    for name, flags in (("run", {}), ("run_speculate", {"speculate": 3})):
        server.run(port=0, synthetic="tiny", adapters=None, **flags)
        kw = dict(caught["kw"], port=0, adapter_names=["a1", "a2"])
        kw.pop("host", None)
        kw.pop("length_fn", None)
        httpd, engine = real_serve(caught["generate_fn"], **kw)
        try:
            out[name] = drive(httpd, calls, cases=lambda c: not c.startswith("bad:"))
        finally:
            engine.close()
    out["direct"] = {}
    for name, kw in DIRECT.items():
        del calls[:]
        caught["generate_fn"](["a", "bb"], 4, None, **{k: (dict(v) if k == "logprob_info" else v) for k, v in kw.items()})
        out["direct"][name] = list(calls)
    return out


# ---------------------------------------------------------------------------------------------------- 3. the engine level
ENGINE_OPTIONS = {
    "sampling": dict(sampling="per prompt"),
    "adapter": dict(adapter="a1"),
    "logprobs": dict(logprobs=2),
    "penalties": dict(penalties={"repetition_penalty": 1.3, "logit_bias": {5: -2.0}}),
    "n": dict(n=3),
    "best_of": dict(n=2, best_of=4),
    "no_cache": dict(cache_prompt=False),
    "cache_true": dict(cache_prompt=True),
    "two": dict(prompts=["a", "bb"]),
    "image": dict(images="image"),
    "info": dict(info="dict"),
}


def record_engine():
    from PIL import Image
    from phi_3_vision_mlx_amd import engine as E
    carriers = (E.PREFIX_ARGS, E.LOGPROB_ARGS, E.PENALTY_ARGS, E.N_ARGS)
    made, calls = [], []

    class Tok:
        def decode(self, ids):
            return " ".join(map(str, ids))

    class Proc:
        tokenizer = Tok()

        def __call__(self, text, imgs=None):
            made.append({"input_ids": np.zeros((1, 4), dtype=np.int64)})
            if imgs is not None:
                made[-1]["image_sizes"] = np.zeros((len(imgs), 2), dtype=np.int64)
            return made[-1]

    class Stub:
        processor = Proc()
        window = 4096

        def accepts(self, S, max_tokens):
            return True

        def adapter_names(self):
            return ["a1", "a2"]

        def submit(self, inputs, max_tokens, **kw):
            calls.append({"same_object": any(inputs is m for m in made[-1:]), "keys": sorted(k for k in inputs if k in carriers),
                          "carried": {k: plain(None, inputs[k]) for k in carriers if k in inputs}, "max_tokens": max_tokens,
                          "kw": {k: plain(None, kw[k]) for k in sorted(kw)}})
            s = kw.get("sampling")
            want = E.requested_logprobs(inputs)
            r = E.Request(inputs, max_tokens, sampling=None if s is None else (s.get("temperature", 0.0), s.get("top_k", 0), s.get("top_p", 1.0), s["seed"]),
                          logprobs=want)
            fam = E.requested_n(inputs)
            if fam is not None:
                E.make_family(r, fam["n"], fam["best_of"] or fam["n"])
            for m in r.members:
                m.tokens = [11, EOS]
                m.logprob_records = [dict(token=t, logprob=-0.5, rank=1, top=[]) for t in m.tokens] if m.logprobs is not None else []
                m.done.set()
            r.settle()
            return r

    def one(front, opts, store):
        kw = {}
        for k in opts:
            kw.update(ENGINE_OPTIONS[k])
        prompts = kw.pop("prompts", "a")
        n_prompts = 1 if isinstance(prompts, str) else len(prompts)
        images = None
        if kw.pop("images", None):
            images = [[Image.fromarray(np.full((8, 8, 3), 200, dtype=np.uint8))]] + [None] * (n_prompts - 1)
        if "sampling" in kw:
            kw["sampling"] = [dict(temperature=0.7, top_k=5, top_p=1.0, seed=11 + b) for b in range(n_prompts)]
        info = {} if kw.pop("info", None) else None
        del calls[:], made[:]
        try:
            if front == "text":
                stub = Stub()
                if store:
                    stub.prefix_cache = object()
                out = E._generate_text(stub, stub.processor, prompts, images, 4, 5.0, info=info, **kw)
            else:
                stub = Stub()
                if store:
                    stub.prefix_cache = object()
                out = E.RegimeRouter([stub]).generate(prompts, images, 4, 5.0, info=info, **kw)
            res = {"out": out}
        except ValueError as e:
            res = {"error": str(e)}
        if info is not None:
            res["info"] = plain(None, info)
        return dict(res, calls=list(calls))

    out = {}
    names = list(ENGINE_OPTIONS)
    combos = [()] + [(a,) for a in names] + list(itertools.combinations(names, 2))
    for front in ("text", "router"):
        for store in (False, True):
            out[f"{front}{'_store' if store else ''}"] = {"+".join(c) or "plain": one(front, c, store) for c in combos}
    # a router's own submit: what rides beside the inputs passes through as it is
    stub = Stub()
    router, passed = E.RegimeRouter([stub]), {}
    base = {"input_ids": np.zeros((1, 4), dtype=np.int64)}
    for name, inputs, kw in (("plain", base, {}), ("sampling", base, {"sampling": {"temperature": 0.5, "seed": 3}}),
                             ("adapter", base, {"adapter": "a2"}),
                             ("carriers", E.n_args(E.cache_args(E.logprob_args(E.penalty_args(base, presence_penalty=0.5), 1), ["d"], False, 2), 2, 3), {})):
        del calls[:]
        made[:] = [inputs]
        router.submit(inputs, 4, **kw)
        passed[name] = list(calls)
    out["router_submit"] = passed
    return out


def record_all(patch):
    return {"http": record_http(), "run": record_run(patch), "engine": record_engine()}


def dumps(rec):
    """One case per line: compact, and a change shows up as the lines of the cases it touches."""
    lines = []
    for part, groups in rec.items():
        for group, cases in groups.items():
            for case, value in cases.items():
                lines.append(json.dumps([part, group, case, value], sort_keys=True, separators=(",", ":")))
    return "[\n" + ",\n".join(lines) + "\n]\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        text = dumps(record_all(patch))
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
    with open(PATH, "w") as f:
        f.write(text)
    print(f"wrote {PATH}: {len(text)} bytes")
