"""Embeddings and retrieval without a device: the host logic of retrieval.VDB under an injected embed function and a NumPy search,
the /v1/embeddings handler under a fake embed function, and the loud failure of the two ops without a GPU."""
import base64
import json
import threading
import urllib.error
import urllib.request
import zlib
from http.server import ThreadingHTTPServer

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------- VDB
def _texts(n):
    return [f"item {i}" for i in range(n)]


def _fake_embed(texts, D=32):
    """A deterministic un-normalised vector per text."""
    out = np.zeros((len(texts), D), dtype=np.float32)
    for r, t in enumerate(texts):
        rng = np.random.default_rng(zlib.crc32(t.encode()))
        out[r] = rng.standard_normal(D) * (1 + r % 3)
    return out


class NumpySearch:
    """The device search's contract in NumPy; records the chunks it was given."""

    def __init__(self):
        self.calls = []

    def __call__(self, index, n, queries, k):
        self.calls.append((int(index.shape[0]), int(n), int(queries.shape[0]), int(k)))
        rows = index[:n].float().numpy().astype(np.float64)
        q = torch.as_tensor(queries).to(torch.bfloat16).float().numpy().astype(np.float64)
        s = q @ rows.T
        idx = np.full((len(q), k), -1, dtype=np.int32)
        sc = np.full((len(q), k), -np.inf, dtype=np.float32)
        for i in range(len(q)):
            order = np.lexsort((np.arange(n), -s[i]))[:k]
            idx[i, :len(order)], sc[i, :len(order)] = order, s[i, order]
        return idx, sc


def _vdb(items=None, **kw):
    from phi_3_vision_mlx_amd import VDB
    search = NumpySearch()
    return VDB(items, embed_fn=_fake_embed, search_fn=search, device="cpu", **kw), search


def test_vdb_grows_by_doubling_and_keeps_its_rows():
    db, _ = _vdb(batch=8)
    assert len(db) == 0 and db.capacity == 0
    caps = []
    for i in range(0, 40, 5):
        db.add(_texts(40)[i:i + 5])
        caps.append(db.capacity)
    assert caps == [16, 16, 16, 32, 32, 32, 64, 64] and len(db) == 40 and db.items == _texts(40)
    rows = db.index[:40].float().numpy()
    want = _fake_embed(_texts(40))
    want = want / np.linalg.norm(want, axis=1, keepdims=True)
    assert np.allclose(np.linalg.norm(rows, axis=1), 1.0, atol=1e-2) and np.abs(rows - want).max() <= 2.0 ** -8
    assert db.index.dtype == torch.bfloat16 and not bool(db.index[40:].any())


def test_vdb_add_vectors_and_the_call_contract():
    from phi_3_vision_mlx_amd import api
    db, _ = _vdb()
    eye = np.eye(16, dtype=np.float32) * 3.0
    db.add_vectors(eye[:5], ["a", "b", "c", "d", {"k": 5}])
    assert api.VDB is type(db) and len(db) == 5
    idx, score = db.search(eye[2:4] + 0.25 * eye[0], n_topk=2)
    assert idx.tolist() == [[2, 0], [3, 0]] and idx.dtype == np.int32 and score.dtype == np.float32 and score.shape == (2, 2)
    assert db(eye[4:5], 1) == [[{"k": 5}]]                           # [[item, ...], ...]: the reference's VDB.__call__
    assert db(eye[1], n_topk=8)[0][0] == "b" and len(db(eye[1], n_topk=8)[0]) == 5      # fewer rows than k: what there is
    with pytest.raises(ValueError, match="5 items"):
        db.add_vectors(eye[:4], ["x"] * 5)
    with pytest.raises(ValueError, match="width"):
        db.add_vectors(np.ones((1, 24), dtype=np.float32), ["x"])
    with pytest.raises(ValueError, match="multiple of 8"):
        _vdb()[0].add_vectors(np.ones((1, 12), dtype=np.float32), ["x"])
    empty, _ = _vdb()
    assert empty("anything", 3) == [[]] and empty.search(["a", "b"], 2)[0].tolist() == [[-1, -1], [-1, -1]]


def test_vdb_text_queries_find_themselves_in_chunks_of_16():
    texts = _texts(40)
    db, search = _vdb(texts, key=str, batch=8)
    search.calls.clear()
    out = db(texts, n_topk=3)
    assert [c[2] for c in search.calls] == [16, 16, 8] and all(c[:2] == (64, 40) and c[3] == 3 for c in search.calls)
    assert [row[0] for row in out] == texts and all(len(row) == 3 for row in out)
    assert db("item 7") == [["item 7"]]
    keyed, _ = _vdb([{"t": t} for t in texts[:4]], key=lambda it: it["t"])
    assert keyed("item 2") == [[{"t": "item 2"}]]


def test_vdb_refuses_more_than_the_kernel_keeps():
    db, _ = _vdb(_texts(3))
    for bad in (0, 33, 1000):
        with pytest.raises(ValueError, match="P3V_SIM_TOPK_MAX"):
            db.search("item 1", n_topk=bad)
    with pytest.raises(ValueError, match="'last' or 'mean'"):
        _vdb(pooling="max")


def test_api_embed_checks_its_arguments_before_any_model():
    from phi_3_vision_mlx_amd import api

    class NoModel:
        def __getattr__(self, name):
            raise AssertionError("the model was touched")

    with pytest.raises(ValueError, match="'last' or 'mean'"):
        api.embed("hi", preload=(NoModel(), None), pooling="cls")
    with pytest.raises(ValueError, match="Images cannot be provided when prompt is a list"):
        api.embed(["a", "b"], images=["x"], preload=(NoModel(), None))
    import phi_3_vision_mlx_amd as pkg
    assert pkg.embed is api.embed and pkg.VDB is api.VDB


# ---------------------------------------------------------------------------------------------------- the handler
def _post(port, payload, path="/v1/embeddings"):
    req = urllib.request.Request(f"http://127.0.0.1:{port}{path}", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(req, timeout=10) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        body = e.read()
        try:
            return e.code, json.loads(body)
        except ValueError:
            return e.code, {}


def _serving(**kw):
    from phi_3_vision_mlx_amd.server import serve
    httpd, engine = serve(lambda prompts, max_tokens: ["x"] * len(prompts), port=0, **kw)
    threading.Thread(target=httpd.serve_forever, args=(0.02,), daemon=True).start()
    return httpd, engine


@pytest.fixture(scope="module")
def embed_server():
    calls = []

    def fake_embed(prompts, images=None, pooling="last", normalize=True, adapter=None):
        calls.append(dict(prompts=list(prompts), images=images, pooling=pooling, normalize=normalize, adapter=adapter,
                          thread=threading.current_thread().name))
        vec = np.stack([np.arange(4, dtype=np.float32) + len(p) + (0.5 if pooling == "mean" else 0.0) for p in prompts])
        return vec, [len(p.split()) + 2 for p in prompts]

    httpd, engine = _serving(embed_fn=fake_embed, adapter_names=["law"])
    yield httpd.server_address[1], calls, engine
    httpd.shutdown()
    engine.close()


def test_embeddings_round_trip_in_both_encodings(embed_server):
    port, calls, engine = embed_server
    calls.clear()
    code, out = _post(port, {"input": "two words"})
    assert code == 200 and out["object"] == "list" and out["model"] == "phi-3-vision"
    assert out["data"] == [{"object": "embedding", "index": 0, "embedding": [9.0, 10.0, 11.0, 12.0]}]
    assert out["usage"] == {"prompt_tokens": 4, "total_tokens": 4}
    code, out = _post(port, {"input": ["a", "bb cc"], "pooling": "mean", "normalize": False, "encoding_format": "base64",
                             "adapter": ["law", None]})
    assert code == 200 and [d["index"] for d in out["data"]] == [0, 1] and out["usage"] == {"prompt_tokens": 7, "total_tokens": 7}
    rows = [np.frombuffer(base64.b64decode(d["embedding"]), dtype="<f4") for d in out["data"]]
    assert rows[0].tolist() == [1.5, 2.5, 3.5, 4.5] and rows[1].tolist() == [5.5, 6.5, 7.5, 8.5]
    assert calls[1]["pooling"] == "mean" and calls[1]["normalize"] is False and calls[1]["adapter"] == ["law", None]
    assert calls[0]["images"] is None and calls[0]["adapter"] is None
    assert all(c["thread"] == engine.thread.name for c in calls)                        # the queue's worker, not the HTTP thread
    assert _post(port, {"prompt": "still here"}, "/v1/completions") == (200, {"model": "phi-3-vision", "responses": ["x"]})


@pytest.mark.parametrize("body, needle", [
    ({"input": 5}, "input must be"),
    ({"input": ["a", 5]}, "input must be"),
    ({"input": []}, "input must be"),
    ({}, "input must be"),
    ({"input": "a", "pooling": "max"}, "'last' or 'mean'"),
    ({"input": "a", "encoding_format": "hex"}, "'float' or 'base64'"),
    ({"input": "a", "normalize": "yes"}, "normalize"),
    ({"input": ["a", "b"], "images": [None]}, "one entry (or null) per input"),
    ({"input": ["a", "b"], "images": ["data:image/png;base64,AAAA", None]}, "Images cannot be provided"),
    ({"input": "a", "adapter": "nope"}, "unknown adapter"),
])
def test_embeddings_bad_fields_are_400_with_the_reason(embed_server, body, needle):
    port, calls, _ = embed_server
    calls.clear()
    code, out = _post(port, body)
    assert code == 400 and needle in out["error"], out
    assert calls == []


def test_embeddings_errors_of_the_embed_function_are_reported(embed_server):
    port, calls, engine = embed_server

    def boom(*a, **k):
        raise ValueError("embed: a prompt of 9000 tokens is outside this engine's window of 4096")
    keep, engine.embed_fn = engine.embed_fn, boom
    try:
        code, out = _post(port, {"input": "a"})
    finally:
        engine.embed_fn = keep
    assert code == 400 and "window" in out["error"]


def test_embeddings_path_is_404_without_an_embed_function():
    httpd, engine = _serving()
    try:
        code, _ = _post(httpd.server_address[1], {"input": "a"})
        assert code == 404
        assert _post(httpd.server_address[1], {"prompt": "a"}, "/v1/completions")[0] == 200
    finally:
        httpd.shutdown()
        engine.close()


def test_embeddings_behind_a_router_or_a_fleet_is_400_naming_the_limit():
    from phi_3_vision_mlx_amd.server import ContinuousBackend, make_handler

    class Leaf:
        processor = None

        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def adapter_names(self):
            return []

    class Router(Leaf):
        def __init__(self):
            self.engines = [Leaf(), Leaf()]

    class Fleet(Leaf):
        def __init__(self):
            self.engine = Leaf()

    for front, code_want in ((Router(), 400), (Fleet(), 400), (Leaf(), 404)):
        backend = ContinuousBackend(front)
        httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(backend))
        threading.Thread(target=httpd.serve_forever, args=(0.02,), daemon=True).start()
        try:
            code, out = _post(httpd.server_address[1], {"input": "a"})
            assert code == code_want
            if code == 400:
                assert "fleet" in out["error"] and "regime router" in out["error"] and "process group" in out["error"]
        finally:
            httpd.shutdown()
            backend.close()
    httpd, engine = _serving(embed_fn=lambda *a, **k: (np.zeros((1, 4)), [1]), embed_refusal="not on a process group")
    try:
        assert _post(httpd.server_address[1], {"input": "a"}) == (400, {"error": "not on a process group"})
    finally:
        httpd.shutdown()
        engine.close()


def test_continuous_backend_embeds_through_the_engine_handle():
    """ContinuousBackend.embed: chat template, processor, engine.embed, the handle's result and the live-token count."""
    from phi_3_vision_mlx_amd.engine import EmbedJob
    from phi_3_vision_mlx_amd.server import ContinuousBackend
    seen = []

    class Eng:
        def processor(self, text, images=None):
            seen.append(("proc", text, images))
            if isinstance(text, list):
                return {"input_ids": np.ones((2, 5), dtype=np.int64), "mask": np.array([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]])}
            return {"input_ids": np.ones((1, 7), dtype=np.int64)}

        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def embed(self, inputs, pooling="last", normalize=True, adapter=None):
            seen.append(("embed", pooling, normalize, adapter))
            job = EmbedJob(inputs, pooling, normalize, adapter)
            job.result = np.zeros((np.asarray(inputs["input_ids"]).shape[0], 4), dtype=np.float32)
            job.done.set()
            return job

    backend = ContinuousBackend(Eng())
    try:
        assert backend.embed_refusal is None
        vec, n = backend.embed(["a", "b"], None, "mean", False, ["law", None])
        assert vec.shape == (2, 4) and n == [3, 5] and seen[-1] == ("embed", "mean", False, ["law", None])
        assert seen[0][0] == "proc" and isinstance(seen[0][1], list) and all("<|user|>" in t for t in seen[0][1])
        vec, n = backend.embed(["a"], None, "last", True, None)
        assert vec.shape == (1, 4) and n == [7] and isinstance(seen[-2][1], str)
    finally:
        backend.close()


def test_engine_embed_refuses_at_submission():
    """ContinuousEngine.embed: above the window, a bad pooling -- ValueError before anything is queued (no model needed)."""
    import collections
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    eng = ContinuousEngine.__new__(ContinuousEngine)
    eng.window, eng.dead, eng.lock, eng.embed_jobs, eng.model = 64, None, threading.Lock(), collections.deque(), None
    with pytest.raises(ValueError, match="window of 64"):
        eng.embed({"input_ids": np.ones((1, 65), dtype=np.int64)})
    with pytest.raises(ValueError, match="'last' or 'mean'"):
        eng.embed({"input_ids": np.ones((1, 5), dtype=np.int64)}, pooling="max")
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.embed({"input_ids": np.ones((1, 5), dtype=np.int64)}, adapter="law")
    job = eng.embed({"input_ids": np.ones((2, 64), dtype=np.int64)}, "mean", False)
    assert list(eng.embed_jobs) == [job] and not job.done.is_set() and (job.pooling, job.normalize, job.adapter) == ("mean", False, None)
    job.cancel()
    eng._serve_embeds()                                                  # a cancelled job is dropped, not run (model is None)
    assert job.done.is_set() and job.result is None and job.error is None and not eng.embed_jobs


# ---------------------------------------------------------------------------------------------------- ops
def test_ops_fail_loudly_without_a_device():
    from phi_3_vision_mlx_amd import ops
    bf = torch.bfloat16
    if not torch.cuda.is_available():                                    # (with one, tests/test_embed_kernels_gpu.py runs the kernels)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.embed_pool(torch.zeros((1, 2, 8), dtype=bf), torch.zeros((8,), dtype=bf), 1e-5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sim_topk(torch.zeros((4, 8), dtype=bf), torch.zeros((1, 8), dtype=bf), 1)
    with pytest.raises(ValueError, match="'last' or 'mean'"):
        ops.embed_pool(torch.zeros((1, 2, 8), dtype=bf), torch.zeros((8,), dtype=bf), 1e-5, pooling="max")
    assert ops.sim_topk_plan(4099, 16, 32, 3072) == (256, 17, 32)
