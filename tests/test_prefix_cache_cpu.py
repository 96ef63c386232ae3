"""Host logic of the prompt prefix cache (prefix.py + its plumbing in engine.py / server.py), no GPU: the matching rule on
hand-made id arrays, the capture policy, LRU by bytes on CPU tensors, the counters, `submit`'s argument checks and the
engine's admission on the slot stub of tests/test_engine_cpu.py, the server's field parsing, and the argument checks of
p3v_kv_copy that return before anything is launched."""
import ctypes
import json
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import prefix
from phi_3_vision_mlx_amd.engine import ContinuousEngine, RegimeRouter, cache_args
from phi_3_vision_mlx_amd.prefix import PrefixCache, capture_len, match_len, slot_runs
from test_engine_cpu import SlotStub, req

KEY = PrefixCache.key(0, None, False, "bf16")


def prompt(head, n_img, tail, img_id=1):
    """ids: `head` text tokens, n_img slots of image `img_id`, `tail` text tokens."""
    return np.asarray(list(head) + [-img_id] * n_img + list(tail), dtype=np.int64)


def fake_kv(n_bytes):
    return (torch.zeros(n_bytes // 2, dtype=torch.uint8), torch.zeros(n_bytes - n_bytes // 2, dtype=torch.uint8))


# ----------------------------------------------------------------------------- the matching rule
def test_slot_runs_and_capture_len():
    ids = np.asarray([1, 5, -1, -1, -1, 7, -2, -2, 9, 9])
    assert slot_runs(ids) == [(2, 5, 0), (6, 8, 1)]
    assert slot_runs(np.asarray([1, 2, 3])) == []
    assert capture_len(ids) == 8                                 # through the LAST image slot
    assert capture_len(np.arange(1, 50)) == 49                   # no image: the whole prompt
    assert capture_len(ids, prefix_len=6) == 6 and capture_len(ids, prefix_len=100) == 10
    assert capture_len(ids, prefix_len=4) == 2 and capture_len(ids, prefix_len=7) == 6      # never inside a slot run


def test_match_is_cut_so_that_one_token_is_left_to_compute():
    ids = np.arange(1, 101)
    assert match_len(ids, None, ids, None) == 99                  # identical prompt: P <= S - 1
    assert match_len(ids, None, np.arange(1, 201), None) == 99
    assert match_len(np.arange(1, 201), None, ids, None) == 100   # the entry is the shorter one: all of it
    other = ids.copy()
    other[40] = 999
    assert match_len(other, None, ids, None) == 40
    assert match_len(ids, None, ids, None, leave=0) == 100
    assert match_len(np.asarray([5]), None, np.asarray([5, 6]), None) == 0


def test_match_never_ends_inside_a_slot_run():
    e = prompt([1, 2], 10, [7, 8, 9])
    # the request's picture has MORE slots: the common prefix ends inside its run -> none of that image
    assert match_len(prompt([1, 2], 12, [7, 8, 9]), ["d"], e, ["d"]) == 2
    # ... or FEWER slots: the entry's run goes on where the request's text starts
    assert match_len(prompt([1, 2], 8, [7, 8, 9]), ["d"], e, ["d"]) == 2
    # the S - 1 cut lands inside the run as well
    assert match_len(prompt([1, 2], 10, []), ["d"], e, ["d"]) == 2
    assert match_len(prompt([1, 2], 10, [7]), ["d"], e, ["d"]) == 12
    assert match_len(prompt([1, 2], 10, [7, 8, 5, 5]), ["d"], e, ["d"]) == 14


def test_digest_mismatch_is_a_miss_although_the_ids_are_equal():
    e = prompt([1, 2], 100, [7, 8, 9])
    r = e.copy()
    assert match_len(r, ["noise"], e, ["noise"]) == 104
    assert match_len(r, ["waves"], e, ["noise"]) == 2             # equal ids, another picture: only the text in front of it
    assert match_len(r, None, e, ["noise"]) == 2                  # no digest given: never trusted
    assert match_len(r, ["noise"], e, [None]) == 2
    store = PrefixCache(1 << 20, min_tokens=64)
    store.insert(e[:102], ["noise"], KEY, fake_kv(100))
    assert store.lookup(r, ["waves"], KEY) is None and store.lookup(r, ["noise"], KEY)[1] == 102
    assert (store.hits, store.misses, store.tokens_reused) == (1, 1, 102)


def test_two_images_first_cached_second_computed():
    e = np.concatenate([prompt([1], 70, [3]), prompt([], 50, [9, 9], img_id=2)])
    r = e.copy()
    assert slot_runs(e) == [(1, 71, 0), (72, 122, 1)]
    assert match_len(r, ["a", "b"], e, ["a", "b"]) == 123
    assert match_len(r, ["a", "x"], e, ["a", "b"]) == 72          # the second picture differs: through the first one's slots + text
    assert match_len(r, ["x", "b"], e, ["a", "b"]) == 1


def test_min_tokens_and_key_separation():
    ids = np.arange(1, 201)
    store = PrefixCache(1 << 20, min_tokens=64)
    store.insert(ids, None, KEY, fake_kv(64))
    assert store.lookup(np.concatenate([ids[:63], [999, 998]]), None, KEY) is None          # 63 common tokens < min_tokens
    assert store.lookup(np.concatenate([ids[:64], [999, 998]]), None, KEY)[1] == 64
    for other in (PrefixCache.key(0, "A", False, "bf16"), PrefixCache.key(0, None, True, "bf16"), PrefixCache.key(0, None, False, "int8")):
        assert store.lookup(ids, None, other) is None, other
    assert store.entries == 1
    assert store.lookup(ids, None, PrefixCache.key(1, None, False, "bf16")) is None          # a newer epoch: stale entries are dropped
    assert store.entries == 0 and store.bytes == 0
    with pytest.raises(ValueError):
        PrefixCache.key(0, None, False, "mlx4")


def test_longest_entry_wins():
    ids = np.arange(1, 301)
    store = PrefixCache(1 << 20, min_tokens=8)
    a = store.insert(ids[:100], None, KEY, fake_kv(10))
    b = store.insert(ids[:200], None, KEY, fake_kv(10))
    e, P = store.lookup(ids, None, KEY)
    assert e is b and P == 200
    e, P = store.lookup(np.concatenate([ids[:150], [7, 7]]), None, KEY)
    assert e is b and P == 150
    e, P = store.lookup(np.concatenate([ids[:50], [7, 7]]), None, KEY)
    assert P == 50 and e in (a, b)


# ----------------------------------------------------------------------------- capture policy, LRU, counters
def test_capture_policy():
    store = PrefixCache(1000, min_tokens=64)
    ids = prompt([1, 2], 100, [7, 8, 9])
    assert store.wants(ids, ["d"], KEY, capture_len(ids))
    assert not store.wants(ids, ["d"], KEY, 63)                   # shorter than min_tokens
    assert not store.wants(ids, ["d"], KEY, 102, nbytes=1001)     # larger than the whole budget
    assert store.insert(ids[:102], ["d"], KEY, fake_kv(400)) is not None
    assert not store.wants(ids, ["d"], KEY, 102)                  # covered already: no new entry
    assert not store.wants(prompt([1, 2], 100, [5, 5]), ["d"], KEY, 102)
    assert store.wants(ids, ["other"], KEY, 102)                  # the same ids with another picture are NOT covered
    assert store.wants(ids, ["d"], PrefixCache.key(0, "A", False, "bf16"), 102)
    assert store.wants(ids, ["d"], KEY, 105)                      # a longer range is not covered by the shorter entry
    assert store.insert(ids, ["d"], KEY, fake_kv(1001)) is None and store.entries == 1       # over budget: not stored, nothing evicted


def test_lru_by_bytes_and_counters():
    store = PrefixCache(1000, min_tokens=4)
    p = [np.arange(100 * k, 100 * k + 50) + 1 for k in range(4)]
    for k in range(2):
        store.insert(p[k], None, KEY, fake_kv(400))
    assert (store.entries, store.bytes, store.evictions) == (2, 800, 0)
    assert store.lookup(p[0], None, KEY)[1] == 49                 # touches entry 0: entry 1 is now the least recently used
    store.insert(p[2], None, KEY, fake_kv(400))
    assert (store.entries, store.bytes, store.evictions) == (2, 800, 1)
    assert store.lookup(p[1], None, KEY) is None and store.lookup(p[0], None, KEY) is not None and store.lookup(p[2], None, KEY) is not None
    store.insert(p[3], None, KEY, fake_kv(900))                   # needs both out
    assert (store.entries, store.bytes, store.evictions) == (1, 900, 3)
    store.bypass()
    c = store.counters()
    assert c == {"hits": 3, "misses": 1, "bypassed": 1, "tokens_reused": 147, "entries": 1, "bytes": 900, "evictions": 3,
                 "max_bytes": 1000, "min_tokens": 4}
    e = store.lookup(p[3], None, KEY)[0]
    assert not e.ids.flags.writeable                              # entries are immutable
    with pytest.raises(ValueError):
        PrefixCache(-1)


def test_entry_sizes():
    assert prefix.kv_bytes(2513, 32, 32, 96, "bf16") == 2 * 32 * 32 * 2520 * 96 * 2
    assert prefix.kv_bytes(8, 2, 4, 96, "int8") == 2 * 2 * 4 * 8 * 100
    kv = prefix.alloc_kv(13, 2, 4, 96, "int8", "cpu")
    assert [tuple(t.shape) for t in kv] == [(2, 4, 16, 96), (2, 4, 96, 16), (2, 4, 16), (2, 4, 16)]
    assert sum(t.numel() * t.element_size() for t in kv) == prefix.kv_bytes(13, 2, 4, 96, "int8")
    kv = prefix.alloc_kv(16, 2, 4, 96, "bf16", "cpu")
    assert [tuple(t.shape) for t in kv] == [(2, 4, 16, 96), (2, 4, 96, 16)] and kv[0].dtype == torch.bfloat16
    assert sum(t.numel() * t.element_size() for t in kv) == prefix.kv_bytes(16, 2, 4, 96, "bf16")


def test_image_digest_is_of_the_source_image():
    from PIL import Image
    a = Image.fromarray(np.zeros((4, 6, 3), dtype=np.uint8), "RGB")
    b = Image.fromarray(np.zeros((6, 4, 3), dtype=np.uint8), "RGB")          # the same bytes, another size
    c = Image.fromarray(np.zeros((4, 6, 3), dtype=np.uint8), "RGB")
    c.putpixel((5, 3), (0, 0, 1))
    assert prefix.image_digest(a) == prefix.image_digest(a.copy())
    assert len({prefix.image_digest(i) for i in (a, b, c, a.convert("L"))}) == 4
    assert prefix.image_digests(None) is None and prefix.image_digests(a) == [prefix.image_digest(a)]


# ----------------------------------------------------------------------------- the engine on the slot stub
class PrefixStub(SlotStub):
    """The stub with the two model calls of the prefix cache; token arithmetic as SlotStub (a row's tokens depend on its prompt only)."""
    epoch = 0

    def __init__(self):
        super().__init__()
        self.warm, self.captures = [], []

    def prefill_slot(self, st, row, inputs, prefix=None):
        if prefix is not None:
            entry, P = prefix
            ids = np.asarray(inputs["input_ids"]).reshape(-1)
            assert 1 <= P <= ids.size - 1 and np.array_equal(entry.ids[:P], ids[:P])
            self.warm.append((row, int(P)))
        return super().prefill_slot(st, row, inputs)

    def capture_prefix(self, st, row, pad, P):
        assert pad == st.offset - int(st.offset - st.pad_len[row])
        self.captures.append((row, int(pad), int(P)))
        return fake_kv(64)


def shared(n_common, n_own, seed):
    ids = np.concatenate([np.arange(3, 3 + n_common), np.random.default_rng(seed).integers(700, 900, n_own)]).astype(np.int64)
    return {"input_ids": ids[None]}


def test_engine_without_a_store_calls_the_model_exactly_as_before():
    m = SlotStub()                                               # its prefill_slot takes no `prefix`, it has no capture_prefix
    e = ContinuousEngine(m, None, slots=2, window=4096)
    r = [e.submit(shared(100, 5, 1), 4), e.submit(cache_args(shared(100, 9, 2), cache_prompt=False), 4)]
    e.run_until_idle()
    assert all(x.error is None and len(x.tokens) == 4 and x.cached_tokens == 0 for x in r)


def test_engine_hits_are_prefilled_alone_and_misses_are_captured():
    m = PrefixStub()
    store = PrefixCache(1 << 20, min_tokens=64)
    e = ContinuousEngine(m, None, slots=3, window=4096, prefix_cache=store)
    a = e.submit(shared(100, 6, 1), 3)
    e.run_until_idle()
    assert a.error is None and a.cached_tokens == 0 and m.captures == [(0, 0, 106)] and store.entries == 1
    b, c, d = e.submit(shared(100, 6, 2), 3), e.submit(shared(100, 5, 3), 3), e.submit(cache_args(shared(100, 6, 1), cache_prompt=False), 3)
    e.run_until_idle()
    assert [x.error for x in (b, c, d)] == [None] * 3
    assert (b.cached_tokens, c.cached_tokens, d.cached_tokens) == (100, 100, 105)           # d: its own prompt again, one token left
    assert sorted(P for _, P in m.warm) == [100, 100, 105]
    assert all(len(lens) == 1 for _, lens in m.prefills[1:])     # nearly equal lengths, but hits never share a prefill pass
    assert store.hits == 3 and store.misses == 1 and store.tokens_reused == 305
    assert store.entries == 3 and len(m.captures) == 3           # b and c left their own prompts; d asked not to
    # tokens are what the same requests give without a store
    plain = ContinuousEngine(SlotStub(), None, slots=3, window=4096)
    q = [plain.submit(shared(100, 6, 2), 3), plain.submit(shared(100, 5, 3), 3)]
    plain.run_until_idle()
    assert [x.tokens for x in q] == [b.tokens, c.tokens]


def test_engine_failed_warm_prefill_fails_that_request_only_and_is_not_captured():
    m = PrefixStub()
    store = PrefixCache(1 << 20, min_tokens=64)
    e = ContinuousEngine(m, None, slots=2, window=4096, prefix_cache=store)
    e.submit(shared(100, 6, 1), 2)
    e.run_until_idle()
    bad = shared(100, 6, 4)
    bad["input_ids"][0, -1] = 666                                # SlotStub: "bad request"
    x, y = e.submit(bad, 2), e.submit(shared(100, 7, 5), 2)
    e.run_until_idle()
    assert isinstance(x.error, ValueError) and y.error is None and y.cached_tokens == 100
    assert store.entries == 2 and e.failures == 0                # the failed one left nothing behind
    e._recover(RuntimeError("boom"))                             # the slot state is rebuilt; the store (immutable copies) stays
    assert e.prefix_cache is store and store.entries == 2
    z = e.submit(shared(100, 3, 6), 2)
    e.run_until_idle()
    assert z.error is None and z.cached_tokens == 100


def test_submit_argument_validation():
    e = ContinuousEngine(PrefixStub(), None, slots=2, window=4096, prefix_cache=PrefixCache(1 << 20))
    ok = shared(80, 4, 1)
    img = dict(shared(80, 4, 1), image_sizes=np.asarray([[336, 336]]))
    for kw in (dict(image_digests="abc"), dict(image_digests=["a"]), dict(image_digests=[1]), dict(prefix_len=0), dict(prefix_len=-3),
               dict(prefix_len=2.5), dict(prefix_len=True), dict(cache_prompt="no")):
        r = e.submit(cache_args(ok, **kw), 4)
        assert r.done.is_set() and isinstance(r.error, ValueError), kw
    assert isinstance(e.submit(cache_args(img, image_digests=["a", "b"]), 4).error, ValueError)
    assert not e.waiting
    good = [e.submit(cache_args(img, image_digests=["a"]), 4), e.submit(cache_args(ok, prefix_len=70), 4), e.submit(cache_args(ok, cache_prompt=False), 4)]
    assert "prefix_cache_args" not in ok and "prefix_cache_args" not in img      # the processor's own result is never touched
    e.run_until_idle()
    assert all(r.error is None for r in good)
    # the arguments ride beside the inputs: a router hands them on as they are
    router = RegimeRouter([ContinuousEngine(PrefixStub(), None, slots=2, window=4096, prefix_cache=PrefixCache(1 << 20))])
    r = router.submit(cache_args(ok, prefix_len=70), 4)
    router.engines[0].run_until_idle()
    assert r.error is None and router.engines[0].model.captures == [(0, 0, 70)]
    plain = RegimeRouter([ContinuousEngine(SlotStub(), None, slots=2, window=4096)])
    r = plain.submit(ok, 4)
    plain.engines[0].run_until_idle()
    assert r.error is None


def test_explicit_prefix_len_and_mlx4_bypass():
    m = PrefixStub()
    store = PrefixCache(1 << 20, min_tokens=64)
    e = ContinuousEngine(m, None, slots=2, window=4096, prefix_cache=store)
    e.submit(cache_args(shared(100, 20, 1), prefix_len=90), 2)
    e.run_until_idle()
    assert m.captures == [(0, 0, 90)]
    e.st.mlx4 = True                                             # cache_format="mlx4": cold path, counted
    r = e.submit(shared(100, 20, 2), 2)
    e.run_until_idle()
    assert r.error is None and r.cached_tokens == 0 and store.bypassed == 1 and store.entries == 1 and m.warm == []


# ----------------------------------------------------------------------------- server
class FakeBackend:
    """What make_handler drives: `submit` + (optionally) `prefix_counters`."""

    def __init__(self, with_store):
        self.calls = []
        if with_store:
            self.prefix_counters = lambda: {"hits": 1, "misses": 2}

    def submit(self, prompts, max_tokens, images=None, **kw):
        self.calls.append(kw)
        if "info" in kw:
            kw["info"]["cached_tokens"] = [7] * len(prompts)
        return ["ok"] * len(prompts)


def _serve(backend):
    from http.server import ThreadingHTTPServer
    from phi_3_vision_mlx_amd.server import make_handler
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(backend))
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    return httpd, httpd.server_address[1]


def _post(port, body):
    rq = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(rq, timeout=30) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read() or b"{}")


def test_server_field_parsing():
    from phi_3_vision_mlx_amd.server import parse_cache_prompt
    assert parse_cache_prompt({}) is None and parse_cache_prompt({"cache_prompt": True}) is None
    assert parse_cache_prompt({"cache_prompt": False}) is False
    for bad in (0, 1, "false", None, [False]):
        with pytest.raises(ValueError):
            parse_cache_prompt({"cache_prompt": bad})
    b = FakeBackend(with_store=True)
    httpd, port = _serve(b)
    try:
        code, out = _post(port, {"prompt": ["a", "b"], "max_tokens": 2})
        assert code == 200 and out["cached_tokens"] == [7, 7] and "cache_prompt" not in b.calls[-1]
        code, out = _post(port, {"prompt": "a", "max_tokens": 2, "cache_prompt": False})
        assert code == 200 and b.calls[-1]["cache_prompt"] is False
        code, out = _post(port, {"prompt": "a", "cache_prompt": "no"})
        assert code == 400 and "cache_prompt" in out["error"]
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/v1/prefix_cache", timeout=30) as r:
            assert json.loads(r.read())["prefix_cache"] == {"hits": 1, "misses": 2}
    finally:
        httpd.shutdown()
    b = FakeBackend(with_store=False)                            # no store: no field, no endpoint, submit as before
    httpd, port = _serve(b)
    try:
        code, out = _post(port, {"prompt": "a", "max_tokens": 2, "cache_prompt": False})
        assert code == 200 and "cached_tokens" not in out and b.calls[-1] == {}
        with pytest.raises(urllib.error.HTTPError) as ei:
            urllib.request.urlopen(f"http://127.0.0.1:{port}/v1/prefix_cache", timeout=30)
        assert ei.value.code == 404
    finally:
        httpd.shutdown()


def test_continuous_backend_sums_the_engines_counters():
    from phi_3_vision_mlx_amd.server import ContinuousBackend, prefix_counters
    e1 = ContinuousEngine(PrefixStub(), None, slots=1, window=4096, prefix_cache=PrefixCache(1000, min_tokens=8))
    e2 = ContinuousEngine(PrefixStub(), None, slots=1, window=8192, prefix_cache=PrefixCache(500, min_tokens=8))
    e1.prefix_cache.insert(np.arange(1, 20), None, KEY, fake_kv(100))
    e2.prefix_cache.bypass()
    b = ContinuousBackend(RegimeRouter([e1, e2]))
    try:
        c = prefix_counters(b)
        assert c["entries"] == 1 and c["bytes"] == 100 and c["bypassed"] == 1 and c["max_bytes"] == 1500 and c["min_tokens"] == 8
    finally:
        b.close()
    b = ContinuousBackend(ContinuousEngine(SlotStub(), None, slots=1, window=4096))
    try:
        assert prefix_counters(b) is None
    finally:
        b.close()


# ----------------------------------------------------------------------------- the library's argument checks (nothing is launched)
def test_kv_copy_is_bound_and_refuses_bad_arguments_before_any_launch():
    from phi_3_vision_mlx_amd import _lib
    assert "p3v_kv_copy" in _lib.SIGNATURES and _lib.KV_COPY_MAX_JOBS >= 4 and ctypes.sizeof(_lib.KvCopyJob) == 104
    lib = _lib.lib()
    assert lib.p3v_version() == 600

    def job(**kw):
        j = _lib.KvCopyJob()
        j.k_src, j.v_src, j.k_dst, j.v_dst = 0x10000, 0x20000, 0x30000, 0x40000          # never dereferenced: every call below is refused
        j.B_src, j.T_src, j.B_dst, j.T_dst, j.n_tok = 1, 64, 2, 128, 8
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def call(j, n_jobs=1, nl=2, nkv=2, hd=96, es=2):
        arr = (_lib.KvCopyJob * 4)(j, j, j, j)
        return lib.p3v_kv_copy(arr, n_jobs, nl, nkv, hd, es, None)

    bad = [call(job(), n_jobs=0), call(job(), n_jobs=5), call(job(), es=4), call(job(), hd=100), call(job(), nl=0),
           call(job(t0_src=57)), call(job(t0_dst=121)), call(job(b_dst=2)), call(job(b_src=-1)), call(job(n_tok=-1)),
           call(job(k_src=0)), call(job(k_dst=0x30008)), call(job(v_src=0x20001)), call(job(ks_dst=0x50000)),
           call(job(k_dst=0x10000, B_dst=1, T_dst=64, t0_dst=4)),          # source and destination overlap
           call(job(), n_jobs=2)]                                           # two jobs with the same destination run
    assert bad == [-22] * len(bad), bad
    assert call(job(n_tok=0)) == 0                                          # an empty job: fine, and nothing to launch
