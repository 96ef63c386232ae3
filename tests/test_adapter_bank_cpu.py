"""Host logic of per-request LoRA adapters: `set_adapter_bank` argument checks that need no device, the engine's adapter plumbing
on a CPU stand-in for the model's slot interface, the server's "adapter" field on a stub generate function, the public
signatures, and the witnesses of tests/golden/tiny_adapters_oracle.npz recomputed from its stored tokens and margins."""
import inspect
import json
import os
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from gen_golden_adapters import ADAPTER_SPECS, ASSIGN, FIXTURE, VARIANTS, find_witnesses, fixture_adapter, synth_adapter, witnesses_cover

EOS = 32007


# ------------------------------------------------------------------ model: argument checks reachable without a device
def _host_model():
    """A Phi3VModel shell with the attributes the bank's checks read (no GPU: __init__ is not run)."""
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.model import Phi3VModel
    from phi_3_vision_mlx_amd.weights import synth_weights
    cfg = make_config(tiny_config_dict(vision=False))
    m = Phi3VModel.__new__(Phi3VModel)
    m.cfg, m.w, m.w8, m.w4, m.adapters, m._bank, m.adapter_names = cfg, synth_weights(cfg, seed=0), {}, {}, {}, {}, []
    return m


def test_set_adapter_bank_argument_checks():
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    m = _host_model()
    good = resolve_adapter(m.cfg, *fixture_adapter(m.cfg, "B"))
    key = next(iter(good))
    a, b, s = good[key]
    with pytest.raises(ValueError, match="do not fit"):
        m.set_adapter_bank({"x": {key: (a[:-1], b, s)}})                              # lora_a rows != the projection's input width
    with pytest.raises(ValueError, match="do not fit"):
        m.set_adapter_bank({"x": {key: (a, b[:, :-1], s)}})
    with pytest.raises(ValueError, match="do not fit"):
        m.set_adapter_bank({"x": {key: (a, torch.cat([b, b]), s)}})                   # ranks of lora_a and lora_b disagree
    wide = torch.zeros                                                                  # rank 65 (resolve_adapter itself refuses it: built by hand)
    with pytest.raises(ValueError, match="outside 1..64"):
        m.set_adapter_bank({"x": {key: (wide((a.shape[0], 65)), wide((65, b.shape[1])), 1.0)}})
    with pytest.raises(ValueError, match="not a decoder projection"):
        m.set_adapter_bank({"x": {"lm_head.weight": (a, b, s)}})
    with pytest.raises(ValueError, match="names"):
        m.set_adapter_bank({"": good})
    m.adapters = {key: (a, b, s)}                                                      # a set_adapters adapter is attached
    with pytest.raises(ValueError, match="one or the other"):
        m.set_adapter_bank({"x": good})
    m.adapters, m._bank = {}, {key: (None, 1)}                                          # a bank is attached
    with pytest.raises(ValueError, match="one or the other"):
        m.set_adapters(good)


def test_signatures():
    import phi_3_vision_mlx_amd as pkg
    from phi_3_vision_mlx_amd import api, engine, fleet, server
    assert inspect.signature(api.generate).parameters["adapter"].default is None
    assert inspect.signature(api._generate).parameters["adapter"].default is None
    assert list(inspect.signature(api.load_adapters).parameters)[:2] == ["preload", "adapters"]
    # the package-level generate keeps the reference's exact list (tests/test_host_logic.py pins the same)
    assert list(inspect.signature(pkg.generate).parameters) == [
        "prompt", "images", "preload", "blind_model", "quantize_model", "quantize_cache", "use_adapter", "max_tokens", "verbose",
        "return_tps", "early_stop", "stream", "apply_chat_template", "enable_api"]
    for fn in (engine.ContinuousEngine.submit, engine.RegimeRouter.submit, fleet.EngineFleet.submit):
        assert list(inspect.signature(fn).parameters) == ["self", "inputs", "max_tokens", "sampling", "adapter"]
    for fn in (engine.ContinuousEngine.generate, engine.RegimeRouter.generate, fleet.EngineFleet.generate, server.ContinuousBackend.submit,
               server.EngineQueue.submit):
        assert inspect.signature(fn).parameters["adapter"].default is None
    from phi_3_vision_mlx_amd.model import Phi3VModel
    assert list(inspect.signature(Phi3VModel.set_row_adapters).parameters) == ["self", "st", "adapters", "row0"]
    assert inspect.signature(Phi3VModel.__call__).parameters["row_adapters"].default is None


def test_library_binds_the_gathered_entry_points():
    from phi_3_vision_mlx_amd import _lib
    for name in ("p3v_lora_down_rows", "p3v_lora_up_rows", "p3v_lora_rows_slices"):
        assert name in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.p3v_lora_rows_slices(3072) == 12 and lib.p3v_lora_rows_slices(8192) == 32 and lib.p3v_lora_rows_slices(1) == 1
    assert lib.p3v_lora_down_rows(0, 0, 0.0, 0, 0, 0, 1, 256, 8, 1, 0) == -22          # null pointers: refused before any launch
    assert lib.p3v_lora_up_rows(0, 0, 0, 0, 0, 0, 0, 1, 256, 256, 8, 1, 0) == -22
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p3v.h")).read()
    assert f"#define P3V_LORA_SLICE_K {_lib.LORA_SLICE_K}" in h and "p3v_lora_entry_t" in h


# ------------------------------------------------------------------ engine host logic on a stand-in
class _State:
    def __init__(self, slots, window):
        self.pad_len = torch.full((slots,), window, dtype=torch.int32)
        self.offset, self.T, self.graphs = 0, window, {}


class SlotStub:
    """tests/test_engine_cpu.py's stand-in (each row's tokens are a function of its own prompt, step -- and here its adapter), plus
    a log of set_row_adapters and prefill_slot calls in order."""
    device = "cpu"

    def __init__(self, adapter_names=("A", "B")):
        self.adapter_names = list(adapter_names)
        self.log = []                                           # ("rows", row0, [names]) | ("prefill", row0, n)

    def new_slot_state(self, slots, window):
        st = _State(slots, window)
        st.key, st.step = np.zeros(slots, dtype=np.int64), np.zeros(slots, dtype=np.int64)
        st.adapter = np.full(slots, -1, dtype=np.int64)
        return st

    def decode_graph(self, st):
        g = st.graphs.get("greedy")
        if g is None:
            from phi_3_vision_mlx_amd.model import AttnPlan
            g = st.graphs["greedy"] = {"tok": torch.zeros(len(st.pad_len), dtype=torch.int32), "host_tok": None,
                                       "bufs": {"plan": AttnPlan(ws=torch.full((8,), -1, dtype=torch.int32).view(torch.float32))}}
        return g

    def set_row_adapters(self, st, adapters, row0=0):
        self.log.append(("rows", row0, list(adapters)))
        for i, a in enumerate(adapters):
            st.adapter[row0 + i] = -1 if a is None else self.adapter_names.index(a)

    def _tok(self, st):
        t = (st.key * 31 + st.step * 7919 + (st.adapter + 1) * 101) % 31000 + 3
        return np.where((st.key + st.step) % 29 == 28, EOS, t)

    def prefill_slot(self, st, row, inputs):
        ids = np.asarray(inputs["input_ids"])
        ids = ids[None] if ids.ndim == 1 else ids
        n, S = ids.shape
        m = np.asarray(inputs["mask"]).reshape(n, S) if "mask" in inputs else np.ones_like(ids)
        self.log.append(("prefill", row, n))
        st.key[row:row + n] = (ids * m).sum(1)
        st.step[row:row + n] = 0
        st.pad_len[row:row + n] = torch.as_tensor(st.offset - m.sum(1), dtype=torch.int32)
        return torch.as_tensor(self._tok(st)[row:row + n, None].astype(np.int32))

    def greedy_step(self, token, cache):
        st = cache[0].state
        st.step += 1
        st.offset += 1
        g = self.decode_graph(st)
        g["host_tok"] = torch.as_tensor(self._tok(st).astype(np.int32)[:, None])
        return None, g["host_tok"]


def req(n, seed=0):
    return {"input_ids": np.random.default_rng(seed).integers(3, 600, (1, n)).astype(np.int64)}


def solo(inputs, max_tokens, adapter):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    e = ContinuousEngine(SlotStub(), None, slots=1, window=4096)
    r = e.submit(inputs, max_tokens, adapter=adapter)
    e.run_until_idle()
    assert r.error is None
    return r.tokens


def test_engine_writes_the_rows_adapter_before_its_prefill_and_rewrites_refilled_rows():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    m = SlotStub()
    e = ContinuousEngine(m, None, slots=2, window=4096)
    plan = [(req(40, 1), 3, "A"), (req(38, 2), 9, None), (req(20, 3), 6, "B"), (req(12, 4), 5, None)]
    hs = [e.submit(i, mt, adapter=a) for i, mt, a in plan[:2]]
    e.step(), e.step()
    hs += [e.submit(i, mt, adapter=a) for i, mt, a in plan[2:]]        # refill rows mid-flight
    e.run_until_idle()
    assert all(h.done.is_set() and h.error is None for h in hs)
    for h, (i, mt, a) in zip(hs, plan):
        assert h.adapter == a and h.tokens == solo(i, mt, a)          # each row ran with ITS adapter, whatever its row had before
        if a is not None:
            assert h.tokens != solo(i, mt, None)
    # every prefill is preceded -- immediately -- by the write of exactly its rows
    for k, ev in enumerate(m.log):
        if ev[0] == "prefill":
            prev = m.log[k - 1]
            assert k > 0 and prev[0] == "rows" and prev[1] == ev[1] and len(prev[2]) == ev[2], m.log
    rows = {}
    for ev in m.log:
        if ev[0] == "rows":
            for i, a in enumerate(ev[2]):
                rows.setdefault(ev[1] + i, []).append(a)
    assert sorted(a for h in rows.values() for a in h if a) == ["A", "B"]
    assert any(h[i] is not None and h[i + 1] is None for h in rows.values() for i in range(len(h) - 1)), rows   # refilled row -> -1


def test_unknown_adapter_fails_its_handle_at_once_and_disturbs_nobody():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, RegimeRouter
    m = SlotStub()
    e = ContinuousEngine(m, None, slots=2, window=4096)
    ok = e.submit(req(10, 1), 4, adapter="A")
    for bad_name in ("C", 3, ["A"]):
        bad = e.submit(req(10, 2), 4, adapter=bad_name)
        assert bad.done.is_set() and isinstance(bad.error, ValueError) and "['A', 'B']" in str(bad.error)
    assert list(e.waiting) == [ok]
    e.run_until_idle()
    assert ok.error is None and ok.tokens == solo(req(10, 1), 4, "A") and e.failures == 0
    router = RegimeRouter([e])
    assert router.adapter_names() == ["A", "B"]
    assert isinstance(router.submit(req(10, 2), 4, adapter="C").error, ValueError)
    r = router.submit(req(10, 3), 4, adapter="B")
    e.run_until_idle()
    assert r.error is None and r.tokens == solo(req(10, 3), 4, "B")
    # a model without a bank: plain requests never touch set_row_adapters, a named adapter is refused
    plain = SlotStub(adapter_names=())
    e2 = ContinuousEngine(plain, None, slots=1, window=4096)
    r2 = e2.submit(req(10, 1), 3)
    e2.run_until_idle()
    assert r2.error is None and not any(ev[0] == "rows" for ev in plain.log)
    assert isinstance(e2.submit(req(10, 1), 3, adapter="A").error, ValueError)


def test_fleet_front_checks_the_name_and_passes_it_on():
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    e = ContinuousEngine(SlotStub(), None, slots=1, window=4096)
    front = fleet.EngineFleet(e, (None, None), world=1)
    assert front.adapter_names() == ["A", "B"]
    bad = front.submit(req(10, 1), 3, adapter="C")
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and front.sent == [0]
    h = front.submit(req(10, 1), 3, adapter="B")
    e.run_until_idle()
    assert h.error is None and h.adapter == "B" and h.tokens == solo(req(10, 1), 3, "B")


def _fleet_rank(rank, world, port, out_dir):
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_adapter_bank_cpu import SlotStub as Stub, req as mk, solo as alone
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, Request
    eng = ContinuousEngine(Stub(), None, slots=2, window=4096)  # every rank holds the same bank
    groups = fleet.make_groups()
    if rank:
        fleet.worker(eng, groups)
        open(os.path.join(out_dir, f"worker{rank}"), "w").write("ok")
        dist.destroy_process_group()
        return
    front = fleet.EngineFleet(eng, groups, world)
    front.local = [Request(mk(5, 0), 1) for _ in range(8)]     # rank 0 looks loaded: everything goes to rank 1
    plan = [(mk(20, 1), 5, "A"), (mk(22, 2), 4, None), (mk(18, 3), 6, "B")]
    hs = [front.submit(i, m, adapter=a) for i, m, a in plan]
    assert all(h.rank == 1 for h in hs)
    assert all(h.done.wait(60) for h in hs) and all(h.error is None for h in hs), [h.error for h in hs]
    for h, (i, m, a) in zip(hs, plan):
        assert h.tokens == alone(i, m, a)                       # the remote row ran with the adapter the message named
    bad = front.submit(mk(20, 4), 3, adapter="C")              # refused on rank 0: nothing is sent
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and sum(front.sent) == 3
    front.local = []
    front.close()
    open(os.path.join(out_dir, "front"), "w").write("ok")
    dist.destroy_process_group()


def test_fleet_two_ranks_gloo_carry_the_adapter_name(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_fleet_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "front") and os.path.exists(tmp_path / "worker1")


# ------------------------------------------------------------------ server parsing on a stub generate function
def _call(port, path, payload=None):
    data = None if payload is None else json.dumps(payload).encode()
    r = urllib.request.Request(f"http://127.0.0.1:{port}{path}", data=data, headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(r, timeout=10) as resp:
        return resp.status, json.loads(resp.read())


@pytest.fixture
def adapter_server():
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, sampling=None, adapter=None):
        calls.append((list(prompts), adapter))
        return [f"{p}|{a}" for p, a in zip(prompts, adapter or [None] * len(prompts))]

    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", adapter_names=["A", "B"],
                          sharded_fn=lambda prompts, images: images is not None)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    yield httpd.server_address[1], calls
    httpd.shutdown()
    engine.close()


def test_server_adapter_field(adapter_server):
    port, calls = adapter_server
    assert _call(port, "/v1/adapters") == (200, {"model": "phi-3-vision", "adapters": ["A", "B"]})
    assert _call(port, "/v1/completions", {"prompt": "p", "adapter": "A"})[1]["responses"] == ["p|A"]
    assert _call(port, "/v1/completions", {"prompt": ["p", "q", "r"], "adapter": ["B", None, "A"]})[1]["responses"] == ["p|B", "q|None", "r|A"]
    assert _call(port, "/v1/completions", {"prompt": ["p", "q"], "adapter": "B"})[1]["responses"] == ["p|B", "q|B"]
    assert _call(port, "/v1/completions", {"prompt": "p", "adapter": None})[1]["responses"] == ["p|None"]
    assert _call(port, "/v1/completions", {"prompt": "p"})[1]["responses"] == ["p|None"]
    assert calls[-1] == (["p"], None) and calls[-2] == (["p"], None)         # null / absent: the plain call, no adapter keyword
    for bad in ("C", 7, {"name": "A"}, ["A", "B"], [3], ["A", "C"]):        # unknown, wrong types, wrong count (one prompt)
        with pytest.raises(urllib.error.HTTPError) as e:
            _call(port, "/v1/completions", {"prompt": "p", "adapter": bad})
        assert e.value.code == 400
        assert "known adapters: ['A', 'B']" in json.loads(e.value.read())["error"], bad
    with pytest.raises(urllib.error.HTTPError) as e:                         # two prompts, second name unknown
        _call(port, "/v1/completions", {"prompt": ["p", "q"], "adapter": ["A", "C"]})
    assert e.value.code == 400 and "unknown adapter 'C'" in json.loads(e.value.read())["error"]
    with pytest.raises(urllib.error.HTTPError) as e:                         # the batch-sharded path refuses the field
        _call(port, "/v1/completions", {"prompt": "p", "adapter": "A", "images": ["data:image/png;base64,"]})
    assert e.value.code == 400
    with pytest.raises(urllib.error.HTTPError) as e:
        _call(port, "/v1/other")
    assert e.value.code == 404
    assert _call(port, "/v1/completions", {"prompt": "still alive"})[0] == 200


def test_server_without_a_bank_lists_nothing_and_refuses_names():
    from phi_3_vision_mlx_amd.server import parse_adapter, serve
    httpd, engine = serve(lambda prompts, max_tokens: [p for p in prompts], port=0, host="127.0.0.1")
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        port = httpd.server_address[1]
        assert _call(port, "/v1/adapters")[1]["adapters"] == []
        with pytest.raises(urllib.error.HTTPError) as e:
            _call(port, "/v1/completions", {"prompt": "p", "adapter": "A"})
        assert e.value.code == 400
        assert _call(port, "/v1/completions", {"prompt": "p"})[1]["responses"] == ["p"]
    finally:
        httpd.shutdown()
        engine.close()
    assert parse_adapter({}, 2, ["A"]) is None and parse_adapter({"adapter": [None, None]}, 2, ["A"]) is None
    assert parse_adapter({"adapter": [None, "A"]}, 2, ["A"]) == [None, "A"]


def test_sharded_path_refuses_the_adapter_field(adapter_server):
    """An image request of the queue server runs on the batch-sharded path: the field is refused there, as sampling is."""
    import base64
    from io import BytesIO
    from PIL import Image
    port, _ = adapter_server
    buf = BytesIO()
    Image.new("RGB", (8, 8)).save(buf, format="PNG")
    uri = "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()
    with pytest.raises(urllib.error.HTTPError) as e:
        _call(port, "/v1/completions", {"prompt": "p", "adapter": "A", "images": [uri]})
    assert e.value.code == 400 and "batch-sharded" in json.loads(e.value.read())["error"]


# ------------------------------------------------------------------ the fixture
def test_fixture_witnesses_recomputed_from_its_tokens_and_margins():
    from golden_inputs import SERVE_STEPS
    g = np.load(FIXTURE)
    assert [VARIANTS[i] for i in g["assign"]] == ASSIGN
    assert g["tokens"].shape == g["margins"].shape == (6, 3, SERVE_STEPS)
    assert g["adapter_seeds"].tolist() == [ADAPTER_SPECS["A"]["seed"], ADAPTER_SPECS["B"]["seed"]] == [5, 6]
    assert g["adapter_scales"].tolist() == [3.0, 10.0]
    wit = find_witnesses(g["tokens"], g["margins"])
    assert wit == [tuple(w) for w in g["witnesses"].tolist()] and witnesses_cover(wit)
    for i, a, b, s in wit:                                       # a witness: both runs clear up to the step, tokens differ there
        assert (g["margins"][i, a, :s + 1] > 1.0).all() and (g["margins"][i, b, :s + 1] > 1.0).all()
        assert g["tokens"][i, a, s] != g["tokens"][i, b, s] and a == g["assign"][i] != b
    for i, a in enumerate(g["assign"]):                          # every assigned run is clear on its first step, with some variety
        assert g["margins"][i, a, 0] > 1.0 and len(set(g["tokens"][i, a].tolist())) >= 2
    assert os.path.getsize(FIXTURE) < 16 << 10


def test_fixture_adapters_have_the_stated_shapes():
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    cfg = make_config(tiny_config_dict(vision=False))
    A, B = (resolve_adapter(cfg, *fixture_adapter(cfg, n)) for n in ("A", "B"))
    assert len(A) == 4 * cfg.num_hidden_layers and all(a.shape[1] == 8 for a, _, _ in A.values())
    assert list(B) == [f"model.layers.{cfg.num_hidden_layers - 1}.self_attn.qkv_proj.weight"] and B[list(B)[0]][0].shape[1] == 1
    assert {round(s, 6) for _, _, s in A.values()} == {6.0} and B[list(B)[0]][2] == 20.0      # scale * alpha / rank, alpha = 2 * rank
    c1, t1 = synth_adapter(cfg, ["self_attn.qkv_proj"], 1, 1, 6, 10.0)
    c2, t2 = fixture_adapter(cfg, "B")
    assert c1 == c2 and all(torch.equal(t1[k], t2[k]) for k in t1)
