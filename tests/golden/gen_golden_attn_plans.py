"""Records the decode attention's host side -- the fixture of tests/test_attn_plans_cpu.py (tests/golden/attn_plans.json).  No GPU,
no library: a Phi3VModel shell on `meta` tensors, the ops replaced by stand-ins.

    python tests/golden/gen_golden_attn_plans.py          # rewrites tests/golden/attn_plans.json
    python tests/golden/gen_golden_attn_plans.py --time   # host cost of one Phi3VModel._plan call on the shell below

Two recordings, both through interfaces that did not change when the plan became a record (Phi3VModel._plan, Phi3VModel._layers);
`plan_fields` is the one place that knows where a plan keeps its values.
  "plans"   Phi3VModel._plan(st, B, L, fuse_o=True, captured=True) over STATES x CAN x CUS x BS x LS x TS, then once per entry of
            VARIANTS (a knob, the o_proj weight's format or owner, the layer count, a caller that asks for no fused o_proj) over
            STATES x BS x LS x TS.  Per case: n_split, merge in launch, fuse_o, family, past_lb, the workspace request and whether
            the two all-ones buffers exist.  One symbol per case against the table of distinct outcomes, in `grid()`'s order.
  "layers"  Phi3VModel._layers on a two-layer shell with the projections stubbed, per route: the ops.attention* /
            rope_kv_append / kv_* calls in order, with n_split, merge_in_launch, past, rope_bstride, the tensors that play `out`
            and `o_rearm`, and the o_proj keywords given.
"""
import contextlib
import inspect
import itertools
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "attn_plans.json")
BF16 = torch.bfloat16
NH, HD, H, I, OFFSET = 32, 96, 3072, 8192, 37

STATES = ("bf16", "int8", "mlx4", "family", "slots", "serving")
BS = (1, 2, 8, 16)
LS = (1, 4, 16, 17)
TS = (64, 128, 1024, 1088, 1152, 2048, 2560, 6144, 6208, 8192, 32768)
CAN = ((0, 0), (0, 2), (1, 0), (1, 2))          # what the two can_fuse stand-ins answer (with the merge in the launch, without)
CUS = (256, 64)
KNOBS = ("P3V_ATTN_TILE128", "P3V_ATTN_NSPLIT", "P3V_ATTN_FUSED_MERGE", "P3V_ATTN_FUSE_OPROJ", "P3V_PROFILING")
# name -> (environment, shell keywords, _plan's fuse_o); each runs with CAN (1, 2) on 256 CUs
VARIANTS = {"P3V_ATTN_TILE128=0": ({"P3V_ATTN_TILE128": "0"}, {}, True), "P3V_ATTN_NSPLIT=7": ({"P3V_ATTN_NSPLIT": "7"}, {}, True),
            "P3V_ATTN_FUSED_MERGE=0": ({"P3V_ATTN_FUSED_MERGE": "0"}, {}, True), "P3V_ATTN_FUSED_MERGE=2": ({"P3V_ATTN_FUSED_MERGE": "2"}, {}, True),
            "P3V_ATTN_FUSE_OPROJ=0": ({"P3V_ATTN_FUSE_OPROJ": "0"}, {}, True), "P3V_PROFILING=1": ({"P3V_PROFILING": "1"}, {}, True),
            "o_proj_format_mismatch": ({}, {"mismatch": True}, True), "o_proj_adapter": ({}, {"adapter": True}, True),
            "o_proj_bank": ({}, {"bank": True}, True), "odd_layers": ({}, {"layers": 3}, True), "model_serving": ({}, {"serving": True}, True),
            "no_fused_oproj": ({}, {}, False)}
SYMBOLS = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")


def grid():
    return itertools.product(BS, LS, TS)


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def environ(values):
    """The five knobs as `values` names them, every other one unset."""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def plan_fields(bufs):
    """The plan's values, wherever this tree keeps them: in a record held by the buffers, or in the buffers themselves."""
    get = bufs.get if "plan" not in bufs else lambda k, d=None: getattr(bufs["plan"], k, d)
    out = {k: get(k) for k in ("n_split", "ws", "past_lb", "rope_cos", "rope_sin", "o_f", "o_f2")}
    out.update({k: bool(get(k, False)) for k in ("attn_merge", "fuse_o", "family")})
    return out


# ------------------------------------------------------------------ the shell
def shell(weights="bf16", layers=2, mismatch=False, adapter=False, bank=False, serving=False):
    """A Phi3VModel that was never constructed: the full model's attention shape, o_proj weights in the given format."""
    from phi_3_vision_mlx_amd.model import Phi3VModel

    class Weights(dict):                                         # (a norm weight is only ever handed on)
        def __missing__(self, key):
            return key

    m = Phi3VModel.__new__(Phi3VModel)
    m.cfg = types.SimpleNamespace(num_attention_heads=NH, num_key_value_heads=NH, hidden_size=H, intermediate_size=I, num_hidden_layers=layers,
                                  rms_norm_eps=1e-5)
    m.hd, m.device, m.serving, m.hidden_hook, m.epoch = HD, "meta", serving, None, 0
    m.w, m.w8, m.w4, m.w13, m.adapters, m._bank = Weights(), {}, {}, {}, {}, {}
    if mismatch:
        weights = "bf16" if weights == "fp8" else "fp8"
    for i in range(layers):
        key = f"model.layers.{i}.self_attn.o_proj.weight"
        if weights == "fp8":
            m.w8[key] = (f"w8.{i}", f"w8_scale.{i}")
        elif weights == "q4":
            m.w4[key] = (f"w4.{i}", f"sb.{i}")
        else:
            m.w[key] = f"w.{i}"
    if adapter:
        m.adapters["model.layers.0.self_attn.o_proj.weight"] = "lora"
    if bank:
        m._bank["model.layers.1.self_attn.o_proj.weight"] = "bank"
    m._proj = lambda *a, **kw: None
    m._proj_resid_norm = lambda *a, **kw: False
    m._state_rows = lambda st: torch.empty((st.B,), device="meta")
    return m


def state(kind, B, T):
    st = types.SimpleNamespace(B=B, Tp=T, T=T + 8, offset=OFFSET, quantized=kind == "int8", mlx4=kind == "mlx4", slots=kind == "slots",
                               serving=kind == "serving", family="family" if kind == "family" else None, family_host=None, pad_len=None,
                               fresh_rows=False, mlx4_tokens=0, k_tmp="k_tmp", v_tmp="v_tmp")
    st.cos, st.sin = torch.empty((B, T + 8, HD // 2), device="meta"), torch.empty((B, T + 8, HD // 2), device="meta")
    for name in ("k", "v", "k8", "v8", "ks", "vs"):
        setattr(st, name, [f"{name}.{i}" for i in range(3)])
    return st


def stand_ins(can, cus, ws_log):
    def attention_ws(B, L, nh, hd, n_split, device):
        ws_log.append((B, L, nh, hd, n_split))
        return "ws"

    def can_fuse(B, L, nh, hd, n_split, T, o_n, merge_in_launch):
        return bool(can[0] if merge_in_launch else can[1])

    return dict(attention_ws=attention_ws, attention_decode_can_fuse_oproj=can_fuse, attention_decode_q8_can_fuse_oproj=can_fuse,
                device_props=lambda device=0: {"cu_count": cus})


# ------------------------------------------------------------------ recording "plans"
def plan_case(m, kind, B, L, T, fuse_o, ws_log):
    del ws_log[:]
    f = plan_fields(m._plan(state(kind, B, T), B, L, fuse_o, captured=True))
    assert (f["o_f"] is None) == (f["o_f2"] is None) == (not f["fuse_o"]) and len(ws_log) <= 1
    ws = None if not ws_log else "B,L" if ws_log[0] == (B, L, NH, HD, f["n_split"]) else "B,1" if ws_log[0] == (B, 1, NH, HD, f["n_split"]) \
        else list(ws_log[0])
    assert (f["ws"] is None) == (ws is None) and f["rope_cos"].shape == f["rope_sin"].shape == (B, L, HD // 2)
    return json.dumps([f["n_split"], int(f["attn_merge"]), int(f["fuse_o"]), int(f["family"]), f["past_lb"], ws, int(f["o_f"] is not None)],
                      separators=(",", ":"))


def record_plans():
    from phi_3_vision_mlx_amd import ops
    table, cases, ws_log = [], {}, []

    def run(kind, can, cus, env, kw, fuse_o):
        m = shell("fp8" if kind == "int8" else "bf16", **kw)
        out = []
        with patched(ops, **stand_ins(can, cus, ws_log)), environ(env):
            for B, L, T in grid():
                outcome = plan_case(m, kind, B, L, T, fuse_o, ws_log)
                if outcome not in table:
                    table.append(outcome)
                out.append(table.index(outcome))
        return out

    for kind, can, cus in itertools.product(STATES, CAN, CUS):
        cases[f"{kind},can={can[0]}{can[1]},cus={cus}"] = run(kind, can, cus, {}, {}, True)
    for name, (env, kw, fuse_o) in VARIANTS.items():
        for kind in STATES:
            cases[f"{kind},{name}"] = run(kind, (1, 2), 256, env, kw, fuse_o)
    width = 1 if len(table) <= len(SYMBOLS) else 2
    sym = [SYMBOLS[i] if width == 1 else SYMBOLS[i // len(SYMBOLS)] + SYMBOLS[i % len(SYMBOLS)] for i in range(len(table))]
    return {"axes": {"state": STATES, "B": BS, "L": LS, "T": TS, "can_fuse": ["%d%d" % c for c in CAN], "cu_count": CUS, "variant": list(VARIANTS)},
            "outcome": ["n_split", "merge_in_launch", "fuse_o", "family", "past_lb", "ws_request", "all_ones_buffers"], "width": width,
            "outcomes": dict(zip(sym, table)), "cases": {k: "".join(sym[i] for i in v) for k, v in cases.items()}}


def time_plan(repeats=5, calls=2000):
    """Median (and min .. max) over `repeats` timings of one _plan call, in microseconds."""
    from phi_3_vision_mlx_amd import ops
    out = {}
    with patched(ops, **stand_ins((1, 2), 256, [])), environ({}):
        for name, kind, B, captured in (("eager B=L=1", "bf16", 1, False), ("captured B=1", "bf16", 1, True), ("captured B=16", "bf16", 16, True),
                                        ("family B=8", "family", 8, True)):
            m, st = shell(), state(kind, B, 2560)
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    m._plan(st, B, 1, True, captured=captured)
                times.append((time.perf_counter() - t0) / calls * 1e6)
            out[name] = (statistics.median(times), min(times), max(times))
    return out


# ------------------------------------------------------------------ recording "layers"
LOGGED = ("attention", "rope_kv_append", "kv_")
# route -> (weights, state kind, B, L, n_beam, T, can_fuse answers)
ROUTES = {"bf16": ("bf16", "bf16", 1, 1, 1, 2048, (0, 0)), "bf16,B=2,L=4": ("bf16", "bf16", 2, 4, 1, 2048, (1, 2)),
          "bf16,fused_in_launch": ("bf16", "bf16", 1, 1, 1, 2048, (1, 2)), "bf16,fused_in_merge": ("bf16", "bf16", 1, 1, 1, 128, (0, 2)),
          "q4,fused_in_launch": ("q4", "bf16", 1, 1, 1, 2048, (1, 2)), "q8": ("fp8", "int8", 1, 1, 1, 2048, (0, 0)),
          "q8,fused_in_launch": ("fp8", "int8", 1, 1, 1, 2048, (1, 2)), "q8,fused_in_merge": ("fp8", "int8", 1, 1, 1, 8192, (0, 2)),
          "family": ("bf16", "family", 2, 1, 1, 2048, (1, 2)), "beams": ("bf16", "bf16", 2, 1, 2, 2048, (1, 2)),
          "prefill": ("bf16", "bf16", 1, 17, 1, 2048, (1, 2)), "q8,prefill": ("fp8", "int8", 1, 17, 1, 2048, (1, 2))}


def layers_case(ops, weights, kind, B, L, n_beam, T, can, replay):
    m, st, calls, plans, roles = shell(weights), state(kind, B, T), [], [], {}

    def role(t):
        return t if isinstance(t, str) or t is None else roles.get(id(t), "?")

    def logger(name, fn):
        sig = inspect.signature(fn)

        def f(*a, **kw):
            b = sig.bind(*a, **kw).arguments
            rec = {"op": name}
            rec.update({k: b[k] for k in ("n_split", "merge_in_launch", "past", "rope_bstride") if k in b})
            rec.update({k: role(b[k]) for k in ("out", "o_rearm", "ws") if k in b})
            if o_kw := sorted(k for k in b if k.startswith("o_proj")):
                rec["o_proj"] = o_kw
            calls.append(rec)
        return f

    def note(bufs):
        plans.append(bufs)
        f = plan_fields(bufs)
        roles.update({id(bufs["o"]): "o", id(f["o_f"]): "o_f", id(f["o_f2"]): "o_f2"})
        return bufs

    fixed = stand_ins(can, 256, [])
    logged = {n: logger(n, getattr(ops, n)) for n in dir(ops) if n.startswith(LOGGED) and n not in fixed and
              n not in ("attention_ws_bytes", "attention_family_chunk") and inspect.isfunction(getattr(ops, n))}
    plan = m._plan
    m._plan = lambda *a, **kw: note(plan(*a, **kw))
    x = torch.empty((B * L, H), dtype=BF16, device="meta")
    with patched(ops, **fixed, **logged), environ({}):
        if replay:
            m._layers(x, st, B, L, 0, n_beam, bufs=m._plan(st, B, L, True, captured=True), d_past="d_past")
        else:
            m._layers(x, st, B, L, OFFSET, n_beam)
    f = plan_fields(plans[0])
    return {"plan": [f["n_split"], int(f["attn_merge"]), int(f["fuse_o"]), int(f["family"])], "calls": calls}


def record_layers():
    from phi_3_vision_mlx_amd import ops
    out = {}
    for name, (weights, kind, B, L, n_beam, T, can) in ROUTES.items():
        out[f"{name},eager"] = layers_case(ops, weights, kind, B, L, n_beam, T, can, False)
        if L <= ops.L.DECODE_MAX_L and n_beam == 1:
            out[f"{name},d_past"] = layers_case(ops, weights, kind, B, L, n_beam, T, can, True)
    return out


def record_all():
    return {"plans": record_plans(), "layers": record_layers()}


def dumps(rec):
    """One case per line: compact, and a change shows up as the lines of the cases it touches."""
    lines = []
    for part, groups in rec.items():
        for group, value in groups.items():
            if isinstance(value, dict) and group in ("outcomes", "cases"):
                lines += [json.dumps([part, group, k, v], separators=(",", ":")) for k, v in value.items()]
            else:
                lines.append(json.dumps([part, group, value], separators=(",", ":")))
    return "[\n" + ",\n".join(lines) + "\n]\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--time" in sys.argv:
        for case, (med, lo, hi) in time_plan().items():
            print(f"{case:14s} median {med:7.2f} us  (min {lo:7.2f}, max {hi:7.2f})")
        sys.exit(0)
    text = dumps(record_all())
    with open(PATH, "w") as f:
        f.write(text)
    print(f"wrote {PATH}: {len(text)} bytes")
