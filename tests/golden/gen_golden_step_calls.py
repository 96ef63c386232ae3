"""Records every call the decode-step callers make on the model, for all 16 combinations of a request's step options -- the
fixture of tests/test_step_calls_cpu.py (tests/golden/step_calls.json).  No GPU, no real model: a stub logs each call's name, its
row range, the shapes and small plain values of its arguments, which keywords were present and the counter `sampling.pack` was
given; never a tensor's contents.

    python tests/golden/gen_golden_step_calls.py        # rewrites tests/golden/step_calls.json

Three recordings:
  "engine"  ContinuousEngine, a request with each combination of {sampling, penalties (with a logit_bias), guide, logprobs} in six
            situations: alone in one slot, in a group of two beside a plain request, as a family of three, followed in its slot by
            a plain request, with `prefill_slot` raising for the group, with `prefill_slot` raising for the family.  Per situation
            the ordered model calls, the step methods taken until idle and how each request ended.
  "loop"    api.greedy_loop on CPU tensors (the one-sync-per-token path), the same combinations, four steps each.
  "generate" api._generate around that loop, the same combinations, each as one prompt, as two prompts and as n = 3 completions of
            one prompt: the prefill call, the fork, the setters and the first token's draw and record.  `api.model_ops` is replaced
            by a logging stub for the run (its kernels refuse CPU tensors); its calls are logged as `model_ops.name(...)`.
Sampling always carries a seed, so nothing is random.
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "step_calls.json")
EOS = 32007
VOCAB = 32064
OPTIONS = ("sampling", "penalties", "guide", "logprobs")
COMBOS = [c for k in range(len(OPTIONS) + 1) for c in itertools.combinations(OPTIONS, k)]
SITUATIONS = ("alone", "group", "family", "refill", "group_raises", "family_raises")
STEPS = ("greedy_step", "sample_step", "logprob_step", "sample_logprob_step", "penal_step", "penal_logprob_step", "guide_step",
         "guide_logprob_step")


def plain(v):
    """A logged value: small plain data as it is, a tensor or an array as its shape, a guide as its pattern."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, slice):
        return f"{v.start}:{v.stop}"
    if torch.is_tensor(v):
        return "T" + "x".join(map(str, v.shape))
    if isinstance(v, np.ndarray):
        return "A" + "x".join(map(str, v.shape))
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in sorted(v.items())}
    if hasattr(v, "pattern") and hasattr(v, "delta"):
        return "dfa:" + str(v.pattern)
    return type(v).__name__


class State:
    def __init__(self, slots, window):
        self.B = slots
        self.pad_len = torch.full((slots,), window, dtype=torch.int32)
        self.offset, self.T, self.graphs = 0, window, {}
        self.sample_rows = self.penalty = self.guide = self.logprob_want = None


class Recorder:
    """The model interface the engine and the loop drive, every call logged as one compact string `name(arg=value,..|keywords)`;
    the first argument (the state) is not logged."""
    device = "cpu"
    cfg = type("Cfg", (), {"vocab_size": VOCAB})()

    def __init__(self, raises=None):
        self.log, self.steps = [], []
        self.raises = raises                                      # "group": prefill_slot raises for n > 1; "all": always

    def __call__(self, **kw):
        """The prefill of `_generate`: zero logits of the last position and a one-layer cache over a new State."""
        self._note("model", (), (), kw)
        B, S = np.asarray(kw["input_ids"]).shape
        return torch.zeros((B, 1, VOCAB)), [type("L", (), {"state": State(B, S + kw["max_tokens"])})()]

    def fork_state(self, st, *a, **kw):
        self._note("fork_state", ("n",), a, kw)
        return [type("L", (), {"state": State(a[0], st.T)})()]

    def set_row_adapters(self, st, *a, **kw):
        self._note("set_row_adapters", ("names", "row0"), a, kw)

    def _note(self, name, names, args, kw, **extra):
        vals = dict(zip(names, args))
        vals.update(kw)
        vals.update(extra)
        body = ",".join(f"{k}={json.dumps(plain(v), separators=(',', ':'))}" for k, v in vals.items())
        self.log.append(f"{name}({body}|{len(args)}|{','.join(sorted(kw))})")

    # ---- states and captures
    def new_slot_state(self, slots, window):
        self.log.append(f"new_slot_state({slots},{window})")
        return State(slots, window)

    def decode_graph(self, st):
        self.log.append("decode_graph()")
        return self._g(st)

    def _g(self, st):
        from phi_3_vision_mlx_amd import logprobs
        return st.graphs.setdefault("greedy", {"tok": torch.zeros(st.B, dtype=torch.int32), "host_tok": None, "n_replays": 0,
                                               "history": torch.zeros((st.B, 2), dtype=torch.int32), "bufs": {},   # (two slots: a third scored step restarts)
                                               "records": torch.zeros((st.B, 4, logprobs.RECORD_WORDS), dtype=torch.int32)})

    def restart_history(self, st):
        self.log.append("restart_history()")
        self._g(st)["n_replays"] = 0

    # ---- setters
    def set_sampling(self, st, *a, **kw):
        from phi_3_vision_mlx_amd import sampling
        records = a[0] if a else kw["records"]
        recs = sampling.unpack(records)
        st.sample_rows = True
        self._note("set_sampling", ("records", "row0"), a, kw, counter=[r["counter"] for r in recs],
                   greedy=[r["temperature"] == 0.0 for r in recs])

    def set_penalties(self, st, *a, **kw):
        from phi_3_vision_mlx_amd import penalties
        st.penalty = True
        self._note("set_penalties", ("records", "prompt_ids", "row0"), a, kw, flags=[r["flags"] for r in penalties.unpack(a[0])])

    def rebuild_penalties(self, st, *a, **kw):
        self._note("rebuild_penalties", ("prompt_ids", "emitted", "row0", "pad"), a, kw)

    def clear_penalties(self, st, *a, **kw):
        self._note("clear_penalties", ("row0", "n"), a, kw)

    def set_guide_vocab(self, *a, **kw):
        self._note("set_guide_vocab", ("table", "eos"), a, kw, n=a[0].n)

    def set_guides(self, st, *a, **kw):
        st.guide = True
        self._note("set_guides", ("guides", "row0"), a, kw)

    def clear_guides(self, st, *a, **kw):
        self._note("clear_guides", ("row0", "n"), a, kw)

    def set_logprobs(self, st, *a, **kw):
        st.logprob_want = True
        self._note("set_logprobs", ("wants", "row0"), a, kw)

    # ---- eager pieces of a prefill
    def prefill_slot(self, st, *a, **kw):
        self._note("prefill_slot", ("row", "inputs"), (a[0], np.asarray(a[1]["input_ids"])) + a[2:], kw)
        ids = np.asarray(a[1]["input_ids"])
        n = 1 if ids.ndim == 1 else ids.shape[0]
        if self.raises == "all" or (self.raises == "group" and n > 1):
            raise RuntimeError("stub: prefill failed")
        toks = torch.arange(100 + a[0], 100 + a[0] + n, dtype=torch.int32)[:, None]
        return (toks, torch.zeros((n, 1, 8))) if kw.get("return_logits") else toks

    def fork_rows(self, st, *a, **kw):
        self._note("fork_rows", ("src_row", "dst_rows"), a, kw)

    def penalized_logits(self, st, *a, **kw):
        self._note("penalized_logits", ("logits", "row0"), a, kw)
        return a[0]

    def guided_logits(self, st, *a, **kw):
        self._note("guided_logits", ("logits", "row0"), a, kw)
        return a[0]

    def sample_logits(self, st, *a, **kw):
        self._note("sample_logits", ("logits", "row0"), a, kw)
        row0 = a[1] if len(a) > 1 else kw.get("row0", 0)
        return torch.arange(200 + row0, 200 + row0 + a[0].shape[0], dtype=torch.int32)[:, None]

    def logprobs_of(self, st, *a, **kw):
        from phi_3_vision_mlx_amd import logprobs
        self._note("logprobs_of", ("logits", "tokens", "row0"), a, kw)
        return torch.zeros((a[0].shape[0], logprobs.RECORD_WORDS), dtype=torch.int32)

    # ---- the eight steps
    def _step(self, name, token, cache):
        st = cache[0].state
        g = self._g(st)
        self.log.append(f"{name}({plain(token)},{'host_tok' if token is g['host_tok'] else 'other'})")
        self.steps.append(name)
        st.offset += 1
        g["n_replays"] += 1
        g["host_tok"] = torch.arange(300, 300 + st.B, dtype=torch.int32)[:, None]
        return torch.zeros((st.B, 1, 8)), g["host_tok"]


for _name in STEPS:
    setattr(Recorder, _name, (lambda name: lambda self, token, cache: self._step(name, token, cache))(_name))


def _ids(n, seed):
    return {"input_ids": np.random.default_rng(seed).integers(3, 600, (1, n)).astype(np.int64)}


def _request(engine_mod, combo, seed, n=None):
    """-> (inputs with the combination's carriers, submit keywords)"""
    inputs = _ids(12, seed)
    if "penalties" in combo:
        inputs = engine_mod.penalty_args(inputs, repetition_penalty=1.3, logit_bias={"5": -2.0})
    if "guide" in combo:
        inputs = engine_mod.guide_args(inputs, regex="[0-9]+")
    if "logprobs" in combo:
        inputs = engine_mod.logprob_args(inputs, 2)
    if n is not None:
        inputs = engine_mod.n_args(inputs, n)
    return inputs, ({"sampling": {"temperature": 0.7, "top_k": 5, "seed": 11}} if "sampling" in combo else {})


def record_engine():
    from phi_3_vision_mlx_amd import engine as E
    from phi_3_vision_mlx_amd.processor import ByteTokenizer
    proc = type("Proc", (), {"tokenizer": ByteTokenizer()})()
    out = {}
    for combo in COMBOS:
        for situation in SITUATIONS:
            m = Recorder({"group_raises": "group", "family_raises": "all"}.get(situation))
            slots = {"alone": 1, "refill": 1, "group": 2, "group_raises": 2}.get(situation, 3)
            e = E.ContinuousEngine(m, proc, slots=slots, window=4096)
            inputs, kw = _request(E, combo, 1, n=3 if situation.startswith("family") else None)
            reqs = [e.submit(inputs, 4, **kw)]
            if situation in ("group", "group_raises", "refill"):
                reqs.append(e.submit(_ids(12, 2), 6))             # the plain neighbour (group) or successor (refill)
            e.run_until_idle(max_steps=64)
            ends = [[len(x.tokens), None if x.error is None else type(x.error).__name__, len(x.logprob_records)]
                    for r in reqs for x in r.members]
            out.setdefault("+".join(combo) or "plain", {})[situation] = {"calls": m.log, "steps": m.steps, "ends": ends}
    return out


def record_loop():
    from phi_3_vision_mlx_amd import api, guide, logprobs, sampling
    from phi_3_vision_mlx_amd.processor import ByteTokenizer
    table = guide.vocab_for(ByteTokenizer(), VOCAB)
    out = {}
    for combo in COMBOS:
        m = Recorder()
        st = m.new_slot_state(2, 64)
        cache = [type("L", (), {"state": st})()]
        kw, streamed = {}, []
        if "sampling" in combo:
            kw["sampling"] = sampling.rows(2, 0.7, 5, 1.0, 11)
        if "logprobs" in combo:
            kw["logprobs"] = logprobs.Collector([2, logprobs.OFF])
        if "penalties" in combo:
            kw["penalties"] = dict(prompt_ids=np.zeros((2, 5), dtype=np.int64), pad=None)
        if "guide" in combo:
            kw["guides"] = dict(dfas=[guide.compile_regex("[0-9]+"), None], table=table, eos=EOS)
        token = api.greedy_loop(m, torch.tensor([[7], [8]], dtype=torch.int32), cache, 4, lambda rows: streamed.append(len(rows)),
                                lambda rows: False, **kw)
        out["+".join(combo) or "plain"] = {"calls": m.log, "steps": m.steps, "streamed": streamed, "returned": plain(token),
                                           "collected": [len(r) for r in kw["logprobs"].rows] if "logprobs" in kw else None}
    return {"cpu": out}


class OpsLog:
    """Stands in for `api.model_ops` while `_generate` runs on the Recorder: the three launches it makes itself, logged."""

    def __init__(self, m):
        self.m = m

    def argmax(self, *a, **kw):
        self.m._note("model_ops.argmax", ("logits",), a, kw)
        return torch.arange(400, 400 + a[0].shape[0], dtype=torch.int32)

    def sample(self, *a, **kw):
        from phi_3_vision_mlx_amd import sampling
        recs = sampling.unpack(a[1])
        self.m._note("model_ops.sample", ("logits", "records"), a, kw, counter=[r["counter"] for r in recs],
                     greedy=[r["temperature"] == 0.0 for r in recs])
        return torch.arange(500, 500 + a[0].shape[0], dtype=torch.int32)

    def logprobs(self, *a, **kw):
        from phi_3_vision_mlx_amd import logprobs
        self.m._note("model_ops.logprobs", ("logits", "tokens", "wants"), a, kw, want=a[2].tolist())
        return torch.zeros((a[0].shape[0], logprobs.RECORD_WORDS), dtype=torch.int32)


def record_generate():
    from phi_3_vision_mlx_amd import api, row_options
    from phi_3_vision_mlx_amd.processor import ByteTokenizer, Phi3FProcessor
    proc = Phi3FProcessor(tokenizer=ByteTokenizer())
    shapes = {"one": ("a prompt", {}), "two": (["a prompt", "another, longer"], {}), "n3": ("a prompt", {"n": 3})}
    out, real_ops = {}, api.model_ops
    for combo in COMBOS:
        kw = {}
        if "sampling" in combo:
            kw.update(temperature=0.7, top_k=5, seed=11)
        if "penalties" in combo:
            kw.update(repetition_penalty=1.3, logit_bias={"5": -2.0})
        if "guide" in combo:
            kw.update(guided_regex="[0-9]+")
        if "logprobs" in combo:
            kw.update(logprobs=2)
        for shape, (prompt, kw_shape) in shapes.items():
            m, info = Recorder(), {}
            api.model_ops = row_options.model_ops = OpsLog(m)
            try:
                result = api._generate(m, proc, prompt, max_tokens=5, verbose=False, mute=True, logprob_info=info, **kw, **kw_shape)
            finally:
                api.model_ops = row_options.model_ops = real_ops
            out.setdefault("+".join(combo) or "plain", {})[shape] = {
                "calls": m.log, "steps": m.steps, "results": len(result) if isinstance(result, list) else 1,
                "collected": [None if t is None else len(t) for t in info["token_ids"]] if info else None}
    return out


def record_all():
    return {"engine": record_engine(), "loop": record_loop(), "generate": record_generate()}


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
    text = dumps(record_all())
    with open(PATH, "w") as f:
        f.write(text)
    print(f"wrote {PATH}: {len(text)} bytes")
