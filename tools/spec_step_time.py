"""Cost of a speculative verify step against the plain captured step, full-size synthetic bf16 model, one process.

Per context length: the plain captured greedy step (median over replays), then the verify step for K draft rows with FORCED
drafts that the model accepts 0, K // 2 or K of, and with the device's own drafter; every replay timed on its own between two
events (the host writes forced drafts before the first event).  For this table the final norm's weight is zeroed in place, so
every arg-max is token 0 and the acceptance can be forced exactly (main() says why); launches, shapes and bytes are unchanged.  Per cell: step time, its ratio to the plain step, the break-even acceptance (ratio - 1 extra tokens per step) and the
acceptance the replays really had.  Then one end-to-end row: tokens/s of generate(speculate=K) against speculate=0 on a prompt
whose continuation repeats, with the acceptance it reached (random weights: that acceptance says nothing about a checkpoint).

    python tools/spec_step_time.py [--ctx 128,2531,32768] [--ks 2,4,7,15] [--steps 20] [--note TEXT]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phi_3_vision_mlx_amd import api, ops  # noqa: E402

PROMPT = "Repeat the list: shelf one holds maps, shelf two holds maps, shelf three holds maps, shelf four holds maps."


def plain_steps(model, tok, cache, n):
    """n replays of the plain step, each timed on its own: (median us, tokens)."""
    times, toks = [], []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, tok = model.greedy_step(tok, cache)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
        toks.append(int(tok.reshape(-1)[0]))
    return statistics.median(times), toks


def verify_cell(model, cache, ids, first, K, want, steps):
    """`steps` verify replays from the prompt's end: (median us, mean accepted, replays).  The model answers 0 to everything
    (see main), so forced drafts of `want` zeros and K - `want` ones are accepted `want` at a time; want=None: the device's own
    prompt-lookup drafter (on a run of equal tokens its most recent match overlaps the suffix: one-token drafts)."""
    st = cache[0].state
    st.offset = len(ids)
    g = model.spec_start(cache, ids, torch.tensor([[first]], dtype=torch.int32), K, forced=want is not None)
    times, acc = [], []
    for _ in range(steps + 3):
        if want is not None:
            model.spec_force(cache, [0] * want + [1] * (K - want))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.spec_step(cache, K)
        b.record()
        b.synchronize()
        toks = model.spec_sync(cache)
        assert not any(toks), "the zeroed final norm must make every token 0"
        times.append(a.elapsed_time(b) * 1e3)
        acc.append(int(g["rec"][g["n_replays"] - 1, 0]) - 1)
    times, acc = times[3:], acc[3:]                                   # (the first replays warm the graph)
    return statistics.median(times), sum(acc) / len(acc), len(times)


class _Count:
    """Counts the library's kernel launches by name while it stands in for the loaded library."""

    def __init__(self):
        from phi_3_vision_mlx_amd import _lib
        self._lib, self.real, self.n = _lib, _lib.lib(), {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name.startswith(("p3v_graph", "p3v_event")) or name.endswith(("_bytes", "_slices", "_role", "_can_fuse_oproj", "_props", "_tuning")):
            return fn

        def counted(*a):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a)
        return counted

    def __enter__(self):
        self._lib._lib = self
        return self

    def __exit__(self, *a):
        self._lib._lib = self.real


def launches(model, cache, ids, first, K):
    """Library calls of ONE verify step (run eagerly: the same launches the capture holds), by entry point."""
    cache[0].state.offset = len(ids)
    model.spec_start(cache, ids, torch.tensor([[first]], dtype=torch.int32), K, forced=True)
    with _Count() as c:
        model.spec_step(cache, K, eager=True)
    model.spec_sync(cache)
    return c.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", default="128,2531,32768")
    ap.add_argument("--ks", default="2,4,7,15")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--e2e-tokens", type=int, default=256)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    model, proc = api.load_synthetic(device="cuda:0", lm_head_spread=4.0)
    p = ops.device_props(0)
    print(f"# speculative verify step vs plain captured step; full-size synthetic bf16 model, bf16 KV cache, B = 1")
    print(f"# {a.note}")
    print(f"# device {p['arch']}, {p['cu_count']} CUs, engine clock limit {p['clock_khz'] // 1000} MHz, memory clock {p['mem_clock_khz'] // 1000} MHz; "
          f"every replay timed between two events, medians over {a.steps} replays after 3 warm-up replays")
    print(f"# {'keys':>6} {'K':>3} {'forced acc':>10} {'real acc':>8} {'step us':>9} {'ratio':>6} {'break-even':>10} {'replays':>7}")
    # The random full-size model's logits are near-ties, so a verify step (L rows) and the plain step need not agree on a token
    # and no draft could be forced to a wanted acceptance.  For the step-time table the final norm's weight is zeroed IN PLACE:
    # every logit is 0, every arg-max is token 0 on both paths, and the launches, shapes and bytes of a step are unchanged.
    norm_w = model.w["model.norm.weight"]
    saved = norm_w.clone()
    norm_w.zero_()
    budget = (a.steps + 4) * (max(ks) + 1) + 8
    for ctx in [int(c) for c in a.ctx.split(",")]:
        ids = torch.randint(3, 32000, (1, ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(ctx)).numpy().astype(np.int32)
        logits, cache = model(input_ids=ids, max_tokens=budget, extra_tokens=max(ks))
        tok = ops.argmax(logits[:, -1].contiguous())[:, None]
        first = int(tok[0, 0])
        plain_steps(model, tok, cache, 8)                             # capture + warm the plain graph
        cache[0].state.offset = ctx
        t_plain, toks = plain_steps(model, torch.tensor([[first]], dtype=torch.int32, device="cuda:0"), cache, a.steps + 3)
        assert first == 0 and not any(toks)
        print(f"  {ctx:>6} {'-':>3} {'plain':>10} {'-':>8} {t_plain:9.1f} {1.0:6.3f} {'-':>10} {a.steps + 3:>7}", flush=True)
        for K in ks:
            if K == 4:
                n = launches(model, cache, ids.reshape(-1), first, K)
                print(f"# {ctx} keys, K = 4: {sum(n.values())} library calls per verify step: "
                      + ", ".join(f"{v} {k[4:]}" for k, v in sorted(n.items())), flush=True)
            for want in sorted({0, K // 2, K}) + [None]:
                t, acc, n = verify_cell(model, cache, ids.reshape(-1), first, K, want, a.steps)
                print(f"  {ctx:>6} {K:>3} {'drafter' if want is None else want:>10} {acc:8.2f} {t:9.1f} {t / t_plain:6.3f} "
                      f"{t / t_plain - 1:10.3f} {n:>7}", flush=True)
        del logits, cache
        torch.cuda.empty_cache()
    norm_w.copy_(saved)
    # end to end: a prompt whose continuation repeats (the fixture's recipe at full size)
    print("# end to end, generate() on the repeated-list prompt (random weights: the acceptance says nothing about real checkpoints)")
    prompt, _ = api._apply_chat_template(PROMPT, None, False)
    kw = dict(max_tokens=a.e2e_tokens, verbose=False, stream=False, mute=True, return_tps=True)
    for K in (0, 4, 0, 4):
        info = {}
        _, tps = api._generate(model, proc, prompt, speculate=K, spec_info=info, **kw)
        extra = (f"  {info['steps']} verify steps, {info['accepted']} of {info['drafted']} drafts accepted, "
                 f"{info['emitted'] / max(info['steps'], 1):.2f} tokens per step") if K else ""
        print(f"  speculate={K}: {tps:8.1f} tokens/s over {a.e2e_tokens} tokens{extra}", flush=True)


if __name__ == "__main__":
    main()
