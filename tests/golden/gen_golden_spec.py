"""Generator of tests/golden/tiny_spec_oracle.npz: the speculative-decoding fixture on the tiny TEXT model, from the CPU oracle.

One prompt with repeated phrases (chat-templated, `Phi3VProcessor(None)`), `synth_weights(cfg, seed=0, std_scale=4.0)`, STEPS
greedy steps of the oracle under a searched decisive lm_head.  The generator walks head seeds upwards and keeps the first one with
  * the first NEED_CLEAR steps all clear (margins > 1: the project's clearance rule at REL_TOL), and
  * at least MIN_DISTINCT distinct tokens in the run, and
  * under speculate.propose / accept with K = 4 simulated on the oracle's OWN tokens (prompt ids + tokens as the context):
    at least MIN_ACCEPTED accepted drafts and at least MIN_REJECT steps in which a non-empty draft is rejected at its first
    token or later -- both branches of the rule get exercised.
Stored: head seed, spread, rel_tol, ids, tokens [1, STEPS], margins [1, STEPS], the simulated statistics (`sim`: steps, drafted,
accepted, rejecting steps) and the first unclear step.  Tests compare tokens up to the run's first unclear step (>= NEED_CLEAR
by construction).  Regenerating reproduces the file byte for byte:

    python tests/golden/gen_golden_spec.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "tiny_spec_oracle.npz")
STEPS = 48
NEED_CLEAR = 24
MIN_DISTINCT = 4
SIM_K = 4
MIN_ACCEPTED = 8
MIN_REJECT = 8
MAX_SEEDS = 20000
PROMPT = "Repeat the list: shelf one holds maps, shelf two holds maps, shelf three holds maps, shelf four holds maps."


def chat_text():
    return f"<|user|>\n{PROMPT.strip()}<|end|>\n<|assistant|>\n"


def simulate(ids, tokens, K, vocab):
    """The verify steps of a run whose model answers with `tokens` (tokens[0] = the prefill token): (steps, drafted, accepted,
    steps that rejected part of a non-empty draft).  A run is cut at the end of `tokens`."""
    from phi_3_vision_mlx_amd import speculate
    ctx = [int(t) for t in ids] + [int(tokens[0])]
    i, steps, drafted, accepted, rejecting = 1, 0, 0, 0, 0
    while i < len(tokens):
        d = speculate.propose(ctx, K, vocab=vocab)
        amax = [int(t) for t in tokens[i:i + len(d) + 1]]
        d = d[:max(len(amax) - 1, 0)]                              # (the last rows of the run: no arg-max to check them against)
        acc, out = speculate.accept(d, amax)
        steps, drafted, accepted = steps + 1, drafted + len(d), accepted + acc
        rejecting += int(len(d) > 0 and acc < len(d))
        ctx += out
        i += len(out)
    return steps, drafted, accepted, rejecting


def main():
    import torch
    import phi3v_oracle as orc
    from gen_golden_oracle import COMMON, REL_TOL, SPREAD, Prefilled, clearance, row_norms
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.processor import Phi3VProcessor
    from phi_3_vision_mlx_amd.weights import peaked_lm_head, synth_weights
    cfg = make_config(tiny_config_dict(vision=False))
    w = synth_weights(cfg, seed=0, std_scale=4.0)
    base = w["lm_head.weight"].to(torch.float32)
    o = orc.OraclePhi3V(cfg, w, cache_fp32=True)
    inp = Phi3VProcessor(None)(chat_text())
    run = Prefilled(o, dict(inp), STEPS)
    ids = np.asarray(inp["input_ids"]).reshape(-1).astype(np.int32)
    for hs in range(MAX_SEEDS):
        head = peaked_lm_head(base, SPREAD, hs)
        norms = row_norms(head)
        if clearance(orc._linear(run.h0, head)[:, -1], norms, REL_TOL).min().item() <= 1.0:
            continue
        if run.greedy(head, 6, need_clear_steps=6, norms=norms) is None:       # cheap filter: six clear steps
            continue
        res = run.greedy(head, STEPS, need_clear_steps=NEED_CLEAR, norms=norms)
        if res is None:
            continue
        toks, _, mgs = res
        t = toks.reshape(-1).tolist()
        sim = simulate(ids, t, SIM_K, cfg.vocab_size)
        unclear = [i for i, m in enumerate(mgs.reshape(-1).tolist()) if m <= 1.0]
        first_unclear = unclear[0] if unclear else STEPS
        print(f"  head seed {hs}: first unclear step {first_unclear}, {len(set(t))} distinct, simulated (steps, drafted, accepted, "
              f"rejecting) = {sim}", flush=True)
        if len(set(t)) >= MIN_DISTINCT and sim[2] >= MIN_ACCEPTED and sim[3] >= MIN_REJECT:
            break
    else:
        raise RuntimeError("no lm_head seed found")
    out = dict(COMMON, head_seed=np.asarray([hs], dtype=np.int32), ids=ids, tokens=toks.numpy().astype(np.int32),
               margins=mgs.numpy().astype(np.float32), sim=np.asarray(sim, dtype=np.int32), sim_k=np.asarray([SIM_K], dtype=np.int32),
               first_unclear=np.asarray([first_unclear], dtype=np.int32))
    assert first_unclear >= NEED_CLEAR
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.basename(FIXTURE)}: head seed {hs}, {ids.size} ids, tokens {t}, first unclear step {first_unclear}")


if __name__ == "__main__":
    main()
