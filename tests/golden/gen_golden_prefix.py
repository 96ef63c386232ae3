"""Generator of tests/golden/tiny_prefix_oracle.npz: the prompt prefix cache's requests on the tiny VISION model, from the CPU oracle.

Seven requests, every one run on its own at B = 1 (`synth_weights(cfg, seed=0, std_scale=4.0)`), STEPS greedy steps, ONE lm_head:

  img0      "What is shown?"                    make_image(336, 336, "noise", 0)
  img0_q2   "Describe the colours in detail."   the same picture
  img0_q3   "What is shown? And where?"         the same picture
  img1      "What is shown?"                    make_image(336, 336, "waves", 0)  -- token ids EQUAL to img0's
  sys_q1 / sys_q2   a shared instruction of ~300 tokens + two different questions, no image
  short     "hi"

A warm request (prefix restored from the store, the rest computed) is compared with ITS OWN oracle run here, never with the
cold run of the code under test.  The generator walks lm_head seeds upwards and keeps the first one under which
  * the six requests other than img1 are clear on their first 2 steps and show two distinct tokens (search_head, need=2);
    later steps are taken as they come (a test compares tokens up to a request's first unclear step);
  * img1 -- run under that head as it comes -- is the WRONG-IMAGE WITNESS at logit level: at least half of its first-step
    logits lie outside img0's tolerance, and the reverse (`outside_fraction`: the tolerance model of logits_vs_fixture).  A
    test that feeds img1 after img0 was cached and holds img1's logits to img1's oracle cannot pass when the picture's
    digest is ignored: the ids of img0 and img1 are identical.
Stored: head seed, spread, rel_tol, names, n_ids, tokens / margins [7, STEPS], the first-step full logits of every request
(`<name>_logits_bf16` [1, 1, V], with `<name>_tokens` / `<name>_margins` [1, STEPS] beside them: the layout
test_model_gpu.logits_vs_fixture reads), the two witness fractions.  Regenerating reproduces the file byte for byte:

    python tests/golden/gen_golden_prefix.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "tiny_prefix_oracle.npz")
STEPS = 6
MAX_SEEDS = 20000
WITNESS_MIN = 0.5
NAMES = ["img0", "img0_q2", "img0_q3", "img1", "sys_q1", "sys_q2", "short"]
SYSTEM = ("You are a careful assistant for a picture archive. Answer in plain words and keep to what can be seen or what the "
          "question states. When an answer needs an item of the archive list, name the item, its shelf and its year before "
          "anything else. Say so when the list does not tell.")
PROMPTS = {"img0": "What is shown?", "img0_q2": "Describe the colours in detail.", "img0_q3": "What is shown? And where?",
           "img1": "What is shown?", "sys_q1": SYSTEM + " Which shelf holds item three?",
           "sys_q2": SYSTEM + " In which year was item seven filed, and by whom?", "short": "hi"}
IMAGES = {"img0": (336, 336, "noise", 0), "img0_q2": (336, 336, "noise", 0), "img0_q3": (336, 336, "noise", 0),
          "img1": (336, 336, "waves", 0)}


def source_image(name):
    """The request's source picture (PIL) or None."""
    from golden_inputs import make_image
    return make_image(*IMAGES[name]) if name in IMAGES else None


def chat_text(name):
    """The prompt as the chat template renders it (api._apply_chat_template: `<|image_1|>` first)."""
    return f"<|user|>\n{'<|image_1|>' + chr(10) if name in IMAGES else ''}{PROMPTS[name].strip()}<|end|>\n<|assistant|>\n"


def request(proc, name):
    """B = 1 model inputs of one fixture request."""
    img = source_image(name)
    return proc(chat_text(name), [img]) if img is not None else proc(chat_text(name))


def outside_fraction(logits, ref, norms, rel_tol):
    """Share of the vocabulary on which `logits` lies outside the tolerance of `ref` (logits_vs_fixture's rule), and the worst
    entry in units of the tolerance."""
    import torch
    ref, got = ref.to(torch.float32).reshape(-1), logits.to(torch.float32).reshape(-1)
    E = rel_tol * (ref / norms).abs().max()
    over = ((got - ref).abs() - 2.0 ** -7 * ref.abs()).clamp_min(0) / (E * norms)
    return float((over > 1.0).float().mean()), float(over.max())


def main():
    import torch
    import phi3v_oracle as orc
    from gen_golden_oracle import COMMON, REL_TOL, SPREAD, Prefilled, bits, row_norms, search_head
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.processor import Phi3VProcessor
    from phi_3_vision_mlx_amd.weights import peaked_lm_head, synth_weights
    cfg = make_config(tiny_config_dict(vision=True))
    w = synth_weights(cfg, seed=0, std_scale=4.0)
    base = w["lm_head.weight"]
    o = orc.OraclePhi3V(cfg, w, cache_fp32=True)
    proc = Phi3VProcessor(None)
    runs = {}
    for name in NAMES:
        inp = request(proc, name)
        runs[name] = Prefilled(o, {k: (torch.from_numpy(np.asarray(v.cpu() if torch.is_tensor(v) else v)) if k == "pixel_values" else v)
                                   for k, v in inp.items()}, STEPS)
    ids = {n: np.asarray(runs[n].inputs["input_ids"]).reshape(-1) for n in NAMES}
    assert np.array_equal(ids["img0"], ids["img1"]), "img0 and img1 must have identical token ids"
    six = [n for n in NAMES if n != "img1"]
    first = 0
    while True:
        hs, res = search_head([runs[n] for n in six], base, STEPS, max_seeds=MAX_SEEDS - first, first_seed=first, need=2, min_distinct=2)
        head = peaked_lm_head(base.to(torch.float32), SPREAD, hs)
        norms = row_norms(head)
        results = dict(zip(six, res))
        results["img1"] = runs["img1"].greedy(head, STEPS, need_clear_steps=0, norms=norms)
        lg0, lg1 = results["img0"][1][0, 0], results["img1"][1][0, 0]
        f01, w01 = outside_fraction(lg1, lg0, norms, REL_TOL)    # img1's logits held to img0's oracle
        f10, w10 = outside_fraction(lg0, lg1, norms, REL_TOL)
        print(f"  head seed {hs}: img1 outside img0's tolerance on {f01:.1%} (worst {w01:.1f} x), reverse {f10:.1%} ({w10:.1f} x)", flush=True)
        if f01 >= WITNESS_MIN and f10 >= WITNESS_MIN:
            break
        first = hs + 1
    out = dict(COMMON, head_seed=np.asarray([hs], dtype=np.int32), names=np.asarray(NAMES),
               n_ids=np.asarray([runs[n].S for n in NAMES], dtype=np.int32),
               tokens=np.concatenate([results[n][0].numpy() for n in NAMES]).astype(np.int32),
               margins=np.concatenate([results[n][2].numpy() for n in NAMES]).astype(np.float32),
               witness=np.asarray([f01, w01, f10, w10], dtype=np.float32))
    for n in NAMES:
        toks, lgs, mgs = results[n]
        out[n + "_tokens"] = toks.numpy().astype(np.int32)
        out[n + "_logits_bf16"] = bits(lgs[:, :1])
        out[n + "_margins"] = mgs.numpy().astype(np.float32)
    assert all((out["margins"][NAMES.index(n), :2] > 1.0).all() for n in six)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.basename(FIXTURE)}: head seed {hs}, n_ids {out['n_ids'].tolist()}, tokens {out['tokens'].tolist()}, "
          f"clear {(out['margins'] > 1.0).sum(1).tolist()}")


if __name__ == "__main__":
    main()
