"""Golden vectors from the REFERENCE'S OWN model and loop code, executed over the functional MLX stand-in.

Runs only in the build container (needs /root/reference; `ref_env.py` explains how it is imported and why nothing of it
travels).  What executes is the reference's `_load` -> `Phi3VForCausalLM` / `Phi3ForCausalLM` (phi.py:135-617: CLIP tower, HD
merge + projector + scatter, SuRoPE, KVCache incl. rewind and beam view, Mask4D, decoder) and its `_generate`,
`_choose_from`, `_constrain` loops with its own processors (phi_3_vision_mlx.py:257-274, 376-409, 466-619; phi.py:228-372)
on the TINY synthetic checkpoint (config.tiny_config_dict, weights.synth_weights: data, written to an HF-layout directory
that the reference loads itself).  Output: `ref_model_tiny.npz` + `ref_model_tiny.json`, same layout as the oracle fixtures
(per greedy step: token, full last-position logits as bf16 bits, clearance) so tests/test_model_gpu.py's `run_fixture`
checks the HIP path against them unchanged, and tests/test_refmodel.py checks the oracle against them.

The lm_head seeds are searched with the oracle (fast, replayable decode) so that every step is clear; the reference is then
run under that head and the clearance is recomputed from ITS logits.

    python tests/golden/gen_golden_refmodel.py
    python tests/golden/gen_golden_refmodel.py live      (ref_live_blind.json only)
"""
import hashlib
import json
import os
import shutil
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import phi3v_oracle as orc  # noqa: E402
import ref_env  # noqa: E402
from gen_golden_oracle import REL_TOL, SPREAD, Prefilled, bits, clearance, row_norms, search_head  # noqa: E402
from golden_inputs import (LIVE_BEAM, LIVE_GEN_PROMPTS, LIVE_PROMPTS, LIVE_STEP, live_blind_weights, make_image,  # noqa: E402
                           one_thread, tensor_digest)
from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict  # noqa: E402
from phi_3_vision_mlx_amd.processor import ByteTokenizer, Phi3FProcessor, Phi3VProcessor  # noqa: E402
from phi_3_vision_mlx_amd.weights import peaked_lm_head, save_adapter, save_safetensors_dir, synth_weights  # noqa: E402

TMP = os.environ.get("P3V_REF_TMP", "/tmp/p3v_refmodel")
TINY_PROMPTS = ["<|user|>\nPick A or B.<|end|>\n<|assistant|>\n", "<|user|>\nName a colour of the sky.<|end|>\n<|assistant|>\n"]
VIS_PROMPT = "<|user|>\n<|image_1|>\nWhat is shown?<|end|>\n<|assistant|>\n"
VIS2_PROMPT = "<|user|>\n<|image_1|>\n<|image_2|>\nCompare the two.<|end|>\n<|assistant|>\n"
LONG_PROMPT = "<|user|>\n" + ("the quick brown fox jumps over the lazy dog. " * 92) + "<|end|>\n<|assistant|>\n"     # > 4096 ids -> long factors
CONSTRAINT = (3, " The answer is")
IMAGES = {"sq": (336, 336, "noise", 0), "land": (640, 480, "smooth", 1)}
LORA = dict(targets=["self_attn.qkv_proj", "mlp.down_proj"], layers=1, rank=2, alpha=4.0, scale=1.5)


def img(name):
    return make_image(*IMAGES[name])


# name -> (blind?, prompt, image names, steps)
CASES = {
    "text": (True, TINY_PROMPTS[0], None, 8),
    "batch": (True, TINY_PROMPTS, None, 6),
    "long": (True, LONG_PROMPT, None, 3),
    "vis": (False, VIS_PROMPT, ["sq"], 4),
    "visns": (False, VIS_PROMPT, ["land"], 4),
    "vis2": (False, VIS2_PROMPT, ["sq", "land"], 4),
}


class Ref:
    """One reference model (blind or vision) loaded by the reference's `_load`, with a swappable lm_head."""

    def __init__(self, blind, adapter_path=None):
        self.blind = blind
        self.d = tiny_config_dict(vision=not blind)
        self.cfg = make_config(self.d)
        self.w = synth_weights(self.cfg, seed=0, std_scale=4.0)
        self.base = self.w["lm_head.weight"]
        self.dir = os.path.join(TMP, "blind" if blind else "vision")
        shutil.rmtree(self.dir, ignore_errors=True)
        save_safetensors_dir(self.w, self.d, self.dir)
        self.mx, self.phi, self.loops = ref_env.load_reference()
        self.model, self.proc = ref_env.load_model(self.dir, ByteTokenizer(), clip_cfg=self.d.get("clip"), adapter_path=adapter_path)
        self.oracle = orc.OraclePhi3V(self.cfg, dict(self.w), cache_fp32=True)
        self.my_proc = (Phi3FProcessor if blind else Phi3VProcessor)(None)

    def head(self, hs):
        h = peaked_lm_head(self.base, SPREAD, int(hs))
        self.model.lm_head.weight = self.mx.array(h)
        self.oracle.w["lm_head.weight"] = h
        self.oracle._f32.pop("lm_head.weight", None)
        return h


def as_t(a):
    return a._t if hasattr(a, "_t") else torch.as_tensor(np.asarray(a))


def generate_case(r, name, out, meta):
    blind, prompt, images, n = CASES[name]
    imgs = [img(i) for i in images] if images else None
    # inputs from the REFERENCE's processor; the build's processor must produce the same model inputs
    ref_in = r.proc(prompt, imgs)
    my_in = r.my_proc(prompt, imgs) if imgs else r.my_proc(prompt)
    ids = as_t(ref_in["input_ids"]).long()
    assert torch.equal(ids, torch.as_tensor(np.asarray(my_in["input_ids"])).long()), f"{name}: processors disagree on input_ids"
    # head seed: oracle search (every step clear), then the reference under that head
    o_in = {k: (torch.from_numpy(np.asarray(v)) if k == "pixel_values" else v) for k, v in my_in.items()}
    hs, _ = search_head([Prefilled(r.oracle, o_in, n)], r.base, n, min_distinct=2)
    for attempt in range(20):
        head = r.head(hs)
        rec = ref_env.Recorder(r.model)
        t0 = time.time()
        texts = r.loops._generate(rec, r.proc, prompt, imgs, max_tokens=n, verbose=False, stream=False, mute=True)
        lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)                       # [B, n, V] bf16
        toks = torch.argmax(lgs.float(), dim=-1)
        fed = torch.cat([as_t(c["input_ids"]).long() for c in rec.calls[1:]], 1)
        assert torch.equal(fed, toks[:, :-1]), f"{name}: the loop fed other tokens than its own argmax"
        mg = clearance(lgs, row_norms(head), REL_TOL)
        if mg.min().item() > 1.0 and lgs.shape[1] == n:
            break
        hs, _ = search_head([Prefilled(r.oracle, o_in, n)], r.base, n, min_distinct=2, first_seed=hs + 1)
    else:
        raise RuntimeError(f"{name}: no head seed is clear under the reference's logits")
    out[name + "_head_seed"] = np.asarray([hs], dtype=np.int32)
    out[name + "_tokens"] = toks.numpy().astype(np.int32)
    out[name + "_logits_bf16"] = bits(lgs)
    out[name + "_margins"] = mg.numpy().astype(np.float32)
    out[name + "_input_ids"] = ids.numpy().astype(np.int32)
    m = {"prompt_chars": len(prompt) if isinstance(prompt, str) else [len(p) for p in prompt], "S": int(ids.shape[1]), "steps": n,
         "texts": texts, "images": images, "offset_after": int(rec.calls[-1]["offset"])}
    if "pids" in ref_in:
        out[name + "_pids"] = as_t(ref_in["pids"]).numpy().astype(np.int32)
        out[name + "_mask"] = as_t(ref_in["mask"]).numpy().astype(np.int32)
    if imgs:
        pv = np.ascontiguousarray(np.asarray(as_t(ref_in["pixel_values"]).numpy(), dtype=np.float32))
        m["pixel_values_f32_sha256"] = hashlib.sha256(pv.tobytes()).hexdigest()
        m["image_sizes"] = as_t(ref_in["image_sizes"]).tolist()
        pos = as_t(ref_in["positions"])
        m["positions_first_last"] = [pos[0].tolist(), pos[-1].tolist()]
        m["n_positions"] = int(pos.shape[0])
    meta[name] = m
    print(f"  {name}: S={ids.shape[1]} head_seed {hs} tokens {toks.tolist()} min clearance {mg.min().item():.2f} "
          f"({time.time() - t0:.1f}s per reference run)", flush=True)


def digest_calls(calls, idc):
    """Compact record of every model call of a loop: the ids it was fed, its arguments, and per (row, position) the top-8
    logits (values + ids), the fp32 log-sum-exp and the logits of the constraint ids -- what the loop's decisions read."""
    L = max(as_t(c["input_ids"]).shape[1] for c in calls)
    B = max(as_t(c["input_ids"]).shape[0] for c in calls)
    n = len(calls)
    ids = np.full((n, B, L), -1, dtype=np.int32)
    args = np.zeros((n, 4), dtype=np.int32)                      # rows, L, advance_offset (-1 = None), n_beam
    P = min(L, len(idc) + 1)
    topv = np.zeros((n, B, P, 8), dtype=np.uint16)
    topi = np.zeros((n, B, P, 8), dtype=np.int32)
    lse = np.zeros((n, B, P), dtype=np.float32)
    cons = np.zeros((n, B, P, len(idc)), dtype=np.uint16)
    for k, c in enumerate(calls):
        t = as_t(c["input_ids"]).long()
        b, l = t.shape
        ids[k, :b, :l] = t.numpy()
        args[k] = (b, l, -1 if c["advance_offset"] is None else c["advance_offset"], c["n_beam"])
        lg = c["logits"]._t                                          # [b, l, V]
        lg = lg[:, -P:] if l > P else lg
        v, i = torch.sort(lg.float(), dim=-1, descending=True, stable=True)
        p = lg.shape[1]
        topv[k, :b, :p] = bits(v[..., :8].to(torch.bfloat16))
        topi[k, :b, :p] = i[..., :8].numpy()
        lse[k, :b, :p] = torch.logsumexp(lg.float(), dim=-1).numpy()
        cons[k, :b, :p] = bits(lg[..., torch.as_tensor(idc).long()])
    return dict(ids=ids, args=args, topv=topv, topi=topi, lse=lse, cons=cons)


def loops_case(r, out, meta):
    """choose + constrain (plain / beam) through the reference's loops on the blind model."""
    proc, my = r.proc, r.my_proc
    idc = my.tokenizer.encode(CONSTRAINT[1], add_special_tokens=False)[1:]
    opts = my([f" {c}" for c in "ABCDE"])["input_ids"][:, -1]
    # a head under which the option pick of `choose` is clear (as tiny_oracle.npz's); the constrain loops' score comparisons
    # are never clear in that sense (means of log-probabilities differ by ~2 % of max|logit|), so their decisions are recorded
    # as they come: the oracle is bit-exact to this path on CPU, and the GPU test walks a live oracle's decisions.
    oi = torch.as_tensor(opts).long()
    for hs in range(4000):
        head = r.head(hs)
        lg, _ = r.oracle(**my(TINY_PROMPTS), max_tokens=0)
        lf, nn_ = lg[:, -1].float(), row_norms(head)
        v2, i2 = lf[:, oi].topk(2, dim=-1)
        E = REL_TOL * (lf / nn_).abs().amax(-1)
        m = ((v2[:, 0] - v2[:, 1]) / (E * (nn_[oi][i2[:, 0]] + nn_[oi][i2[:, 1]]))).min().item()
        if m > 1.0:
            break
    else:
        raise RuntimeError("no clear choose seed")
    out["loops_head_seed"] = np.asarray([hs], dtype=np.int32)
    out["loops_choose_clearance"] = np.asarray([m], dtype=np.float32)
    meta["loops"] = {"head_seed": hs, "choose_clearance": m, "constraint": list(CONSTRAINT), "prompts": TINY_PROMPTS}
    meta["loops"]["choose"] = r.loops._choose_from(r.model, proc, TINY_PROMPTS, "ABCDE", mute=True)
    meta["loops"]["choose_single"] = r.loops._choose_from(r.model, proc, TINY_PROMPTS[1], "ABCDE", mute=True)
    for ub in (False, True):
        ps = TINY_PROMPTS if not ub else TINY_PROMPTS[:1] * 2
        rec = ref_env.Recorder(r.model)
        full = r.loops._constrain(rec, proc, list(ps), [CONSTRAINT], return_full_text=True, mute=True, use_beam=ub, verbose=False)
        cont = r.loops._constrain(r.model, proc, list(ps), [CONSTRAINT, "AB"], mute=True, use_beam=ub, verbose=False)
        meta["loops"][f"constrain_beam{int(ub)}"] = {"full_text": full, "with_choice": cont, "n_calls": len(rec.calls)}
        for k, v in digest_calls(rec.calls, idc).items():
            out[f"constrain_beam{int(ub)}_{k}"] = v
        print(f"  constrain beam={ub}: {len(rec.calls)} model calls, texts {[t[-24:] for t in full]}", flush=True)
    print(f"  loops: head_seed {hs}, choose clearance {m:.2f}, choose {meta['loops']['choose']}", flush=True)


CLEAR_MARGIN = 0.03          # constrain_clear_case: every decision's margin, as a fraction of max |logit| of the forward behind it


def constrain_clear_case(r, out, meta):
    """Round 5: `_constrain` under heads whose EVERY data-dependent decision is clear.  The loop's score
    comparisons are means of log-probabilities that usually sit a fraction of a percent of max |logit| apart, so under the
    `choose` head above its outcome on the GPU can legitimately differ from the reference's.  Here the head seed is searched,
    separately for the plain and the beam loop, on the oracle's decision trace (phi3v_oracle.constrain_one(trace=...): argmax and
    top-3 picks, beam pick, pre-vs-post and score-vs-best comparisons) until the smallest margin of the whole loop exceeds
    CLEAR_MARGIN; the REFERENCE's `_constrain` then runs under that head and its final texts are recorded -- the GPU test asserts
    them (tests/test_model_gpu.py::test_reference_choose_fixture)."""
    proc, my = r.proc, r.my_proc
    idc = my.tokenizer.encode(CONSTRAINT[1], add_special_tokens=False)[1:]
    meta["loops_clear"] = {"constraint": list(CONSTRAINT), "clear_margin": CLEAR_MARGIN}
    for ub in (False, True):
        ps = TINY_PROMPTS if not ub else TINY_PROMPTS[:1] * 2
        best = (-1.0, -1)
        for hs in range(6000):
            r.head(hs)
            tr = []
            orc.constrain_one(r.oracle, dict(my(list(ps))), CONSTRAINT, idc, use_beam=ub, trace=tr)
            m = min(t[1] for t in tr)
            best = max(best, (m, hs))
            if m > CLEAR_MARGIN:
                break
        else:
            raise RuntimeError(f"constrain beam={ub}: no head seed with every margin > {CLEAR_MARGIN} (best {best})")
        r.head(hs)
        rec = ref_env.Recorder(r.model)
        full = r.loops._constrain(rec, proc, list(ps), [CONSTRAINT], return_full_text=True, mute=True, use_beam=ub, verbose=False)
        tr = []
        synth, _ = orc.constrain_one(r.oracle, dict(my(list(ps))), CONSTRAINT, idc, use_beam=ub, trace=tr)
        out[f"clear_beam{int(ub)}_head_seed"] = np.asarray([hs], dtype=np.int32)
        out[f"clear_beam{int(ub)}_synth"] = synth.numpy().astype(np.int32)
        meta["loops_clear"][f"beam{int(ub)}"] = {"head_seed": hs, "min_margin": m, "n_decisions": len(tr), "n_calls": len(rec.calls),
                                                "full_text": full}
        print(f"  constrain (clear) beam={ub}: head_seed {hs}, {len(tr)} decisions, min margin {m:.4f}, texts {[t[-24:] for t in full]}", flush=True)


def lora_case(out, meta):
    """The reference's adapter path: `_load(adapter_path=...)` -> `_linear_to_lora_layers` + `LoRALinear.__call__`
    (phi_3_vision_mlx.py:234-245, 266-271; phi.py:96-133) on seeded lora_a / lora_b."""
    d = tiny_config_dict(vision=False)
    cfg = make_config(d)
    g = torch.Generator().manual_seed(5)
    n_layers = cfg.num_hidden_layers
    shapes = {"self_attn.qkv_proj": (cfg.hidden_size, 3 * cfg.hidden_size), "mlp.down_proj": (cfg.intermediate_size, cfg.hidden_size)}
    tensors = {}
    for i in range(n_layers - LORA["layers"], n_layers):
        for t in LORA["targets"]:
            fi, fo = shapes[t]
            tensors[f"model.layers.{i}.{t}.lora_a"] = (torch.randn(fi, LORA["rank"], generator=g) * 0.05).float()
            tensors[f"model.layers.{i}.{t}.lora_b"] = (torch.randn(LORA["rank"], fo, generator=g) * 0.05).float()
    ad = os.path.join(TMP, "adapter")
    shutil.rmtree(ad, ignore_errors=True)
    lcfg = {"model_path": os.path.join(TMP, "blind"), "adapter_path": ad, "lora_layers": LORA["layers"], "lora_targets": LORA["targets"],
            "lora_parameters": {"rank": LORA["rank"], "alpha": LORA["alpha"], "dropout": 0.0, "scale": LORA["scale"]}}
    save_adapter(ad, lcfg, tensors)
    r = Ref(True, adapter_path=ad)
    from phi_3_vision_mlx_amd.weights import load_adapter, resolve_adapter
    r.oracle.adapters = resolve_adapter(cfg, *load_adapter(ad))
    for k, v in tensors.items():
        out["lora_" + k.replace(".", "__")] = v.numpy()
    meta["lora_adapter"] = {k: v for k, v in lcfg.items() if k not in ("model_path", "adapter_path")}
    CASES["lora"] = (True, TINY_PROMPTS[1], None, 4)
    generate_case(r, "lora", out, meta)


# (q4batch, round 6: the two prompts as ONE left-padded batch -- QuantizedLinear at B = 2 under the reference's Mask4D / position ids)
Q4_CASES = {"q4text": (TINY_PROMPTS[1], None, 4), "q4vis": (VIS_PROMPT, ["sq"], 3), "q4batch": (TINY_PROMPTS, None, 4)}


def q4_case(out, meta):
    """The reference's 4-bit path end to end: its `_quantize` (phi_3_vision_mlx.py:291-305: `nn.quantize(model, 64, 4)` + save of
    `quantized_model.safetensors` + config['quantized'] / ['sanitized']) writes the checkpoint from the tiny bf16 directory, its
    `_load` reads it back (`nn.quantize` BEFORE `load_weights`, :264) and `_generate` runs on `QuantizedLinear` /
    `QuantizedEmbedding`.  Recorded: which tensors the reference quantises (names, shapes, dtypes, sha256 of every tensor of the
    file it wrote) and the greedy logits of a text and an image prompt.  The affine group quantiser runs in the stand-in's OWN
    statement of mlx 0.15.0's composite (mlx_shim.quantize; round 6: it no longer calls `weights.mlx_quantize`, and
    tests/test_host_logic.py holds the two to bit equality): this pins the format AND everything around it -- traversal, naming, file layout,
    config keys, load order, which layers run quantised (every Linear incl. the ViT's and the projector's, both embeddings and the
    CLIP position table; not the patch convolution, not the norms)."""
    import gen_golden_oracle as ggo
    from safetensors.torch import load_file
    from phi_3_vision_mlx_amd.weights import mlx_dequantize, mlx_quantize
    d = tiny_config_dict(vision=True)
    cfg = make_config(d)
    w = synth_weights(cfg, seed=0, std_scale=4.0)
    base = w["lm_head.weight"]
    mx, phi, loops = ref_env.load_reference()
    import types
    phi.Phi3ImageEmbedding.CLIP_VIT_LARGE_PATCH14_336_CONFIG = types.SimpleNamespace(**d["clip"])     # tiny CLIP geometry (as ref_env.load_model)
    src, dst = os.path.join(TMP, "q4_src"), os.path.join(TMP, "q4_dst")
    my = Phi3VProcessor(None)

    def q4_head(b, spread, hs):                                     # what the head is after the reference's quantiser: fp32 scale * q + bias
        return mlx_dequantize(*mlx_quantize(peaked_lm_head(b.to(torch.bfloat16), spread, hs))).float()

    def oracle_weights(path):
        t = load_file(os.path.join(path, "quantized_model.safetensors"))
        ow = {}
        for k, v in t.items():
            if k.endswith(".scales") or k.endswith(".biases"):
                continue
            base_k = k[:-len(".weight")] if k.endswith(".weight") else None
            if base_k is not None and base_k + ".scales" in t:
                is_table = "vision_embed_tokens.img_projection" not in k and ("embed_tokens.weight" in k or "position_embedding" in k)
                # embedding tables leave mx.dequantize as bf16 ARRAYS (nn.QuantizedEmbedding: multiply and add each round to bf16);
                # the Linears run mx.quantized_matmul: scale * q + bias in fp32 on the fly
                ow[k] = mlx_dequantize(v, t[base_k + ".scales"], t[base_k + ".biases"], dtype=torch.bfloat16 if is_table else None)
            elif "patch_embedding.weight" in k:
                ow[k] = v.permute(0, 3, 1, 2).contiguous()            # sanitized file: OHWI -> the oracle's OIHW
            else:
                ow[k] = v
        return t, ow
    for name, (prompt, images, n) in Q4_CASES.items():
        imgs = [img(i) for i in images] if images else None
        my_in = my(prompt, imgs) if imgs else my(prompt)
        # head seed: oracle on the dequantised checkpoint (seed-independent part quantised once), every step clear
        shutil.rmtree(src, ignore_errors=True), shutil.rmtree(dst, ignore_errors=True)
        save_safetensors_dir(w, d, src)
        loops._quantize(from_path=src, to_path=dst)
        _, ow = oracle_weights(dst)
        o = orc.OraclePhi3V(cfg, ow, cache_fp32=True)
        o_in = {k: (torch.from_numpy(np.asarray(v)) if k == "pixel_values" else v) for k, v in my_in.items()}
        plain = ggo.peaked_lm_head
        r = Prefilled(o, o_in, n)
        r.rel_tol = 0.045
        first = 0
        for attempt in range(8):                                    # the oracle picks a candidate; the REFERENCE's own logits decide
            ggo.peaked_lm_head = q4_head
            try:
                hs, _ = search_head([r], base, n, min_distinct=2, first_seed=first)
            finally:
                ggo.peaked_lm_head = plain
            # the reference on a checkpoint whose bf16 source carries that head
            w2 = dict(w)
            w2["lm_head.weight"] = peaked_lm_head(base, SPREAD, hs)
            shutil.rmtree(src, ignore_errors=True), shutil.rmtree(dst, ignore_errors=True)
            save_safetensors_dir(w2, d, src)
            loops._quantize(from_path=src, to_path=dst)
            tens, _ = oracle_weights(dst)
            model, proc = ref_env.load_model(dst, ByteTokenizer(), clip_cfg=d["clip"])
            rec = ref_env.Recorder(model)
            loops._generate(rec, proc, prompt, imgs, max_tokens=n, verbose=False, stream=False, mute=True)
            lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)
            toks = torch.argmax(lgs.float(), dim=-1)
            mg = clearance(lgs, row_norms(q4_head(base, SPREAD, hs)), 0.045)
            if mg.min().item() > 1.0:
                break
            print(f"  {name}: head seed {hs} is clear for the oracle, not for the reference ({mg.min().item():.2f}); next", flush=True)
            first = hs + 1
        assert mg.min().item() > 1.0, f"{name}: not clear under the reference's logits ({mg.tolist()})"
        out[name + "_head_seed"] = np.asarray([hs], dtype=np.int32)
        out[name + "_tokens"] = toks.numpy().astype(np.int32)
        out[name + "_logits_bf16"] = bits(lgs)
        out[name + "_margins"] = mg.numpy().astype(np.float32)
        out[name + "_rel_tol"] = np.asarray([0.045], dtype=np.float32)
        with open(os.path.join(dst, "config.json")) as f:
            qcfg = json.load(f)
        meta[name] = {"S": int(np.asarray(my_in["input_ids"]).shape[1]), "steps": n, "images": images,
                      "config_flags": {k: qcfg.get(k) for k in ("quantized", "sanitized")},
                      "file": "quantized_model.safetensors",
                      "tensors": {k: [str(v.dtype).replace("torch.", ""), list(v.shape), hashlib.sha256(v.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()]
                                  for k, v in sorted(tens.items())}}
        nq = sum(1 for k in tens if k.endswith(".scales"))
        print(f"  {name}: head_seed {hs}, {nq} quantised tensors of {len(tens)}, tokens {toks.tolist()}, min clearance {mg.min().item():.2f}", flush=True)


def main():
    t0 = time.time()
    os.makedirs(TMP, exist_ok=True)
    out = dict(rel_tol=np.asarray([REL_TOL], dtype=np.float32), spread=np.asarray([SPREAD], dtype=np.float32))
    meta = {"generator": "tests/golden/gen_golden_refmodel.py", "reference": "phi.py + phi_3_vision_mlx.py over tests/golden/mlx_shim.py"}
    rb = Ref(True)
    for name in ("text", "batch", "long"):
        generate_case(rb, name, out, meta)
    loops_case(rb, out, meta)
    constrain_clear_case(rb, out, meta)
    rv = Ref(False)
    for name in ("vis", "visns", "vis2"):
        generate_case(rv, name, out, meta)
    lora_case(out, meta)
    q4_case(out, meta)
    q4cache_case(out, meta)
    np.savez_compressed(os.path.join(HERE, "ref_model_tiny.npz"), **out)
    with open(os.path.join(HERE, "ref_model_tiny.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"wrote ref_model_tiny.npz/.json in {time.time() - t0:.0f}s")


class TableTokenizer:
    """A tokenizer stand-in for the FULL-SIZE runs: `table` maps whole strings (a prompt, or the chunks `_merge` cuts a prompt
    into, phi.py:265) to prepared id lists, so that the reference's processors + `_generate` run on exactly the ids of the
    oracle fixtures (random ids up to 32000 have no spelling in the byte tokenizer).  Decoding returns the ids as text."""

    def __init__(self, table):
        self.table = table

    def __call__(self, texts, **kw):
        return ByteTokenizer.__call__.__globals__["_Enc"](self.table[texts] if isinstance(texts, str) else [self.table[t] for t in texts])

    def decode(self, ids, **kw):
        return " ".join(str(int(i)) for i in ids)

    def batch_decode(self, seqs, **kw):
        return [self.decode(s) for s in seqs]


def full():
    """`ref_model_full.npz`: the reference's own code at FULL size (3072 / 32 layers / 32 heads / vocab 32064; CLIP ViT-L/14-336, 17
    crops) on the requests of c1_oracle.npz (128 random ids) and c2_oracle.npz (bench.py's image request, 2531 ids), under those
    fixtures' lm_head seeds: prefill + 3 (c1) / 2 (c2) greedy steps through `_generate`.  Pins the full-size HIP path to the
    reference directly (tests/test_model_gpu.py::test_reference_model_fixture_full_size) and shows oracle == reference at full
    size by comparing with the oracle fixtures of the same requests (tests/test_refmodel.py)."""
    from gen_golden_oracle import REL_TOL_LONG, REL_TOL_SHORT
    from golden_inputs import vqa_request
    from phi_3_vision_mlx_amd.config import phi3v_config_dict
    torch.set_num_threads(8)
    out = dict(spread=np.asarray([SPREAD], dtype=np.float32))
    meta = {"generator": "tests/golden/gen_golden_refmodel.py full"}
    d = phi3v_config_dict(vision=True)
    cfg = make_config(d)
    t0 = time.time()
    w = synth_weights(cfg, seed=0)
    base = w["lm_head.weight"]
    path = os.path.join(TMP, "full_vision")
    shutil.rmtree(path, ignore_errors=True)
    save_safetensors_dir(w, d, path)
    print(f"weights written {time.time() - t0:.0f}s", flush=True)
    g1, g2 = np.load(os.path.join(HERE, "c1_oracle.npz")), np.load(os.path.join(HERE, "c2_oracle.npz"))
    inp2 = vqa_request(Phi3VProcessor(None).img_processor, 0)
    ids2 = np.asarray(inp2["input_ids"])[0]
    n_img = int((ids2 < 0).sum())
    first_neg = int(np.argmax(ids2 < 0))
    table = {"<C1>": [int(t) for t in g1["ids"][0]], "A": [int(t) for t in ids2[:first_neg]], "B": [int(t) for t in ids2[first_neg + n_img:]]}
    mx, phi, loops = ref_env.load_reference()
    model, proc = ref_env.load_model(path, TableTokenizer(table), clip_cfg=d["clip"])
    del w
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))      # vqa_request's image (seed 0)
    for name, prompt, imgs, n, hs, rel_tol, ref_ids in (("c1", "<C1>", None, 4, int(g1["head_seed"][0]), REL_TOL_SHORT, g1["ids"]),
                                                       ("c2", "A<|image_1|>B", [img], 3, int(g2["head_seed"][0]), REL_TOL_LONG, ids2[None])):
        head = peaked_lm_head(base, SPREAD, hs)
        model.lm_head.weight = mx.array(head)
        rec = ref_env.Recorder(model)
        t0 = time.time()
        texts = loops._generate(rec, proc, prompt, imgs, max_tokens=n, verbose=False, stream=False, mute=True)
        ids = as_t(rec.calls[0]["input_ids"]).long()
        assert np.array_equal(ids.numpy(), np.asarray(ref_ids)), f"{name}: the reference's processor built other ids than the fixture's request"
        lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)
        toks = torch.argmax(lgs.float(), dim=-1)
        mg = clearance(lgs, row_norms(head), rel_tol)
        out[name + "_head_seed"] = np.asarray([hs], dtype=np.int32)
        out[name + "_rel_tol"] = np.asarray([rel_tol], dtype=np.float32)
        out[name + "_tokens"] = toks.numpy().astype(np.int32)
        out[name + "_logits_bf16"] = bits(lgs)
        out[name + "_margins"] = mg.numpy().astype(np.float32)
        meta[name] = {"S": int(ids.shape[1]), "steps": n, "texts": texts, "seconds": round(time.time() - t0)}
        print(f"  {name}: S={ids.shape[1]} tokens {toks.tolist()} min clearance {mg.min().item():.2f} ({time.time() - t0:.0f}s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "ref_model_full.npz"), **out)
    with open(os.path.join(HERE, "ref_model_full.json"), "w") as f:
        json.dump(meta, f, indent=1)
    shutil.rmtree(path, ignore_errors=True)
    print("wrote ref_model_full.npz/.json")


Q4CACHE_REL_TOL = 0.10


def q4cache_case(out, meta):
    """Round 5: the reference's OWN quantised KV cache -- `_load(..., use_quantized_cache=True)` -> KVCache keeps
    mx.quantize(keys / values of the first call, group_size=32) and attends on mx.dequantize of them from the second call on, later
    tokens unquantised (phi.py:528-540) -- through `_generate` on the tiny text model.  The head seed is searched ON THE REFERENCE
    until every step is clear at Q4CACHE_REL_TOL = 10 % (the other tiny cases: 3 %).  Why so wide: the oracle (which restates this
    cache too, phi3v_oracle.OracleKVCache, and reproduces this fixture BIT FOR BIT on the CPU) and the HIP path agree on layer 0's
    codes, but from layer 1 on their inputs differ by the usual ~1 % of rounding noise, which flips ~10 % of the 4-bit codes -- each
    flip moves a key or value by a full quantisation step (1/15 of its group's range).  Two correct implementations of a 4-bit cache
    part at that level: 1.3 - 2.9 % of max |logit| against the oracle on this model (tools/scratch/q4cache_dbg.py), up to 6.5 % in
    the tolerance's own unit under the peaked heads.  tests/test_model_gpu.py pins the mechanism exactly instead
    (test_kv_quantize_mlx4_*: codes / scales / biases bit-identical to mx.quantize on equal inputs)."""
    d = tiny_config_dict(vision=False)
    cfg = make_config(d)
    w = synth_weights(cfg, seed=0, std_scale=4.0)
    base = w["lm_head.weight"]
    path = os.path.join(TMP, "q4cache_blind")
    shutil.rmtree(path, ignore_errors=True)
    save_safetensors_dir(w, d, path)
    mx, phi, loops = ref_env.load_reference()
    model, proc = ref_env.load_model(path, ByteTokenizer(), use_quantized_cache=True)
    assert model.config.use_quantized_cache if hasattr(model, "config") else True
    prompt, n = TINY_PROMPTS[0], 4
    for hs in range(2000):
        head = peaked_lm_head(base, SPREAD, hs)
        model.lm_head.weight = mx.array(head)
        rec = ref_env.Recorder(model)
        texts = loops._generate(rec, proc, prompt, None, max_tokens=n, verbose=False, stream=False, mute=True)
        lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)
        if lgs.shape[1] != n:
            continue
        mg = clearance(lgs, row_norms(head), Q4CACHE_REL_TOL)
        toks = torch.argmax(lgs.float(), dim=-1)
        if mg.min().item() > 1.0 and len(set(toks.reshape(-1).tolist())) >= 2:
            break
    else:
        raise RuntimeError("q4cache: no clear head seed")
    out["q4cache_rel_tol"] = np.asarray([Q4CACHE_REL_TOL], dtype=np.float32)
    kv = rec.calls[0]  # noqa: F841
    ids = as_t(rec.calls[0]["input_ids"]).long()
    out["q4cache_head_seed"] = np.asarray([hs], dtype=np.int32)
    out["q4cache_tokens"] = toks.numpy().astype(np.int32)
    out["q4cache_logits_bf16"] = bits(lgs)
    out["q4cache_margins"] = mg.numpy().astype(np.float32)
    out["q4cache_input_ids"] = ids.numpy().astype(np.int32)
    meta["q4cache"] = {"S": int(ids.shape[1]), "steps": n, "texts": texts, "head_seed": hs, "cache": "mx.quantize group 32, 4 bits, prompt only (phi.py:528-540)"}
    print(f"  q4cache: S={ids.shape[1]} head_seed {hs} tokens {toks.tolist()} min clearance {mg.min().item():.2f}", flush=True)
    shutil.rmtree(path, ignore_errors=True)


RESIDUAL_SCALE_WC = 1.0 / 1024


def wc():
    """`ref_model_wc.npz` (round 5): the reference's own code at FULL size on a WELL-CONDITIONED checkpoint -- the seeded synthetic
    text model with its residual-branch output projections (o_proj, down_proj) scaled by RESIDUAL_SCALE_WC = 1 / 1024
    (weights.synth_weights(residual_scale=...)), so that the 64 branches together carry about a quarter of the amplitude of the embedding
    stream instead of replacing it layer after layer (the depth-scaled initialisation 1 / sqrt(2 * 32) = 1 / 8 is not enough for
    that: the plain N(0, 0.02) gate_up / down pair alone has a gain of ~40; tools/scratch/wc_probe.py measured the decode-vs-prefill
    self-consistency at 5.8 / 5.4 / 4.2 / 2.6 / 1.1 % of max |logit| for scales 1, 1/8, 1/64, 1/256, 1/1024 -- 0.7 % of that is one
    bf16 ulp of the logits themselves) -- over the benchmark's horizon: config 1's 128-token prompt,
    128 greedy tokens through `_generate`, under two UNSEARCHED heads: the plain N(0, 0.02) lm_head bench.py times and the peaked
    head of seed 0.  Per step the compact record of gen_golden_oracle.pack_long (token, top-8, 256 seeded entries, max |z|,
    log-sum-exp, clearance) at rel_tol = REL_TOL_WC.  tests/test_model_gpu.py::test_well_conditioned_reference_long_horizon holds
    the HIP path to it: every step's logits inside 1.5 %, tokens exact on every clear step, at least 100 of the 128 steps clear."""
    from gen_golden_oracle import N_SAMPLE, REL_TOL_WC, pack_long
    from phi_3_vision_mlx_amd.config import phi3v_config_dict
    torch.set_num_threads(8)
    n_steps = 128
    out = dict(spread=np.asarray([SPREAD], dtype=np.float32), rel_tol=np.asarray([REL_TOL_WC], dtype=np.float32))
    meta = {"generator": "tests/golden/gen_golden_refmodel.py wc", "residual_scale": RESIDUAL_SCALE_WC, "steps": n_steps}
    out["residual_scale"] = np.asarray([RESIDUAL_SCALE_WC], dtype=np.float32)
    d = phi3v_config_dict(vision=False)
    cfg = make_config(d)
    t0 = time.time()
    w = synth_weights(cfg, seed=0, residual_scale=RESIDUAL_SCALE_WC)
    base = w["lm_head.weight"]
    path = os.path.join(TMP, "wc_blind")
    shutil.rmtree(path, ignore_errors=True)
    save_safetensors_dir(w, d, path)
    print(f"weights written {time.time() - t0:.0f}s", flush=True)
    g1 = np.load(os.path.join(HERE, "c1_oracle.npz"))
    table = {"<C1>": [int(t) for t in g1["ids"][0]]}
    mx, phi, loops = ref_env.load_reference()
    model, proc = ref_env.load_model(path, TableTokenizer(table))
    del w
    out["n_ids"] = np.asarray([g1["ids"].shape[1]], dtype=np.int32)
    for prefix, head in (("plain_", base), ("peaked0_", peaked_lm_head(base, SPREAD, 0))):
        model.lm_head.weight = mx.array(head)
        rec = ref_env.Recorder(model)
        t0 = time.time()
        # (EOS suppressed: the table tokenizer never maps an id to <|end|>, and the stop check reads the decoded id)
        texts = loops._generate(rec, proc, "<C1>", None, max_tokens=n_steps, verbose=False, stream=False, mute=True)
        ids = as_t(rec.calls[0]["input_ids"]).long()
        assert np.array_equal(ids.numpy(), np.asarray(g1["ids"])), "the reference's processor built other ids than the fixture's request"
        lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)                     # [1, n, V] bf16
        toks = torch.argmax(lgs.float(), dim=-1)
        fed = torch.cat([as_t(c["input_ids"]).long() for c in rec.calls[1:]], 1)
        assert torch.equal(fed, toks[:, :-1]), "the loop fed other tokens than its own argmax"
        mg = clearance(lgs, row_norms(head), REL_TOL_WC)
        pack_long(prefix, head, (toks, lgs, mg), out, REL_TOL_WC)
        meta[prefix[:-1]] = {"steps": int(lgs.shape[1]), "clear": int((mg > 1.0).sum()), "seconds": round(time.time() - t0)}
        print(f"  {prefix[:-1]}: {lgs.shape[1]} steps, {int((mg > 1.0).sum())} clear at rel_tol {REL_TOL_WC} ({time.time() - t0:.0f}s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "ref_model_wc.npz"), **out)
    with open(os.path.join(HERE, "ref_model_wc.json"), "w") as f:
        json.dump(meta, f, indent=1)
    shutil.rmtree(path, ignore_errors=True)
    print("wrote ref_model_wc.npz/.json")


REL_TOL_WC_C2 = 0.012           # VERDICT r05 item 1c asked for <= 2 % on the image path of a well-conditioned checkpoint; measured HIP-vs-reference 0.76 %


def wc_c2():
    """`ref_model_wc_c2.npz` (round 6): the REFERENCE'S OWN code at full size on the WELL-CONDITIONED vision checkpoint (decoder
    residual branches x 1 / 1024, as `wc`; the CLIP tower and the projector as they are) for BASELINE config 2's request -- bench.py's
    seeded 336 x 336 image -> 17 crops -> 2509 image tokens + 22 text tokens -- over 16 greedy steps through `_generate`, under two
    UNSEARCHED heads (plain N(0, 0.02) and the peaked head of seed 0).  The image path (ViT + HD merge + projector + scatter) feeds a
    decoder that does not amplify: what differs between two correct programs there (fp32 tower association, bf16 GEMM inputs of the
    build) reaches the logits at its own size.  pack_long records per step; tests/test_model_gpu.py holds the HIP path to
    REL_TOL_WC_C2."""
    from gen_golden_oracle import pack_long
    from golden_inputs import vqa_request
    from phi_3_vision_mlx_amd.config import phi3v_config_dict
    torch.set_num_threads(8)
    n_steps = 16
    out = dict(spread=np.asarray([SPREAD], dtype=np.float32), rel_tol=np.asarray([REL_TOL_WC_C2], dtype=np.float32),
               residual_scale=np.asarray([RESIDUAL_SCALE_WC], dtype=np.float32))
    meta = {"generator": "tests/golden/gen_golden_refmodel.py wc_c2", "residual_scale": RESIDUAL_SCALE_WC, "steps": n_steps}
    d = phi3v_config_dict(vision=True)
    cfg = make_config(d)
    t0 = time.time()
    w = synth_weights(cfg, seed=0, residual_scale=RESIDUAL_SCALE_WC)
    base = w["lm_head.weight"]
    path = os.path.join(TMP, "wc_vision")
    shutil.rmtree(path, ignore_errors=True)
    save_safetensors_dir(w, d, path)
    print(f"weights written {time.time() - t0:.0f}s", flush=True)
    inp2 = vqa_request(Phi3VProcessor(None).img_processor, 0)
    ids2 = np.asarray(inp2["input_ids"])[0]
    n_img = int((ids2 < 0).sum())
    first_neg = int(np.argmax(ids2 < 0))
    table = {"A": [int(t) for t in ids2[:first_neg]], "B": [int(t) for t in ids2[first_neg + n_img:]]}
    mx, phi, loops = ref_env.load_reference()
    model, proc = ref_env.load_model(path, TableTokenizer(table), clip_cfg=d["clip"])
    del w
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))      # vqa_request's image (seed 0)
    out["n_ids"] = np.asarray([ids2.shape[0]], dtype=np.int32)
    for prefix, head in (("plain_", base), ("peaked0_", peaked_lm_head(base, SPREAD, 0))):
        model.lm_head.weight = mx.array(head)
        rec = ref_env.Recorder(model)
        t0 = time.time()
        loops._generate(rec, proc, "A<|image_1|>B", [img], max_tokens=n_steps, verbose=False, stream=False, mute=True)
        ids = as_t(rec.calls[0]["input_ids"]).long()
        assert np.array_equal(ids.numpy(), ids2[None]), "the reference's processor built other ids than bench.py's request"
        lgs = torch.stack([c["logits"]._t[:, -1] for c in rec.calls], 1)
        toks = torch.argmax(lgs.float(), dim=-1)
        mg = clearance(lgs, row_norms(head), REL_TOL_WC_C2)
        pack_long(prefix, head, (toks, lgs, mg), out, REL_TOL_WC_C2)
        meta[prefix[:-1]] = {"steps": int(lgs.shape[1]), "clear": int((mg > 1.0).sum()), "seconds": round(time.time() - t0)}
        print(f"  {prefix[:-1]}: {lgs.shape[1]} steps, {int((mg > 1.0).sum())} clear at rel_tol {REL_TOL_WC_C2} ({time.time() - t0:.0f}s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "ref_model_wc_c2.npz"), **out)
    with open(os.path.join(HERE, "ref_model_wc_c2.json"), "w") as f:
        json.dump(meta, f, indent=1)
    shutil.rmtree(path, ignore_errors=True)
    print("wrote ref_model_wc_c2.npz/.json")


def wc_retol():
    """Re-state ref_model_wc.npz at the current REL_TOL_WC without re-running the reference (12 minutes of CPU per head): the clearance
    of a step is (top-2 margin) / (sum of the two entries' tolerances), i.e. inversely proportional to rel_tol -- an exact rescale."""
    from gen_golden_oracle import REL_TOL_WC
    f = os.path.join(HERE, "ref_model_wc.npz")
    g = dict(np.load(f))
    old = float(g["rel_tol"][0])
    for k in [k for k in g if k.endswith("margins")]:
        g[k] = (g[k].astype(np.float64) * (old / REL_TOL_WC)).astype(np.float32)
    g["rel_tol"] = np.asarray([REL_TOL_WC], dtype=np.float32)
    np.savez_compressed(f, **g)
    with open(os.path.join(HERE, "ref_model_wc.json")) as fh:
        meta = json.load(fh)
    meta["rel_tol"] = REL_TOL_WC
    for k in ("plain", "peaked0"):
        meta[k]["clear"] = int((g[k + "_margins"] > 1.0).sum())
    with open(os.path.join(HERE, "ref_model_wc.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"ref_model_wc: rel_tol {old} -> {REL_TOL_WC}; clear steps plain {meta['plain']['clear']}, peaked0 {meta['peaked0']['clear']}")


def live():
    """ref_live_blind.json: the reference's model-level contract (all-position prefill logits, cached L > 1 calls with
    advance_offset 0 / 1 / None, a read-only n_beam=3 view, the fp32 cache contents) and `_generate` with EOS + Streamer on a
    blind tiny checkpoint and prompts that are NOT in ref_model_tiny.  The tensors are recorded as sha256 digests of their
    bits (the all-position logits alone are MBs); tests/test_refmodel.py holds the oracle to them bit for bit.  The oracle is
    run beside the reference here too, and the file is only written when the two agree."""
    t0 = time.time()
    d, w = live_blind_weights()
    cfg = make_config(d)
    path = os.path.join(TMP, "live_blind")
    shutil.rmtree(path, ignore_errors=True)
    os.makedirs(path)
    save_safetensors_dir(w, d, path)
    mx, _, loops = ref_env.load_reference()
    model, proc = ref_env.load_model(path, ByteTokenizer())
    oracle, my = orc.OraclePhi3V(cfg, w, cache_fp32=True), Phi3FProcessor(None)
    meta = {"generator": "tests/golden/gen_golden_refmodel.py live", "reference": "phi.py + phi_3_vision_mlx.py over tests/golden/mlx_shim.py",
            "weights": "tiny blind, synth_weights(seed=3, std_scale=4.0, lm_head_spread=4.0, lm_head_seed=1)", "threads": 1, "calls": []}
    with one_thread():
        live_calls(mx, model, proc, oracle, my, meta)
    texts = loops._generate(model, proc, LIVE_GEN_PROMPTS, max_tokens=9, verbose=False, stream=False, mute=True)
    toks, _ = orc.greedy_generate(oracle, dict(my(LIVE_GEN_PROMPTS)), 9)
    rows = [(r[:r.index(orc.ID_EOS) + 1] if orc.ID_EOS in r else r) for r in toks.tolist()]
    assert my.tokenizer.batch_decode(rows) == texts
    meta["generate"] = {"prompts": LIVE_GEN_PROMPTS, "max_tokens": 9, "texts": texts}
    with open(os.path.join(HERE, "ref_live_blind.json"), "w") as f:
        json.dump(meta, f, indent=1)
    shutil.rmtree(path, ignore_errors=True)
    print(f"wrote ref_live_blind.json in {time.time() - t0:.0f}s")


def live_calls(mx, model, proc, oracle, my, meta):
    """The model-level calls of ref_live_blind.json, reference and oracle side by side (see live())."""
    def rec(what, rl, rc, ol, oc, valid=None):
        r, o = (rl._t, ol) if valid is None else (rl._t[valid], ol[valid])
        assert torch.equal(r, o) and rc[0].offset == oc[0].offset, f"{what}: oracle and reference differ"
        meta["calls"].append({"call": what, "logits": tensor_digest(r), "offset": int(rc[0].offset)})
    r_in, o_in = proc(LIVE_PROMPTS), my(LIVE_PROMPTS)
    rl, rc = model(**r_in, max_tokens=12)
    ol, oc = oracle(**o_in, max_tokens=12)
    rec("prefill", rl, rc, ol, oc, torch.as_tensor(np.asarray(o_in["mask"])).bool())     # pad query rows are undefined (Q7)
    step = torch.tensor(LIVE_STEP)
    for adv in (0, 1, None):
        rl, rc = model(input_ids=mx.array(step.numpy()), cache=rc, advance_offset=adv)
        ol, oc = oracle(input_ids=step, cache=oc, advance_offset=adv)
        rec(f"step_advance_{adv}", rl, rc, ol, oc)
    beam = torch.tensor(LIVE_BEAM)
    rl, _ = model(input_ids=mx.array(beam.numpy()), cache=rc, n_beam=3, advance_offset=0)
    ol, _ = oracle(input_ids=beam, cache=oc, n_beam=3, advance_offset=0)
    rec("beam_view", rl, rc, ol, oc)
    meta["cache"] = []
    for a, b in zip(rc, oc):
        assert torch.equal(a.kv._t[:, :, :, :a.offset], b.kv[:, :, :, :b.offset])
        meta["cache"].append(tensor_digest(a.kv._t[:, :, :, :a.offset]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "live":
        live()
    elif len(sys.argv) > 1 and sys.argv[1] == "wc":
        wc()
    elif len(sys.argv) > 1 and sys.argv[1] == "wc_retol":
        wc_retol()
    elif len(sys.argv) > 1 and sys.argv[1] == "wc_c2":
        wc_c2()
    elif len(sys.argv) > 1 and sys.argv[1] in ("constrain", "q4cache"):   # one case, merged into the existing fixture
        out, meta = {}, {}
        if sys.argv[1] == "constrain":
            constrain_clear_case(Ref(True), out, meta)
        else:
            q4cache_case(out, meta)
        g = dict(np.load(os.path.join(HERE, "ref_model_tiny.npz")))
        g.update(out)
        np.savez_compressed(os.path.join(HERE, "ref_model_tiny.npz"), **g)
        with open(os.path.join(HERE, "ref_model_tiny.json")) as f:
            m = json.load(f)
        m.update(meta)
        with open(os.path.join(HERE, "ref_model_tiny.json"), "w") as f:
            json.dump(m, f, indent=1)
        print(f"merged the {sys.argv[1]} case(s) into ref_model_tiny.npz/.json")
    elif len(sys.argv) > 1 and sys.argv[1] == "q4":                   # only the 4-bit cases, merged into the existing fixture
        out, meta = {}, {}
        q4_case(out, meta)
        g = dict(np.load(os.path.join(HERE, "ref_model_tiny.npz")))
        g.update(out)
        np.savez_compressed(os.path.join(HERE, "ref_model_tiny.npz"), **g)
        with open(os.path.join(HERE, "ref_model_tiny.json")) as f:
            m = json.load(f)
        m.update(meta)
        with open(os.path.join(HERE, "ref_model_tiny.json"), "w") as f:
            json.dump(m, f, indent=1)
        print("merged the q4 cases into ref_model_tiny.npz/.json")
    elif len(sys.argv) > 1 and sys.argv[1] == "full":
        full()
    else:
        main()
