"""HTTP façade over `generate` -- the endpoint contract of the reference's server.py (server.py:8-29):

    POST /v1/completions   {"prompt": str | [str, ...], "max_tokens": int (default 512)}
      -> 200 {"model": "phi-3-vision", "responses": [str, ...]}            anything else -> 404
    (extension: "temperature" (default 0 = greedy), "top_k" (0 = off), "top_p" (1 = off), "seed" (default: 64 random bits) --
     seeded sampling, include/p3v.h; a sampled response adds "seeds": [one per prompt], which reproduce it.)
    (extension: "adapter": a name, or a list of one name / null per prompt -- the LoRA adapter of the server's bank
     (`--adapter NAME=DIR`, repeatable) that prompt runs with; absent / null = the base model.  GET /v1/adapters lists the names;
     an unknown name or a wrong type -> 400 with that list.  Rows with different adapters share one engine and one set of weights.)
    (extension: prompt prefix cache, `--prefix-cache-gb G` with `--continuous`: the K/V of a prompt's prefix -- through its last
     image slot, or the whole prompt -- is kept under an LRU byte budget and restored for later requests that start with the same
     tokens AND the same pictures (prefix.py).  "cache_prompt": false keeps a request's prompt out of the store (it may still
     reuse entries); responses gain "cached_tokens": [one per prompt]; GET /v1/prefix_cache returns the counters.  Without
     the flag none of this exists: no field in the response, 404 for the GET.)
    (extension: "speculate": K (0 .. 15; default: the server's `--speculate K`, default 0) -- speculative greedy decoding on the
     one-request path: K prompt-lookup draft tokens verified per decode step, the same text in fewer steps (api.speculative_loop).
     The response gains "speculation": {"steps", "drafted", "accepted"}.  One prompt, greedy, no image; an explicit K > 0 anywhere
     else -- a list of prompts, temperature > 0, a server started with --continuous or --merge -- is answered with 400.)
    (extension: "logprobs": N (0 .. 8; absent / null = off) -- every generated token's log-probability under the RAW logits (no
     temperature, no top-k, no top-p: the OpenAI / vLLM convention), its rank and the N most likely tokens at its position
     (include/p3v.h: p3v_logprob_t).  The response gains "logprobs": one object per prompt with the aligned lists "token_ids",
     "tokens" (the decoded pieces), "token_logprobs", "ranks" and "top_logprobs" (per token a list of {"id", "token", "logprob"});
     non-finite values travel as null.  A bool, a string or a value outside 0 .. 8 -> 400 naming the range; so does an explicit
     "speculate" > 0 next to it, and the batch-sharded path.  Merged requests keep their own N.)
    (extension: "repetition_penalty" (> 0; 1 = off; prompt and output, the HF / vLLM convention), "presence_penalty" and
     "frequency_penalty" (0 = off; output only) and "logit_bias": {"<token id>": bias} (string keys, as JSON has them; a bias of
     -Infinity -- or any value <= -1e30 -- bans the token) -- one setting per request, applied to every prompt of it: the rule
     of include/p3v.h (p3v_penalty_row_t) on each step's logits before temperature / top-k / top-p.  "logprobs" stay those of
     the raw logits.  A bad value -> 400 with the reason; so does an explicit "speculate" > 0 next to them, and the
     batch-sharded path.  Honoured on the one-request, the merged and the --continuous path; merged requests keep their own.)
    (extension: "guided_regex": a pattern (guide.py's subset), or "guided_choice": a non-empty list of strings -- one of them per
     request, applied to every prompt of it: the generated text up to EOS full-matches it (its UTF-8 bytes; a `▁` of a
     sentencepiece vocabulary counts as a space); "max_tokens" can still cut it short.  The guide is a byte-level DFA walked on
     the device (include/p3v.h: p3v_guide_row_t).  A bad type, an unsupported construct or more than 255 states -> 400 with the
     reason; so does an explicit "speculate" > 0 next to it, and the batch-sharded path.  Honoured on the one-request, the
     merged and the --continuous path; merged requests keep their own.
     "guided_json": a JSON schema (an object, or its JSON text) is the third kind and excludes the other two: the generated text
     is the JSON text of an instance, keys in declared order, at most one space after ':' and ',' (guide.json_regex names the
     keywords it translates and refuses).  The OpenAI form "response_format": {"type": "json_schema", "json_schema": {"schema":
     {...}}} means the same; {"type": "text"} is no guide; {"type": "json_object"} -> 400: free-form JSON is not a regular
     language, and the guide is a finite automaton of at most 65,536 table entries -- send a schema.  A refused keyword, or a
     schema whose automaton exceeds that bound -> 400 with the keyword, or with the state and class counts.)
    (extension: "n": 1 .. 16 completions of ONE prompt (a string), and "best_of": n .. 16 -- the prompt is prefilled once, its
     K/V forked into the other rows (include/p3v.h: p3v_kv_fork_t), and "responses" has n entries; "best_of" generates that many
     and returns the n with the largest cumulative raw-logit log-probability, best first.  A sampled request's "seeds" has
     one entry per response -- completion j of seed s runs under (s + j) mod 2^64 -- and posting a returned seed alone with
     "n": 1 reproduces its text; "logprobs" has one object per response.  At temperature 0 the n responses are equal.  A bad
     value, a list of prompts with n > 1, a server started with --merge, or an explicit "speculate" > 0 beside n > 1 -> 400
     with the reason.  Served by the one-request path and by --continuous; without "n" a response is byte for byte today's.)
    (extension: "num_beams": W (2 .. 8; 1 or absent: today's request) and "length_penalty": p (>= 0, default 1.0) -- beam
     search for ONE prompt (with or without an image) on the one-request path (api.generate(num_beams=...): include/p3v.h
     "beam search"); "responses" has the best hypothesis' text and the response gains "beam": {"score", "steps"}.  A bad
     value, a list of prompts, temperature > 0, an explicit "speculate" > 0, n / best_of, logprobs, penalties, logit_bias, a
     guide, an adapter, a server started with --continuous or --merge, or a process group -> 400 with the reason.)
    (extension: "images": [null | "data:image/...;base64,..." per prompt] -- the reference's endpoint is text-only.
     Only INLINE images by default: a path or URL in a request body would let any client make the server open local files
     or fetch arbitrary URLs.  `ImagePolicy(allow_dir=..., allow_hosts=...)` / `--image-dir` / `--image-host` opt in to an
     allow-listed directory / host list.  Images are always fetched AND decoded in the HTTP handler thread, with a timeout,
     a byte cap and a pixel cap -- never on the engine thread -- and errors never echo the path.)
    POST /v1/embeddings    {"input": str | [str, ...], "images": as above (with ONE input only), "pooling": "last" | "mean",
                            "normalize": bool, "adapter": as above, "encoding_format": "float" | "base64" (little-endian fp32)}
      -> 200 {"object": "list", "model": ..., "data": [{"object": "embedding", "index": i, "embedding": [...] | "..."}],
              "usage": {"prompt_tokens": n, "total_tokens": n}}
    (extension: the prompt as a vector, api.embed: one prefill that ends in p3v_embed_pool instead of lm_head; a list is one
     left-padded batch.  Runs on the engine thread in order with generation; under --continuous between two decode steps, on
     a state of its own.  A bad field -> 400 with the reason; behind a fleet, a regime router or a process group -> 400 naming
     that limit; a backend started without an embed function keeps answering 404.)

with one difference in the plumbing: requests do not call the model from the HTTP thread.  They go into a queue that a
single engine thread drains (the model object holds one in-flight sequence group).  By default every
request is its own `generate` call, as in the reference's server -- a client's output never depends on who else is in
flight.  `merge=True` (opt-in, `--merge`) folds requests that wait at the same time and ask for the same `max_tokens`
into ONE batched call: throughput for left-pad geometry that now depends on the longest co-batched prompt (results of
valid rows are pad-invariant EXCEPT the one-shot short/long RoPE choice, phi.py:492 -- so requests are only merged
while prompt + max_tokens of the merged batch stays on the same side of the 4096-token window as each request alone;
`regime_fn` supplies the prompt lengths).  `max_tokens` is clamped to `max_tokens_cap` (an unbounded value would size
the KV cache).  Malformed bodies get 400 instead of a dropped connection; a request that waits longer than `timeout_s`
gets 500.

`--continuous` replaces the queue by `engine.ContinuousEngine`: requests are prefilled into free batch rows between the
decode steps of the rows already generating and leave at their own EOS / budget (no request waits for a batch to drain).

Which keywords a request hands to a backend, to the engine and to a queued job is said once, by `in_use`; where an option cannot
run (under speculation, on the batch-sharded path), by the `REFUSALS` table; how a queued group becomes `api.generate` keywords,
by `generate_kwargs`.

    python -m phi_3_vision_mlx_amd.server --port 8000 [--synthetic] [--blind] [--merge | --continuous]
"""
import json
import queue
import os
import threading
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

MODEL_NAME = "phi-3-vision"


def in_use(sampling=None, adapter=None, logprobs=None, penalties=None, n=None, best_of=None, speculate=0, cache_prompt=None, info=None,
           guide=None, beam=None):
    """The keywords of the options a request really uses -- what the handler passes to a backend's `submit`, what
    ContinuousBackend passes to the engine's `generate`, and what a queued job keeps.  The rules, stated once:

      * a plain request passes no keyword at all (a backend that knows nothing of an option keeps serving plain requests);
        `images` is positional, and only when not None;
      * sampling, adapter, logprobs, penalties and guide are present only when not None;
      * n and best_of (both) are present only for a family -- m > 1 rows; the caller passes n=None otherwise;
      * speculate is present only when K > 0;
      * beam ({"num_beams": W, "length_penalty": p}) is present only for W > 1;
      * cache_prompt is present only when not None, and the handler passes it on only to a backend with a prefix store;
      * info (the dict a backend reports into) is present only when not None; the handler makes one exactly when the request is
        a family, asks for logprobs, speculates (K > 0), searches with beams, or the backend has a prefix store."""
    kw = {k: v for k, v in (("sampling", sampling), ("adapter", adapter), ("logprobs", logprobs), ("penalties", penalties),
                            ("cache_prompt", cache_prompt), ("info", info), ("guide", guide), ("beam", beam)) if v is not None}
    if n is not None:
        kw.update(n=n, best_of=best_of)
    if speculate:
        kw["speculate"] = speculate
    return kw


class _Job:
    __slots__ = ("prompts", "max_tokens", "images", "opts", "speculate", "info", "done", "result", "error")

    def __init__(self, prompts, max_tokens, images=None, opts=None, speculate=0, info=None):
        self.prompts, self.max_tokens, self.images = prompts, max_tokens, images
        self.opts = opts or {}                  # `in_use` of the request: per-prompt lists; n, best_of: a family (never merged)
        self.speculate, self.info = speculate, info             # draft rows per verify step (0 = off), the caller's statistics dict
        self.done, self.result, self.error = threading.Event(), None, None


SAMPLING_FIELDS = ("temperature", "top_k", "top_p", "seed")


class _EmbedJob:
    """One /v1/embeddings request on the queue: served by the worker thread, in order with generation."""

    def __init__(self, prompts, images, pooling, normalize, adapter):
        self.prompts, self.images, self.pooling, self.normalize, self.adapter = prompts, images, pooling, normalize, adapter
        self.done = threading.Event()
        self.result = None
        self.error = None


EMBED_NOT_BUILT = ("embeddings are not available on a fleet, a regime router (--long-window) or the batch-sharded path of a process "
                   "group: run one engine (--continuous without --long-window and WORLD_SIZE 1, or the queue server)")


def parse_embeddings(request):
    """The fields of a POST /v1/embeddings body, checked: (inputs, image specs or None, pooling, normalize, encoding)."""
    from .api import check_pooling
    inputs = request.get("input")
    inputs = [inputs] if isinstance(inputs, str) else inputs
    if not isinstance(inputs, list) or not inputs or not all(isinstance(p, str) for p in inputs):
        raise ValueError("input must be a string or a non-empty list of strings")
    images = request.get("images")
    if images is not None:
        images = [images] if isinstance(images, str) else list(images)
        if len(images) != len(inputs):
            raise ValueError("images must list one entry (or null) per input")
        if len(inputs) > 1 and any(i is not None for i in images):
            raise ValueError("Images cannot be provided when input is a list")
    pooling = check_pooling(request.get("pooling", "last"))
    normalize = request.get("normalize", True)
    if not isinstance(normalize, bool):
        raise ValueError("normalize must be true or false")
    encoding = request.get("encoding_format", "float")
    if encoding not in ("float", "base64"):
        raise ValueError(f"encoding_format must be 'float' or 'base64', got {encoding!r}")
    return inputs, images, pooling, normalize, encoding


def format_embeddings(vectors, n_tokens, encoding):
    """-> the response body: the OpenAI embeddings list ("base64": little-endian fp32)."""
    import base64
    import numpy as np
    rows = np.asarray(vectors, dtype="<f4")
    rows = rows[None] if rows.ndim == 1 else rows
    data = [{"object": "embedding", "index": i,
             "embedding": base64.b64encode(r.tobytes()).decode("ascii") if encoding == "base64" else [float(x) for x in r]}
            for i, r in enumerate(rows)]
    n = int(sum(n_tokens))
    return {"object": "list", "model": MODEL_NAME, "data": data, "usage": {"prompt_tokens": n, "total_tokens": n}}


def parse_sampling(request, n_prompts):
    """The sampling fields of a request body -> None (greedy: none given, or temperature 0) or one settings dict per prompt
    {"temperature", "top_k", "top_p", "seed"} with a concrete seed: the client's (row b of the request gets seed + b), or 64
    random bits drawn here, before the request is queued -- so its text does not depend on who shares its batch.  ValueError
    (-> 400) on a bad type or range, whether or not temperature is 0."""
    from .sampling import rows
    if not any(f in request for f in SAMPLING_FIELDS):
        return None
    t, k, p, seed = (request.get("temperature", 0.0), request.get("top_k", 0), request.get("top_p", 1.0), request.get("seed"))
    for name, v in (("temperature", t), ("top_k", k), ("top_p", p), ("seed", seed)):
        if isinstance(v, (list, tuple, dict)):
            raise ValueError(f"{name} must be a single value")
    recs = rows(n_prompts, t, k, p, seed)
    if recs[0][0] == 0.0:
        return None
    return [dict(temperature=r[0], top_k=r[1], top_p=r[2], seed=r[3]) for r in recs]


def known_adapters(engine):
    """Adapter names a backend serves: its `adapter_names` (a list, or a method returning one); [] when it has none."""
    names = getattr(engine, "adapter_names", None)
    return list((names() if callable(names) else names) or [])


def parse_adapter(request, n_prompts, known):
    """The "adapter" field of a request body -> None (absent, null, or null for every prompt: the base model) or one name / None per
    prompt.  ValueError (-> 400) naming the known adapters on a wrong type, a wrong count or an unknown name."""
    a = request.get("adapter")
    if a is None:
        return None
    hint = f"known adapters: {sorted(known)}"
    if isinstance(a, str):
        a = [a] * n_prompts
    elif isinstance(a, list):
        if len(a) != n_prompts:
            raise ValueError(f"adapter must be a name or list one name (or null) per prompt; {hint}")
    else:
        raise ValueError(f"adapter must be a string or a list of strings / nulls, got {type(a).__name__}; {hint}")
    for name in a:
        if name is not None and not isinstance(name, str):
            raise ValueError(f"adapter names are strings (or null), got {type(name).__name__}; {hint}")
        if name is not None and name not in known:
            raise ValueError(f"unknown adapter {name!r}; {hint}")
    return None if all(name is None for name in a) else a


SPECULATE_MAX = 15                              # P3V_DECODE_MAX_L - 1 draft rows


def parse_speculate(request, n_prompts, engine, sampling=None):
    """The "speculate" field of a request body -> K (0 = off; absent: the engine's `speculate_default`, the server's
    --speculate flag).  ValueError (-> 400) on a wrong type or range, and for K > 0 wherever speculative decoding does not run:
    a backend without it (the continuous engine, the merging queue), more than one prompt, a sampled request."""
    K = request.get("speculate", None)
    explicit = K is not None
    if not explicit:
        K = int(getattr(engine, "speculate_default", 0) or 0)
    if isinstance(K, bool) or not isinstance(K, int):
        raise ValueError(f"speculate must be an integer 0 .. {SPECULATE_MAX}, got {type(K).__name__}")
    if not 0 <= K <= SPECULATE_MAX:
        raise ValueError(f"speculate must be 0 .. {SPECULATE_MAX} (draft tokens per verify step), got {K}")
    if K == 0:
        return 0
    why = None
    if not getattr(engine, "speculate", False):
        why = ("speculative decoding runs on the one-request path only: this server was started with --continuous or --merge "
               "(per-row acceptance in the batched engine is not built)")
    elif n_prompts != 1:
        why = "speculative decoding takes one prompt per request (B = 1)"
    elif sampling is not None and any(float(r["temperature"]) > 0 for r in sampling):
        why = "speculative decoding is greedy only (temperature must be 0)"
    if why is None:
        return K
    if explicit:
        raise ValueError(why)
    return 0                                    # (the server-wide default applies where it can; only an explicit field is refused)


def parse_beam(request, prompts, images, engine, sampling=None, adapter=None, speculate_explicit=False, family=None, logprobs=None,
               penalties=None, guide=None):
    """The "num_beams" and "length_penalty" fields of a request body -> None (absent, or num_beams = 1: today's request) or
    {"num_beams": W, "length_penalty": p}.  ValueError (-> 400) naming the limit on a bad value, and for W > 1 wherever beam
    search does not run: a backend without it (--continuous, --merge), the batch-sharded path, and everything
    beam.check_request refuses (a list of prompts, sampling, an explicit "speculate" > 0, n / best_of, logprobs, penalties,
    a guide, an adapter)."""
    from .beam import check_request
    if request.get("num_beams") is None and request.get("length_penalty") is None:
        return None
    W, lp = check_request(request.get("num_beams", 1), request.get("length_penalty", 1.0))
    if W == 1:
        return None
    if not getattr(engine, "beam", False):
        raise ValueError(f"num_beams={W}: beam search runs on the one-request path only: this server was started with --continuous "
                         "or --merge (beams in the batched engine are not built)")
    check_request(W, lp, batched=len(prompts) != 1 or isinstance(request.get("prompt"), list),
                  sampled=sampling is not None and any(float(r["temperature"]) > 0 for r in sampling), speculate=speculate_explicit,
                  family=family is not None, logprobs=logprobs is not None, penalties=penalties is not None, guides=guide is not None,
                  adapter=adapter is not None)
    sharded = getattr(engine, "sharded_fn", None)                # (an image rides along, as a family's does: api.generate takes it)
    if sharded is not None and sharded(prompts, None):
        raise ValueError(f"num_beams={W}: beam search is not available{_SHARDED}")
    return {"num_beams": W, "length_penalty": lp}


def parse_logprobs(request, n_prompts):
    """The "logprobs" field of a request body -> None (absent or null: off) or [N] * n_prompts.  ValueError (-> 400) naming the
    range on a bool, a string, a list, or a value outside 0 .. 8."""
    from .logprobs import OFF, check
    v = request.get("logprobs")
    if isinstance(v, (list, tuple, dict)):
        raise ValueError(f"logprobs must be a single integer 0 .. 8 (or null), got {type(v).__name__}")
    want = check(v)
    return None if want == OFF else [want] * n_prompts


def parse_n(request, prompts, engine, speculate_explicit=False):
    """The "n" and "best_of" fields of a request body -> None (absent, or n = 1 without best_of > 1: today's request) or
    (n, best_of).  ValueError (-> 400) naming the limit on a bad type or range, and for more than one completion wherever a
    family does not run: a list of prompts, the merging queue, an explicit "speculate" > 0."""
    from .parallel import check, refusal
    if request.get("n") is None and request.get("best_of") is None:
        return None
    n, m = check(request.get("n", 1), request.get("best_of"))
    if m <= 1:
        return None
    why = refusal(m, batched=len(prompts) != 1 or isinstance(request.get("prompt"), list), speculate=speculate_explicit)
    if why is None and getattr(engine, "merge", False):
        why = "n > 1: not on a server started with --merge (a family is one prompt's rows, never merged with other requests)"
    if why is None:                                              # --share-prefix on a model whose cache the family launch does not read
        why = getattr(engine, "share_refusal", None)
    if why:
        raise ValueError(why)
    return n, request.get("best_of")


PENALTY_BAN = -1e30                             # a logit_bias at or below this bans the token (JSON has no -Infinity)


def vocab_of(engine):
    """The vocabulary size behind a backend (the bound of logit_bias keys), or None when it does not say."""
    from .engine import leaf_engines
    sizes = [getattr(engine, "vocab_size", None)] + [getattr(getattr(getattr(e, "model", None), "cfg", None), "vocab_size", None)
                                                     for e in leaf_engines(engine)]
    return next((int(v) for v in sizes if v is not None), None)


def parse_penalties(request, n_prompts, vocab=None):
    """The "repetition_penalty", "presence_penalty", "frequency_penalty" and "logit_bias" fields of a request body -> None (all
    absent, null or at their defaults) or one checked dict per prompt (the same for each).  ValueError (-> 400) with the reason
    (penalties.rows) on a value of the wrong type or range, a logit_bias that is no object, a key that is no token id below
    `vocab`, or a bias that is NaN or +inf."""
    from . import penalties as penalties_mod
    d = {k: request[k] for k in penalties_mod.FIELDS if request.get(k) is not None}
    if not d:
        return None
    lb = d.get("logit_bias")
    if lb is not None:
        if not isinstance(lb, dict):
            raise ValueError(f"logit_bias must be an object of token id -> bias, got {type(lb).__name__}")
        d["logit_bias"] = {k: (float("-inf") if isinstance(v, (int, float)) and not isinstance(v, bool) and v <= PENALTY_BAN else v)
                           for k, v in lb.items()}
    if penalties_mod.request_row(d, vocab) is None:
        return None
    return [d] * n_prompts


def _response_format_schema(fmt):
    """The OpenAI "response_format" field -> a JSON schema, or None for {"type": "text"}."""
    if not isinstance(fmt, dict) or not isinstance(fmt.get("type"), str):
        raise ValueError('response_format must be an object with a "type": "text" or "json_schema"')
    kind = fmt["type"]
    if kind == "text":
        return None
    if kind == "json_object":
        raise ValueError('response_format {"type": "json_object"} is not supported: free-form JSON is not a regular language, and '
                         'a guide is a finite automaton of at most 65536 table entries; send {"type": "json_schema", '
                         '"json_schema": {"schema": {...}}} or "guided_json"')
    if kind != "json_schema":
        raise ValueError(f'response_format type {kind!r} is not supported: "text" or "json_schema"')
    inner = fmt.get("json_schema")
    if not isinstance(inner, dict) or not isinstance(inner.get("schema"), (dict, str)):
        raise ValueError('response_format {"type": "json_schema"} needs "json_schema": {"schema": {...}}')
    return inner["schema"]


def parse_guide(request, n_prompts):
    """The "guided_regex" (a string), "guided_choice" (a non-empty list of strings) and "guided_json" (a JSON schema: an object
    or its JSON text; also as the OpenAI "response_format" of type "json_schema") fields of a request body -> None (all absent or
    null) or one {"regex": pattern} / {"choice": [...]} / {"schema": ...} dict per prompt (the same for each).  ValueError (->
    400) with the reason on a wrong type, two at once, an unsupported construct or keyword, more than 255 states of a pattern or
    more than 65,536 table entries of a schema: the guide is compiled here (the compiled form is cached, so the backend's own
    compilation is a look-up)."""
    from . import guide as guide_mod
    regex, choice, schema = request.get("guided_regex"), request.get("guided_choice"), request.get("guided_json")
    if request.get("response_format") is not None:
        fmt = _response_format_schema(request["response_format"])
        if fmt is not None and schema is not None:
            raise ValueError("guided_json and response_format exclude each other: send one")
        schema = fmt if schema is None else schema
    if regex is None and choice is None and schema is None:
        return None
    if regex is not None and choice is not None:
        raise ValueError("guided_regex and guided_choice exclude each other: send one")
    if schema is not None and (regex is not None or choice is not None):
        raise ValueError(f"{'guided_regex' if regex is not None else 'guided_choice'} and guided_json exclude each other: send one")
    if regex is not None and not isinstance(regex, str):
        raise ValueError(f"guided_regex must be a string, got {type(regex).__name__}")
    if choice is not None and (not isinstance(choice, list) or not choice or not all(isinstance(c, str) for c in choice)):
        raise ValueError("guided_choice must be a non-empty list of strings")
    if schema is not None and not isinstance(schema, (dict, str)):
        raise ValueError(f"guided_json must be a JSON schema (an object or its JSON text), got {type(schema).__name__}")
    d = {"regex": regex} if regex is not None else {"choice": list(choice)} if choice is not None else {"schema": schema}
    guide_mod.request_guide(d)
    return [d] * n_prompts


def token_decoder(engine):
    """id -> text piece for the "tokens" of a logprobs response: the backend's `decode_fn`, or its tokenizer; None without one."""
    from .engine import leaf_engines
    fn = getattr(engine, "decode_fn", None)
    if fn is not None:
        return fn
    tok = getattr(getattr(next(leaf_engines(engine)), "processor", None), "tokenizer", None)
    return None if tok is None else (lambda i: tok.decode([int(i)]))


def format_logprobs(entry, decode=None, eos_id=None):
    """One prompt's logprobs.entry (or None) -> the response object: lists cut behind the first `eos_id` (where the text ends),
    decoded pieces beside the ids, null for every non-finite value."""
    from .logprobs import finite_or_none
    if entry is None:
        return None
    ids = list(entry["token_ids"])
    n = ids.index(eos_id) + 1 if eos_id is not None and eos_id in ids else len(ids)

    def piece(i):
        return decode(i) if decode is not None and i >= 0 else None
    return {"token_ids": ids[:n], "tokens": [piece(i) for i in ids[:n]],
            "token_logprobs": [finite_or_none(x) for x in entry["token_logprobs"][:n]],
            "ranks": list(entry["ranks"][:n]),
            "top_logprobs": [[{"id": i, "token": piece(i), "logprob": finite_or_none(lp)} for i, lp in top]
                             for top in entry["top_logprobs"][:n]]}


def parse_cache_prompt(request):
    """The "cache_prompt" field of a request body -> None (absent or true: the default) or False.  ValueError (-> 400) on a
    value that is not a boolean."""
    v = request.get("cache_prompt", True)
    if not isinstance(v, bool):
        raise ValueError(f"cache_prompt must be true or false, got {type(v).__name__}")
    return None if v else False


def prefix_counters(engine):
    """Counters of the prefix store(s) behind a backend (summed over the engines of a router), or None when it has none."""
    fn = getattr(engine, "prefix_counters", None)
    return fn() if callable(fn) else None


class ImagePolicy:
    """What the `images` field of a request may name.  Default: inline `data:` URIs only."""

    def __init__(self, allow_dir=None, allow_hosts=(), max_bytes=16 << 20, max_pixels=64 << 20, timeout_s=5.0):
        import os
        self.allow_dir = os.path.realpath(allow_dir) if allow_dir else None
        self.allow_hosts = frozenset(h.lower() for h in allow_hosts)
        self.max_bytes, self.max_pixels, self.timeout_s = int(max_bytes), int(max_pixels), float(timeout_s)


def _open_image(raw, policy):
    """bytes -> a fully decoded RGB PIL image (decoded HERE, in the caller's thread), under the policy's caps."""
    from io import BytesIO
    from PIL import Image
    if len(raw) > policy.max_bytes:
        raise ValueError("image larger than the server's byte limit")
    try:
        im = Image.open(BytesIO(raw))
        if im.width * im.height > policy.max_pixels:
            raise ValueError("image larger than the server's pixel limit")
        im.load()
        return im.convert("RGB")
    except ValueError:
        raise
    except Exception:                           # noqa: BLE001 -- PIL raises many types; none of them is the client's business
        raise ValueError("image could not be decoded") from None


def decode_image(spec, policy=None):
    """One entry of a request's `images` list -> None or a decoded PIL image.  ValueError (-> HTTP 400) for anything the
    policy does not allow; messages never contain the path / URL (no file-existence oracle)."""
    policy = policy or ImagePolicy()
    if spec is None:
        return None
    if not isinstance(spec, str):
        raise ValueError("images entries must be null or strings")
    if spec.startswith("data:"):
        import base64
        import binascii
        head, _, payload = spec.partition(",")
        if not head.endswith(";base64") or len(payload) > policy.max_bytes * 4 // 3 + 4:
            raise ValueError("images: expected a base64 data URI within the size limit")
        try:
            raw = base64.b64decode(payload, validate=True)
        except (binascii.Error, ValueError):
            raise ValueError("images: invalid base64 payload") from None
        return _open_image(raw, policy)
    if spec.startswith(("http://", "https://")):
        from urllib.parse import urlsplit
        host = (urlsplit(spec).hostname or "").lower()
        if host not in policy.allow_hosts:
            raise ValueError("images: URLs are not accepted by this server (inline data: URIs only)")
        import requests
        try:
            with requests.get(spec, stream=True, timeout=policy.timeout_s, allow_redirects=False) as resp:
                resp.raise_for_status()
                raw = resp.raw.read(policy.max_bytes + 1, decode_content=True)
        except Exception:                       # noqa: BLE001
            raise ValueError("images: fetch failed") from None
        return _open_image(raw, policy)
    if policy.allow_dir is None:
        raise ValueError("images: file paths are not accepted by this server (inline data: URIs only)")
    import os
    path = os.path.realpath(os.path.join(policy.allow_dir, spec))
    if os.path.commonpath([path, policy.allow_dir]) != policy.allow_dir or not os.path.isfile(path):
        raise ValueError("images: not an image of the served directory")
    if os.path.getsize(path) > policy.max_bytes:
        raise ValueError("image larger than the server's byte limit")
    with open(path, "rb") as f:
        return _open_image(f.read(), policy)


class EngineQueue:
    """Single consumer in front of a non-re-entrant `generate_fn(prompts: list[str], max_tokens) -> str | list[str]`."""

    def __init__(self, generate_fn, max_batch=64, window_s=0.005, merge=False, max_tokens_cap=4096, timeout_s=600.0,
                 length_fn=None, window_tokens=4096, device=None, sharded_fn=None, adapter_names=(), speculate=False,
                 speculate_default=0, decode_fn=None, vocab_size=None, share_refusal=None, embed_fn=None, embed_refusal=None, beam=False):
        # embed_fn(prompts, images, pooling, normalize, adapter) -> (vectors [n, H], prompt tokens per prompt): /v1/embeddings, run
        # by the worker thread in order with generation; None: the path does not exist (404).  embed_refusal: why it cannot be
        # served here (-> 400), or None
        self.embed_fn, self.embed_refusal = embed_fn, embed_refusal
        self.embed = self._embed if embed_fn is not None else None
        self.share_refusal = share_refusal                      # --share-prefix: why a family cannot share its prefix here (-> 400), or None
        self.vocab_size = vocab_size                            # bound of a request's logit_bias keys (None: checked by generate_fn)
        self.decode_fn = decode_fn                              # token id -> text piece (the "tokens" of a logprobs response)
        # speculate: generate_fn takes `speculate=K, spec_info=dict` (one prompt, greedy); never with merge (B > 1 batches)
        self.speculate, self.speculate_default = bool(speculate) and not merge, int(speculate_default)
        self.beam = bool(beam) and not merge                    # generate_fn takes `beam={...}, beam_info=dict` (one prompt); never merged
        self.adapter_names = list(adapter_names)                # what generate_fn's `adapter` keyword may name (GET /v1/adapters)
        # sharded_fn(prompts, images) -> True when generate_fn would run that request on the batch-sharded path (dist.py), which
        # does not sample: the handler answers 400 to a sampled request bound there
        self.sharded_fn = sharded_fn
        self.generate_fn, self.max_batch, self.window_s = generate_fn, max_batch, window_s
        self.merge, self.max_tokens_cap, self.timeout_s = merge, max_tokens_cap, timeout_s
        self.length_fn, self.window_tokens, self.device = length_fn, window_tokens, device
        self.jobs = queue.Queue()
        self.batches = []                       # sizes of the generate calls issued (observability / tests)
        self._stop = False
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def submit(self, prompts, max_tokens, images=None, sampling=None, adapter=None, speculate=0, info=None, logprobs=None,
               penalties=None, n=None, best_of=None, guide=None, beam=None):
        job = _Job(prompts, max(1, min(int(max_tokens), self.max_tokens_cap)), images,
                   in_use(sampling, adapter, logprobs, penalties, n, best_of, guide=guide, beam=beam), speculate, info)
        self.jobs.put(job)
        if not job.done.wait(self.timeout_s):
            raise TimeoutError(f"no result within {self.timeout_s} s")
        if job.error is not None:
            raise job.error
        return job.result

    def _embed(self, prompts, images=None, pooling="last", normalize=True, adapter=None):
        job = _EmbedJob(prompts, images, pooling, normalize, adapter)
        self.jobs.put(job)
        if not job.done.wait(self.timeout_s):
            raise TimeoutError(f"no result within {self.timeout_s} s")
        if job.error is not None:
            raise job.error
        return job.result

    def close(self):
        self._stop = True
        self.jobs.put(None)
        self.thread.join(timeout=5)

    def _regime(self, prompts, max_tokens):
        """Side of the RoPE window the batch falls on (phi.py:492: long factors iff longest prompt + max_tokens > 4096)."""
        if self.length_fn is None:
            return None
        return max(self.length_fn(p) for p in prompts) + max_tokens > self.window_tokens

    def _collect(self, first):
        """merge=False: `first` alone.  merge=True: plus every queued job with the same max_tokens that fits and keeps the
        RoPE regime of each member unchanged, waiting at most `window_s` for stragglers."""
        def alone(job):                         # image / adapter requests and families are never merged
            return job.images is not None or "adapter" in job.opts or "n" in job.opts or "beam" in job.opts
        group, n, held = [first], len(first.prompts), []
        if not self.merge or alone(first):
            return group
        regime = self._regime(first.prompts, first.max_tokens)
        while n < self.max_batch:
            try:
                job = self.jobs.get(timeout=self.window_s)
            except queue.Empty:
                break
            if job is None:
                self.jobs.put(None)
                break
            if isinstance(job, _EmbedJob):      # keeps its place behind this group
                held.append(job)
                continue
            if not alone(job) and job.max_tokens == first.max_tokens and n + len(job.prompts) <= self.max_batch \
                    and self._regime(job.prompts, job.max_tokens) == regime and ("sampling" in job.opts) == ("sampling" in first.opts):
                group.append(job)
                n += len(job.prompts)
            else:
                held.append(job)
        for job in held:                        # different budget: next round, order kept
            self.jobs.put(job)
        return group

    def _run(self):
        if self.device is not None:                             # a new thread starts on GPU 0 whatever the loader used
            import torch
            torch.cuda.set_device(self.device)
        while not self._stop:
            first = self.jobs.get()
            if first is None:
                break
            if isinstance(first, _EmbedJob):
                try:
                    first.result = self.embed_fn(first.prompts, first.images, first.pooling, first.normalize, first.adapter)
                except Exception as e:          # noqa: BLE001 -- reported to the waiting request
                    first.error = e
                first.done.set()
                continue
            group = self._collect(first)
            flat = [p for j in group for p in j.prompts]
            try:
                # ONE call for the group.  `images` is positional unless the call is plain (no keyword, no image: a plain
                # `generate_fn(prompts, max_tokens)` keeps serving plain requests).  adapter, n, best_of: the first job's (such jobs
                # are never merged).  logprobs / penalties / sampling: one value per row of the group, None for the rows of a job
                # that did not ask (sampled jobs merge only with sampled jobs).  Each statistics dict comes in with what fills it;
                # speculate: one greedy prompt, never a family, never merged (self.speculate excludes merge).
                opts, fam = first.opts, "n" in first.opts
                beam = opts.get("beam")
                spec = 0 if fam or beam else first.speculate
                kw = {k: opts[k] for k in ("adapter", "n", "best_of") if k in opts}
                for k in ("logprobs", "penalties", "guide") + (() if spec else ("sampling",)):
                    if any(k in j.opts for j in group):
                        kw[k] = [v for j in group for v in (j.opts.get(k) or [None] * len(j.prompts))]
                lp_info, fam_info, stats, beam_info = {}, {}, {}, {}
                if beam:
                    kw.update(beam=beam, beam_info=beam_info)
                if "logprobs" in kw:
                    kw["logprob_info"] = lp_info
                if fam:
                    kw["family_info"] = fam_info
                if spec:
                    kw.update(speculate=spec, spec_info=stats)
                out = self.generate_fn(flat, first.max_tokens, *([first.images] if kw or first.images is not None else []), **kw)
                if fam:                                         # ONE prompt, n texts back (one prefill, forked)
                    if first.info is not None and "sampling" in opts:
                        first.info["seeds"] = [int(x) for x in fam_info.get("seeds", [])]
                    out = [out] if isinstance(out, str) else list(out)
                    if len(out) != opts["n"]:
                        raise RuntimeError(f"generate returned {len(out)} texts for n = {opts['n']}")
                    flat = out                                  # (one result per completion from here on)
                if beam and first.info is not None:
                    best = (beam_info.get("hypotheses") or [{}])[0]
                    first.info["beam"] = {"score": best.get("score"), "steps": int(beam_info.get("steps", 0))}
                if spec and first.info is not None:
                    first.info["speculation"] = {k: int(stats.get(k, 0)) for k in ("steps", "drafted", "accepted")}
                out = [out] if isinstance(out, str) else list(out)
                if len(out) != len(flat):
                    raise RuntimeError(f"generate returned {len(out)} texts for {len(flat)} prompts")
                self.batches.append(len(flat))
                i = 0
                for j in group:
                    k = j.opts.get("n", len(j.prompts))          # (a family: its one prompt has n results)
                    j.result = out[i:i + k]
                    if "logprobs" in j.opts and j.info is not None:
                        j.info["logprobs"] = [None if lp_info["token_ids"][b] is None else {k_: lp_info[k_][b] for k_ in lp_info}
                                              for b in range(i, i + k)]
                    i += k
            except Exception as e:              # noqa: BLE001 -- reported to every waiting request
                for j in group:
                    j.error = e
            for j in group:
                j.done.set()


# Where an option cannot run, in the order it is checked: (option present, where -- "speculate": the request speculates (K > 0),
# "sharded": it is bound for the batch-sharded path --, the 400's text, refused only for an explicit "speculate" field?).  Where only
# the explicit field is refused, a server-wide --speculate default steps aside silently (speculate becomes 0).
_SHARDED = " on the batch-sharded path (image requests and process groups of the queue server)"
REFUSALS = (
    ("penalties", "speculate", "penalties and logit_bias are not available under speculative decoding (a verify step scores several "
     "tokens per replay against one table); send speculate 0", True),
    ("penalties", "sharded", f"penalties and logit_bias are not available{_SHARDED}; run the server with --continuous, or send none", False),
    ("guide", "speculate", "guided decoding is not available under speculative decoding (a verify step scores several tokens per "
     "replay against one guide state); send speculate 0", True),
    ("guide", "sharded", f"guided decoding is not available{_SHARDED}; run the server with --continuous, or send no guide", False),
    ("logprobs", "speculate", "logprobs are not available under speculative decoding (a verify step emits several tokens per replay); "
     "send speculate 0", True),
    ("logprobs", "sharded", f"logprobs are not available{_SHARDED}; run the server with --continuous, or send no logprobs", False),
    ("speculate", "sharded", f"speculative decoding is not available{_SHARDED}", True),
    ("sampling", "sharded", f"sampling is not available{_SHARDED}; run the server with --continuous to sample, or send temperature 0", False),
    ("adapter", "sharded", f"adapters are not available{_SHARDED}; run the server with --continuous, or send no adapter", False),
)


def make_handler(engine, image_policy=None):
    image_policy = image_policy or ImagePolicy()

    class CompletionHandler(BaseHTTPRequestHandler):
        def _send(self, code, payload):
            body = json.dumps(payload).encode("utf-8")
            self.send_response(code)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def do_GET(self):
            if self.path == "/v1/prefix_cache" and prefix_counters(engine) is not None:
                self._send(200, {"model": MODEL_NAME, "prefix_cache": prefix_counters(engine)})
                return
            if self.path != "/v1/adapters":
                self.send_error(404, "Not Found")
                return
            self._send(200, {"model": MODEL_NAME, "adapters": known_adapters(engine)})

        def _embeddings(self):
            try:
                request = json.loads(self.rfile.read(int(self.headers.get("Content-Length", 0))).decode("utf-8"))
                refusal = getattr(engine, "embed_refusal", None)
                if refusal:
                    raise ValueError(refusal)
                inputs, images, pooling, normalize, encoding = parse_embeddings(request)
                if images is not None:
                    images = [decode_image(i, image_policy) for i in images]          # fetched + decoded in THIS thread
                    images = None if all(i is None for i in images) else images
                adapter = parse_adapter(request, len(inputs), known_adapters(engine))
            except (ValueError, TypeError, AttributeError, OSError) as e:
                self._send(400, {"error": str(e)})
                return
            try:
                vectors, n_tokens = engine.embed(inputs, images, pooling, normalize, adapter)
            except ValueError as e:             # (a prompt beyond the engine's window, ...)
                self._send(400, {"error": str(e)})
                return
            except Exception as e:              # noqa: BLE001
                self._send(500, {"error": f"{type(e).__name__}: {e}"})
                return
            self._send(200, format_embeddings(vectors, n_tokens, encoding))

        def do_POST(self):
            if self.path == "/v1/embeddings" and (getattr(engine, "embed", None) is not None or getattr(engine, "embed_refusal", None)):
                self._embeddings()
                return
            if self.path != "/v1/completions":
                self.send_error(404, "Not Found")
                return
            try:
                request = json.loads(self.rfile.read(int(self.headers.get("Content-Length", 0))).decode("utf-8"))
                prompts = request.get("prompt", "")
                max_tokens = int(request.get("max_tokens", 512))
                prompts = [prompts] if isinstance(prompts, str) else list(prompts)
                if not prompts or not all(isinstance(p, str) for p in prompts):
                    raise ValueError("prompt must be a string or a list of strings")
                images = request.get("images")
                if images is not None:
                    images = [images] if isinstance(images, str) else list(images)
                    if len(images) != len(prompts):
                        raise ValueError("images must list one entry (or null) per prompt")
                    images = [decode_image(i, image_policy) for i in images]      # fetched + decoded in THIS thread
                    images = None if all(i is None for i in images) else images
                sampling = parse_sampling(request, len(prompts))
                adapter = parse_adapter(request, len(prompts), known_adapters(engine))
                cache_prompt = parse_cache_prompt(request)
                speculate = parse_speculate(request, len(prompts), engine, sampling)
                family = parse_n(request, prompts, engine, bool(speculate) and "speculate" in request)
                if family is not None:
                    speculate = 0                               # (the server-wide default steps aside)
                logprobs = parse_logprobs(request, len(prompts))
                penalties = parse_penalties(request, len(prompts), vocab_of(engine))
                guide = parse_guide(request, len(prompts))
                beam = parse_beam(request, prompts, images, engine, sampling, adapter, bool(speculate) and "speculate" in request, family,
                                  logprobs, penalties, guide)
                if beam is not None:
                    speculate = 0                               # (the server-wide default steps aside)
                sharded = None if family is not None else getattr(engine, "sharded_fn", None)   # (a family runs api.generate, images too)
                asked = {"sampling": sampling, "adapter": adapter, "logprobs": logprobs, "penalties": penalties, "guide": guide}
                for option, where, message, explicit_only in REFUSALS:      # in order: the first that fails answers
                    present = speculate if option == "speculate" else asked[option] is not None
                    if not present or not (speculate if where == "speculate" else sharded is not None and sharded(prompts, images)):
                        continue
                    if not explicit_only or "speculate" in request:
                        raise ValueError(message)
                    speculate = 0                               # (the server-wide default steps aside)
            except (ValueError, TypeError, AttributeError, OSError) as e:
                self._send(400, {"error": str(e)})
                return
            store = prefix_counters(engine) is not None         # a backend with a prefix store reports what each prompt reused
            info = {} if family is not None or logprobs is not None or speculate or store or beam is not None else None
            try:
                kw = in_use(sampling, adapter, logprobs, penalties, *(family or (None, None)), speculate, cache_prompt if store else None, info,
                            guide=guide, beam=beam)
                responses = engine.submit(prompts, max_tokens, *([images] if images is not None else []), **kw)
            except Exception as e:              # noqa: BLE001
                self._send(500, {"error": f"{type(e).__name__}: {e}"})
                return
            out = {"model": MODEL_NAME, "responses": responses}
            if sampling is not None:
                out["seeds"] = [r["seed"] for r in sampling] if family is None else list(info.get("seeds", []))
            if beam is not None:
                from .logprobs import finite_or_none
                got = info.get("beam") or {}
                out["beam"] = {"score": finite_or_none(got.get("score")), "steps": int(got.get("steps", 0))}
            if speculate:
                out["speculation"] = info.get("speculation", {"steps": 0, "drafted": 0, "accepted": 0})
            elif info is not None and (prefix_counters(engine) is not None or (logprobs is None and family is None and beam is None)):
                out["cached_tokens"] = list(info.get("cached_tokens", [0] * len(prompts)))
            if logprobs is not None:
                from .api import ID_EOS
                decode = token_decoder(engine)
                out["logprobs"] = [format_logprobs(e, decode, ID_EOS) for e in info.get("logprobs") or [None] * len(responses)]
            self._send(200, out)

        def log_message(self, *args):           # quiet
            pass

    return CompletionHandler


def serve(generate_fn, port=8000, host="127.0.0.1", max_batch=64, image_policy=None, embed_fn=None, **engine_kwargs):
    """-> (httpd, engine); call httpd.serve_forever() (or run it in a thread) and engine.close() at the end.
    Binds the loopback interface unless told otherwise (`host=""` = all interfaces, as the reference's server.py:31).
    embed_fn(prompts, images, pooling, normalize, adapter) -> (vectors, prompt tokens per prompt) serves POST /v1/embeddings on
    the queue's worker thread; without it that path is a 404."""
    engine = EngineQueue(generate_fn, max_batch=max_batch, embed_fn=embed_fn, **engine_kwargs)
    httpd = ThreadingHTTPServer((host, port), make_handler(engine, image_policy))
    return httpd, engine


class ContinuousBackend:
    """The handler's `submit` on top of engine.ContinuousEngine (its own stepping thread)."""

    def __init__(self, engine, max_tokens_cap=4096, timeout_s=600.0):
        self.engine, self.max_tokens_cap, self.timeout_s = engine, max_tokens_cap, timeout_s
        self.stop = threading.Event()
        self.thread = threading.Thread(target=engine.serve_forever, args=(self.stop,), daemon=True)
        self.thread.start()

    def adapter_names(self):
        return known_adapters(self.engine)

    def _stores(self):
        from .engine import leaf_engines
        return [e.prefix_cache for e in leaf_engines(self.engine) if getattr(e, "prefix_cache", None) is not None]

    @property
    def prefix_counters(self):
        """None without a store; else a callable -> the counters, summed over the engines' stores."""
        stores = self._stores()
        if not stores:
            return None

        def counters():
            out = {}
            for s in stores:
                for k, v in s.counters().items():
                    out[k] = v if k == "min_tokens" else out.get(k, 0) + v
            return out
        return counters

    def submit(self, prompts, max_tokens, images=None, sampling=None, adapter=None, cache_prompt=None, info=None, logprobs=None,
               penalties=None, n=None, best_of=None, guide=None):
        kw = in_use(sampling, adapter, logprobs, penalties, n, best_of, 0, cache_prompt, info, guide=guide)
        if "n" in kw and not isinstance(prompts, str) and len(prompts) == 1:
            prompts = prompts[0]                                 # a family: one prompt (a string for the engine), n texts back
        return self.engine.generate(prompts, images, max(1, min(int(max_tokens), self.max_tokens_cap)), self.timeout_s, **kw)

    @property
    def embed_refusal(self):
        """Why /v1/embeddings cannot be served here (a router or a fleet in front: -> 400), or None."""
        in_front = hasattr(self.engine, "engines") or hasattr(self.engine, "engine")      # RegimeRouter / fleet.EngineFleet
        return EMBED_NOT_BUILT if in_front and not hasattr(self.engine, "embed") else None

    @property
    def embed(self):
        """None where the engine has no `embed` (-> 404, or 400 with `embed_refusal`)."""
        return self._embed if hasattr(self.engine, "embed") else None

    def _embed(self, prompts, images=None, pooling="last", normalize=True, adapter=None):
        from .api import _apply_chat_template, prompt_token_counts
        single = len(prompts) == 1
        text, imgs = _apply_chat_template(prompts[0] if single else list(prompts), images[0] if single and images is not None else None, False)
        inputs = self.engine.processor(text, imgs)
        job = self.engine.embed(inputs, pooling, normalize, None if adapter is None else (adapter[0] if single else list(adapter)))
        if not job.done.wait(self.timeout_s):
            job.cancel()
            raise TimeoutError(f"no result within {self.timeout_s} s")
        if job.error is not None:
            raise job.error
        return job.result, prompt_token_counts(inputs)

    def close(self):
        self.stop.set()
        self.thread.join(timeout=5)


def serve_continuous(engine, port=8000, host="127.0.0.1", image_policy=None, **kw):
    backend = ContinuousBackend(engine, **kw)
    return ThreadingHTTPServer((host, port), make_handler(backend, image_policy)), backend


def generate_kwargs(sampling, adapter, logprobs, penalties, n, best_of, speculate, n_prompts, guide=None):
    """The per-row lists a queued group carries (EngineQueue._run) -> the keywords of `api.generate` for them.  A family (n is
    not None: one prompt) takes scalars -- its sampling record's fields, the penalty fields it gave, its N, its adapter --, n and
    best_of.  A speculating request (one greedy prompt) takes `speculate` and its adapter.  Any other request takes one value per
    row (a single prompt: its adapter as a name), a row that asked for no penalty the defaults.  guide: the rows' {"regex"} /
    {"choice"} / {"schema"} dicts (None for a row without one) -> `guided_regex` / `guided_choice` / `guided_json`, one value per row."""
    fam = n is not None
    if speculate and not fam:
        sampling = logprobs = penalties = guide = None
    kw = {}
    if guide is not None and any(d is not None for d in guide):
        for f, name in (("regex", "guided_regex"), ("choice", "guided_choice"), ("schema", "guided_json")):
            vals = [None if d is None else d.get(f) for d in guide]
            if any(v is not None for v in vals):
                kw[name] = vals[0] if fam else vals
    if sampling is not None:
        kw.update({f: sampling[0][f] if fam else [r[f] for r in sampling] for f in SAMPLING_FIELDS})
    if penalties is not None and fam:
        kw.update({f: v for f, v in (penalties[0] or {}).items() if v is not None})
    elif penalties is not None:
        for f, dflt in (("repetition_penalty", 1.0), ("presence_penalty", 0.0), ("frequency_penalty", 0.0), ("logit_bias", None)):
            kw[f] = [dflt if d is None or d.get(f) is None else d[f] for d in penalties]
    if logprobs is not None:
        kw["logprobs"] = logprobs[0] if fam else logprobs
    if adapter is not None:
        kw["adapter"] = adapter if n_prompts > 1 else adapter[0]
    if fam:
        kw.update(n=n, best_of=best_of)
    elif speculate:
        kw["speculate"] = speculate
    return kw


def run(port=8000, synthetic=False, blind_model=False, merge=False, continuous=False, host="127.0.0.1", image_policy=None,
        long_window=0, slots=8, adapters=None, prefix_cache_gb=0.0, speculate=0, share_prefix=False):
    """adapters: {name: adapter directory} -- the server's adapter bank (every rank of a fleet loads the same one).
    prefix_cache_gb (with continuous): byte budget of the prompt prefix store of EACH engine (0 = off).
    share_prefix: the rows of an "n" > 1 request read their prompt's K/V once per decode step (engine.ContinuousEngine /
    api.generate: share_prefix); every rank of a fleet builds its engine from the same flag.  No request field, same responses."""
    from .api import _apply_chat_template, embed, generate, load, load_adapters
    preload = load(blind_model=blind_model, synthetic=synthetic or None)
    if adapters:
        load_adapters(preload, adapters)
    processor = preload[1]
    preload[0].serving = True            # a server does not own the GPU: no launch that needs its whole grid resident at once (model.py)
    if continuous:
        import torch.distributed as dist
        from .engine import ContinuousEngine, RegimeRouter
        def store():                                                 # one store per engine: its key carries the engine's regime
            if prefix_cache_gb <= 0:
                return {}
            from .prefix import PrefixCache
            return {"prefix_cache": PrefixCache(int(prefix_cache_gb * (1 << 30)))}
        share = {"share_prefix": True} if share_prefix else {}       # (off: the engines are built exactly as without the flag)
        eng = ContinuousEngine(*preload, slots=slots, **store(), **share)   # requests with prompt + max_tokens <= 4096 (short RoPE factors)
        if long_window > 4096:                                       # + one engine for the long-RoPE regime (phi.py:492)
            eng = RegimeRouter([eng, ContinuousEngine(*preload, slots=max(1, slots // 2), window=long_window, **store(), **share)])
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        front = None
        if world > 1:                                                # one engine per rank (= per GPU), rank 0 dispatches (fleet.py)
            from . import fleet
            groups = fleet.make_groups()
            if dist.get_rank() != 0:
                fleet.worker(eng, groups)
                return
            eng = front = fleet.EngineFleet(eng, groups, world)
        httpd, engine = serve_continuous(eng, port=port, host=host, image_policy=image_policy)
        print(f"Starting server on port {port} (continuous batching{f', {world} engines' if world > 1 else ''})")
        try:
            httpd.serve_forever()
        finally:
            engine.close()
            if front is not None:
                front.close()
        return

    def sharded_fn(prompts, images):
        import torch.distributed as dist
        return images is not None or (dist.is_available() and dist.is_initialized())

    def generate_fn(prompts, max_tokens, images=None, sampling=None, adapter=None, speculate=0, spec_info=None, logprobs=None,
                    logprob_info=None, penalties=None, n=None, best_of=None, family_info=None, guide=None, beam=None, beam_info=None):
        import torch.distributed as dist
        kw = generate_kwargs(sampling, adapter, logprobs, penalties, n, best_of, speculate, len(prompts), guide)
        if beam:                                                     # one prompt (image or not), one prefill forked into the beams
            kw.update(beam, beam_info=beam_info, images=None if images is None else images[0],
                      **({"share_prefix": True} if share_prefix else {}))
        if "logprobs" in kw:
            kw["logprob_info"] = logprob_info
        if "speculate" in kw:
            kw["spec_info"] = spec_info
        if n is not None:                                            # a family: one prompt (image or not), prefilled once, n texts
            kw.update(images=None if images is None else images[0], family_info=family_info, **({"share_prefix": True} if share_prefix else {}))
        elif not kw and (images is not None or (dist.is_available() and dist.is_initialized() and len(prompts) > 1)):
            # mixed image + text requests -- and text-only batches whenever a process group exists -- go through the
            # batch-sharded path (dist.py: one left-padded batch per rank; world size 1 = this GPU alone); the handler kept
            # every request with an option off it
            from .dist import generate_sharded
            return generate_sharded(prompts, images if images is not None else [None] * len(prompts), preload=preload,
                                    max_tokens=max_tokens)
        return generate(prompts if len(prompts) > 1 else prompts[0], preload=preload, max_tokens=max_tokens, verbose=False, **kw)

    def length_fn(prompt):
        return len(processor.tokenizer(_apply_chat_template(prompt, None, False)[0]).input_ids)

    def embed_fn(prompts, images=None, pooling="last", normalize=True, adapter=None):
        info, single = {}, len(prompts) == 1
        out = embed(prompts[0] if single else prompts, images[0] if single and images is not None else None, preload=preload,
                    pooling=pooling, normalize=normalize, adapter=None if adapter is None else (adapter[0] if single else adapter), info=info)
        return out, info["prompt_tokens"]

    import torch.distributed as dist
    grouped = dist.is_available() and dist.is_initialized()          # a process group: batches go down the batch-sharded path
    httpd, engine = serve(generate_fn, embed_fn=embed_fn, **({"embed_refusal": EMBED_NOT_BUILT} if grouped else {}),
                          port=port, host=host, merge=merge, length_fn=length_fn, device=preload[0].device,
                          image_policy=image_policy, sharded_fn=sharded_fn, adapter_names=list(adapters or {}), speculate=True, beam=True,
                          speculate_default=speculate, decode_fn=lambda i: processor.tokenizer.decode([int(i)]),
                          vocab_size=getattr(getattr(preload[0], "cfg", None), "vocab_size", None),
                          **({"share_refusal": preload[0].family_refusal()} if share_prefix and hasattr(preload[0], "family_refusal") else {}))
    print(f"Starting server on port {port}")
    try:
        httpd.serve_forever()
    finally:
        engine.close()


def arg_parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--synthetic", action="store_true", help="seeded random weights instead of models/phi3_v")
    ap.add_argument("--tiny", action="store_true", help="with --synthetic: the 2-layer test model (smoke tests)")
    ap.add_argument("--blind", action="store_true", help="text-only Phi-3-mini-128K")
    ap.add_argument("--merge", action="store_true", help="fold concurrent same-budget requests into one batched generate (opt-in)")
    ap.add_argument("--continuous", action="store_true", help="continuous batching engine (requests join / leave between decode steps)")
    ap.add_argument("--long-window", type=int, default=0, help="with --continuous: also serve prompt + max_tokens > 4096 up to this many tokens")
    ap.add_argument("--slots", type=int, default=8, help="with --continuous: batch rows of the engine")
    ap.add_argument("--adapter", action="append", default=[], metavar="NAME=DIR",
                    help="load the LoRA adapter in DIR (adapter_config.json + adapters.safetensors) into the adapter bank as NAME "
                         "(repeatable); a request picks one with its \"adapter\" field")
    ap.add_argument("--prefix-cache-gb", type=float, default=0.0, metavar="G",
                    help="with --continuous: keep up to G GiB of prompt-prefix K/V per engine and reuse it for requests that start with "
                         "the same tokens and pictures (393 KB per token at full size: ~1 GB per cached image)")
    ap.add_argument("--speculate", type=int, default=0, metavar="K",
                    help="default of the request field \"speculate\": verify K prompt-lookup draft tokens per decode step (one-request "
                         "path, greedy; 0 = off).  Not with --continuous / --merge")
    ap.add_argument("--share-prefix", action="store_true",
                    help="the completions of an \"n\" > 1 request read their prompt's K/V once per decode step instead of n times "
                         "(bf16 KV cache; with or without --continuous).  It pays from (n - 1) x prompt tokens >= 4096 on; smaller "
                         "families run unshared.  With --continuous EVERY decode step then runs on the shared-prefix attention plan, "
                         "family in flight or not: 0.15 - 0.7 ms (8 - 15 %) slower per step for ordinary traffic -- for servers whose "
                         "traffic is mostly n > 1 over long prompts")
    ap.add_argument("--host", default="127.0.0.1", help='interface to bind ("" = all, as the reference)')
    ap.add_argument("--image-dir", default=None, help="allow `images` entries naming files under this directory")
    ap.add_argument("--image-host", action="append", default=[], help="allow `images` URLs on this host (repeatable)")
    return ap


if __name__ == "__main__":
    ap = arg_parser()
    a = ap.parse_args()
    bank = {}
    for spec in a.adapter:
        name, sep, path = spec.partition("=")
        if not sep or not name or not path or name in bank:
            ap.error(f"--adapter takes NAME=DIR with distinct names, got {spec!r}")
        bank[name] = path
    if a.speculate and (a.continuous or a.merge):
        ap.error("--speculate runs on the one-request path: not with --continuous or --merge")
    if not 0 <= a.speculate <= SPECULATE_MAX:
        ap.error(f"--speculate takes 0 .. {SPECULATE_MAX}")
    if a.prefix_cache_gb and not a.continuous:
        ap.error("--prefix-cache-gb needs --continuous")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:               # python -m torch.distributed.run --nproc-per-node N -m ...server --continuous
        if not a.continuous:
            # the one-shot paths have no worker loop: every rank would bind the same port and rank 0's batches would wait in
            # generate_sharded for ranks that never join
            ap.error("WORLD_SIZE > 1 needs --continuous (one engine per rank, rank 0 serves HTTP); "
                     "for one-shot batch sharding call dist.generate_sharded from a torchrun script instead")
        import torch
        import torch.distributed as dist
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())   # (fewer GPUs than ranks: shared)
        dist.init_process_group("gloo")                          # requests and token lists only: host memory (fleet.py)
    run(a.port, "tiny" if a.synthetic and a.tiny else a.synthetic, a.blind, a.merge, a.continuous, a.host, ImagePolicy(a.image_dir, a.image_host), a.long_window, a.slots, bank,
        a.prefix_cache_gb, a.speculate, a.share_prefix)
