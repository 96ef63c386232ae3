"""A request's options as ONE record, from the text front to the engine's row.

`submit(inputs, max_tokens, sampling=None, adapter=None)` keeps its parameter list: every other option rides beside the
inputs under a CARRIER key, so a router or a fleet that knows nothing of an option forwards it untouched.  This module is the only
code that knows the carrier keys: `RequestOptions.read` is their one reader, `RequestOptions.send` their one writer, `checked` the
one place where a request's values are checked (the rules themselves live in sampling.py, logprobs.py, penalties.py, parallel.py).
"""
import dataclasses

import numpy as np

PREFIX_ARGS = "prefix_cache_args"   # keys of a request's options inside its `inputs` (no model call forwards them)
LOGPROB_ARGS = "logprobs"
PENALTY_ARGS = "penalties"
N_ARGS = "n_completions"
GUIDE_ARGS = "guide"


@dataclasses.dataclass(frozen=True)
class RequestOptions:
    """Plain values (it pickles); the defaults mean "not asked".  A CHECKED record (`checked`) holds the normalised values a
    Request keeps: sampling as one (temperature, top_k, top_p, seed) tuple, penalties as one (repetition, frequency, presence,
    bias) tuple, logprobs as N or None, n / best_of as checked integers."""
    sampling: object = None         # None (greedy) or {"temperature", "top_k", "top_p", "seed"}
    adapter: object = None          # None (the base model) or the name of an adapter of the model's bank
    logprobs: object = None         # None (off) or N in 0..8
    penalties: object = None        # None (off) or {"repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"}
    guide: object = None            # None (off) or {"regex": pattern} / {"choice": [strings]} / {"schema": JSON schema}; checked: the compiled guide.Dfa
    n: object = 1                   # completions returned ...
    best_of: object = None          # ... of this many generated (None: n)
    image_digests: object = None    # prefix cache: one prefix.image_digest per source image
    cache_prompt: object = True     # ... may this prompt's K/V be captured for later requests
    prefix_len: object = None       # ... how many of its tokens to capture (None: through the last image slot, or all)

    @property
    def m(self):
        """Rows a checked record's request is generated in: best_of, or n without one (m > 1: a family)."""
        return self.n if self.best_of is None else self.best_of

    @classmethod
    def read(cls, inputs, sampling=None, adapter=None):
        """The record of what `submit` received.  ValueError for a carrier that its helper did not make."""
        fields = {}
        for key, names, maker in ((PREFIX_ARGS, ("image_digests", "cache_prompt", "prefix_len"), "cache_args"), (N_ARGS, ("n", "best_of"), "n_args")):
            d = _requested(key)(inputs)
            if d is not None and (not isinstance(d, dict) or set(d) - set(names)):
                raise ValueError(f"{key} must be what engine.{maker} makes")
            fields.update({k: d[k] for k in names if d is not None and k in d})
        return cls(sampling=sampling, adapter=adapter, logprobs=requested_logprobs(inputs), penalties=requested_penalties(inputs),
                   guide=requested_guide(inputs), **fields)

    def checked(self, adapters, vocab=None, inputs=None):
        """The normalised record, or the ValueError that names the bad value.  adapters: the names the model's bank knows;
        vocab: the bound of logit_bias keys (None: only >= 0); inputs: what the digests-per-image count is checked against."""
        from . import logprobs as logprobs_mod
        from .parallel import check
        from .penalties import request_row
        want = logprobs_mod.check(self.logprobs)
        pen = request_row(self.penalties, vocab)
        from .guide import Dfa, request_guide
        dfa = self.guide if isinstance(self.guide, Dfa) else request_guide(self.guide)   # (compiled here: a bad pattern is a ValueError)
        rec = _sampling_row(self.sampling)
        _check_adapter(self.adapter, adapters)
        self._check_prefix(inputs)
        n, m = check(self.n, self.best_of)
        return dataclasses.replace(self, sampling=rec, logprobs=None if want == logprobs_mod.OFF else want, penalties=pen, guide=dfa, n=n,
                                   best_of=None if self.best_of is None else m)

    def _check_prefix(self, inputs):
        if not isinstance(self.cache_prompt, bool):
            raise ValueError("cache_prompt must be True or False")
        digests, prefix_len = self.image_digests, self.prefix_len
        if digests is not None:
            if isinstance(digests, (str, bytes)) or not all(isinstance(d, str) and d for d in digests):
                raise ValueError("image_digests must be a list of non-empty strings, one per image")
            n_img = 0 if inputs is None or inputs.get("image_sizes") is None else len(np.asarray(inputs["image_sizes"]))
            if len(digests) != n_img:
                raise ValueError(f"image_digests: {len(digests)} digests for {n_img} images")
        if prefix_len is not None and (isinstance(prefix_len, bool) or not isinstance(prefix_len, (int, np.integer)) or prefix_len < 1):
            raise ValueError(f"prefix_len must be a positive integer, got {prefix_len!r}")

    def send(self, engine, inputs, max_tokens):
        """`engine.submit` with only what is in use: an engine-like object that knows nothing of an option keeps working for the
        requests that do not ask for it, and a plain request is `submit(inputs, max_tokens)` with the caller's own `inputs`."""
        for key, (used, _) in CARRIERS.items():
            if used(self):
                inputs = carry(inputs, key, self)
        kw = {k: v for k, v in (("sampling", self.sampling), ("adapter", self.adapter)) if v is not None}
        return engine.submit(inputs, max_tokens, **kw)


# the writer table, in the order the carriers are written: key -> (is it in use?, what rides under it)
CARRIERS = {
    N_ARGS: (lambda o: (o.n, o.best_of) != (1, None), lambda o: {"n": o.n, "best_of": o.best_of}),
    PREFIX_ARGS: (lambda o: o.image_digests is not None or o.prefix_len is not None or not o.cache_prompt,
                  lambda o: {"image_digests": o.image_digests, "cache_prompt": o.cache_prompt, "prefix_len": o.prefix_len}),
    LOGPROB_ARGS: (lambda o: o.logprobs is not None, lambda o: o.logprobs),
    PENALTY_ARGS: (lambda o: o.penalties is not None, lambda o: dict(o.penalties)),
    GUIDE_ARGS: (lambda o: o.guide is not None, lambda o: dict(o.guide)),
}


def carry(inputs, key, opts):
    """A copy of a B = 1 `processor(...)` result with one carrier of `opts` beside it.  The processor's own result is not touched."""
    return dict(inputs, **{key: CARRIERS[key][1](opts)})


def _requested(key):
    return lambda inputs: inputs.get(key) if isinstance(inputs, dict) else None


requested_logprobs, requested_penalties, requested_n = _requested(LOGPROB_ARGS), _requested(PENALTY_ARGS), _requested(N_ARGS)
requested_guide = _requested(GUIDE_ARGS)


def _sampling_row(sampling):
    """submit's `sampling` dict -> one checked (temperature, top_k, top_p, seed) tuple; None stays None (greedy)."""
    if sampling is None:
        return None
    if isinstance(sampling, tuple):
        sampling = dict(zip(("temperature", "top_k", "top_p", "seed"), sampling))
    unknown = set(sampling) - {"temperature", "top_k", "top_p", "seed"}
    if unknown:
        raise ValueError(f"unknown sampling settings {sorted(unknown)}")
    from .sampling import rows
    return rows(1, sampling.get("temperature", 0.0), sampling.get("top_k", 0), sampling.get("top_p", 1.0), sampling.get("seed"))[0]


def _check_adapter(adapter, known):
    if adapter is None:
        return
    if not isinstance(adapter, str):
        raise ValueError(f"adapter must be a name (string) or None, got {type(adapter).__name__}; known adapters: {known}")
    if adapter not in known:
        raise ValueError(f"unknown adapter {adapter!r}; known adapters: {known}")


def adapter_list(adapter, n):
    """`adapter` argument of a text-level call (api.generate too) -> one name / None per prompt: a name (or None) serves every
    prompt, a list gives one per prompt."""
    if adapter is None or isinstance(adapter, str):
        return [adapter] * n
    if not isinstance(adapter, (list, tuple)):
        raise ValueError(f"adapter must be a name, None, or a list of one per prompt, got {type(adapter).__name__}")
    if len(adapter) != n:
        raise ValueError(f"adapter: {len(adapter)} names for {n} prompts")
    return list(adapter)


def options_per_prompt(n_prompts, sampling=None, adapter=None, logprobs=None, penalties=None, cache_prompt=None, n=None, best_of=None,
                       guide=None):
    """The arguments of a text-level call -> one record per prompt.  sampling: None or one settings dict per prompt; adapter: None,
    a name, or one name / None per prompt; logprobs: None, N, or one value per prompt; penalties: None, one dict for every prompt,
    or one dict / None per prompt; n / best_of: a family, of one prompt only; guide: None, one {"regex"} / {"choice"} / {"schema"} dict for every
    prompt, or one dict / None per prompt.  ValueError for a list of the wrong length."""
    from .logprobs import OFF, wants
    from .parallel import check, refusal
    m = check(n, best_of)[1]
    why = refusal(m, batched=n_prompts != 1)
    if why:
        raise ValueError(why)
    if sampling is not None and len(sampling) != n_prompts:
        raise ValueError(f"sampling: {len(sampling)} records for {n_prompts} prompts")
    adapter = adapter_list(adapter, n_prompts)
    w = wants(logprobs, n_prompts)
    if penalties is None or isinstance(penalties, dict):
        penalties = [penalties] * n_prompts
    elif len(penalties) != n_prompts:
        raise ValueError(f"penalties: {len(penalties)} values for {n_prompts} prompts")
    if guide is None or isinstance(guide, dict):
        guide = [guide] * n_prompts
    elif len(guide) != n_prompts:
        raise ValueError(f"guide: {len(guide)} values for {n_prompts} prompts")
    family = {"n": 1 if n is None else n, "best_of": best_of} if m > 1 else {}
    return [RequestOptions(sampling=None if sampling is None else sampling[i], adapter=adapter[i],
                           logprobs=None if w is None or w[i] == OFF else w[i], penalties=penalties[i], guide=guide[i],
                           cache_prompt=True if cache_prompt is None else bool(cache_prompt), **family) for i in range(n_prompts)]
