"""Continuous batching at decode-step granularity (the reference has none: its server runs one
`generate` per HTTP request, server.py:17).

One GPU, one captured decode graph over a fixed number of SLOTS (batch rows).  Every row has its own left padding and
its own position table, so rows are independent sequences that merely share the cache column they write next:

  * a waiting request is PREFILLED INTO A FREE ROW between two decode steps, right-aligned to the engine's current column
    (`model.prefill_slot`): left padding = column - prompt length, positions 0..S-1 from there on -- exactly the
    geometry `_tokenize` gives a left-padded batch row (phi.py:238-240), so the row computes what a B = 1 `generate` of
    the request computes (pad keys get zero weight, Q7);
  * every step is ONE graph replay for all rows; finished rows (EOS or budget, phi_3_vision_mlx.py:105-117, :390) are
    released at once and their slot is reusable at the next step -- nobody waits for the slowest row of a batch;
  * a request joins only if prompt <= column and column + max_tokens <= window; when the engine is idle the column
    jumps to the longest waiting prompt (an empty engine has no column to respect).

RoPE regime (phi.py:492: ONE short/long factor choice per call, from prompt + max_tokens > 4096).  An engine instance
serves ONE regime: `window <= 4096` -> short factors and only requests with S + max_tokens <= 4096 (what each of them
alone would pick); `window > 4096` -> long factors and only requests with S + max_tokens > 4096.  `RegimeRouter` puts
one engine of each kind behind a single `submit` and steps both from one thread.  With `quantize_cache=True` models the
slot state keeps the int8 KV cache of BASELINE config 5 (`model.new_slot_state`).

Admission is FIFO with bounded overtaking: a request that does not fit the current column is skipped by newer ones for
at most `patience` decode steps; after that nothing newer is admitted, the engine drains, and the column moves to the
blocked request.  A prefill group that fails is retried one request at a time, so one bad request fails alone.

Failures are loud: an exception inside a step fails every active and waiting request at once (nobody waits for a
timeout), the slot state and its captured graph are rebuilt (the in-launch split-KV merge relies on an all-sentinel
workspace between launches; a failed step may have left it dirty), and if THAT fails the engine marks itself dead and
refuses new work.  A negative token id (the device's report of NaN logits or a timed-out in-launch merge,
include/p3v.h) on an active row fails that request and re-arms the workspace.  A request whose waiter gave up
(`cancel()`) leaves its slot at the next step.

Prompt prefix cache (`prefix_cache=prefix.PrefixCache(...)`, off by default): every admitted request is looked up in the store; a
hit is prefilled ALONE -- its prefix K/V copied into its row, the rest of the prompt computed (`model.prefill_slot(prefix=)`) --
and a miss goes the way it always went and leaves its prefix in the store afterwards (`cache_prompt`).  Without a store no call
into the model changes.

Cost model: a row reads the cache columns [0, column) whatever its own length (static split ranges), so a short request
that joins late pays for the padding it attends over with zero weight; the weights (7.4 GB/step) are shared by all rows.

A request's options are ONE record (request.RequestOptions): `submit` reads it from its arguments and from what rides beside the
inputs (`cache_args`, `logprob_args`, `penalty_args`, `n_args`), checks it once, and the Request keeps the checked values.
"""
import collections
import dataclasses
import threading

import numpy as np
import torch

from . import row_options
from .logprobs import unpack as _unpack_records
from .steps import kind_for
from .request import (GUIDE_ARGS, LOGPROB_ARGS, N_ARGS, PENALTY_ARGS, PREFIX_ARGS, RequestOptions, _check_adapter, adapter_list,  # noqa: F401
                      carry, options_per_prompt, requested_logprobs, requested_n, requested_penalties)

ID_EOS = 32007
ROPE_WINDOW = 4096            # original_max_position_embeddings: the short / long factor boundary (phi.py:492)


def _is_gpu(device):
    return torch.device(device).type == "cuda"


def _sync(device):
    if _is_gpu(device):
        torch.cuda.synchronize(device)


def _set_device(device):
    if _is_gpu(device):                                         # a new thread starts on GPU 0 whatever the loader used
        torch.cuda.set_device(device)


class Request:
    __slots__ = ("inputs", "max_tokens", "tokens", "done", "row", "error", "S", "cancelled", "blocked_at", "sampling", "adapter",
                 "image_digests", "cache_prompt", "prefix_len", "cached_tokens", "hit", "logprobs", "logprob_records", "penalties", "guide",
                 "family", "members", "completions", "family_done", "n", "asked_logprobs", "opts")

    def __init__(self, inputs, max_tokens, opts=None, **fields):
        """opts: the request's CHECKED options record (request.RequestOptions; `fields` replace single values of it).  `step()`
        reads them every step, so they are plain attributes: sampling, adapter, logprobs (one record per token in
        `logprob_records`), penalties, and for an engine with a prefix store image_digests, cache_prompt and prefix_len."""
        self.inputs, self.max_tokens = inputs, int(max_tokens)
        self.opts = opts = dataclasses.replace(opts or RequestOptions(), **fields)
        for f in ("sampling", "adapter", "logprobs", "penalties", "guide", "image_digests", "prefix_len"):
            setattr(self, f, getattr(opts, f))
        self.cache_prompt = bool(opts.cache_prompt)
        self.cached_tokens, self.hit = 0, None                   # prompt tokens restored from the prefix store instead of computed
        self.logprob_records = []                                # (logprobs.unpack dicts, aligned with `tokens`)
        self.S = int(np.asarray(inputs["input_ids"]).shape[-1])
        self.tokens, self.row, self.error = [], None, None
        self.cancelled, self.blocked_at = False, None
        self.done = threading.Event()
        # n completions per prompt (`n_args`): a plain request is its own family of one.  The HEAD of a family (family is self)
        # lists the m generated requests in `members` (itself first) and the n returned ones in `completions` (for best_of:
        # ranked, set when `family_done` is); every member has its own tokens / logprob_records / error / done
        self.family, self.members, self.completions, self.family_done, self.n = None, [self], [self], self.done, 1
        self.asked_logprobs = self.logprobs                      # what the CLIENT asked (best_of scores every member at N >= 0)

    def cancel(self):
        """The waiter gave up (timeout, client gone): the engine drops the request at its next step.  A cancelled head cancels
        its family."""
        self.cancelled = True
        if self.family is self:
            for r in self.members[1:]:
                r.cancelled = True

    def fail(self, error):
        """A head fails with every member that has not finished (refused at submit, a failed prefill, a dead engine)."""
        for r in (self.members if self.family is self else [self]):
            if r is self or not r.done.is_set():
                r.error = error
                r.done.set()
        self.settle()

    def settle(self):
        """After `done` was set: the last member to finish ranks the family (best_of) and sets the head's `family_done`."""
        head = self.family
        if head is None or head.family_done.is_set() or not all(r.done.is_set() for r in head.members):
            return
        if head.completions is None and len(head.members) <= head.n:
            head.completions = list(head.members)                # (a remote head that failed before its completions arrived)
        if head.completions is None:
            from .logprobs import rank_best_of
            ok = [r.error is None for r in head.members]
            order = rank_best_of([r.tokens if g else None for r, g in zip(head.members, ok)],
                                 [[x["logprob"] for x in r.logprob_records] if g else None for r, g in zip(head.members, ok)],
                                 head.n, ID_EOS)
            head.completions = [head.members[j] for j in order]
        head.family_done.set()


def make_family(head, n, m):
    """Turn a fresh Request into the head of a family of m generated rows, n of them returned: member j is the same request
    under the seed (s + j) mod 2^64 (a greedy head: m greedy members).  best_of (m > n): every member is scored (N = 0 where
    the client asked for nothing), `completions` waits for the ranking."""
    from .parallel import seeds
    head.family, head.n, head.family_done = head, n, threading.Event()
    want = head.logprobs if m == n or head.logprobs is not None else 0
    head.logprobs = want
    ss = [None] * m if head.sampling is None else seeds(head.sampling[3], m)
    for j in range(1, m):
        r = Request(head.inputs, head.max_tokens, head.opts, logprobs=want,
                    sampling=None if head.sampling is None else head.sampling[:3] + (ss[j],))
        r.family, r.asked_logprobs = head, head.asked_logprobs
        head.members.append(r)
    head.completions = list(head.members) if m == n else None
    return head


class EmbedJob:
    """Handle of `ContinuousEngine.embed`: wait on `.done`, then read `.result` (np.float32 [B, H]) or `.error`; `cancel()` drops
    a job the engine has not started."""
    __slots__ = ("inputs", "pooling", "normalize", "adapter", "result", "error", "done", "cancelled")

    def __init__(self, inputs, pooling, normalize, adapter):
        self.inputs, self.pooling, self.normalize, self.adapter = inputs, pooling, bool(normalize), adapter
        self.result, self.error, self.cancelled = None, None, False
        self.done = threading.Event()

    def cancel(self):
        self.cancelled = True

    def fail(self, error):
        self.error = error
        self.done.set()


EMBED_INPUT_KEYS = ("input_ids", "pixel_values", "image_sizes", "positions", "pids", "mask")


def generate(self, prompts, images=None, max_tokens=512, timeout=600.0, sampling=None, adapter=None, cache_prompt=None, info=None,
             logprobs=None, penalties=None, n=None, best_of=None, guide=None):
    """Text in, text out (what the HTTP backend calls): the `generate` of ContinuousEngine, RegimeRouter and fleet.EngineFleet."""
    return _generate_text(self, self.processor, prompts, images, max_tokens, timeout, sampling, adapter, cache_prompt, info, logprobs,
                          penalties, n, best_of, **({} if guide is None else {"guide": guide}))


class ContinuousEngine:
    def __init__(self, model, processor, slots=8, window=ROPE_WINDOW, patience=64, prefix_cache=None, share_prefix=False):
        self.model, self.processor, self.slots, self.window, self.patience = model, processor, slots, window, patience
        # share_prefix: the rows of a family (n_args) read their prompt's K/V once per decode step (model.set_families); off --
        # the default -- nothing of it is allocated, launched or captured
        self.share_prefix = bool(share_prefix)
        if self.share_prefix:
            why = model.family_refusal() if hasattr(model, "family_refusal") else None
            if why:
                raise ValueError(why)
        self.families = []                                       # [(rows, share_end)], leader first: what the state's table holds
        self.prefix_cache = prefix_cache                         # prefix.PrefixCache or None (off: every path as without the feature)
        self.long_rope = window > ROPE_WINDOW
        self.rows = [None] * slots                               # row -> active Request
        self.waiting = collections.deque()
        self.embed_jobs = collections.deque()                    # EmbedJob handles, served between two steps (`embed`)
        self.lock = threading.Lock()
        self.steps = 0                                           # decode steps replayed (observability / tests)
        self.joined_mid_flight = 0                               # requests admitted while other rows were generating
        self.failures = 0                                        # steps that raised (each one rebuilt the slot state)
        self.dead = None                                         # the exception that made the engine unusable, if any
        self._new_state()

    def _new_state(self):
        self.st = self.model.new_slot_state(self.slots, self.window)
        self.model.serving = True                               # (the owner is a server: model.py)
        self.st.serving = True                                  # long-lived: the split-KV merge must not lean on dispatch order (model._plan)
        self.cache = [type("L", (), {"state": self.st})()]      # greedy_step reads cache[0].state
        self.families = []
        if self.share_prefix:                                   # the table BEFORE the step is captured: the capture then follows it
            self.model.set_families(self.st, [], create=True)

    # ---- request side (any thread)
    def accepts(self, S, max_tokens):
        """Does a request of this shape belong to this engine's RoPE regime and fit its window?"""
        if max_tokens < 1 or S < 1 or S + max_tokens > self.window:
            return False
        return (S + max_tokens > ROPE_WINDOW) == self.long_rope

    def adapter_names(self):
        """Names of the model's adapter bank (model.set_adapter_bank); empty without one."""
        return list(getattr(self.model, "adapter_names", None) or [])

    def submit(self, inputs, max_tokens, sampling=None, adapter=None):
        """inputs: a B = 1 `processor(text[, images])` result.  Returns the Request; wait on `.done`, read `.tokens`.
        Engines with a `prefix_cache`: `submit(cache_args(inputs, image_digests=, cache_prompt=True, prefix_len=None), ...)` puts
        the request's prefix-cache arguments beside its inputs (they travel with them through a router or a fleet): one
        `prefix.image_digest` per source image -- without them a prompt with images is reused up to its first image slot only --,
        whether this prompt's K/V may be captured for later requests, and how many of its tokens to capture (default: through
        the last image slot, or the whole prompt).  A request always LOOKS UP the store; its `cached_tokens` says how many
        tokens it reused.
        sampling: None (greedy) or {"temperature", "top_k", "top_p", "seed"} (missing keys: 0, 0, 1.0, 64 random bits; see
        sampling.rows) -- the request's tokens are then drawn under its own record, whoever shares the batch.
        adapter: None (the base model) or the name of one adapter of the model's bank: the request's row runs with it, next to
        rows with other adapters or none, in the one captured step.  An unknown name fails the handle at once (ValueError);
        nothing is queued.
        Token log-probabilities: `submit(logprob_args(inputs, N), ...)`, N in 0..8, puts the request's `logprobs` beside its inputs,
        as `cache_args` does (so it travels through a router or a fleet too) -- every token of the request then comes with its
        log-probability under the raw logits, its rank and the N most likely tokens (include/p3v.h: p3v_logprob_t) in
        `logprob_records`, aligned with `tokens`.  While no active request asks, the engine replays exactly what it replays
        without the feature.
        Penalties and logit_bias: `submit(penalty_args(inputs, repetition_penalty=, presence_penalty=, frequency_penalty=,
        logit_bias=), ...)` puts them beside the inputs in the same way -- the request's row then has its logits adjusted by the
        rule of include/p3v.h (p3v_penalty_row_t) before its token is drawn, from its first token on, whoever shares the
        batch; rows that did not ask pass through bit for bit.  While no active request asks, nothing of it runs.
        Guided decoding: `submit(guide_args(inputs, regex=pattern), ...)` or `guide_args(inputs, choice=[...])` puts the request's
        guide beside the inputs in the same way (`guide_args(inputs, schema={...})`: a JSON schema); it is compiled and checked
        against the vocabulary HERE, so a bad pattern or schema fails the handle at once.  The request's row then has its penalised logits masked by the rule of include/p3v.h
        (p3v_guide_row_t) before its token is drawn, from its first token on; a refilled row starts from its own start state.
        While no active request asks, nothing of it runs.
        n completions: `submit(n_args(inputs, n, best_of=None), ...)` puts the count beside the inputs in the same way, so the
        whole family travels to ONE engine.  The handle is then the family's HEAD: `.completions` lists the n returned
        Requests (head first; under best_of the n best of the m generated, best first, once `.family_done` is set), each with
        its own tokens / logprob_records / error / done.  The prompt is prefilled once into one free row and forked into m - 1
        others (model.fork_rows); member j samples under the seed (s + j) mod 2^64.  A family is admitted all or nothing
        (m free rows, not necessarily adjacent); m > slots fails the handle here.  Without `n_args` nothing changes."""
        from .parallel import refusal
        try:
            opts = RequestOptions.read(inputs, sampling, adapter).checked(
                self.adapter_names(), getattr(getattr(self.model, "cfg", None), "vocab_size", None), inputs)
            if opts.guide is not None:                          # ... and can this vocabulary spell it?
                from . import guide as guide_mod
                guide_mod.checked(opts.guide, guide_mod.vocab_for(self.processor.tokenizer, self.model.cfg.vocab_size), ID_EOS)
            m = opts.m
            why = refusal(m, mlx4=bool(getattr(self.st, "mlx4", False)))
            if why:
                raise ValueError(why)
            if m > self.slots:
                raise ValueError(f"n > slots: a family of {m} completions needs {m} rows at once, this engine has {self.slots} slots")
        except ValueError as e:
            r = Request(inputs, max_tokens)
            r.fail(e)
            return r
        r = Request(inputs, max_tokens, opts)
        if m > 1:
            make_family(r, opts.n, m)
        if self.dead is not None:
            r.fail(RuntimeError(f"engine is down: {self.dead!r}"))
        elif not self.accepts(r.S, r.max_tokens):
            r.fail(ValueError(f"prompt {r.S} + max_tokens {r.max_tokens} is outside this engine "
                              f"({'long' if self.long_rope else 'short'}-RoPE regime, window {self.window})"))
        else:
            with self.lock:
                self.waiting.append(r)
        return r

    def embed(self, inputs, pooling="last", normalize=True, adapter=None):
        """inputs: a `processor(text[, images])` result, B >= 1 (a left-padded batch carries its mask).  Returns an EmbedJob.  The
        stepping thread serves it between two decode steps, before it admits new requests, through `model.embed` on the job's
        own transient state: the slot state and its captures are untouched, the rows in flight do not see it.  adapter: None, a
        name, or one name / None per row.  A prompt above the engine's window, an unknown pooling or adapter: ValueError, here."""
        from .api import check_pooling
        check_pooling(pooling)
        ids = np.asarray(inputs["input_ids"])
        B, S = (1, ids.shape[-1]) if ids.ndim == 1 else ids.shape
        if S < 1 or S > self.window:
            raise ValueError(f"embed: a prompt of {S} tokens is outside this engine's window of {self.window}")
        names = adapter_list(adapter, B)
        for a in names:
            _check_adapter(a, self.adapter_names())
        if self.dead is not None:
            raise RuntimeError(f"engine is down: {self.dead!r}")
        job = EmbedJob(inputs, pooling, normalize, None if adapter is None else names)
        with self.lock:
            self.embed_jobs.append(job)
        return job

    # ---- engine side (ONE thread)
    def _serve_embeds(self):
        while self.embed_jobs:
            with self.lock:
                job = self.embed_jobs.popleft()
            if job.cancelled:
                job.done.set()
                continue
            try:
                kw = {k: v for k, v in job.inputs.items() if k in EMBED_INPUT_KEYS}
                if job.adapter is not None:
                    kw["row_adapters"] = job.adapter
                job.result = self.model.embed(**kw, pooling=job.pooling, normalize=job.normalize).cpu().numpy()
            except Exception as e:                              # noqa: BLE001 -- reported to the job, the engine lives on
                job.error = e
            job.done.set()

    def _active(self):
        return [r for r in self.rows if r is not None]

    def _leave_family(self, rows):
        """Rows stop being members BEFORE anything may rewrite them (a refill, a scrub, a rewound column): no table entry names
        a freed row as `lead`.  A leader that leaves hands over to the next member, a family of one is cleared."""
        from .parallel import families_without
        rows = [r for r in rows if r is not None]
        if self.share_prefix and any(r in members for members, _ in self.families for r in rows):
            self.families = families_without(self.families, rows)
            self.model.set_families(self.st, self.families)

    def _release(self, r):
        if r.row is not None and self.rows[r.row] is r:
            self._leave_family([r.row])
            self.rows[r.row] = None
            self.st.pad_len[r.row:r.row + 1].fill_(self.window)  # every key masked: the row idles at zero cost of correctness
            row_options.release(self.model, self.st, r.row, row_options.Asked.of([r]))
        r.done.set()
        r.settle()                                               # (the last member of a family sets its head's family_done)

    _finish = _release

    def _fail_all(self, error):
        with self.lock:
            waiting, self.waiting = list(self.waiting), collections.deque()
        if self.dead is not None:                                # (nobody will serve them any more)
            while self.embed_jobs:
                self.embed_jobs.popleft().fail(error)
        for r in self._active() + [x for h in waiting for x in h.members]:   # (a waiting head: its whole family)
            r.error = error
            if r.row is not None and self.rows[r.row] is r:
                self.rows[r.row] = None
            r.done.set()
            r.settle()
        self.families = []                                       # (the state is rebuilt, or the engine is down)

    def _recover(self, error):
        """A step raised: fail everybody now, then rebuild the slot state + graph (or die loudly)."""
        self.failures += 1
        self._fail_all(error)
        try:
            _sync(self.model.device)
        except Exception:                                       # noqa: BLE001 -- a sticky HIP error surfaces again below
            pass
        try:
            self.st.graphs.clear()
            self.st = self.cache = None                         # free the old cache before the new one is allocated
            self._new_state()
        except Exception as e:                                  # noqa: BLE001
            self.dead = e
            self._fail_all(RuntimeError(f"engine is down: {e!r}"))

    def _rearm_workspace(self):
        """The in-launch split-KV merge expects an all-sentinel workspace (ops.attention_ws); after a poisoned step a late
        partial may have landed on top of the restored sentinels -- refill before the next replay."""
        g = self.st.graphs.get("greedy")
        plan = g and g["bufs"].get("plan")
        ws = plan and plan.ws
        if ws is not None:
            _sync(self.model.device)
            ws.view(torch.int32).fill_(-1)

    def _pick(self):
        """FIFO admission with bounded overtaking (under the lock).  Returns (requests to prefill, their free rows).  The head of
        a family counts as its m rows, all or nothing: one that fits the column but not the free rows waits under the same
        patience rule as a request that does not fit the column."""
        st = self.st
        for r in self.waiting:
            if r.cancelled:
                for x in r.members:
                    x.done.set()
                r.settle()
        self.waiting = collections.deque(r for r in self.waiting if not r.cancelled)
        if not self.waiting:
            return [], []
        if not self._active():
            # idle: the column follows the OLDEST waiting prompts -- but never so far right that the HEAD request no longer
            # fits (column + its max_tokens <= window).  The head itself always qualifies (`accepts`), so an idle engine
            # admits at least the head: a blocked / draining head cannot keep everybody out for ever.
            first = list(self.waiting)[:self.slots]
            head = first[0]
            st.offset = max(r.S for r in first if r.S == head.S or r.S + head.max_tokens <= self.window)
        free = [i for i, r in enumerate(self.rows) if r is None]
        admit, keep, draining, used = [], collections.deque(), False, 0
        for r in self.waiting:
            fits = r.S <= st.offset and st.offset + r.max_tokens <= self.window
            need = len(r.members)
            if not draining and fits and used + need <= len(free):
                admit.append(r)
                used += need
                continue
            if (not fits or need > 1) and not draining:
                if r.blocked_at is None:
                    r.blocked_at = self.steps
                draining = self.steps - r.blocked_at >= self.patience       # nobody newer gets in: the engine drains for r
            keep.append(r)
        self.waiting = keep
        return admit, free

    def _prefill_group(self, group, row0, busy):
        from .processor import collate_requests
        st, n = self.st, len(group)
        g = self.model.decode_graph(st)
        for i, r in enumerate(group):
            r.row = row0 + i
        inputs = collate_requests([r.inputs for r in group]) if n > 1 else group[0].inputs
        hit = group[0].hit if n == 1 else None                   # a request with a hit is prefilled alone (_admit)
        for r in group:
            r.hit = None                                         # (the handle must not pin a store entry once it is served)
        if self.adapter_names():
            # the rows' adapters (None -> -1: a refilled row must not keep its last occupant's) BEFORE their prefill reads them
            self.model.set_row_adapters(st, [r.adapter for r in group], row0)
        toks, first = self._prefill_rows(group, [(row0, n)], inputs, hit)
        g["tok"][row0:row0 + n].copy_(toks.reshape(-1))
        self._seat(group, first, busy)

    def _prefill_family(self, head, rows, busy):
        """n completions of one prompt: every row gets its records first (adapter, then row_options.install), the prompt is
        prefilled ONCE into rows[0] -- with a prefix hit or a capture, as any single request -- and forked into the other rows
        (model.fork_rows: their K/V columns, position tables and pad_len); then every row's first token is drawn from the ONE
        prefill logits row under its own record.  The rows need not be adjacent: every setter is called per row."""
        st, model, members = self.st, self.model, head.members
        g = model.decode_graph(st)
        for r, row in zip(members, rows):
            r.row = row
        hit, head.hit = head.hit, None
        if self.adapter_names():
            for row in rows:
                model.set_row_adapters(st, [head.adapter], row)

        def fork():
            model.fork_rows(st, rows[0], rows[1:], pad=st.offset - head.S)
            if self.share_prefix:                               # columns [pad, offset) of the rows are identical from here on
                from .parallel import families_without
                self.families = families_without(self.families, rows) + [(tuple(rows), int(st.offset))]
                model.set_families(st, self.families)
        _, first = self._prefill_rows(members, [(row, 1) for row in rows], head.inputs, hit, fork)
        for r, t in zip(members, first):
            g["tok"][r.row:r.row + 1].fill_(t)
        self._seat(members, first, busy)

    def _prefill_rows(self, reqs, spans, inputs, hit, fork=None):
        """The rows' option tables, ONE prefill into the first row (its logits kept where the first token is drawn or scored; the
        plain call otherwise: no keyword, and without a hit exactly as without a store), `fork` (a family: the other rows), the
        first tokens and their records (row_options), the prefix capture (after the NaN check).  -> (tokens on the device, as a list)"""
        st, model, row0 = self.st, self.model, spans[0][0]
        asked = row_options.Asked.of(reqs, lead_guide=fork is not None)
        row_options.install(model, st, spans, asked, inputs, self.processor)
        kw = {} if hit is None else {"prefix": hit}
        if asked.drawn or asked.wants is not None:
            toks, logits = model.prefill_slot(st, row0, inputs, return_logits=True, **kw)
        else:
            toks, logits = model.prefill_slot(st, row0, inputs, **kw), None
        if fork is not None:
            fork()
            toks = toks.reshape(-1)[:1].expand(len(reqs))        # greedy: the one arg-max serves every row
        toks, first, words = row_options.first_tokens(model, st, spans, asked, logits, toks)
        for r, rec in zip(reqs, _unpack_records(words) if words is not None else ()):
            if r.logprobs is not None:
                r.logprob_records.append(rec)
        if hit is not None:
            reqs[0].cached_tokens = int(hit[1])
        self._capture(reqs if fork is None else reqs[:1])
        return toks, first

    def _seat(self, reqs, first, busy):
        for r, t in zip(reqs, first):
            self.rows[r.row] = r
            self.joined_mid_flight += int(busy)
            r.tokens.append(t)
            if t == ID_EOS or len(r.tokens) >= r.max_tokens:
                self._release(r)

    # ---- prompt prefix cache
    def _prefix_key(self, adapter=None):
        """The store key of a row of this engine with that adapter, or None when its cache can neither be captured nor restored
        (cache_format="mlx4")."""
        st = self.st
        if getattr(st, "mlx4", False):
            return None
        return self.prefix_cache.key(getattr(self.model, "epoch", 0), adapter, self.long_rope, "int8" if getattr(st, "quantized", False) else "bf16")

    def _lookup(self, r):
        key = self._prefix_key(r.adapter)
        if key is None:
            self.prefix_cache.bypass()
            return None
        return self.prefix_cache.lookup(np.asarray(r.inputs["input_ids"]).reshape(-1), r.image_digests, key)

    def _capture(self, group):
        """After a successful prefill: store the prefix of every request that asks for it and is not covered yet."""
        store = self.prefix_cache
        if store is None:
            return
        if self._prefix_key() is None:
            return
        from .prefix import capture_len, kv_bytes
        for r in group:
            if not r.cache_prompt:
                continue
            try:
                ids = np.asarray(r.inputs["input_ids"]).reshape(-1)
                P, key = capture_len(ids, r.prefix_len), self._prefix_key(r.adapter)
                cfg = getattr(self.model, "cfg", None)
                nbytes = None if cfg is None else kv_bytes(P, cfg.num_hidden_layers, cfg.num_key_value_heads, self.model.hd, key[3])
                if store.wants(ids, r.image_digests, key, P, nbytes):
                    store.insert(ids[:P], r.image_digests, key, self.model.capture_prefix(self.st, r.row, self.st.offset - r.S, P))
            except Exception:                                   # noqa: BLE001 -- (out of memory for the copy, ...) the request itself is fine
                _sync(self.model.device)

    def _admit(self):
        with self.lock:
            admit, free = self._pick()
        if not admit:
            return
        if self.prefix_cache is not None:
            for r in admit:
                r.hit = self._lookup(r)
        busy = bool(self._active())
        # requests of nearly equal length that get ADJACENT free rows are prefilled as one left-padded group (one pass over
        # the weights instead of one per request; dist.GROUP_PAD bounds the padding a request may carry)
        from .dist import GROUP_PAD
        free.sort()
        for head in [r for r in admit if len(r.members) > 1]:   # a family: prefilled alone into its first row, forked into the rest
            rows, free = free[:len(head.members)], free[len(head.members):]
            try:
                self._prefill_family(head, rows, busy)
            except Exception as e:                              # noqa: BLE001 -- a failed prefill releases every row of the family
                self._leave_family([x.row for x in head.members])
                for x in head.members:
                    if x.row is not None:
                        if self.rows[x.row] is x:
                            self.rows[x.row] = None
                        self.st.pad_len[x.row:x.row + 1].fill_(self.window)
                        row_options.release(self.model, self.st, x.row, row_options.Asked.of([x]), if_made=True)
                    del x.logprob_records[:], x.tokens[:]
                head.fail(e)
        admit = [r for r in admit if len(r.members) == 1]
        admit.sort(key=lambda r: -r.S)
        while admit:
            run = 1
            while run < len(free) and free[run] == free[0] + run:
                run += 1
            n = 1
            while n < min(run, len(admit)) and admit[0].S - admit[n].S <= GROUP_PAD and admit[0].hit is None and admit[n].hit is None:
                n += 1
            group, admit = admit[:n], admit[n:]
            row0, free = free[0], free[n:]
            try:
                self._prefill_group(group, row0, busy)
            except Exception as e:                              # noqa: BLE001 -- reported to the request(s), the engine lives on
                for r in group:
                    if self.rows[r.row] is r:
                        self.rows[r.row] = None
                    self.st.pad_len[r.row:r.row + 1].fill_(self.window)
                    del r.logprob_records[:]
                row_options.release(self.model, self.st, row0, row_options.Asked.of(group), if_made=True)
                if n == 1:
                    group[0].fail(e)
                    continue
                for i, r in enumerate(group):                   # one bad request must not fail its neighbours: retry alone
                    try:
                        self._prefill_group([r], row0 + i, busy)
                    except Exception as e1:                     # noqa: BLE001
                        self.st.pad_len[r.row:r.row + 1].fill_(self.window)
                        r.fail(e1)

    def step(self):
        """Admit what fits, then one decode step for every active row.  Returns the number of active rows."""
        if self.dead is not None:
            return 0
        self._serve_embeds()
        self._admit()
        for r in self._active():
            if r.cancelled:
                self._release(r)
        active = self._active()
        if not active:
            return 0
        g = self.model.decode_graph(self.st)
        # ONE kind of replay for all rows (steps.py): the sampled tail while any active row samples (its greedy rows take the
        # arg-max there too), the penalised one while any is penalised (such a row is active from its prefill to its release, so
        # every one of its steps counts the token it is fed; the other rows pass through bit for bit), the guided one while any
        # is guided, each followed by the log-probability launch while any row wants records (the others: one early exit each)
        kind = kind_for(*(any(getattr(r, f) is not None for r in active) for f in ("sampling", "penalties", "guide", "logprobs")))
        # Records are indexed by the capture's step counter, which EVERY replay advances, and have as many slots as `history`: a
        # long-lived state starts the counter afresh when the slots have run out, whether or not the record buffer exists yet.
        if kind.logprobs and g.get("n_replays", 0) >= g["history"].shape[1]:
            self.model.restart_history(self.st)
        replay = getattr(self.model, kind.method)
        _, tok = replay(g["host_tok"] if g["host_tok"] is not None else g["tok"].view(-1, 1), self.cache)
        rows = tok.reshape(-1).tolist()                          # ONE D2H copy per step (the reference's mx.eval)
        recs = _unpack_records(g["records"][:, g["n_replays"] - 1]) if kind.logprobs else None   # (pinned: the step wrote them itself)
        self.steps += 1
        poisoned = False
        for r in active:
            t = rows[r.row]
            if t < 0:                                            # the device's report of a failed step for this row
                poisoned = True
                r.error = RuntimeError(f"device step failed: NaN logits or split merge timeout (token id {t})")
                self._release(r)
                continue
            r.tokens.append(t)
            if r.logprobs is not None:
                r.logprob_records.append(recs[r.row])
            if t == ID_EOS or len(r.tokens) >= r.max_tokens:
                self._release(r)
        if poisoned:
            self._rearm_workspace()
        if self.st.offset + 1 > self.st.T:                       # window exhausted: budgets were checked at admission,
            for r in self._active():                             # so nothing can still be running -- belt and braces
                self._release(r)
        return len(active)

    def safe_step(self):
        """`step` that never raises: an exception fails all requests at once and rebuilds the state (see module doc)."""
        try:
            return self.step()
        except Exception as e:                                  # noqa: BLE001
            self._recover(e)
            return 0

    def run_until_idle(self, max_steps=1 << 20):
        n = 0
        while n < max_steps and (self.step() or self.waiting):
            n += 1
        return n

    def serve_forever(self, stop_event, idle_sleep=0.002):
        """Engine thread body: step while there is work, nap when idle."""
        _set_device(self.model.device)
        while not stop_event.is_set():
            if not self.safe_step() and not self.waiting and not self.embed_jobs:
                stop_event.wait(idle_sleep)

    generate = generate


# What rides beside a request's inputs (request.py has the keys, their one reader and their one writer).  Each helper returns a
# COPY of a B = 1 `processor(...)` result with one carrier added, so the option travels through a router or a fleet with the
# inputs; the processor's own result is not touched, and `submit` checks the values.
def penalty_args(inputs, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None):
    """... the request's penalties and logit_bias, as one plain dict (penalties.request_row checks it)."""
    return carry(inputs, PENALTY_ARGS, RequestOptions(penalties=dict(
        repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, logit_bias=logit_bias)))


def guide_args(inputs, regex=None, choice=None, schema=None):
    """... the request's guide: a regular expression, a choice list or a JSON schema (a dict or its JSON text) -- one of them;
    guide.py compiles and checks it at submit."""
    from .guide import exclusive
    exclusive(regex, choice, schema)
    if regex is None and choice is None and schema is None:
        return inputs
    guide = {"regex": regex} if regex is not None else {"choice": list(choice)} if choice is not None else {"schema": schema}
    return carry(inputs, GUIDE_ARGS, RequestOptions(guide=guide))


def logprob_args(inputs, logprobs):
    """... the request's `logprobs`: None, or N in 0..8."""
    return carry(inputs, LOGPROB_ARGS, RequestOptions(logprobs=logprobs))


def n_args(inputs, n, best_of=None):
    """... the number of completions asked of it (n in 1..16, best_of None or n..16): a router or a fleet hands the WHOLE family
    to one engine."""
    return carry(inputs, N_ARGS, RequestOptions(n=n, best_of=best_of))


def cache_args(inputs, image_digests=None, cache_prompt=True, prefix_len=None):
    """... the request's prefix-cache arguments."""
    return carry(inputs, PREFIX_ARGS, RequestOptions(image_digests=image_digests, cache_prompt=cache_prompt, prefix_len=prefix_len))


def leaf_engines(front):
    """The ContinuousEngines behind a server backend, a fleet (rank 0's own), a router, or an engine itself."""
    inner = getattr(front, "engine", None)
    behind = [inner] if inner is not None else list(getattr(front, "engines", None) or ())
    if not behind:
        yield front
    for e in behind:
        yield from leaf_engines(e)


def has_prefix_cache(engine):
    """Does this engine (or any engine behind a router / fleet) carry a prefix store?"""
    return any(getattr(e, "prefix_cache", None) is not None for e in leaf_engines(engine))


def _generate_text(engine, processor, prompts, images, max_tokens, timeout, sampling=None, adapter=None, cache_prompt=None, info=None,
                   logprobs=None, penalties=None, n=None, best_of=None, guide=None):
    """n / best_of (one prompt only): n completions of it from one prefill (`n_args`) -- the result is then the list of the n
    returned texts, info gains "seeds" (one per returned completion, when sampled) and its "logprobs" has one entry per
    returned completion.
    sampling: None, or one settings dict per prompt (engine.submit); adapter: None, a name, or one name / None per prompt.
    cache_prompt: None / True (the prompt may be captured by the engine's prefix store) or False.  info: a dict that receives
    "cached_tokens" (one count per prompt) and, when a prompt asked for them, "logprobs" (per prompt: logprobs.entry of its
    records -- token_ids / token_logprobs / ranks / top_logprobs over the tokens of the returned text -- or None).
    logprobs: None, N in 0..8, or one such value per prompt.  penalties: None, one {"repetition_penalty", "presence_penalty",
    "frequency_penalty", "logit_bias"} dict for every prompt, or one dict / None per prompt.  guide: None, one {"regex": pattern} /
    {"choice": [strings]} / {"schema": JSON schema} dict for every prompt, or one dict / None per prompt."""
    from . import api
    prompts = [prompts] if isinstance(prompts, str) else list(prompts)
    opts = options_per_prompt(len(prompts), sampling, adapter, logprobs, penalties, cache_prompt, n, best_of,
                              **({} if guide is None else {"guide": guide}))
    fam, lps = opts[0].m > 1, [o.logprobs for o in opts]
    images = images if images is not None else [None] * len(prompts)
    reqs = []
    for o, p, im in zip(opts, prompts, images):
        text, imgs = api._apply_chat_template(p, im, False)
        if imgs is not None and has_prefix_cache(engine):       # of the decoded source images, before the processor runs
            from .prefix import image_digests
            o = dataclasses.replace(o, image_digests=image_digests(imgs))
        reqs.append(o.send(engine, processor(text, imgs) if imgs is not None else processor(text), max_tokens))
    out, kept = [], []
    heads = reqs
    try:
        if fam:                                                 # one prompt: wait for its family, answer with the returned completions
            head = reqs[0]
            if not head.family_done.wait(timeout):
                raise TimeoutError("engine did not finish the request in time")
            if not head.completions:                            # (a remote family that failed before its completions arrived)
                raise head.error or RuntimeError("the family returned no completion")
            reqs, lps = list(head.completions), lps * len(head.completions)
        for r in reqs:
            if not r.done.wait(timeout):
                raise TimeoutError("engine did not finish the request in time")
            if r.error is not None:
                raise r.error
            ids = r.tokens[:r.tokens.index(ID_EOS) + 1] if ID_EOS in r.tokens else r.tokens
            kept.append(ids)
            out.append(processor.tokenizer.decode(ids))
        if info is not None:
            info["cached_tokens"] = [int(getattr(r, "cached_tokens", 0)) for r in heads]
            if fam and all(r.sampling is not None for r in reqs):
                info["seeds"] = [int(r.sampling[3]) for r in reqs]
            if any(w is not None for w in lps):
                from .logprobs import entry
                info["logprobs"] = [None if w is None else entry(list(r.logprob_records)[:len(ids_out)])
                                    for w, r, ids_out in zip(lps, reqs, kept)]
    except BaseException:
        for r in heads:                                         # nobody is waiting for these any more: free their slots (a head: its family's)
            if not getattr(r, "family_done", r.done).is_set():
                r.cancel()
        raise
    return out


class RegimeRouter:
    """One `submit` in front of a short-RoPE engine (window 4096) and a long-RoPE engine (window > 4096), both stepped by
    one thread: a request goes to the engine whose regime it would pick on its own (phi.py:492), so its tokens are what a
    solo `generate` of it produces."""

    def __init__(self, engines):
        self.engines = list(engines)
        self.processor = self.engines[0].processor

    def adapter_names(self):
        return self.engines[0].adapter_names()

    def submit(self, inputs, max_tokens, sampling=None, adapter=None):
        S = int(np.asarray(inputs["input_ids"]).shape[-1])
        for e in self.engines:
            if e.accepts(S, int(max_tokens)):
                return RequestOptions(sampling=sampling, adapter=adapter).send(e, inputs, max_tokens)   # (what rides beside the inputs passes through as it is)
        r = Request(inputs, max_tokens)
        r.fail(ValueError(f"prompt {S} + max_tokens {max_tokens} fits no engine window"))
        return r

    @property
    def waiting(self):
        return any(e.waiting for e in self.engines)

    def safe_step(self):
        return sum(e.safe_step() for e in self.engines)

    def serve_forever(self, stop_event, idle_sleep=0.002):
        _set_device(self.engines[0].model.device)
        while not stop_event.is_set():
            if not self.safe_step() and not self.waiting:
                stop_event.wait(idle_sleep)

    generate = generate
