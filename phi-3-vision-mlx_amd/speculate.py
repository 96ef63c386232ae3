"""Speculative greedy decoding, the rule in plain Python (include/p3v.h: "speculative greedy decoding" states it once more
for the kernels p3v_ngram_propose / p3v_spec_end, which are held to this file exactly).

State of one sequence: ctx[0..n) -- every token id so far, prompt included; the newest token ctx[n-1] is not yet in the cache.

  propose   prompt lookup: the tokens that followed the most recent earlier occurrence of the current suffix;
  accept    greedy verification: the longest run of drafts the model's own arg-maxes confirm, and the tokens emitted;
  step      one verify step on a context (propose happened before it, accept after it);
  run       the host loop's arithmetic on a scripted "model" (the truncation rules of api.speculative_loop).
"""

DEFAULT_K = 4            # P3V_SPEC_DEFAULT_K
N_MAX, N_MIN = 3, 1      # P3V_SPEC_NGRAM_MAX / P3V_SPEC_NGRAM_MIN
MAX_K = 15               # P3V_DECODE_MAX_L - 1


def propose(ctx, K, n_max=N_MAX, n_min=N_MIN, vocab=None):
    """The draft (a list of at most K ids) for the context `ctx`.  For m = n_max down to n_min, skipping m >= n: the LARGEST
    p < n - m with ctx[p:p+m] == ctx[n-m:n]; the draft is ctx[p+m : min(p+m+K, n)], cut in front of the first id outside
    [0, vocab) (vocab None: in front of the first negative id); the first m with a match ends the search."""
    n = len(ctx)
    for m in range(n_max, n_min - 1, -1):
        if m >= n or m < 1:
            continue
        s = list(ctx[n - m:])
        for p in range(n - m - 1, -1, -1):
            if list(ctx[p:p + m]) == s:
                draft = []
                for t in ctx[p + m:min(p + m + K, n)]:
                    t = int(t)
                    if t < 0 or (vocab is not None and t >= vocab):
                        break
                    draft.append(t)
                return draft
    return []


def accept(drafts, argmaxes):
    """(acc, emitted): acc = the largest i <= len(drafts) with drafts[j] == argmaxes[j] for all j < i; emitted =
    argmaxes[0 .. acc].  `argmaxes` holds one arg-max per row of the step (at least len(drafts) + 1)."""
    acc = 0
    while acc < len(drafts) and int(drafts[acc]) == int(argmaxes[acc]):
        acc += 1
    return acc, [int(a) for a in argmaxes[:acc + 1]]


def step(ctx, drafts, argmaxes, n_limit=None):
    """One verify step: the tokens it emits.  A -1 among them (a NaN row) ends the run there: the step failed.  n_limit: the
    context never grows beyond it (the run's token budget: the emitted run is cut, a step at the limit emits nothing)."""
    _, out = accept(drafts, argmaxes)
    if -1 in out:
        return out[:out.index(-1) + 1]
    if n_limit is not None:
        out = out[:max(0, n_limit - len(ctx))]
    return out


def truncate(tokens, max_tokens, stop_id):
    """What the plain loop would have delivered of `tokens` (the prefill token first): at most max_tokens of them, none behind
    the first stop token."""
    out = []
    for t in tokens[:max(max_tokens, 1)]:
        out.append(t)
        if t == stop_id and len(out) > 1:
            break
    return out


def run(prompt, first, next_token, max_tokens, K, stop_id=None, n_max=N_MAX, n_min=N_MIN, vocab=None, stats=None):
    """The speculative loop on a scripted model: `next_token(ctx)` is the model's greedy token after the context `ctx`
    (a list).  Returns the tokens delivered, `first` (the prefill token) included -- the same list the plain loop delivers:
    tokens are emitted run by run, the output is cut at the first stop token behind the prefill token or at max_tokens.
    stats (a dict) receives steps / drafted / accepted / emitted as api.speculative_loop counts them."""
    ctx = list(prompt) + [first]
    out = [first]
    st = dict(steps=0, drafted=0, accepted=0, emitted=0)
    n_limit = len(prompt) + max(max_tokens, 1)
    done = False
    while not done and len(out) < max_tokens:
        drafts = propose(ctx, K, n_max, n_min, vocab)
        rows = [ctx[-1]] + drafts
        argmaxes = [next_token(ctx[:-1] + rows[:j + 1]) for j in range(len(rows))]
        acc, _ = accept(drafts, argmaxes)
        emitted = step(ctx, drafts, argmaxes, n_limit)
        st["steps"] += 1
        st["drafted"] += len(drafts)
        st["accepted"] += max(len(emitted) - 1, 0)                # == acc unless the budget cut the run
        st["emitted"] += len(emitted)
        for t in emitted:
            ctx.append(t)
            out.append(t)
            if t == stop_id:
                done = True
                break
    if stats is not None:
        stats.update(st)
    return out
