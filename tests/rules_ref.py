"""Scalar restatement of the generation rules (include/biogpt_hip.h, biogpt_hip_gen_rules; INTEGRATION.md, "Generation rules"): transformers'
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor and SuppressTokensLogitsProcessor on one row,
in numpy float32 -- pinned to transformers on the CPU (test_rules_restatement.py), then the engine is held to it (test_gpu_rules.py).

    rules: dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=()), any key may be missing.

Not a test module: a helper the tests import."""
import numpy as np

import sample_ref
from oracle import sampler

NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=())


def full(rules):
    return {**NEUTRAL, **(rules or {})}


def apply_rules(row, history, n_prompt, rules, eos=-1):
    """The processed copy of `row` (float32 [n_vocab]: logits in sampled / greedy mode, log-probabilities in beam mode) for a sequence whose
    tokens so far are `history` (prompt + generated), the first n_prompt of them the prompt."""
    r = full(rules)
    s = np.array(row, dtype=np.float32, copy=True)
    h = [int(t) for t in history]
    L = len(h)
    p = np.float32(r["repetition_penalty"])
    if p != np.float32(1.0):
        for t in sorted(set(h)):     # every distinct token once
            s[t] = np.float32(s[t] * p) if s[t] < 0 else np.float32(s[t] / p)
    n = int(r["no_repeat_ngram_size"])
    if n > 0 and L + 1 >= n:
        tail = h[L - n + 1:]
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == tail:
                s[h[i + n - 1]] = -np.inf
    if eos is not None and eos >= 0 and L - int(n_prompt) < int(r["min_new_tokens"]):
        s[eos] = -np.inf
    for t in r["suppress_tokens"]:
        s[int(t)] = -np.inf
    return s


def rules_logprobs(fn, prompt, rules, eos=-1):
    """A beam_ref `logprobs` callback with the rules applied to every row (transformers: log_probs = logits_processor(running sequences, log_probs))."""
    prompt = [int(t) for t in prompt]

    def wrapped(prefixes):
        rows = np.asarray(fn(prefixes), dtype=np.float32)
        return np.stack([apply_rules(rows[b], prompt + [int(t) for t in p], len(prompt), rules, eos) for b, p in enumerate(prefixes)])
    return wrapped


def reference_loop_rules(oracle_model, prompt, n_batch, n_predict, top_k, top_p, temp, seed, rules, eos=-1):
    """sample_ref.reference_loop with apply_rules on the oracle's row in front of oracle.sampler.sample_top_k_top_p.  Returns (ids, the smallest
    sample_ref.decision_margin over the processed rows)."""
    rng = sample_ref.RecordingRng(sampler.Mt19937(seed))
    lg = None
    for at in range(0, len(prompt), n_batch):
        lg = oracle_model.eval(list(prompt[at:at + n_batch]), at)
    n_past, ids, margin = len(prompt), [], float("inf")
    n_predict = min(int(n_predict), oracle_model.n_positions - len(prompt))
    for k in range(n_predict):
        row = apply_rules(lg, list(prompt) + ids, len(prompt), rules, eos)
        before = len(rng.out)
        t = sampler.sample_top_k_top_p(row, top_k, top_p, temp, rng)
        margin = min(margin, sample_ref.decision_margin(row, top_k, top_p, temp, rng.out[before:]))
        ids.append(int(t))
        if eos >= 0 and t == eos:
            break
        if k + 1 < n_predict:
            lg = oracle_model.eval([t], n_past)
            n_past += 1
    return ids, margin


# ---- the invariants of a finished output, checked on the ids alone ----

def ngram_repeats(tokens, n):
    """True if some n-gram occurs twice in `tokens`."""
    seen = set()
    for i in range(len(tokens) - n + 1):
        g = tuple(tokens[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False
