"""The reference's sampled generation loop (main.cpp:91-151) over the CPU oracle and oracle/sampler.py, as biogpt_hip_generate_sample defines its
result ("Sampled generation"), with the margin of every decision that depends on exp(): the engine runs ROCm's exp(double), the
reference glibc's, so a case can hold the engine to the ids only where no draw lies next to a partial-sum border and no cumulative sum next to top_p.

Not a test module: a helper the tests import."""
import math

import numpy as np

from oracle import sampler


class RecordingRng:
    """A generator that remembers its outputs (the margin needs the draw the sampler made)."""

    def __init__(self, rng):
        self.rng = rng
        self.out = []

    def __call__(self):
        v = self.rng()
        self.out.append(v)
        return v


def topk_order(logits, top_k):
    """The selection: value descending, lower id first on equal values."""
    lg = np.asarray(logits, dtype=np.float32)
    return np.argsort(-lg.astype(np.float64), kind="stable")[:top_k]


def decision_margin(logits, top_k, top_p, temp, draws):
    """min(|u - nearest partial sum|, |cumsum_i - top_p| over the i compared) of one sample_top_k_top_p call that made `draws` (0 or 2 outputs):
    the sampler's arithmetic restated in the same doubles."""
    lg = np.asarray(logits, dtype=np.float32)
    scale = 1.0 / float(temp)
    vals = [float(lg[i]) * scale for i in topk_order(lg, top_k)]
    maxl = max(vals)
    probs = [math.exp(v - maxl) for v in vals]
    total = 0.0
    for p in probs:
        total += p
    probs = [p / total for p in probs]
    margin = float("inf")
    if top_p < 1.0:
        cumsum = 0.0
        for i in range(len(probs)):
            cumsum += probs[i]
            margin = min(margin, abs(cumsum - top_p))
            if cumsum >= top_p:
                probs = probs[:i + 1]
                break
        inv = 1.0 / cumsum
        probs = [p * inv for p in probs]
    if len(probs) < 2:
        assert len(draws) == 0
        return margin
    assert len(draws) == 2
    total = 0.0
    for p in probs:
        total += p
    u = (float(draws[0]) + float(draws[1]) * 4294967296.0) / 18446744073709551616.0
    run = 0.0
    for p in probs[:-1]:      # (the last partial sum is forced to 1.0 and u < 1)
        run += p / total
        margin = min(margin, abs(u - run))
    return margin


def reference_loop(oracle_model, prompt, n_batch, n_predict, top_k, top_p, temp, seed, eos=-1):
    """main.cpp:109-151 for one prompt: the prompt in chunks of n_batch, then one token at a time; std::mt19937(seed); stops after the first `eos`.
    Returns (ids, smallest margin)."""
    rng = RecordingRng(sampler.Mt19937(seed))
    lg = None
    for at in range(0, len(prompt), n_batch):
        lg = oracle_model.eval(list(prompt[at:at + n_batch]), at)
    n_past, ids, margin = len(prompt), [], float("inf")
    n_predict = min(int(n_predict), oracle_model.n_positions - len(prompt))
    for k in range(n_predict):
        before = len(rng.out)
        t = sampler.sample_top_k_top_p(lg, top_k, top_p, temp, rng)
        margin = min(margin, decision_margin(lg, top_k, top_p, temp, rng.out[before:]))
        ids.append(int(t))
        if eos >= 0 and t == eos:
            break
        if k + 1 < n_predict:
            lg = oracle_model.eval([t], n_past)
            n_past += 1
    return ids, margin
