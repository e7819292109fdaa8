"""The wide sampler (biogpt_hip_generate_sample_wide, kernels_wide_sample.hip.h) in Python doubles: oracle/sampler.py's sample_top_k_top_p for any top_k,
with the min-p stage between the top-p cut and the draw, NaNs never candidates, and the margin of every decision -- sample_ref.decision_margin's borders
(the compared cumulative sums against top_p, u against the partial sums of the draw) and min-p's (every compared probs[i] / probs[0] against min_p).
A sampler is the tuple (top_k, top_p, min_p, temp); top_k 0 is the whole row.  The generator of the device as 625 words, for comparing states.

Not a test module: a helper the tests import."""
import math

import numpy as np

import sample_ref
from oracle import sampler as oracle_sampler


def S(top_k, top_p, temp, min_p=0.0):
    """A sampler written in the order top_k, top_p, temp, min_p."""
    return (int(top_k), float(top_p), float(min_p), float(temp))


def sample_wide(logits, sampler, rng):
    """One draw from one row.  Returns (id, n_cand, margin): n_cand the candidates left after all cuts (0: a row without a finite value, which gives
    id 0 and takes nothing from rng); margin the smallest distance of a decision from its border."""
    top_k, top_p, min_p, temp = sampler
    lg = np.asarray(logits, dtype=np.float32)
    k = lg.size if top_k == 0 else min(int(top_k), lg.size)
    scale = 1.0 / float(temp)
    scaled = lg.astype(np.float64) * scale
    order = np.argsort(-scaled, kind="stable")            # value descending, lower id first on equal values; NaNs last
    order = order[~np.isnan(lg[order])][:k]
    if order.size == 0 or scaled[order[0]] == -math.inf:
        return 0, 0, math.inf
    vals = scaled[order]
    maxl = float(vals[0])
    probs = np.array([math.exp(float(v) - maxl) for v in vals], dtype=np.float64)
    probs = probs / np.cumsum(probs)[-1]                  # (np.cumsum adds in order, as the reference's loops do)
    margin = math.inf
    if top_p < 1.0:
        cs = np.cumsum(probs)
        hit = np.nonzero(cs >= top_p)[0]
        last = int(hit[0]) if hit.size else probs.size - 1
        margin = min(margin, float(np.min(np.abs(cs[:last + 1] - top_p))))
        probs = probs[:last + 1] * (1.0 / cs[last])
    if min_p > 0.0:
        fail = np.nonzero(~(probs >= min_p * probs[0]))[0]
        keep = int(fail[0]) if fail.size else probs.size
        compared = probs[:min(keep + 1, probs.size)] / probs[0]
        margin = min(margin, float(np.min(np.abs(compared - min_p))))
        probs = probs[:max(keep, 1)]
    n = int(probs.size)
    if n < 2:
        return int(order[0]), n, margin
    cp = np.cumsum(probs / np.cumsum(probs)[-1])
    cp[-1] = 1.0
    u = oracle_sampler.generate_canonical_53(rng)
    margin = min(margin, float(np.min(np.abs(u - cp[:-1]))))
    return int(order[int(np.searchsorted(cp, u, side="left"))]), n, margin


def reference_loop(oracle_model, prompt, n_batch, n_predict, sampler, seed, eos=-1):
    """sample_ref.reference_loop with a sampler of any width.  Returns (ids, smallest margin)."""
    rng = oracle_sampler.Mt19937(seed)
    lg = None
    for at in range(0, len(prompt), n_batch):
        lg = oracle_model.eval(list(prompt[at:at + n_batch]), at)
    n_past, ids, margin = len(prompt), [], math.inf
    n_predict = min(int(n_predict), oracle_model.n_positions - len(prompt))
    for k in range(n_predict):
        t, _, m = sample_wide(lg, sampler, rng)
        margin = min(margin, m)
        ids.append(int(t))
        if eos >= 0 and t == eos:
            break
        if k + 1 < n_predict:
            lg = oracle_model.eval([t], n_past)
            n_past += 1
    return ids, margin


# ---- std::mt19937 as the device holds it: 624 words + the index of the next output ----

def mt_seed(seed):
    st = np.zeros(625, dtype=np.uint32)
    x = int(seed) & 0xFFFFFFFF
    st[0] = x
    for i in range(1, 624):
        x = (1812433253 * (x ^ (x >> 30)) + i) & 0xFFFFFFFF
        st[i] = x
    st[624] = 624
    return st


def _mix(cur, nxt, far):
    y = (cur & np.uint64(0x80000000)) | (nxt & np.uint64(0x7FFFFFFF))
    return far ^ (y >> np.uint64(1)) ^ np.where(y & np.uint64(1), np.uint64(0x9908B0DF), np.uint64(0))


def mt_regenerate(st):
    old = st[:624].astype(np.uint64)
    new = np.empty(624, dtype=np.uint64)
    new[0:227] = _mix(old[0:227], old[1:228], old[397:624])
    new[227:454] = _mix(old[227:454], old[228:455], new[0:227])
    new[454:623] = _mix(old[454:623], old[455:624], new[227:396])
    new[623:624] = _mix(old[623:624], new[0:1], new[396:397])
    st[:624] = new.astype(np.uint32)
    st[624] = 0


class StateRng:
    """The generator over a 625-word state, advanced in place."""

    def __init__(self, st):
        self.st = st

    def __call__(self):
        if int(self.st[624]) >= 624:
            mt_regenerate(self.st)
        y = int(self.st[int(self.st[624])])
        self.st[624] += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def canonical_state(st):
    """A state whose block has run out and the same state with the next block made say the same: the latter."""
    st = np.array(st, dtype=np.uint32)
    if int(st[624]) >= 624:
        mt_regenerate(st)
    return st


# ---- rows of every awkward kind ----

def row_kinds(nv, seed):
    """22 rows of nv entries: N(0, 2.5); N(0, 0.5) (flat: the nucleus is most of the row); rounded to halves (ties at the cut and at the pick); one constant row
    (uniform: the pick is position-by-id) but for one raised entry -- with every entry equal the cumulative sums i / nv lie ON top_p = 0.9 and 0.5 at
    width 70, where no arithmetic but the reference's own can be held to its choice; one row with a single dominant entry (nothing is drawn); rows with half their entries -inf and a few NaNs; an all -inf
    row and an all-NaN row (id 0, no draw)."""
    rng = np.random.default_rng(seed)
    rows = np.empty((22, nv), dtype=np.float32)
    rows[0:5] = (rng.standard_normal((5, nv)) * 2.5).astype(np.float32)
    rows[5:10] = (rng.standard_normal((5, nv)) * 0.5).astype(np.float32)
    rows[10:14] = np.round(rng.standard_normal((4, nv)) * 2.5 * 2.0).astype(np.float32) / 2.0
    rows[14] = 1.25
    rows[14, nv // 3] = 1.75
    rows[15] = (rng.standard_normal(nv) * 0.5).astype(np.float32)
    rows[15, (7 * nv) // 11] = 400.0
    rows[16:20] = (rng.standard_normal((4, nv)) * 2.5).astype(np.float32)
    for r in range(16, 20):
        rows[r, rng.permutation(nv)[:nv // 2]] = -np.inf
        rows[r, rng.permutation(nv)[:5]] = np.nan
    rows[20] = -np.inf
    rows[21] = np.nan
    return rows
