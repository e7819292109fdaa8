"""The token tail, restated in plain numpy: the kernels every generated id of the single-stream path leaves through (the lm_head's arg-max partials, the finisher
over them, topk_kernel) and the host selections of biogpt_hip_eval_topk.  Nothing here has a tolerance.  The tail's one rule (csrc/kernels_rows.hip.h): larger value
first; equal values, lower id first; a NaN is never before anything and nothing is before it.

order / argmax / partials / finish / topk state the rule and nothing else.  topk_kernel, host_topk and host_topk_blocks restate the three selections step by step --
threshold, candidates, cap, ranks; the walk over blocks of 16; the walk over the 64-row blocks -- because what they answer (the k pairs, or a refusal) depends on
those steps, and so that each named mistake (MISTAKES) can be committed where a kernel would commit it: tests/test_tail_restatement.py shows on the CPU that every
one changes an expected output of a case of tests/tail_cases.py."""
import numpy as np

F32 = np.float32
NONE_IDX = 0x7FFFFFFF          # the id of "no comparable value": what a finisher lane starts from
TOPK_CAP = 4096                # topk_kernel's candidate slots
TOPK_REGS = 42 * 1024          # the elements topk_kernel holds in registers; a loop takes the ones beyond

MISTAKES = {
    "tie_higher_id": "a tie resolved to the higher id",
    "tie_within_wave_only": "the tie rule applied inside a wave, but not where waves or parts are combined (there the later one takes a tie)",
    "nan_seed": "a finisher seeded with its first value without a comparison: a NaN there is held, and hides everything combined into it",
    "last_block_dropped": "the last, partial block has no partial",
    "unclamped_empty": "no comparable partial: 0x7fffffff is stored as the next token",
    "candidates_gt": "topk_kernel: candidates taken with > instead of >= at the threshold",
    "cap_off_by_one": "topk_kernel: exactly 4096 candidates refused",
    "rank_by_slot": "topk_kernel: ranks break ties by LDS slot instead of by id",
    "beyond_regs_dropped": "topk_kernel: the elements beyond 43008 dropped",
    "host_ge": "host_topk: a value equal to the current k-th value counts as beating it (the block skip and the insertion taken with >=)",
    "blocks_select_gt": "host_topk_blocks: blocks selected with > instead of >= at the k-th block maximum",
}


def _check(mistake):
    assert mistake is None or mistake in MISTAKES, mistake


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------------------------

def order(row, ids=None):
    """ids by (value descending, id ascending), NaNs left out.  ids: the id of each entry (default: its position)."""
    row = np.asarray(row, dtype=F32)
    ids = np.arange(row.size, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    keep = ~np.isnan(row)
    v, i = row[keep].astype(np.float64), ids[keep]
    return i[np.lexsort((i, -v))]


def argmax(row, n_vocab=None):
    """The first id of order(row), or 0 when it is empty -- or when it lies outside [0, n_vocab)."""
    o = order(row)
    tok = int(o[0]) if o.size else NONE_IDX
    n_vocab = np.asarray(row).size if n_vocab is None else n_vocab
    return tok if 0 <= tok < n_vocab else 0


def _better(v, i, bv, bi, mistake=None):
    if mistake == "tie_higher_id":
        return v > bv or (v == bv and i > bi)
    return v > bv or (v == bv and i < bi)


def _reduce(vals, ids, mistake=None, seed=False):
    """One finisher's walk over (value, id) pairs from (-inf, NONE_IDX).  seed: the first pair is taken without a comparison (the nan_seed mistake)."""
    bv, bi = F32(-np.inf), NONE_IDX
    for n, (v, i) in enumerate(zip(vals, ids)):
        if (seed and n == 0) or _better(v, int(i), bv, bi, mistake):
            bv, bi = F32(v), int(i)
    return bv, bi


def _combine(pairs, mistake=None):
    """Results of waves (or threads) into one.  Under tie_within_wave_only a later result takes a tie."""
    bv, bi = pairs[0]
    for v, i in pairs[1:]:
        if mistake == "tie_within_wave_only":
            if v >= bv:
                bv, bi = v, i
        elif _better(v, i, bv, bi, mistake):
            bv, bi = v, i
    return bv, bi


def partials(row, rows_per_part, mistake=None, waves=4):
    """(values float32 [parts], ids int32 [parts]): the first pair of order() of each part of rows_per_part rows, or (-inf, 0x7fffffff) for a part with no
    comparable value.  Without a mistake the answer does not depend on how a part's rows are spread over lanes and waves; a mistake is committed in a part of
    `waves` waves with consecutive quarters of its rows."""
    _check(mistake)
    row = np.asarray(row, dtype=F32)
    M = row.size
    nparts = M // rows_per_part if mistake == "last_block_dropped" else -(-M // rows_per_part)
    pv, pi = np.full(nparts, -np.inf, F32), np.full(nparts, NONE_IDX, np.int32)
    per_wave = -(-rows_per_part // waves)
    for p in range(nparts):
        r0, r1 = p * rows_per_part, min(M, (p + 1) * rows_per_part)
        if mistake is None:
            o = order(row[r0:r1], np.arange(r0, r1))
            if o.size:
                pv[p], pi[p] = row[o[0]], o[0]
            continue
        res = []
        for w0 in range(r0, r1, per_wave):
            w1 = min(r1, w0 + per_wave)
            res.append(_reduce(row[w0:w1], range(w0, w1), mistake, seed=mistake == "nan_seed"))
        pv[p], pi[p] = _combine(res, mistake)
    return pv, pi


def finish(pmax_val, pmax_idx, n_vocab, mistake=None, threads=256):
    """argmax_kernel's token: the id of the first pair by the rule (the pairs' own ids break ties, not their places), 0 when no pair is comparable or the id lies
    outside [0, n_vocab)."""
    _check(mistake)
    pv, pi = np.asarray(pmax_val, dtype=F32), np.asarray(pmax_idx, dtype=np.int64)
    if mistake is None or mistake in ("unclamped_empty",):
        o = order(pv, pi)
        tok = int(o[0]) if o.size else NONE_IDX
    else:
        res = [_reduce(pv[t::threads], pi[t::threads], mistake, seed=mistake == "nan_seed") for t in range(min(threads, pv.size))]
        tok = _combine(res, mistake)[1]
    if mistake == "unclamped_empty":
        return tok
    return tok if 0 <= tok < n_vocab else 0


def topk(row, k):
    """(values float32, ids int32): the first k of order(row) -- fewer when fewer are comparable."""
    row = np.asarray(row, dtype=F32)
    o = order(row)[:k]
    return row[o], o.astype(np.int32)


def full_row(row, k):
    """topk_full_row, the answer behind a refusal: topk(row, k), then the NaNs by id."""
    row = np.asarray(row, dtype=F32)
    o = np.concatenate([order(row), np.flatnonzero(np.isnan(row))])[:k]
    return row[o], o.astype(np.int32)


# ---- topk_kernel ------------------------------------------------------------------------------------------------------------------------------------------------

def topk_threshold(pmax_val, nparts, k):
    """topk_kernel's t0: the k-th largest maximum of the 128 groups of 8 partial maxima (fmaxf: a NaN counts only in a group of nothing else), or -inf when k
    exceeds the groups or there are more than 1024 partials.  Returns (t0, raced): with k == 1 a group of NaNs alone claims rank 0 beside the true maximum --
    two lanes store t0, either may win; no case does that."""
    pv = np.asarray(pmax_val, dtype=F32)[:nparts]
    np_ = min(nparts, 1024)
    g = np.full(1024, -np.inf, F32)
    g[:np_] = pv[:np_]
    g = g.reshape(128, 8)
    allnan = np.isnan(g).all(axis=1)
    with np.errstate(invalid="ignore"):
        gm = np.where(allnan, F32(np.nan), np.fmax.reduce(g, axis=1)).astype(F32)
    ngroups = (np_ + 7) >> 3
    if not (k <= ngroups and nparts <= 1024):
        return F32(-np.inf), False
    t0, hits = F32(-np.inf), 0
    j = np.arange(128)
    for gi in range(128):
        with np.errstate(invalid="ignore"):
            beat = int(((gm > gm[gi]) | ((gm == gm[gi]) & (j < gi))).sum())
        if beat == k - 1:
            t0, hits = gm[gi], hits + 1
    return t0, hits > 1


def topk_kernel(row, pmax_val, nparts, k, mistake=None):
    """(n, values, ids): n == k with the k pairs, or n == -1 (more than 4096 logits reach the threshold, or fewer than k do) with nothing."""
    _check(mistake)
    row = np.asarray(row, dtype=F32)
    t0, raced = topk_threshold(pmax_val, nparts, k)
    assert not raced, "two groups claim rank k - 1"
    seen = row[:TOPK_REGS] if mistake == "beyond_regs_dropped" else row
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(seen > t0 if mistake == "candidates_gt" else seen >= t0)
    n = cand.size
    if n > TOPK_CAP or (mistake == "cap_off_by_one" and n == TOPK_CAP) or n < k:
        return -1, None, None
    v = row[cand].astype(np.float64)
    o = cand[np.lexsort((-cand if mistake == "rank_by_slot" else cand, -v))][:k]      # (a slot order the atomics may give: descending ids)
    return k, row[o], o.astype(np.int32)


# ---- the host selections ---------------------------------------------------------------------------------------------------------------------------------------

class _Insert:
    """TopkInsert: the k largest of the values offered so far, descending; offered in id order, an equal value stays behind the earlier one."""

    def __init__(self, k, ge=False):
        self.k, self.vals, self.ids, self.thr, self.ge = k, [], [], F32(-np.inf), ge
        self.offers = 0

    def offer(self, v, i):
        self.offers += 1
        full = len(self.vals) == self.k
        if v != v or (full and not (v >= self.thr if self.ge else v > self.thr)):
            return
        pos = len(self.vals) if not full else self.k - 1
        if not full:
            self.vals.append(v), self.ids.append(i)
        while pos > 0 and self.vals[pos - 1] < v:
            self.vals[pos], self.ids[pos] = self.vals[pos - 1], self.ids[pos - 1]
            pos -= 1
        self.vals[pos], self.ids[pos] = v, i
        if len(self.vals) == self.k:
            self.thr = self.vals[-1]

    def result(self):
        return len(self.vals), np.asarray(self.vals, F32), np.asarray(self.ids, np.int32)


def host_topk(row, k, mistake=None):
    """(count, values, ids): one pass; behind the first k comparable values a block of 16 is only looked at when its maximum beats the k-th value."""
    _check(mistake)
    row = np.asarray(row, dtype=F32)
    n, ge = row.size, mistake == "host_ge"
    top = _Insert(k, ge)
    i = 0
    while i < n and len(top.vals) < k:
        top.offer(row[i], i)
        i += 1
    while i + 16 <= n:
        blk = row[i:i + 16]
        m = F32(-np.inf) if np.isnan(blk).all() else F32(np.nanmax(np.append(blk, F32(-np.inf))))
        if (m >= top.thr) if ge else (m > top.thr):
            for j in range(16):
                top.offer(blk[j], i + j)
        i += 16
    while i < n:
        top.offer(row[i], i)
        i += 1
    return top.result()


def block_maxima(row, rows=64):
    """The maxima the resident launch leaves behind the row: fmaxf over each block (-inf for a block of NaNs alone)."""
    row = np.asarray(row, dtype=F32)
    nb = -(-row.size // rows)
    pad = np.full(nb * rows, -np.inf, F32)
    pad[:row.size] = row
    pad[np.isnan(pad)] = -np.inf
    return pad.reshape(nb, rows).max(axis=1)


def host_topk_blocks(row, k, bmax, mistake=None):
    """(count, values, ids): the walk over the 64-row blocks whose maximum reaches the k-th largest block maximum; host_topk when there are fewer than k or more
    than 1024 blocks, or a NaN among the maxima.  bmax must be the true maxima of the row's blocks: the walk never looks into a block whose maximum says no."""
    _check(mistake)
    row, bmax = np.asarray(row, dtype=F32), np.asarray(bmax, dtype=F32)
    nb = bmax.size
    if nb < k or nb > 1024 or np.isnan(bmax).any():
        return host_topk(row, k, mistake)
    t0 = np.sort(bmax)[::-1][k - 1]
    sel = _Insert(k)
    for b in np.flatnonzero(bmax > t0 if mistake == "blocks_select_gt" else bmax >= t0):
        for i in range(b * 64, min(row.size, b * 64 + 64)):
            sel.offer(row[i], i)
    return sel.result()
