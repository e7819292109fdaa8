"""Seeded inputs for the token tail, one stage at a time (biogpt_hip_tail_device): rows no whole call produces -- tied, infinite and NaN -- at the smallest
shapes at which each kernel of the tail can still go wrong.  The reference of a case is tests/tail_ref.py; tests/test_tail_restatement.py shows on the CPU that
the cases are what this text says.

PARTIALS  one column of K = 1024 through the single-token lm_head launch.  Weights are random codes under random f16 scales; duplicated rows give equal logits
          whatever the arithmetic.  Per (format, M) one launch with four ties among the partials' rows: a part's maximum copied to the row beside it (same
          wave), to a row of another wave of the part, into the last -- partial -- part, and the row's maximum copied into the LAST row of an earlier part and
          the FIRST row of a later one (the winner's lowest copy stands late in its own workgroup, the higher copy early in its).  Q8_0 rows get raw-edited scale
          bits in their first block: f16 NaN (a NaN logit), +-inf with codes that make the block's dot positive (a +-inf logit).
FINISH    (value, id) pairs straight into argmax_kernel.
TOPK      rows of small integers (ties everywhere) with the partial maxima of 64-row blocks, true or stale; the same cases go to the host selections."""
import functools

import numpy as np

import chain_cases
import chain_ref as R
import tail_ref as T
from chain_ref import F32

F32_TYPE = 0
PARTIAL_M = (1, 16, 63, 64, 65, 127, 128, 129, 1040, 1045)
FULL_M = 42384
NAN16, PINF16, NINF16 = 0x7E00, 0x7C00, 0xFC00
K = 1024


def _rng(*key):
    return np.random.default_rng([0x5441494C] + [int(k) for k in key])


def rows_per_part(wtype, M, lm_stream=True):
    """Rows behind one partial, by the launch rules of engine.hip: lm_stream_kernel's 64-row blocks from 8192 rows on; matvec_fast_kernel's four waves of
    2 * steps rows (8 steps, halved while the grid stays below 128); the generic kernel's waves of 64 / min(64, K / 4) rows for a float file."""
    if wtype == F32_TYPE:
        nw = 4
        while nw > 1 and -(-M // nw) < 256:
            nw >>= 1
        steps = 1
        while -(-M // (nw * steps)) > 1024:
            steps += 1
        return nw * steps
    if lm_stream and M >= 8192:
        return 64
    steps = 8
    while steps > 1 and -(-M // (8 * steps)) < 128:
        steps >>= 1
    return 8 * steps


def expected_kernel(wtype, M, lm_stream=True):
    return 2 if wtype == F32_TYPE else 0 if (lm_stream and M >= 8192) else 1


@functools.lru_cache(maxsize=None)
def column():
    """x, ln_w, ln_b: an N(0, 1) column under the chain cases' gain and bias (block 5 of the LayerNorm's output is zero: its Q8 scale is 0)."""
    w, b = chain_cases.ln_gain_bias()
    return _rng(1).standard_normal(K, dtype=F32), w, b


def base_weights(wtype, M):
    """File-format bytes uint8 [M, 32, bb] (float32 [M, 1024] for F32): random codes, scales of magnitude 0.005 .. 0.03 of either sign."""
    g = _rng(2, wtype, M)
    if wtype == F32_TYPE:
        return (g.standard_normal((M, K), dtype=F32) * F32(0.02)).astype(F32)
    top = 256 if wtype == R.Q8_0 else 32 if wtype in (R.Q5_0, R.Q5_1) else 16
    codes = g.integers(0, top, size=(M, 32, 32)).astype(np.uint8)
    d = chain_cases.f16_bits(g.uniform(0.005, 0.03, size=(M, 32)) * g.choice([-1.0, 1.0], size=(M, 32)))
    m = chain_cases.f16_bits(g.uniform(-0.01, 0.01, size=(M, 32)))
    return chain_cases.encode_weights(wtype, codes, d, m)


def ref_row(wtype, raw, mistake=None):
    """The logits row as the oracle computes it (chain_ref, bit for bit for the block formats); for a float file the float64 dot of the LayerNorm's row."""
    x, w, b = column()
    if wtype == F32_TYPE:
        with np.errstate(invalid="ignore", over="ignore"):
            return (raw.astype(np.float64) @ R.layer_norm(x, w, b).astype(np.float64)).astype(F32)
    q, d, s = R.lnq(x[None], w, b, R.Q81[wtype])
    with np.errstate(invalid="ignore", over="ignore"):
        return R.block_sums(wtype, raw, raw.shape[0], K, q, d, s)[0]


def place_ties(wtype, raw, rpp):
    """Copies rows of `raw` in place so that the maxima tie as the module text says; returns {kind: (part, rows that tie)}."""
    M = raw.shape[0]
    row = ref_row(wtype, raw)
    nparts = -(-M // rpp)
    made = {}

    def part_rows(p):
        return p * rpp, min(M, (p + 1) * rpp)

    def dup(kind, p, dst):
        r0, r1 = part_rows(p)
        src = r0 + int(np.argmax(row[r0:r1]))
        if dst == src or not (r0 <= dst < r1):
            return
        raw[dst] = raw[src]
        row[dst] = row[src]
        made[kind] = (p, sorted((src, dst)))

    wave = max(rpp // 4, 1)
    if rpp >= 2 and M >= 2:
        r0, r1 = part_rows(0)
        src = r0 + int(np.argmax(row[r0:r1]))
        dup("same wave", 0, src ^ 1 if (src ^ 1) < r1 else src - 1)
    if rpp >= 4 and nparts >= 2:
        r0, r1 = part_rows(1)
        src = r0 + int(np.argmax(row[r0:r1]))
        dup("across waves", 1, r0 + (src - r0 + 2 * wave) % rpp if r0 + (src - r0 + 2 * wave) % rpp < r1 else r0)
    if nparts >= 3 and part_rows(nparts - 1)[1] - part_rows(nparts - 1)[0] >= 2:
        r0, r1 = part_rows(nparts - 1)
        src = r0 + int(np.argmax(row[r0:r1]))
        dup("last part", nparts - 1, r1 - 1 if src != r1 - 1 else r0)
    if nparts >= 5:      # the row's maximum into the last row of part a and the first row of part b > a, both beyond the parts used above
        a, b = 2, nparts - 2
        top = int(np.argmax(np.where(np.isnan(row), -np.inf, row)))
        lo, hi = part_rows(a)[1] - 1, part_rows(b)[0]
        if top not in (lo, hi) and a < b:
            raw[lo], raw[hi] = raw[top], raw[top]
            made["across parts"] = (a, sorted({lo, hi, top}))
    return made


def q8_edit(raw, r, bits):
    """The scale of row r's first block <- bits; for +-inf the block's codes <- the activation's own codes, so that the block's dot is positive."""
    raw[r, 0, 0:2] = np.array([bits], "<u2").view(np.uint8)
    if bits in (PINF16, NINF16):
        x, w, b = column()
        raw[r, 0, 2:34] = R.lnq(x[None], w, b, False)[0][0, :32].view(np.uint8)


# local rows of a 64-row block: (a NaN here, the block's true maximum there) -- the first finisher lane of wave 0 with the maximum on the lane beside it and in
# another wave; a middle lane of lm_stream_kernel's / the in-launch kernels' groups (wave 1, lane 8 -> lane 9) and of matvec_fast_kernel's (wave 2, lane 2 -> 6);
# the last lane of a group (benign: nothing is combined into it)
NAN_PAIRS_64 = ((0, 1), (0, 40), (34, 35), (34, 38), (63, 62))
NAN_PAIRS_8 = ((0, 1), (0, 5), (1, 0), (7, 2))      # an 8-row part of matvec_fast_kernel at small M: waves of two rows


def place_edits(raw, rpp, first_part):
    """Q8_0: NaN / inf scales by part from first_part on; returns {what: part}.  The maximum of a NaN part is a copy of one of the row's largest rows."""
    M = raw.shape[0]
    row = ref_row(R.Q8_0, raw)
    big = [int(i) for i in np.argsort(-row)[:16]]
    pairs = NAN_PAIRS_64 if rpp == 64 else NAN_PAIRS_8
    made, p = {}, first_part
    for n, (at, mx) in enumerate(pairs):
        raw[p * rpp + mx] = raw[big[n]]
        q8_edit(raw, p * rpp + at, NAN16)
        made["nan %d max %d" % (at, mx)] = p
        p += 1
    for r in range(p * rpp, (p + 1) * rpp):
        q8_edit(raw, r, NAN16)
    made["all nan"] = p
    for r in range((p + 1) * rpp, (p + 2) * rpp):
        q8_edit(raw, r, NINF16)
    made["all -inf"] = p + 1
    q8_edit(raw, (p + 2) * rpp + 1, NINF16)
    made["one -inf"] = p + 2
    q8_edit(raw, (p + 3) * rpp + 3, PINF16)
    q8_edit(raw, (p + 3) * rpp + rpp - 1, PINF16)
    made["+inf tied in a part"] = p + 3
    q8_edit(raw, (p + 5) * rpp + 2, PINF16)
    made["+inf in a later part"] = p + 5
    assert (p + 6) * rpp <= M
    return made


@functools.lru_cache(maxsize=4)
def partials_case(wtype, M, edits=False, lm_stream=True):
    """dict(raw, rpp, ties, edits, want): the weights (read-only), the rows per partial, what place_ties / place_edits made, the reference row."""
    rpp = rows_per_part(wtype, M, lm_stream)
    raw = base_weights(wtype, M).copy()
    ties = place_ties(wtype, raw, rpp)
    made = place_edits(raw, rpp, 6) if edits else {}
    raw.setflags(write=False)
    return dict(raw=raw, rpp=rpp, ties=ties, edits=made, want=ref_row(wtype, raw))


def same_row(got, want):
    """Bit for bit, every NaN of one a NaN of the other."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got[~nan].view(np.uint32) == want[~nan].view(np.uint32)).all())


# ---- FINISH -------------------------------------------------------------------------------------------------------------------------------------------------------

FINISH_NPARTS = (1, 255, 256, 257, 663, 4096)
N_VOCAB = 42384


def finish_cases():
    """(name, pmax_val float32 [n], pmax_idx int32 [n]).  A partial's id lies in its own 64-row block unless the case is about ids."""
    out = []
    for n in FINISH_NPARTS:
        g = _rng(3, n)
        idx = (np.arange(n) * 64 + g.integers(0, 64, n)).astype(np.int32) % N_VOCAB if n <= 663 else g.permutation(N_VOCAB)[:n].astype(np.int32)
        val = g.standard_normal(n).astype(F32)
        out.append(("n%d plain" % n, val, idx))
        v = val.copy()
        v[:] = np.round(v * 2) / 2                                                     # a handful of values: ties everywhere
        out.append(("n%d ties" % n, v, idx))
        v = val.copy()
        top = F32(9.0)
        for at in {n - 1, n // 2, min(n - 1, 128), min(n - 1, 255), min(n - 1, 256), n // 3}:      # across the 256 threads, the reduction halves and a thread's own walk
            v[at] = top
        out.append(("n%d top tied" % n, v, idx))
        i2 = idx.copy()
        i2[np.flatnonzero(v == top)] = np.sort(i2[v == top])[::-1]                     # the lowest id in the LAST tied partial
        out.append(("n%d top tied, lowest id last" % n, v, i2))
        out.append(("n%d all -inf" % n, np.full(n, -np.inf, F32), idx))
        out.append(("n%d all nan" % n, np.full(n, np.nan, F32), idx))
        out.append(("n%d never written" % n, np.full(n, -np.inf, F32), np.full(n, T.NONE_IDX, np.int32)))
        v = np.full(n, np.nan, F32)
        v[n // 2] = F32(-3.5)
        out.append(("n%d one comparable among nans" % n, v, idx))
        v = val.copy()
        v[0] = np.nan
        out.append(("n%d nan first" % n, v, idx))
        v = val.copy()
        v[g.integers(0, n)] = np.inf
        out.append(("n%d +inf" % n, v, idx))
    out.append(("id past the vocabulary", np.array([1.0, 2.0], F32), np.array([5, N_VOCAB], np.int32)))
    out.append(("negative id", np.array([1.0, 2.0], F32), np.array([5, -7], np.int32)))
    return out


# ---- TOPK and the host selections ------------------------------------------------------------------------------------------------------------------------------------

TOPK_K = (1, 2, 7, 40, 64)
TOPK_V = (1, 63, 1023, 1024, 1025, 4096, 4097, 42384, 43007, 43008, 43009, 44100)


def _int_row(g, V, levels):
    return g.integers(0, levels, V).astype(F32)


def topk_cases():
    """dicts(name, row, pmax (the partial maxima handed to topk_kernel), k, true_max (pmax is block_maxima(row): the case also goes to host_topk_blocks))."""
    out = []

    def add(name, row, k, pmax=None, true_max=None):
        row = np.asarray(row, F32)
        tm = pmax is None if true_max is None else true_max
        pmax = T.block_maxima(row) if pmax is None else np.asarray(pmax, F32)
        out.append(dict(name=name, row=row, k=k, pmax=pmax, true_max=tm))

    for V in sorted(set(TOPK_V + TOPK_K)):
        for k in TOPK_K:
            if k > V or (V not in TOPK_V and k != V):      # (V == k: the whole row is the answer)
                continue
            g = _rng(4, V, k)
            row = g.standard_normal(V).astype(F32)
            if V >= 43009:                              # members of the answer beyond element 43008
                row[43008:] += F32(6.0) * (g.random(V - 43008) < 0.02)
                row[V - 1] = F32(9.0)
            add("V%d k%d normal" % (V, k), row, k)
            if V >= 63:
                row = _int_row(g, V, 8 if V < 40000 else 4000)
                if V >= 43009:
                    row[V - 3:] = row.max()
                add("V%d k%d ties" % (V, k), row, k)
    g = _rng(5)
    for k in (2, 7, 40, 64):
        # a tie that straddles the k-th place: k - 1 values above, then three equal values
        row = g.standard_normal(40000).astype(F32)                                          # (625 maxima: 79 groups, enough for a threshold at k = 64)
        row[g.permutation(40000)[:k - 1]] = F32(10.0) + np.arange(k - 1, dtype=F32)
        row[[4990, 77, 2500]] = F32(8.0)
        add("k%d tie straddles place k" % k, row, k)
    for k in (1, 7, 64):
        # exactly 4096 / 4097 candidates: that many logits at the top value, every block maximum equal to it
        for n in (4096, 4097):
            row = np.zeros(32768, F32)                                                   # (512 maxima: 64 groups, enough for a threshold at k = 64)
            heads = np.arange(0, 32768, 64)                                              # every one of the blocks holds one
            row[heads] = F32(1.0)
            row[g.permutation(np.setdiff1d(np.arange(32768), heads))[:n - 512]] = F32(1.0)
            add("k%d %d candidates" % (k, n), row, k)
    row = g.standard_normal(640).astype(F32)
    add("nparts 10 < k 40", row, 40)
    for nb in (1024, 1025):
        add("nparts %d" % nb, g.standard_normal(nb * 64 - 5).astype(F32), 7)
    row = g.standard_normal(3000).astype(F32)
    row[[5, 900, 2999]] = np.inf
    row[[6, 1700]] = -np.inf
    row[[0, 64, 901, 2998]] = np.nan
    for k in (1, 2, 7):
        add("k%d +-inf and nan" % k, row, k)
    row = np.full(300, -np.inf, F32)
    row[17] = np.nan
    add("all -inf but a nan", row, 7)
    row = np.full(200, np.nan, F32)
    row[[3, 150, 151]] = [1.0, 2.0, 2.0]
    add("three comparable, k 7", row, 7)
    add("three comparable, k 2", row, 2)
    row = g.standard_normal(4000).astype(F32)
    pm = T.block_maxima(row)
    p2 = pm.copy()
    p2[[1, 9, 33]] = np.nan                               # NaN among the partial maxima, each in a group with others
    add("nan among the maxima", row, 7, p2, true_max=False)
    p2 = pm.copy()
    p2[16:24] = np.nan                                     # a whole group of NaNs (k >= 2: with k == 1 two lanes would claim rank 0)
    add("a group of nan maxima", row, 7, p2, true_max=False)
    add("stale maxima, too high", row, 7, pm + F32(5.0), true_max=False)
    add("stale maxima, too low", row, 7, pm - F32(5.0), true_max=False)
    add("stale maxima, another row's", row, 7, T.block_maxima(g.standard_normal(4000).astype(F32)), true_max=False)
    big = g.standard_normal(9000).astype(F32)
    add("stale maxima, below the whole row", big, 7, T.block_maxima(big) - F32(50.0), true_max=False)
    add("stale maxima, never written", big, 40, np.zeros(141, F32), true_max=False)
    return out
