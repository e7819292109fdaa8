"""Seeded inputs for the four kernels of the embedding tail, one stage at a time (biogpt_hip_embed_device): LayerNorm rows, pooling over packed passes and the
linear head, at the smallest shapes at which each kernel can still go wrong, on rows that no whole call produces.  The reference of a case is tests/embed_ref.py;
tests/test_embed_kernels_capi.py shows on the CPU that the cases are what this text says.

Row kinds (KINDS).  The first five are EXACT: every double sum a kernel takes over them is exact in any order (embed_ref.exact_in_any_order, asserted), so the
expected output is known bit for bit.  The last three are BOUNDED: held to embed_ref's *_bound against an exact sum.

  grid       k * 2^-4, |k| <= 128: short mantissas on a coarse binary grid
  stamp      integers that name their own place: pooled rows (seq * 64 + pos) * 2048 + element; head rows x[r] = (r + 1) e_{37 r mod W} + e_{W - 1} against
             w[o][d] = 2048 o + d + 1, so out[r][o] = (r + 1) w[o][37 r mod W] + w[o][W - 1]
  constant   pooling: every row of a sequence is the same full-mantissa row (the mean of n equal floats is that float); head: x[r] = 0.25 (r + 1) everywhere
             against rows of one full-mantissa value each
  subnormal  integers * 2^-149, with rows of zeros of both signs among them
  one_hot    one element +-2^j per row: normalises to exactly +-1, picks one weight
  gauss      N(0, 1), full mantissa
  mixed      magnitudes 1e18 and 1e-6 in one sum
  cancel     large terms that sum to nearly nothing
"""
import functools

import numpy as np

import embed_ref as E
from embed_ref import F32

EXACT_KINDS = ("grid", "stamp", "constant", "subnormal", "one_hot")
BOUNDED_KINDS = ("gauss", "mixed", "cancel")
KINDS = EXACT_KINDS + BOUNDED_KINDS


def _rng(*key):
    return np.random.default_rng([0x454D4244] + [int(k) for k in key])


def states(seq, pos):
    """[n, 8] int32 column states: n_past in word 0, seq_id in word 3 (bgk::SeqState)."""
    st = np.zeros((len(seq), 8), np.int32)
    st[:, 0], st[:, 3] = pos, seq
    return st


def grid(g, shape):
    return (g.integers(-128, 129, shape).astype(F32) * F32(2.0 ** -4)).astype(F32)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------------------

LN_WIDTHS = (1024, 4, 8, 252, 256, 260, 1028, 1280, 1600)      # 1024: the template; the others the generic kernel, below, at and above one wave's 64 chunks and 256 threads
LN_FAMILIES = ("normal", "outlier", "constant", "huge", "tiny", "offset", "near_zero_mean")
LN_SEEDS = {(4, "huge"): 1}      # (width, family) -> seed, where the default (0) gives a fragile row (chain_ref.ln_fragile)
LN_SCATTER = {1: (0, 0, 1, 1, 2, 2), 4: (0, 3, 5, 4, 9, 10)}      # slot_div -> the seq_id of six columns over three groups
LN_SCATTER_POS = (5, 2, 7, 0, 3, 6)                               # their positions: not monotone, P = 8
LN_P = 8


def ln_gain_bias(W):
    g = _rng(1, W)
    w = (F32(1.0) + g.standard_normal(W, dtype=F32) * F32(0.2)).astype(F32)
    b = (g.standard_normal(W, dtype=F32) * F32(0.1)).astype(F32)
    if W >= 64:      # a block of gain 0 with bias 0, one with a constant bias (tests/wide_models.py)
        w[32:48], b[32:48] = 0.0, 0.0
        w[48:64], b[48:64] = 0.0, 0.3
    return w, b


def ln_row(family, W, seed):
    """One row of chain_cases.ln_rows()'s families at width W; near_zero_mean: grid values and their negatives with one grid step left
    over (sums exact in any order, the mean 2^-4 / W; a mean of exactly 0 sits on the border between the float32 of -err and +err, which ln_fragile refuses)."""
    g = _rng(2, W, LN_FAMILIES.index(family), seed)
    x = g.standard_normal(W, dtype=F32)
    if family == "outlier":
        x[g.choice(W, max(1, min(4, W // 4)), replace=False)] *= F32(1e3)
    elif family == "constant":
        x[:] = F32(0.7)
    elif family == "huge":
        x *= F32(1e18)
    elif family == "tiny":
        x *= F32(1e-6)
    elif family == "offset":
        x += F32(300.0)
    elif family == "near_zero_mean":
        h = grid(g, W // 2)
        x = np.concatenate([h, -h])
        x[0] += F32(2.0 ** -4) if x[0] >= 0 else F32(-2.0 ** -4)
        x = x[g.permutation(W)]
    return x.astype(F32)


@functools.lru_cache(maxsize=None)
def ln_rows(W):
    """[len(LN_FAMILIES), W]: one row per family, none of them fragile (asserted by test_embed_kernels_capi.py)."""
    return np.stack([ln_row(f, W, LN_SEEDS.get((W, f), 0)) for f in LN_FAMILIES])


def ln_cases():
    """(name, kwargs of pkg.embed_device / embed_ref.layer_norm_rows): every width with one row and with a row per family; the scatter forms at two widths."""
    out = []
    for W in LN_WIDTHS:
        w, b = ln_gain_bias(W)
        rows = ln_rows(W)
        out.append(("ln W=%d N=1" % W, dict(x=rows[:1], w=w, b=b)))
        out.append(("ln W=%d N=%d" % (W, len(rows)), dict(x=rows, w=w, b=b)))
    for W in (1024, 260):
        w, b = ln_gain_bias(W)
        for div, seq in LN_SCATTER.items():
            out.append(("ln W=%d scatter slot_div=%d" % (W, div),
                        dict(x=ln_rows(W)[:6], w=w, b=b, states=states(seq, LN_SCATTER_POS), slot_div=div, P=LN_P, n_out_rows=3 * LN_P)))
    return out


# ---- pooling --------------------------------------------------------------------------------------------------------------------------------------------------------

POOL_WIDTHS = (4, 60, 64, 68, 1024, 1600)       # 1, 1, 1, 2, 16 and 25 column blocks of 64; 4, 60, 68: no multiple of 64; 1600: no multiple of 256
POOL_LENS = (15, 1, 16, 2, 17, 33, 40)           # the lengths 1, 2, 15, 16, 17, 33, 40, ordered so that at 16 columns per pass sequence 1 ends on a border, 2
#                                                  starts and ends on one, 3 starts on one, 4, 5 and 6 straddle one or more (flat starts 0, 15, 16, 32, 34, 51, 84)
PACKINGS = ("p16", "one", "p1")
THIRDS_W = 16


def pool_layout(lens, packing):
    """(seq, pos, pass_cols) of the flat token stream of the sequences, cut into passes of 16 columns, one pass, or passes of one column."""
    seq = np.concatenate([np.full(n, s) for s, n in enumerate(lens)])
    pos = np.concatenate([np.arange(n) for n in lens])
    total = len(seq)
    per = {"p16": 16, "one": total, "p1": 1}[packing]
    cols = [min(per, total - at) for at in range(0, total, per)]
    return seq, pos, cols


def pool_rows(kind, seq, pos, lens, W, seed=0):
    """[len(seq), W] float32 rows of one kind for the columns (seq, pos)."""
    g = _rng(3, KINDS.index(kind), W, seed)
    n = len(seq)
    e = np.arange(W)
    if kind == "grid":
        return grid(g, (n, W))
    if kind == "stamp":
        return ((seq[:, None] * 64 + pos[:, None]) * 2048 + e[None, :]).astype(F32)
    if kind == "constant":
        per_seq = g.standard_normal((len(lens), W), dtype=F32)
        return per_seq[seq]
    if kind == "subnormal":
        x = (g.integers(-4000, 4001, (n, W)).astype(np.float64) * 2.0 ** -149).astype(F32)
        zero = np.flatnonzero((seq % 3 == 1) | (pos % 5 == 2))      # whole sequences of zeros, and single rows of them
        x[zero] = np.where(g.integers(0, 2, (len(zero), W)) == 1, F32(-0.0), F32(0.0))
        return x
    if kind == "one_hot":
        x = np.zeros((n, W), F32)
        x[np.arange(n), (7 * seq + 3 * pos) % W] = np.ldexp(F32(1.0), (pos % 9) - 4) * np.where((seq + pos) % 2 == 0, F32(1.0), F32(-1.0))
        return x
    if kind == "gauss":
        return g.standard_normal((n, W), dtype=F32)
    if kind == "mixed":
        x = g.standard_normal((n, W), dtype=F32)
        return (x * np.where(g.integers(0, 2, (n, W)) == 1, F32(1e18), F32(1e-6))).astype(F32)
    if kind == "cancel":      # along a sequence: pairs t, -t, and a small remainder; along a row the same in pairs of elements
        x = (g.standard_normal((n, W), dtype=F32) * F32(1e-3)).astype(F32)
        big = (g.standard_normal((n, W), dtype=F32) * F32(1e6)).astype(F32)
        odd = pos % 2 == 1
        prev = np.flatnonzero(odd)
        big[prev] = -big[prev - 1]
        last_even = np.array([p % 2 == 0 and p == lens[s] - 1 for s, p in zip(seq, pos)])
        big[last_even] = 0.0
        return (x + big).astype(F32)
    raise ValueError(kind)


def _pool_case(name, kind, lens, seq, pos, cols, W, pooling, normalize, expect, seed=0, rows=None):
    x = pool_rows(kind, seq, pos, lens, W, seed) if rows is None else rows
    return dict(name=name, kind=kind, x=x, states=states(seq, pos), pass_cols=cols, lens=list(lens), pooling=pooling, normalize=normalize, expect=expect, W=W)


def thirds_rows():
    """One sequence of three rows at W = 16 whose sums are 3, 4 and 5: means 1, 4/3 and 5/3, two of them no floats, whose float32 roundings have squares on one grid
    2^-46 below 64:
    the normalisation of the ROUNDED mean is exact in any order, and differs from that of the unrounded one."""
    g = _rng(4)
    total = g.integers(3, 6, THIRDS_W).astype(np.float64)
    a, b = grid(g, THIRDS_W), grid(g, THIRDS_W)
    return np.stack([a, b, (total - a.astype(np.float64) - b.astype(np.float64)).astype(F32)])


def pool_cases(W):
    """The POOL cases at one width.  expect: 'bits' (out and acc bit for bit), 'acc' (the accumulator bit for bit, out within normalize_bound of the exact float32
    mean: the squares of a rounded mean are on no common grid), 'bound' (stage by stage, check_pool).  LAST is a copy: bit for bit for every kind."""
    cases = []
    kinds = KINDS if W in (68, 1600) else ("grid", "stamp", "gauss")
    for kind in kinds:
        exact = kind in EXACT_KINDS
        for packing in PACKINGS:
            seq, pos, cols = pool_layout(POOL_LENS, packing)
            tag = "pool W=%d %s %s " % (W, kind, packing)
            cases.append(_pool_case(tag + "last", kind, POOL_LENS, seq, pos, cols, W, "last", False, "bits"))
            cases.append(_pool_case(tag + "mean", kind, POOL_LENS, seq, pos, cols, W, "mean", False, "bits" if exact else "bound"))
            if packing == "p16":
                # x^2 of a full-mantissa row has 48 bits: over W elements on no common grid
                norm_exact = exact and kind != "constant"
                cases.append(_pool_case(tag + "last+normalize", kind, POOL_LENS, seq, pos, cols, W, "last", True, "bits" if norm_exact else "bound"))
                cases.append(_pool_case(tag + "none+normalize", kind, POOL_LENS, seq, pos, cols, W, "none", True, "bits" if norm_exact else "bound"))
                cases.append(_pool_case(tag + "mean+normalize", kind, POOL_LENS, seq, pos, cols, W, "mean", True, "acc" if exact else "bound"))
    # lengths 1, 2 and 16: the means of grid rows are short floats again, so mean + normalize is exact end to end
    lens = (16, 1, 2)
    seq, pos, cols = pool_layout(lens, "p16")
    cases.append(_pool_case("pool W=%d grid dyadic mean+normalize" % W, "grid", lens, seq, pos, cols, W, "mean", True, "bits"))
    # a pass that begins in the middle of a sequence (positions 3 .. 7 of sequence 0, then sequence 1 whole); one sequence of one token
    seq, pos = np.array([0] * 5 + [1] * 3), np.array([3, 4, 5, 6, 7, 0, 1, 2])
    for pooling in ("last", "mean"):
        cases.append(_pool_case("pool W=%d grid mid-sequence %s" % (W, pooling), "grid", (8, 3), seq, pos, [8], W, pooling, False, "bits"))
        cases.append(_pool_case("pool W=%d stamp single %s" % (W, pooling), "stamp", (1,), np.array([0]), np.array([0]), [1], W, pooling, pooling == "mean", "bits"))
    return cases


def thirds_case():
    seq, pos = np.zeros(3, np.int64), np.arange(3)
    return _pool_case("pool W=16 thirds mean+normalize", "grid", (3,), seq, pos, [3], THIRDS_W, "mean", True, "bits", rows=thirds_rows())


def all_pool_cases():
    return [c for W in POOL_WIDTHS for c in pool_cases(W)] + [thirds_case()]


def pool_expected(c, mistake=None):
    return E.pool_stage(c["x"], c["states"], c["pass_cols"], c["lens"], c["pooling"], c["normalize"], mistake)


def pool_sums(c):
    """The terms [n_terms, n_sums] of every double sum the case's kernels take (for exact_in_any_order): a sequence's rows; the squares of the rows normalised."""
    x = c["x"].astype(np.float64)
    sums = []
    seq = c["states"][:, 3]
    rows = x
    if c["pooling"] == "mean":
        sums += [x[seq == s] for s in range(len(c["lens"]))]
        rows = pool_expected(dict(c, normalize=False))[0][:-1].astype(np.float64)
    elif c["pooling"] == "last":
        rows = pool_expected(dict(c, normalize=False))[0][:-1].astype(np.float64)
    if c["normalize"]:
        sums.append((rows * rows).T)
    return sums


# ---- the head -------------------------------------------------------------------------------------------------------------------------------------------------------

# (n_rows, n_out, W): rows 1, 7, 8, 9, 17 (one group short, whole, one over, two over); outputs 1, 3, 4, 5, 256 (fewer than, as many as, more than the 4 waves);
# widths below one chunk per lane (4), 63, 64 and 65 chunks (252, 256, 260), 1024, and 1600 = 51,200 bytes of LDS
HEAD_SHAPES = ((1, 1, 4), (7, 3, 252), (8, 4, 256), (17, 5, 260), (9, 5, 1024), (1, 256, 252), (9, 256, 1600), (17, 3, 1600), (8, 1, 1024))
HEAD_ALL_KINDS = ((17, 5, 260), (7, 3, 252), (17, 3, 1600))      # the shapes every kind runs at; the others: grid, stamp, gauss


def head_inputs(kind, n_rows, n_out, W, seed=0):
    """(x [n_rows, W], w [n_out, W], b [n_out]) of one kind."""
    g = _rng(5, KINDS.index(kind), n_rows, n_out, W, seed)
    b = grid(g, n_out)
    if kind == "grid":
        return grid(g, (n_rows, W)), grid(g, (n_out, W)), b
    if kind == "stamp":
        x = np.zeros((n_rows, W), F32)
        r = np.arange(n_rows)
        x[r, (37 * r) % W] = r + 1
        x[:, W - 1] += 1
        w = (np.arange(n_out)[:, None] * 2048 + np.arange(W)[None, :] + 1).astype(F32)
        return x, w, np.zeros(n_out, F32)
    if kind == "constant":      # W * 0.25 (r + 1) * c: 24 + 5 + 11 bits, a double but no float: the sum is rounded behind the bias, not in front of it
        x = np.repeat((F32(0.25) * (np.arange(n_rows) + 1)).astype(F32)[:, None], W, axis=1)
        w = np.repeat(g.standard_normal(n_out, dtype=F32)[:, None], W, axis=1)
        return x, w, g.standard_normal(n_out, dtype=F32)      # (a full-mantissa bias: finer than the sum's float32 spacing)
    if kind == "subnormal":
        x = (g.integers(-4000, 4001, (n_rows, W)).astype(np.float64) * 2.0 ** -149).astype(F32)
        x[1::3] = np.where(g.integers(0, 2, x[1::3].shape) == 1, F32(-0.0), F32(0.0))
        return x, grid(g, (n_out, W)), (b.astype(np.float64) * 2.0 ** -140).astype(F32)
    if kind == "one_hot":
        x = np.zeros((n_rows, W), F32)
        r = np.arange(n_rows)
        x[r, (11 * r + W - 1) % W] = np.ldexp(F32(1.0), (r % 9) - 4) * np.where(r % 2 == 0, F32(1.0), F32(-1.0))
        return x, g.standard_normal((n_out, W), dtype=F32), np.zeros(n_out, F32)
    if kind == "gauss":
        return g.standard_normal((n_rows, W), dtype=F32), (g.standard_normal((n_out, W), dtype=F32) * F32(0.05)).astype(F32), g.standard_normal(n_out, dtype=F32)
    if kind == "mixed":
        x = g.standard_normal((n_rows, W), dtype=F32)
        x = (x * np.where(g.integers(0, 2, (n_rows, W)) == 1, F32(1e18), F32(1e-6))).astype(F32)
        return x, g.standard_normal((n_out, W), dtype=F32), g.standard_normal(n_out, dtype=F32)
    if kind == "cancel":      # pairs of elements whose products cancel, and a small remainder
        x = (g.standard_normal((n_rows, W), dtype=F32) * F32(1e3)).astype(F32)
        w = (g.standard_normal((n_out, W), dtype=F32) * F32(1e3)).astype(F32)
        x[:, 1::2], w[:, 1::2] = x[:, 0::2], -w[:, 0::2]
        x[:, 0] += F32(1e-3)
        return x, w, (b * F32(1e-3)).astype(F32)
    raise ValueError(kind)


def head_cases():
    cases = []
    for shape in HEAD_SHAPES:
        for kind in (KINDS if shape in HEAD_ALL_KINDS else ("grid", "stamp", "gauss")):
            x, w, b = head_inputs(kind, *shape)
            for bias in (True, False):
                cases.append(dict(name="head rows=%d out=%d W=%d %s%s" % (shape + (kind, " +b" if bias else "")), kind=kind, x=x, w=w, b=b if bias else None,
                                  expect="bits" if kind in EXACT_KINDS else "bound"))
    return cases


def head_border_case():
    """(9, 5, 2048) on the grid kind: the widest rows head_rows_kernel can be launched at (8 * 2048 * 4 = 65,536 bytes of LDS); beside the issue's shapes."""
    x, w, b = head_inputs("grid", 9, 5, 2048)
    return dict(name="head rows=9 out=5 W=2048 grid +b", kind="grid", x=x, w=w, b=b, expect="bits")


def head_expected(c, mistake=None):
    return E.head_stage(c["x"], c["w"], c["b"], mistake)


def head_sums(c):
    return [(c["w"].T.astype(np.float64)[:, None, :] * c["x"].T.astype(np.float64)[:, :, None]).reshape(c["x"].shape[1], -1)]


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------------------------------

def differs_in_bits(a, b):
    return a.shape != b.shape or a.tobytes() != b.tobytes()


def assert_bits(got, want, what):
    """Bit equality of a whole output, guard row included."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.argwhere(got.view(u) != want.view(u))
    if len(bad):
        first = tuple(int(i) for i in bad[0])
        assert False, (what, "%d elements differ" % len(bad), "first at", first, "got", got[first], "want", want[first], "others", [tuple(int(i) for i in b) for b in bad[1:6]])


def assert_guard(a, rows, what):
    """Rows `rows` of a whole output still hold the 0xff preset."""
    assert (a[rows].view(np.uint8) == 0xFF).all(), (what, "guard bytes written", np.argwhere(a[rows].view(np.uint8) != 0xFF)[:4].tolist())


def _normalize_ref(rows):
    """(float64 x / |x| on an exact sum of squares (no pairwise sum), embed_ref.normalize_bound) of float32 rows; a zero row stays zero."""
    r64 = rows.astype(np.float64)
    nrm = np.sqrt(E.exact_sum((r64 * r64).T))[:, None]
    return r64 / np.where(nrm == 0.0, 1.0, nrm), E.normalize_bound(rows)


def check_pool(c, out, acc, what=None):
    """Hold one POOL result -- the probe's, or a mistaken restatement's -- to what the case owes (AssertionError otherwise).  Guard rows keep their preset.  LAST
    is a copy and 'bits' cases are exact: bit for bit, the accumulator too.  Elsewhere stage by stage, each stage on ITS OWN input, within embed_ref's bound
    for that stage and nothing more:
      the accumulator   bit for bit on exact kinds ('acc'); else within n * EPS64 * sum |terms| of the exact sum of the sequence's rows
      the kernel's mean own = (float)(acc / len), one double division and a cast as pool_finish_kernel's: within mean_bound of the exact mean
      MEAN              out is `own`, bit for bit
      + normalize       out within normalize_bound(own) of own / |own| on an exact sum
      LAST / NONE + normalize: the same on the source rows."""
    what = what or c["name"]
    want, want_acc = pool_expected(c)
    assert out.shape == want.shape and out.dtype == F32, (what, out.shape, want.shape)
    assert_guard(out, [-1], what)
    if want_acc is not None:
        assert acc is not None and acc.shape == want_acc.shape and acc.dtype == np.float64, what
        assert_guard(acc, [-1], what + " (acc)")
    if c["expect"] == "bits" or (c["pooling"] == "last" and not c["normalize"]):
        assert_bits(out, want, what)
        if want_acc is not None:
            assert_bits(acc, want_acc, what + " (acc)")
        return
    rows = pool_expected(dict(c, normalize=False))[0][:-1]      # LAST / NONE: the source rows
    if c["pooling"] == "mean":
        x, seq, lens = c["x"], c["states"][:, 3], np.asarray(c["lens"], dtype=np.float64)
        per = [x[seq == s] for s in range(len(lens))]
        if c["expect"] == "acc":
            assert_bits(acc, want_acc, what + " (acc)")
        else:
            exact = np.stack([E.exact_sum(r.astype(np.float64)) for r in per])
            allow = np.stack([len(r) * E.EPS64 * np.abs(r.astype(np.float64)).sum(axis=0) for r in per])
            assert np.isfinite(acc[:-1]).all() and (np.abs(acc[:-1] - exact) <= allow).all(), (what, "accumulator beyond n * EPS64 * sum |terms| of the exact sum")
        with np.errstate(all="ignore"):
            own = (acc[:-1] / lens[:, None]).astype(F32)
        if c["expect"] != "acc":      # ('acc': the accumulator is the exact sum, bit for bit, so `own` is the restated mean)
            mean_ref = np.stack([E.exact_sum(r.astype(np.float64)) / len(r) for r in per])
            assert_within(own, mean_ref, np.stack([E.mean_bound(r) for r in per]), what + " (the mean of the returned accumulator)")
        if not c["normalize"]:
            assert_bits(out[:-1], own, what + " (out against (float)(acc / len))")
            return
        rows = own
    ref, bound = _normalize_ref(rows)
    assert_within(out[:-1], ref, bound, what)


def head_bound(c):
    x, w = c["x"].astype(np.float64), c["w"].astype(np.float64)
    t = E.exact_sum(w.T[:, None, :] * x.T[:, :, None])
    return (t if c["b"] is None else t + c["b"].astype(np.float64)), E.head_bound(c["x"], c["w"], c["b"])


def assert_within(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: %s, max |diff| %.2e, at most %.3f of the bound" % (what, got.shape, float(err.max()), worst))
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, worst)
