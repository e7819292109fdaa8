"""Scalar restatement of contrastive search as biogpt_hip_generate_contrastive defines it ("Contrastive search"):
transformers' GenerationMixin._contrastive_search for one prompt, one EOS id or none, no logits processors -- with its unspecified orders
made explicit.  Driven by a callback, so that the same code can be pinned to transformers on the CPU (test_contrast_restatement.py) and
then hold the engine to it (test_gpu_contrast.py).

    rows(prefixes) -> (hidden float32 [len(prefixes)][d], logits float32 [len(prefixes)][n_vocab]): the hidden row after the final
    LayerNorm and the logits row of the LAST token of prompt + prefix.  The empty prefix is the prompt's last token.

The order of a dot (csrc/kernels_contrast.hip.h): the row is d / 4 chunks of 4 elements, chunk c belongs to lane c % 64; a lane adds its
exact f32 x f32 products in ascending element order into one double; the 64 lane sums are combined as wave_sum_f64 combines them (lane
i with i ^ 1, then i ^ 2, then its mirror inside each 8, then inside each 16, then (s0 + s16) + (s32 + s48)).

Not a test module: a helper the tests import."""
import numpy as np

_I = np.arange(64)
_STEPS = (_I ^ 1, _I ^ 2, (_I & ~7) | (7 - (_I & 7)), (_I & ~15) | (15 - (_I & 15)))


def wave_sum(v):
    """wave_sum_f64 over the last axis (64 doubles)."""
    v = np.asarray(v, dtype=np.float64)
    for perm in _STEPS:
        v = v + v[..., perm]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def dots(a, rows):
    """dot(a, rows[t]) for every row t, in the kernel's order.  a: [d], rows: [T][d], 4 | d.  Returns float64 [T]."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    T, d = r.shape
    assert d % 4 == 0 and a.shape == (d,)
    pad = (-d) % 256
    prod = np.pad(r * a[None, :], ((0, 0), (0, pad))).reshape(T, -1, 64, 4)      # (an f32 x f32 product is exact in double)
    acc = np.zeros((T, 64), dtype=np.float64)
    for i in range(prod.shape[1]):
        for c in range(4):
            acc = acc + prod[:, i, :, c]
    return wave_sum(acc)


def sq_norms(rows):
    r = np.asarray(rows, dtype=np.float32)
    return np.array([dots(r[t], r[t:t + 1])[0] for t in range(r.shape[0])], dtype=np.float64)


def penalties(cand, ctx_rows, ctx_norms=None):
    """pen_j = max_i sim(cand[j], ctx_rows[i]), sim = (float)(dot / sqrt(na * nb)), 0 where a norm is 0.  float32 [k]."""
    cand = np.asarray(cand, dtype=np.float32)
    ctx_rows = np.asarray(ctx_rows, dtype=np.float32)
    nb = sq_norms(ctx_rows) if ctx_norms is None else np.asarray(ctx_norms, dtype=np.float64)
    out = np.zeros(cand.shape[0], dtype=np.float32)
    for j in range(cand.shape[0]):
        na = dots(cand[j], cand[j:j + 1])[0]
        dt = dots(cand[j], ctx_rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            sim = (dt / np.sqrt(na * nb)).astype(np.float32)
        sim[(nb == 0.0) | (na == 0.0)] = np.float32(0.0)
        out[j] = sim.max()
    return out


def scores_of(probs, pen, alpha):
    """score_j = (float)((1 - (double)alpha) * (double)p_j - (double)alpha * (double)pen_j), alpha a float."""
    a = float(np.float32(alpha))
    p = np.asarray(probs, dtype=np.float32).astype(np.float64)
    q = np.asarray(pen, dtype=np.float32).astype(np.float64)
    return ((1.0 - a) * p - a * q).astype(np.float32)


def pick(scores):
    """(winner: highest score, lowest j on ties; margin: best minus second best, inf for a single candidate)."""
    s = np.asarray(scores, dtype=np.float32)
    w = int(np.argmax(s))       # the first maximum
    rest = np.delete(s, w)
    return w, (float(s[w]) - float(rest.max()) if rest.size else float("inf"))


def rank(cand, ctx_rows, probs, alpha):
    """What biogpt_hip_contrast_rank_device computes: (pen, score, winner, margin)."""
    pen = penalties(cand, ctx_rows)
    sc = scores_of(probs, pen, alpha)
    w, margin = pick(sc)
    return pen, sc, w, margin


def candidates(logits_row, k):
    """The k largest values (value descending, lower id first on equal values) and p_j = (float)(exp((double)l_j - (double)m) / S), m and S as
    lp_row_stats has them up to the order of the exponential sum (S sums f32 exp(l - m) terms)."""
    l = np.asarray(logits_row, dtype=np.float32)
    ids = np.lexsort((np.arange(l.size), -l.astype(np.float64)))[:k]
    m = l.max()
    S = np.exp((l - m).astype(np.float32)).astype(np.float64).sum()
    p = (np.exp(l[ids].astype(np.float64) - float(m)) / S).astype(np.float32)
    return [int(i) for i in ids], p


def search(rows, prompt_hidden, n_predict, top_k, alpha, eos_id=-1):
    """prompt_hidden: float32 [L - 1][d], the hidden rows of the prompt without its last token.  Returns (ids, scores float32, margins)."""
    h0, l0 = rows([[]])
    ctx = [np.asarray(r, dtype=np.float32) for r in np.asarray(prompt_hidden, dtype=np.float32).reshape(-1, np.asarray(h0).shape[1])]
    ctx.append(np.asarray(h0[0], dtype=np.float32))
    norms = list(sq_norms(np.stack(ctx)))
    cand_row = np.asarray(l0[0], dtype=np.float32)
    ids, scores, margins = [], [], []
    for _ in range(n_predict):
        cid, p = candidates(cand_row, top_k)
        hid, lg = rows([ids + [c] for c in cid])
        hid = np.asarray(hid, dtype=np.float32)
        pen = penalties(hid, np.stack(ctx), norms)
        sc = scores_of(p, pen, alpha)
        w, margin = pick(sc)
        ids.append(cid[w]); scores.append(sc[w]); margins.append(margin)
        if eos_id >= 0 and cid[w] == eos_id:
            break
        ctx.append(hid[w]); norms.append(dots(hid[w], hid[w:w + 1])[0])
        cand_row = np.asarray(lg[w], dtype=np.float32)
    return ids, np.asarray(scores, dtype=np.float32), margins


class OracleRows:
    """rows() from the CPU oracle in the engine's order: the prompt in chunks of n_batch (the reference's unmasked chunk) with the hidden tap after
    the final LayerNorm, then each prefix of generated tokens one at a time from n_past = n_prompt.  tap(model, tokens, n_past) -> (hidden rows
    of every token fed, logits row of the last).  A prefix is re-fed from where it leaves the one fed before it; rows are cached per prefix."""

    def __init__(self, oracle_model, prompt, n_batch, tap):
        self.o, self.tap, self.n_prompt = oracle_model, tap, len(prompt)
        hid, lg = [], None
        for at in range(0, len(prompt), n_batch):
            h, lg = tap(self.o, list(prompt[at:at + n_batch]), at)
            hid.append(np.asarray(h, dtype=np.float32))
        hid = np.concatenate(hid)
        self.prompt_hidden = hid[:-1].copy()
        self.cache = {(): (hid[-1].copy(), np.asarray(lg, dtype=np.float32).copy())}
        self.fed = []

    def row(self, prefix):
        prefix = tuple(prefix)
        if prefix in self.cache:
            return self.cache[prefix]
        common = 0
        while common < min(len(self.fed), len(prefix)) and self.fed[common] == prefix[common]:
            common += 1
        if common == len(prefix):
            common -= 1
        self.fed = list(self.fed[:common])
        for j in range(common, len(prefix)):
            h, lg = self.tap(self.o, [prefix[j]], self.n_prompt + j)
            self.fed.append(prefix[j])
            self.cache[tuple(self.fed)] = (np.asarray(h, dtype=np.float32)[-1].copy(), np.asarray(lg, dtype=np.float32).copy())
        return self.cache[prefix]

    def __call__(self, prefixes):
        got = [self.row(p) for p in prefixes]
        return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
