"""Inputs of the SIMD association's tests, shared by tests/test_assoc_restatement.py (CPU: the restatement against the oracle, and that the inputs tell the two
associations apart) and tests/test_gpu_assoc_kernels.py (GPU: the kernels against the restatement).  Everything follows from a seed."""
import numpy as np

import assoc_ref as A
import chain_ref as R

F32 = np.float32
SENTINEL = F32(3.0e30)                  # large and finite: a row the kernel must not read shows in the result


def _seed(*parts):
    return abs(hash(tuple(int(p) for p in parts))) % (2 ** 32)


# ---- activation rows: three hostile blocks and random ones ---------------------------------------------------------------------------------------------------

def tie_block():
    """amax = 127: d = 1, id = 1, and 31 elements k + 0.5 -- nearest-even and roundf part on every one of them."""
    k = np.arange(31, dtype=F32)
    v = (k + F32(0.5)) * np.where(np.arange(31) % 2 == 0, F32(1), F32(-1))
    return np.concatenate([[F32(127.0)], v]).astype(F32)


def recip_amax():
    """The first amax on a fixed walk with fl(127 / amax) != fl(1 / fl(amax / 127)): the two ways to the inverse scale part."""
    rng = np.random.default_rng(127)
    for a in rng.uniform(0.5, 4.0, 4096).astype(F32):
        d = F32(a / F32(127.0))
        if F32(F32(127.0) / a) != F32(F32(1.0) / d):
            return F32(a)
    raise AssertionError("no such amax on the walk")


def recip_block():
    a = recip_amax()
    rng = np.random.default_rng(5)
    v = (rng.uniform(-1.0, 1.0, 32) * float(a)).astype(F32)
    v[7] = -a
    return v


def q8_rows(K, seed=0):
    """float32 [8, K]: random rows of mixed scale; block 0 of rows 0 / 1 / 2 is the tie block / the recip block / all zeros."""
    rng = np.random.default_rng(_seed(K, seed, 1))
    x = (rng.standard_normal((8, K)) * rng.uniform(0.05, 6.0, (8, 1))).astype(F32)
    x[0, :32], x[1, :32], x[2, :32] = tie_block(), recip_block(), 0.0
    return x


# ---- mat-vec --------------------------------------------------------------------------------------------------------------------------------------------------

def weight_rows(wtype, M, K, seed=0):
    """uint8 [M * K / 32 * block bytes]: M rows in the file's format with random codes and random f16 scales (and minima) of mixed sign."""
    rng = np.random.default_rng(_seed(wtype, M, K, seed, 2))
    nb = K // 32
    b = rng.integers(0, 256, (M, nb, R.BLOCK_BYTES[wtype]), dtype=np.uint8)
    d = (rng.uniform(0.002, 0.06, (M, nb)) * rng.choice([-1.0, 1.0], (M, nb))).astype(np.float16)
    b[:, :, 0:2] = d.view(np.uint8).reshape(M, nb, 2)
    if R.Q81[wtype]:
        m = rng.uniform(-0.5, 0.5, (M, nb)).astype(np.float16)
        b[:, :, 2:4] = m.view(np.uint8).reshape(M, nb, 2)
    return b.reshape(-1)


def columns(K, N, seed=0):
    rng = np.random.default_rng(_seed(K, N, seed, 3))
    return (rng.standard_normal((N, K)) * rng.uniform(0.3, 3.0, (N, 1))).astype(F32)


def ln_params(K, seed=0):
    rng = np.random.default_rng(_seed(K, seed, 4))
    return (1.0 + 0.2 * rng.standard_normal(K)).astype(F32), (0.1 * rng.standard_normal(K)).astype(F32)


def sturdy_columns(K, N, seed=0):
    """columns() whose LayerNorm statistics do not hang on the association of the double sums (chain_ref.ln_fragile): the kernel sums them in another order."""
    for s in range(seed, seed + 64):
        x = columns(K, N, s)
        if not any(R.ln_fragile(r) for r in x):
            return x
    raise AssertionError("no sturdy columns")


class MatvecCase:
    """One launch: weights, columns, the prologue's and the epilogue's operands -- and what the two associations make of them (memo)."""

    def __init__(self, wtype, epi, M, K, N, seed=0):
        self.wtype, self.epi, self.M, self.K, self.N = wtype, epi, M, K, N
        self.ln = epi != "RESID"
        self.w = weight_rows(wtype, M, K, seed)
        self.x = sturdy_columns(K, N, seed) if self.ln else columns(K, N, seed)
        self.ln_w, self.ln_b = ln_params(K, seed) if self.ln else (None, None)
        rng = np.random.default_rng(_seed(wtype, M, K, N, seed, 5))
        self.bias = None if epi == "LOGITS" else rng.standard_normal(M).astype(F32)
        self.resid = rng.standard_normal((N, M)).astype(F32) if epi == "RESID" else None
        self._acc = {}

    @property
    def name(self):
        return "%s-%s-M%d-K%d-N%d" % (R.NAMES[self.wtype], self.epi, self.M, self.K, self.N)

    def acc(self, simd=True):
        """float32 [N, M]: the row values in front of the epilogue, in the SIMD or the scalar association (each with its own Q8 rows)."""
        if simd not in self._acc:
            q81 = R.Q81[self.wtype]
            y = np.stack([R.layer_norm(r, self.ln_w, self.ln_b) for r in self.x]) if self.ln else self.x
            if simd:
                self._acc[simd] = A.block_sums(self.wtype, self.w, self.M, self.K, *A.quantize_q8(y, q81))
            else:
                self._acc[simd] = R.block_sums(self.wtype, self.w, self.M, self.K, *R.quantize_q8(y, q81))
        return self._acc[simd]

    def expected(self, simd=True):
        """The epilogue on acc(): RESID / GELU / LOGITS float32 [N, M]; QKV (q [N, K], k [N, K], v [N, K])."""
        acc = self.acc(simd)
        if self.epi == "RESID":
            return R.epi_resid(acc, self.bias, self.resid)
        if self.epi == "GELU":
            return R.gelu_table()[R._f16_index((self.bias[None, :] + acc).astype(F32))]
        if self.epi == "LOGITS":
            return acc
        K = self.K
        q = ((self.bias[None, :K] + acc[:, :K]).astype(F32) * R.Q_SCALE).astype(F32)
        kv = (self.bias[None, K:] + acc[:, K:]).astype(F32)
        return q, kv[:, :K], kv[:, K:]


def telling_case(wtype, epi, M, K, N):
    """The first seed's case in which the two associations differ in at least a third of the output rows (a case of one row and one column is a coin: its
    seed is chosen on the references alone, never on what a kernel gives)."""
    for seed in range(32):
        case = MatvecCase(wtype, epi, M, K, N, seed)
        if share_differing(case) >= 1 / 3:
            return case
    raise AssertionError("no seed tells the associations apart")


def matvec_cases(wtype):
    """The launches of one format: every K x M x N of the residual form; the LayerNorm forms at the sizes where their path differs."""
    out = []
    for K in (32, 64, 1024, 4096):
        for M in (1, 7, 65):
            for N in (1, 2, 8):
                out.append(telling_case(wtype, "RESID", M, K, N))
    for K, M, N in ((32, 7, 2), (64, 65, 8), (1024, 65, 1), (1024, 7, 8), (4096, 65, 2)):
        out.append(telling_case(wtype, "GELU", M, K, N))
    for K, N in ((64, 1), (64, 2), (64, 8), (1024, 8)):
        out.append(telling_case(wtype, "QKV", 3 * K, K, N))
    for K, M, N in ((1024, 1000, 1), (64, 65, 8), (32, 7, 2), (1024, 1, 1)):      # (1000: no multiple of 16, several workgroups)
        out.append(telling_case(wtype, "LOGITS", M, K, N))
    return out


def lm_head_case():
    """The vocabulary of BioGPT, once."""
    return telling_case(R.Q4_0, "LOGITS", 42384, 1024, 1)


def share_differing(case):
    """Share of the output rows in which the two associations' values differ."""
    a, b = case.acc(True), case.acc(False)
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


def partials_of(row, rows_per_part):
    """The arg-max partial of every workgroup's rows: (values, indices), lowest index first among equals."""
    n = (row.size + rows_per_part - 1) // rows_per_part
    val, idx = np.zeros(n, F32), np.zeros(n, np.int32)
    for g in range(n):
        seg = row[g * rows_per_part:(g + 1) * rows_per_part]
        j = int(np.argmax(seg))
        val[g], idx[g] = seg[j], g * rows_per_part + j
    return val, idx


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------------------

ATTN_T = (1, 31, 32, 33, 63, 64, 65, 257, 1024)


def attn_inputs(H, N, P, seed=0):
    """q [N, H * 64], K / V [H, P, 64] of moderate scores (the softmax keeps many keys alive)."""
    rng = np.random.default_rng(_seed(H, N, P, seed, 6))
    q = (0.35 * rng.standard_normal((N, H * 64))).astype(F32)
    K = rng.standard_normal((H, P, 64)).astype(F32)
    V = rng.standard_normal((H, P, 64)).astype(F32)
    return q, K, V
