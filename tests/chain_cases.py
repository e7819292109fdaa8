"""Seeded inputs for the linear stages of the many-column chain, one kernel at a time (biogpt_hip_chain_device): every route of every op for the five block
formats, at the column counts on both sides of each launch choice, on weights, activations, biases and LayerNorm rows that no whole call produces.  The
reference of a case is tests/chain_ref.py; tests/test_chain_restatement.py shows on the CPU that the inputs are what this text says and that every expected
output is finite.

Blocks are told apart by r = b % 8 (b: the block's index in its row), so that no product of two extremes leaves float32 (or, at fc1, the f16 range):

  weights   quantizer output of N(0, 0.02) everywhere, then in the HOSTILE rows (the first and last rows of 16-row tiles, of 64-row workgroups, of the matrix):
            kind A "codes": every code the minimum (even b) or the maximum (odd b) with every qh bit to match -- Q8_0: -128 / 127 --, d = +-0.02, m = +-0.01;
            kind B "scales": random codes, d by r: 0 -> 0 (m = 0.01: "d = 0, m != 0"), 1 -> the smallest f16 subnormal, 2 -> -0.02, 3 -> a zero block,
            4 -> +65504, 5 -> -65504, 6 -> 0.02, 7 -> minus the subnormal.
  columns   quantizer output of N(0, 1) rows, then column 1: zero blocks (d = 0) at r in {0, 1}; column 2: every code +-127; column 3: d = BIG at r == 3 and
            TINY at r == 4 (Q8_1: 1e30 / 1e-30; Q8_0, whose d is an f16: 65504 / 2^-24); column 4: all +127 (even b) / all -127 (odd b), so s = +-4064 d;
            column 5: codes 64 .. 127, all positive -- against a hostile row's equal codes the integer dot has 15 significant bits, so that dot * d_w is
            rounded (an ordinary block's dot fits 12 bits and its products with two f16 scales are exact in either order).
            BIG meets the hostile rows' zero block, TINY their +-65504.
  fc1       its pre-activations must stay below 65504 after the f16 round: EVERY row has the zero block at r == 3, EVERY column has TINY at r == 4, +-65504 sits
            at r == 4 alone (the sign alternates with b // 8).  Four 32-row groups have zero weights, so their bias alone sets exact pre-activations: three
            with values >= 8 (where the table returns its argument) that put the group's Q8 block on amax = 127 * 2^j (j = -3, 0, 4) and its codes on
            roundf ties k + 0.5; one with +-60000, +-65519 (f16: 65504) and values over the table's range.
"""
import functools

import numpy as np

import chain_ref as R
from chain_ref import F32, Q81

SHAPES = {"QKV": (3072, 1024), "OPROJ": (1024, 1024), "FC1_LN": (4096, 1024), "FC1_Q8": (4096, 1024), "FC2": (1024, 4096)}
VALU_COLS = (1, 7, 8, 9, 17, 63)
MFMA_COLS = (48, 49, 63, 64, 65, 79, 81)
BORDER_COLS = {"FC1_Q8": (240, 241, 257), "QKV": (336, 337, 353)}       # both sides of (M / 128) * ceil(N / 16) >= 512, and a tail tile with one live column behind it
LM_SWEEP_M = 1040                                                         # the lm_head of the column sweep: 65 tiles, the last workgroup with one live wave
LM_ROWS = (64, 80, 96, 112, 1040)                                         # the last workgroup with 4, 1, 2, 3, 1 live waves
LM_ODD = (1045, 1043)                                                     # no whole tiles: the 8-column kernel alone
LM_FULL = 42384
MFMA_MIN_DECODE_COLS, MFMA_MIN_PASS_COLS = 48, 64
ZERO_GROUPS = (1, 66, 97, 127)                                            # fc1: 32-row groups of zero weights
SUB = 0x0001                                                              # the smallest f16 subnormal, as bits


def _rng(*key):
    return np.random.default_rng([0x43484149] + [int(k) for k in key])


def two_tiles(op, wtype, M, N):
    """mfma_tu.hip: a wave walks two row tiles at fc1 and q/k/v, for the formats without a min term, when 32 | M and the launch keeps 512 workgroups."""
    return op in ("QKV", "FC1_Q8") and not Q81[wtype] and M % 32 == 0 and (M // 128) * ((N + 15) // 16) >= 512


def expected_launch(op, route, wtype, M, K, N):
    """(kernel, threads, grid x, grid y, dynamic LDS bytes) as the launch helpers report them."""
    nb = K // 32
    if route in ("VALU_1", "VALU_8"):
        nc = 1 if route == "VALU_1" else 8
        steps = 4 if op in ("FC1_LN", "FC1_Q8", "LMHEAD") else 1
        rpw = (64 // min(nb, 64)) * steps
        gelu = op in ("FC1_LN", "FC1_Q8")
        lds = K + 2 * nb * 4 + (64 + (32 * nc if gelu else 0)) * 4 + 4 * rpw * nc * (nb + 4) * 4 + 64
        return (0 if nc == 1 else 1, 256, (M + 4 * rpw - 1) // (4 * rpw), (N + nc - 1) // nc, lds)
    J = 2 if route == "MFMA_2" else 1
    q81 = Q81[wtype]
    off_w = 16 * (1024 + 16) + 16 * 32 * 4 * (2 if q81 else 1)
    buf = off_w + 4 * J * 32 * (32 if q81 else 16) * 4
    lds = max(buf * (2 if K > 1024 else 1), 16 * 64 * 4 if op == "FC1_Q8" else 0)
    return (3 if J == 2 else 2, 320 if K > 1024 else 256, (M + 64 * J - 1) // (64 * J), (N + 15) // 16, lds)


# ---- weights -----------------------------------------------------------------------------------------------------------------------------------------

def encode_weights(wtype, codes, d_bits, m_bits=None):
    """codes uint8 [R, nb, 32] in the format's own domain (Q8_0: int8 as uint8), d / m as f16 bit patterns [R, nb] -> file-format bytes [R, nb, bb]."""
    Rn, nb = d_bits.shape
    out = np.zeros((Rn, nb, R.BLOCK_BYTES[wtype]), dtype=np.uint8)
    out[:, :, 0:2] = d_bits.astype("<u2")[..., None].view(np.uint8).reshape(Rn, nb, 2)
    at = 2
    if Q81[wtype]:
        out[:, :, 2:4] = m_bits.astype("<u2")[..., None].view(np.uint8).reshape(Rn, nb, 2)
        at = 4
    if wtype == R.Q8_0:
        out[:, :, 2:34] = codes
        return out
    c = codes.astype(np.uint32)
    if wtype in (R.Q5_0, R.Q5_1):
        j = np.arange(16, dtype=np.uint32)
        qh = (((c[:, :, :16] >> 4) & 1) << j).sum(axis=2) | (((c[:, :, 16:] >> 4) & 1) << (j + 16)).sum(axis=2)
        out[:, :, at:at + 4] = qh.astype("<u4")[..., None].view(np.uint8).reshape(Rn, nb, 4)
        at += 4
    out[:, :, at:at + 16] = ((c[:, :, :16] & 0x0F) | ((c[:, :, 16:] & 0x0F) << 4)).astype(np.uint8)
    return out


def f16_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16)


def hostile_rows(M):
    """The first and last rows of tiles, workgroups and the matrix; kind A and B alternate along the list."""
    c = {0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 65, M // 2 + 5, M - 65, M - 64, M - 49, M - 48, M - 33, M - 32, M - 17, M - 16, M - 15, M - 2, M - 1}
    return sorted(r for r in c if 0 <= r < M)


@functools.lru_cache(maxsize=4)
def weights(oracle, op, wtype, M, K):
    """File-format bytes uint8 [M, nb, bb] of the case matrix for (op, type)."""
    fc1 = op in ("FC1_LN", "FC1_Q8")
    g = _rng(1, R.TYPES.index(wtype), M, K, sum(map(ord, op)))
    nb, bb = K // 32, R.BLOCK_BYTES[wtype]
    base = (g.standard_normal((M, K), dtype=F32) * F32(0.02)).astype(F32)
    raw = oracle.quantize(wtype, base, K).reshape(M, nb, bb).copy()
    del base
    top = 255 if wtype == R.Q8_0 else 31 if wtype in (R.Q5_0, R.Q5_1) else 15
    b = np.arange(nb)
    r = b % 8
    for i, row in enumerate(hostile_rows(M)):
        if i % 2 == 0:      # kind A: the extreme codes
            lo, hi = (0x80, 0x7F) if wtype == R.Q8_0 else (0, top)
            codes = np.where((b % 2 == 0)[:, None], lo, hi).astype(np.uint8) * np.ones((1, 32), np.uint8)
            d = np.where(b % 4 >= 2, f16_bits(-0.02), f16_bits(0.02))
            m = np.where(b % 3 == 0, f16_bits(-0.01), f16_bits(0.01))
        else:               # kind B: the extreme scales
            codes = g.integers(0, top + 1, size=(nb, 32)).astype(np.uint8)
            tab = np.array([0, SUB, f16_bits(-0.02), 0, f16_bits(65504.0), f16_bits(-65504.0), f16_bits(0.02), 0x8000 | SUB], dtype=np.uint16)
            d = tab[r]
            if fc1:
                d = np.where(r == 4, np.where((b // 8) % 2 == 0, f16_bits(65504.0), f16_bits(-65504.0)), np.where(r == 5, f16_bits(-0.02), d))
            m = np.where(r == 3, 0, f16_bits(0.01))
            codes[r == 3] = 0x00
        raw[row] = encode_weights(wtype, codes[None], d[None].astype(np.uint16), m[None].astype(np.uint16))[0]
    if fc1:
        raw[:, r == 3, :] = 0
        for grp in ZERO_GROUPS:
            raw[32 * grp:32 * grp + 32] = 0
    raw.setflags(write=False)
    return raw


# ---- activation columns ------------------------------------------------------------------------------------------------------------------------------

def _consistent(q, d, q81):
    """(d as stored, s) of blocks with codes q and scale d, as a producer leaves them."""
    isum = q.reshape(q.shape[0], -1, 32).astype(np.int32).sum(axis=2)
    if q81:
        return d, (isum.astype(F32) * d).astype(F32).view(np.uint32)
    return d.astype(np.float16).astype(F32), isum.astype(np.int32).view(np.uint32)


@functools.lru_cache(maxsize=8)
def columns(op, q81, K, n):
    """(q int8 [n, K], d float32 [n, K / 32], s uint32 [n, K / 32]): the first n columns of the site's activation pool."""
    nb = K // 32
    g = _rng(2, int(q81), K, sum(map(ord, op)))
    q, d, s = R.quantize_q8(g.standard_normal((n, K), dtype=F32), q81)
    q, d = q.copy(), d.copy()
    r = np.arange(nb) % 8
    big, tiny = (F32(1e30), F32(1e-30)) if q81 else (F32(65504.0), F32(2.0 ** -24))
    qb = q.reshape(n, nb, 32)
    if n > 1:
        qb[1][r <= 1] = 0
        d[1][r <= 1] = 0
    if n > 2:
        qb[2] = np.where(np.arange(32) % 3 == 0, -127, 127)[None, :]
        d[2] = F32(0.02)
    if n > 3:
        d[3][r == 3] = big
        d[3][r == 4] = tiny
    if n > 4:
        qb[4] = np.where((np.arange(nb) % 2 == 0)[:, None], 127, -127)
        d[4] = F32(0.02)
    if n > 5:
        qb[5] = g.integers(64, 128, size=(nb, 32))
    if op in ("FC1_LN", "FC1_Q8"):
        d[:, r == 4] = tiny
    d, s = _consistent(q, d, q81)
    for a in (q, d, s):
        a.setflags(write=False)
    return q, d, s


# ---- biases, residuals, column states ----------------------------------------------------------------------------------------------------------------------

TIE_GROUPS = {1: -3, 66: 0, 97: 4}      # fc1 zero-weight group -> j: the group's Q8 block has amax = 127 * 2^j, d = 2^j, and codes on ties


def fc1_bias(seed):
    b = (_rng(3, seed).standard_normal(4096, dtype=F32) * F32(0.5)).astype(F32)
    for grp, j in TIE_GROUPS.items():
        step = F32(2.0 ** j)
        k0 = int(np.ceil(8.0 / float(step)))                       # values >= 8: the table returns its argument there
        k = np.minimum(k0 + 3 * np.arange(32), 126)
        v = ((k.astype(F32) + F32(0.5)) * step).astype(F32)        # code k + 0.5: a roundf tie
        v[5] = F32(127.0) * step                                   # amax
        v[9] = np.maximum(F32(8.0), F32(k0) * step)                # an exact code beside the ties
        assert (v.astype(np.float16).astype(F32) == v).all() and (v >= 8).all()
        b[32 * grp:32 * grp + 32] = v
    edge = np.array([60000.0, -60000.0, 65519.0, -65519.0, 1000.0, -1000.0, 17.0, -17.0, 8.0, -8.0, 65504.0, -65504.0, 40000.5, -33.25, 12.0, -12.0], dtype=F32)
    b[32 * 127:32 * 127 + 32] = np.concatenate([edge, edge[::-1]])
    return b


def bias_resid(op, wtype, acc, seed):
    """bias [M] and resid [N, M] for the residual sites: random, with rows whose bias cancels column 0's sum and a column (1, when there is one) whose residual
    cancels sum + bias."""
    N, M = acc.shape
    g = _rng(4, seed, M)
    bias = (g.standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
    rows = np.arange(3, M, 37)
    bias[rows] = -acc[0, rows]
    resid = g.standard_normal((N, M), dtype=F32)
    c = 1 if N > 1 else 0
    resid[c] = -(acc[c] + bias).astype(F32)
    return bias, resid


def qkv_states(form, N, seed):
    """form 0: the context's own columns (dev_state); 1: one column per sequence (col_mode 0); 2: packed columns of three slots in scrambled order (col_mode 1).
    -> dict(dev_state, seq_states, col_mode, P, n_slots, slot [N], pos [N]); positions 0 and P - 1 are written in every form."""
    g = _rng(5, form, N, seed)
    if form == 0:
        P = N + (seed % 2) * 3                                     # n_past 0, or the last column at P - 1
        n_past = P - N
        return dict(dev_state=np.array([n_past, 0, 0, 0], np.int32), seq_states=None, col_mode=0, P=P, n_slots=1, slot=np.zeros(N, int), pos=n_past + np.arange(N))
    st = np.zeros((N, 8), dtype=np.int32)
    if form == 1:
        P = 5
        pos = (np.arange(N) * 7 + seed) % P
        if N > 1:
            pos[0], pos[-1] = 0, P - 1
        slot = np.arange(N)
        st[:, 0], st[:, 3] = pos, g.integers(0, 1 << 20, N)        # seq_id is not read with col_mode 0
        return dict(dev_state=None, seq_states=st, col_mode=0, P=P, n_slots=N, slot=slot, pos=pos)
    per = (N + 2) // 3
    P = per + 1
    order = g.permutation(N)
    slot, pos = np.zeros(N, int), np.zeros(N, int)
    perm = [2, 0, 1]
    for j, i in enumerate(order):
        slot[i], pos[i] = perm[j % 3], (P - 1 - j // 3 if j % 3 == 0 else j // 3)      # slot 2 filled from P - 1 down, the others from 0 up
    st[:, 0], st[:, 3], st[:, 4] = pos, slot, pos + 1
    return dict(dev_state=None, seq_states=st, col_mode=1, P=P, n_slots=3, slot=slot, pos=pos)


# ---- LayerNorm rows ----------------------------------------------------------------------------------------------------------------------------------------------

OUT_ZERO_BLOCK, OUT_CONST_BLOCK = 5, 21     # tests/wide_models.py: gain 0 with bias 0 / 0.3
LN_FAMILIES = ("normal", "normal", "outlier", "outlier", "constant", "huge", "tiny", "offset", "normal")


def ln_gain_bias(fc1=False):
    g = _rng(6)
    w = (F32(1.0) + g.standard_normal(1024, dtype=F32) * F32(0.2)).astype(F32)
    b = (g.standard_normal(1024, dtype=F32) * F32(0.1)).astype(F32)
    for blk, c in ((OUT_ZERO_BLOCK, 0.0), (OUT_CONST_BLOCK, 0.3)):
        w[32 * blk:32 * blk + 32], b[32 * blk:32 * blk + 32] = 0.0, c
    if fc1:     # the blocks that meet fc1's +-65504 scales come out TINY
        for blk in range(4, 32, 8):
            w[32 * blk:32 * blk + 32], b[32 * blk:32 * blk + 32] = 1e-6, 0.0
    return w, b


def ln_rows():
    """[len(LN_FAMILIES), 1024]: N(0, 1) rows; rows with the wide models' outlier channels (a few channels 1e3 times the others); a constant row (variance 0);
    a row of magnitude 1e18; one of 1e-6; one far from zero (mean 300)."""
    g = _rng(7)
    rows = []
    for f in LN_FAMILIES:
        x = g.standard_normal(1024, dtype=F32)
        if f == "outlier":
            x[g.choice(1024, 4, replace=False)] *= F32(1e3)
        elif f == "constant":
            x[:] = F32(0.7)
        elif f == "huge":
            x *= F32(1e18)
        elif f == "tiny":
            x *= F32(1e-6)
        elif f == "offset":
            x += F32(300.0)
        rows.append(x.astype(F32))
    return np.stack(rows)


# ---- the case list ------------------------------------------------------------------------------------------------------------------------------------------------------

def legal_routes(op, wtype, M, N, form=None):
    """The routes the engine may take for the site at N columns: the VALU kernel always (a context without the image), the matrix cores from their threshold."""
    if op == "FC1_LN":
        return ["VALU_1"]
    one = N == 1 and op in ("OPROJ", "FC2")
    routes = ["VALU_1" if one else "VALU_8"]
    need = MFMA_MIN_PASS_COLS if (op == "QKV" and form != 1) else MFMA_MIN_DECODE_COLS
    if N >= need and M % 16 == 0:
        routes.append("MFMA_2" if two_tiles(op, wtype, M, N) else "MFMA_1")
    return routes


def column_counts(op, wtype):
    ns = sorted(set(VALU_COLS) | set(MFMA_COLS) | set(BORDER_COLS.get(op, ())))
    if op == "FC2" and wtype == R.Q8_0:
        ns.append(512)
    return ns


def qkv_form(N):
    """Which column states a q/k/v case of N columns has: below 64 columns only a decode step (form 1) reaches the matrix cores."""
    return 1 if N in (48, 49, 63, 17, 337) else 2 if N in (7, 9, 65, 81, 353) else 0


# ---- a case: the probe's arguments and the whole expected outputs ---------------------------------------------------------------------------------------------------------

def shape_of(op, M=None):
    return (M, 1024) if op == "LMHEAD" else SHAPES[op]


@functools.lru_cache(maxsize=2)
def sums(oracle, op, wtype, M, n):
    """acc float32 [n, M] of the site's matrix against the first n columns of its pool (chain_ref.block_sums), shared by the cases of (op, type, M)."""
    K = shape_of(op, M)[1]
    acc = R.block_sums(wtype, weights(oracle, op, wtype, M, K), M, K, *columns(op, Q81[wtype], K, n))
    acc.setflags(write=False)
    return acc


def whole(rows, cols, ld, dtype):
    """The rows inside an output of cols x ld preset to 0xff bytes."""
    out = np.full((cols, ld), 0xff, dtype=np.uint8).repeat(np.dtype(dtype).itemsize, axis=1).view(dtype)
    out[:rows.shape[0], :rows.shape[1]] = rows
    return out


def geometry(M, N):
    return ((N + 15) & ~15) + 1, ((M + 127) & ~127) + 16


def build(oracle, op, wtype, N, M=None, n_pool=None, mistake=None):
    """-> (args, want): the keyword arguments of pkg.chain_device but for `route`, and the whole expected outputs by name (as chain_device returns them)."""
    M, K = shape_of(op, M)
    q81 = Q81[wtype]
    cols, ldo = geometry(M, N)
    aq = tuple(a[:N] for a in columns(op, q81, K, max(N, n_pool or N)))
    acc = sums(oracle, op, wtype, M, max(N, n_pool or N))[:N]
    if mistake in ("dropped_last_block", "previous_tile_scale", "dx_before_dw", "product_first", "fused_min_term", "pairwise_sum"):
        acc = R.block_sums(wtype, weights(oracle, op, wtype, M, K), M, K, *aq, mistake=mistake)
    args = dict(op=op, wtype=wtype, M=M, N=N, w_rows=weights(oracle, op, wtype, M, K), aq_q=aq[0], aq_d=aq[1], aq_s=aq[2])
    want = {}
    seed = N + 1000 * R.TYPES.index(wtype)

    def clamp(rows):        # the mistake that stores a column clamped to N - 1
        return np.concatenate([rows, rows[-1:]]) if mistake == "clamped_column_stored" else rows

    if op == "LMHEAD":
        want["out"] = whole(clamp(acc), cols, ldo, F32)
    elif op in ("OPROJ", "FC2"):
        clean = sums(oracle, op, wtype, M, max(N, n_pool or N))[:N]
        args["bias"], args["resid"] = bias_resid(op, wtype, clean, seed)
        want["out"] = whole(clamp(R.epi_resid(acc, args["bias"], args["resid"], mistake)), cols, ldo, F32)
    elif op == "FC1_Q8":
        args["bias"] = fc1_bias(seed)
        (q, d, s), want["gelu"] = R.epi_gelu_q8(acc, args["bias"], q81, mistake)
        want["out_q"], want["out_d"], want["out_s"] = whole(clamp(q), cols, M, np.int8), whole(clamp(d), cols, M // 32, F32), whole(clamp(s), cols, M // 32, np.uint32)
    elif op == "QKV":
        st = qkv_states(qkv_form(N), N, seed)
        args["bias"] = (_rng(8, seed).standard_normal(M, dtype=F32) * F32(0.1)).astype(F32)
        q, k, v = R.epi_qkv(acc, args["bias"], mistake)
        want["out"] = whole(clamp(q), cols, 1024, F32)
        for name, rows in (("k", k), ("v", v)):
            slots = np.full((st["n_slots"], 16, st["P"], 64), 0xff, dtype=np.uint8).repeat(4, axis=3).view(F32)
            slots[st["slot"], :, st["pos"], :] = rows.reshape(N, 16, 64)
            want[name] = slots
        args.update(dev_state=st["dev_state"], seq_states=st["seq_states"], col_mode=st["col_mode"], P=st["P"])
        args["k_slots"] = args["v_slots"] = np.full((st["n_slots"], 16, st["P"], 64), 0xff, dtype=np.uint8).repeat(4, axis=3).view(F32)
    else:
        raise ValueError(op)
    return args, want


def build_lnq(q81, mistake=None):
    x = ln_rows()
    w, b = ln_gain_bias()
    N = x.shape[0]
    cols = geometry(1024, N)[0]
    q, d, s = R.lnq(x, w, b, q81, mistake)
    return dict(op="LNQ", N=N, x=x, ln_w=w, ln_b=b, q81=int(q81)), dict(out_q=whole(q, cols, 1024, np.int8), out_d=whole(d, cols, 32, F32), out_s=whole(s, cols, 32, np.uint32))


def build_fc1_ln(oracle, wtype, row, mistake=None):
    """The 1-column fc1 with LayerNorm fused, on LayerNorm row `row` of ln_rows()."""
    M, K = SHAPES["FC1_LN"]
    q81 = Q81[wtype]
    x = ln_rows()[row:row + 1]
    w, b = ln_gain_bias(fc1=True)
    aq = R.lnq(x, w, b, q81, mistake)
    W = weights(oracle, "FC1_LN", wtype, M, K)
    acc = R.block_sums(wtype, W, M, K, *aq, mistake=mistake)
    bias = fc1_bias(row)
    (q, d, s), g = R.epi_gelu_q8(acc, bias, q81, mistake)
    cols = geometry(M, 1)[0]
    return (dict(op="FC1_LN", wtype=wtype, M=M, N=1, w_rows=W, x=x, ln_w=w, ln_b=b, bias=bias),
            dict(out_q=whole(q, cols, M, np.int8), out_d=whole(d, cols, M // 32, F32), out_s=whole(s, cols, M // 32, np.uint32), gelu=g, aq=aq))


FC1_LN_ROWS = (0, 2, 4)      # normal, outlier, constant


def compare(got, want, what):
    """Bit equality of every output the case names, guard bytes included; K / V slots whole."""
    for name in ("out", "out_q", "out_d", "out_s", "k", "v"):
        if name not in want:
            continue
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gb, wb = g.view(np.uint8).reshape(g.shape[0], -1), w.view(np.uint8).reshape(w.shape[0], -1)
        if (gb == wb).all():
            continue
        u = np.uint32 if g.dtype.itemsize == 4 else np.uint8
        bad = np.argwhere(g.view(u) != w.view(u))
        first = tuple(int(i) for i in bad[0])
        assert False, (what, name, "%d elements differ" % len(bad), "first at", first, "got", g[first], "want", w[first], "others", [tuple(int(i) for i in b) for b in bad[1:6]])
