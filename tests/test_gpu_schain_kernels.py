"""Each kernel of the SIMD chain (csrc/kernels_schain.hip.h) alone, through biogpt_hip_schain_device -- the launch functions of a pass over column states of a
context on the SIMD chain -- bit for bit against tests/assoc_ref.py (the Q8 producer: lnq / quantize_q8; the linear stage: block_sums and the epilogues of
tests/assoc_cases.py) and tests/schain_ref.py (the attention: assoc_ref.attn_head on each column's gathered rows), guard rows and bytes intact.

The stage's cases are assoc_cases.telling_case inputs: in each of them at least a third of the rows differ between the scalar and the SIMD association on the
references alone (asserted here on the CPU), so a kernel that computed the scalar sums could not pass.  Every case runs at each forced tile shape and at the
launch's own choice; all four give identical bytes.  K = 4096 is four K phases of the kernel, K = 1056 one phase and a partial one."""
import numpy as np
import pytest

import assoc_cases as AC
import assoc_ref as A
import chain_ref as R
import schain_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32
TYPE_IDS = [R.NAMES[t] for t in R.TYPES]
TILE_COLS = {0: 4, 1: 16, 2: 32}      # columns of a workgroup at each tile shape; its rows are 64 at every shape


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def untouched(a):
    """Every byte as the probe preset it."""
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def states(rows):
    """[N][8] SeqState words from (n_past, seq_id, t_vis, n_shared, shared_slot)."""
    return np.array([[n_past, 0, 0, seq_id, t_vis, n_shared, slot, 0] for n_past, seq_id, t_vis, n_shared, slot in rows], dtype=np.int32)


# ---- the producer ----------------------------------------------------------------------------------------------------------------------------------------------

def hostile_rows(K, N):
    """float32 [N, K]: assoc_cases.q8_rows stacked -- block 0 of rows 0 / 1 / 2 of every eight is the tie block / the 127 / amax block / all zeros."""
    return np.concatenate([AC.q8_rows(K, seed=s) for s in range((N + 7) // 8)])[:N]


@pytest.mark.parametrize("N", [1, 9, 33])
@pytest.mark.parametrize("K", [32, 64, 1024])
@pytest.mark.parametrize("q81", [False, True], ids=["q8_0", "q8_1"])
def test_producer(pkg, K, N, q81):
    x = hostile_rows(K, N)
    assert (x[0, :32] == AC.tie_block()).all() and (N < 2 or (x[1, :32] == AC.recip_block()).all())
    got = pkg.schain_device("Q8", wtype=R.Q4_1 if q81 else R.Q4_0, K=K, x=x)
    q, d, s = A.quantize_q8(x, q81)
    assert (got["q"][:N] == q).all()
    assert (bits(got["d"][:N]) == bits(d)).all()
    assert (got["s"][:N] == s).all()
    assert untouched(got["q"][N]) and untouched(got["d"][N]) and untouched(got["s"][N])
    assert list(got["launched"][:3]) == [256, N, 1]


@pytest.mark.parametrize("N", [1, 9, 33])
@pytest.mark.parametrize("K", [32, 64, 1024])
@pytest.mark.parametrize("q81", [False, True], ids=["q8_0", "q8_1"])
def test_producer_behind_the_layer_norm(pkg, K, N, q81):
    x = AC.sturdy_columns(K, N, seed=9)
    lw, lb = AC.ln_params(K, 9)
    got = pkg.schain_device("Q8", wtype=R.Q5_1 if q81 else R.Q8_0, K=K, x=x, ln_w=lw, ln_b=lb)
    q, d, s = A.lnq(x, lw, lb, q81)
    assert (got["q"][:N] == q).all() and (bits(got["d"][:N]) == bits(d)).all() and (got["s"][:N] == s).all()
    assert untouched(got["q"][N]) and untouched(got["d"][N]) and untouched(got["s"][N])


# ---- the linear stage ------------------------------------------------------------------------------------------------------------------------------------------

# (K, M, N): M = 63 / 65 the row tile's height - 1 / + 1, 2053 odd; N = 3 / 5, 15 / 17, 31 / 33 a column tile's width - 1 / + 1
STAGE_SHAPES = {
    "RESID": [(32, 1, 1), (32, 7, 7), (64, 65, 8), (64, 63, 9), (64, 2053, 9), (1024, 65, 3), (1024, 7, 5), (1024, 63, 15), (1024, 1, 17), (1024, 65, 31),
              (1024, 7, 33), (1056, 65, 9), (4096, 65, 4)],
    "GELU": [(32, 7, 4), (64, 65, 9), (1024, 63, 17), (1056, 7, 33)],
    "LOGITS": [(64, 2053, 7), (1024, 65, 8), (1024, 1, 1), (32, 7, 33)],
}


def run_all_shapes(pkg, case, **kw):
    """The case at every forced tile shape and at the launch's own choice: identical bytes.  Returns the result of the launch's own choice."""
    args = dict(wtype=case.wtype, M=case.M, K=case.K, w_rows=case.w, x=case.x, ln_w=case.ln_w, ln_b=case.ln_b, epi=case.epi, bias=case.bias, resid=case.resid, **kw)
    own = pkg.schain_device("STAGE", cfg=-1, **args)
    threads, gx, gy, lds, cols, ldo, cfg, tn = (int(v) for v in own["launched"])
    assert threads == 256 and cfg in TILE_COLS and tn == TILE_COLS[cfg] and gx == (case.M + 63) // 64 and gy == (case.N + tn - 1) // tn and lds <= 65536, case.name
    for forced in (0, 1, 2):
        got = pkg.schain_device("STAGE", cfg=forced, **args)
        assert int(got["launched"][6]) == forced and int(got["launched"][7]) == TILE_COLS[forced], case.name
        for name in ("out", "k", "v"):
            if name in own:
                assert (got[name].view(np.uint32) == own[name].view(np.uint32)).all(), (case.name, forced, name)
    return own


@pytest.mark.parametrize("wtype", R.TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("epi", ["RESID", "GELU", "LOGITS"])
def test_stage(pkg, wtype, epi):
    for K, M, N in STAGE_SHAPES[epi]:
        case = AC.telling_case(wtype, epi, M, K, N)
        assert AC.share_differing(case) >= 1 / 3, case.name
        got = run_all_shapes(pkg, case)
        out = got["out"]
        assert out.shape == (((N + 31) & ~31) + 1, ((M + 63) & ~63) + 16), case.name
        assert (bits(out[:N, :M]) == bits(case.expected())).all(), case.name
        assert untouched(out[N:]) and untouched(out[:, M:]), case.name      # no write at or beyond row M, none beyond column N


def qkv_check(case, got, k0, v0, where):
    """where [N]: (slot, position) of every column.  The q rows, both caches in place, everything else as it was."""
    N, H = case.N, case.K // 64
    q, k, v = case.expected()
    assert (bits(got["out"][:N]) == bits(q)).all() and untouched(got["out"][N:]), case.name
    for name, before, rows in (("k", k0, k), ("v", v0, v)):
        want = before.copy()
        for i, (slot, pos) in enumerate(where):
            want[slot, :, pos, :] = rows[i].reshape(H, 64)      # head-major: [slot][H][P][64]
        assert (bits(got[name]) == bits(want)).all(), (case.name, name)


@pytest.mark.parametrize("wtype", R.TYPES, ids=TYPE_IDS)
def test_stage_qkv_of_the_contexts_own_columns(pkg, wtype):
    """dev_state with one slot: column i at n_past + i."""
    for K, N in ((64, 1), (64, 9), (64, 33)):
        case = AC.telling_case(wtype, "QKV", 3 * K, K, N)
        assert AC.share_differing(case) >= 1 / 3, case.name
        P, n_past, H = 48, 5, K // 64
        rng = np.random.default_rng(K + N)
        k0, v0 = rng.standard_normal((1, H, P, 64)).astype(F32), rng.standard_normal((1, H, P, 64)).astype(F32)
        got = run_all_shapes(pkg, case, dev_state=[n_past, 0, 0, 0], P=P, k_slots=k0, v_slots=v0)
        qkv_check(case, got, k0, v0, [(0, n_past + i) for i in range(N)])


@pytest.mark.parametrize("wtype", R.TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("col_mode", [0, 1])
def test_stage_qkv_over_column_states(pkg, wtype, col_mode):
    """Three slots, a distinct n_past per column.  col_mode 0: column i appends to slot i; 1: to slot seq_id (five columns on two of the slots: the third is
    never touched)."""
    for K in (64, 1024):
        P, H = 24, K // 64
        if col_mode == 0:
            rows = [(7, 9, 0, 0, 0), (0, 9, 0, 0, 0), (23, 9, 0, 0, 0)]                      # (seq_id 9 is not read)
            where = [(i, r[0]) for i, r in enumerate(rows)]
        else:
            rows = [(3, 2, 4, 0, 0), (4, 2, 5, 0, 0), (11, 0, 12, 0, 0), (5, 2, 6, 0, 0), (23, 0, 24, 0, 0)]
            where = [(r[1], r[0]) for r in rows]
        N = len(rows)
        case = AC.telling_case(wtype, "QKV", 3 * K, K, N)
        assert AC.share_differing(case) >= 1 / 3, case.name
        rng = np.random.default_rng(K + N + col_mode)
        k0, v0 = rng.standard_normal((3, H, P, 64)).astype(F32), rng.standard_normal((3, H, P, 64)).astype(F32)
        got = run_all_shapes(pkg, case, seq_states=states(rows), col_mode=col_mode, P=P, k_slots=k0, v_slots=v0)
        qkv_check(case, got, k0, v0, where)
        if col_mode == 1:
            assert (bits(got["k"][1]) == bits(k0[1])).all() and (bits(got["v"][1]) == bits(v0[1])).all()


# ---- the attention ---------------------------------------------------------------------------------------------------------------------------------------------

def nan_beyond(slots, counts):
    """Rows at or beyond a slot's largest visible count read NaN (a slot no column reads: all of it)."""
    for s in range(slots.shape[0]):
        slots[s, :, counts.get(s, 0):] = np.nan


@pytest.mark.parametrize("T", [1, 31, 32, 33, 65, 257, 1024])
@pytest.mark.parametrize("H", [2, 3])
def test_attention_eight_columns_in_three_slots(pkg, T, H):
    """col_mode 1: eight columns with their own visible counts in slots 0 .. 2; slot 3 is read by nobody."""
    P, N = max(T + 3, 8), 8
    counts = [T, max(1, T - 1), max(1, T // 2), 1, T, max(1, T - 31), min(T, 33), max(1, T - 32)]
    slot_of = [0, 1, 2, 0, 1, 2, 0, 1]
    q, _, _ = AC.attn_inputs(H, N, P, seed=T)
    rng = np.random.default_rng(T * 7 + H)
    K, V = rng.standard_normal((4, H, P, 64)).astype(F32), rng.standard_normal((4, H, P, 64)).astype(F32)
    most = {}
    for c, s in zip(counts, slot_of):
        most[s] = max(most.get(s, 0), c)
    nan_beyond(K, most); nan_beyond(V, most)
    st = states([(c - 1, s, c, 0, 0) for c, s in zip(counts, slot_of)])
    got = pkg.schain_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, seq_states=st, col_mode=1)
    want = S.attn_columns(q, K, V, st, col_mode=1, shared=0)
    assert np.isfinite(want).all()
    assert (bits(got["out"][:N]) == bits(want)).all()
    assert untouched(got["out"][N])
    assert list(got["launched"][:3]) == [256, H, N]


def test_attention_column_i_in_slot_i(pkg):
    """col_mode 0: column i reads slot i and n_past + 1 keys; seq_id and t_vis are not looked at."""
    H, P, N = 2, 80, 3
    counts = [33, 1, 70]
    q, _, _ = AC.attn_inputs(H, N, P, seed=5)
    rng = np.random.default_rng(55)
    K, V = rng.standard_normal((N, H, P, 64)).astype(F32), rng.standard_normal((N, H, P, 64)).astype(F32)
    nan_beyond(K, dict(enumerate(counts))); nan_beyond(V, dict(enumerate(counts)))
    st = states([(c - 1, 2 - i, 999, 0, 0) for i, c in enumerate(counts)])
    got = pkg.schain_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, seq_states=st, col_mode=0)
    want = S.attn_columns(q, K, V, st, col_mode=0, shared=0)
    assert np.isfinite(want).all() and (bits(got["out"][:N]) == bits(want)).all() and untouched(got["out"][N])


@pytest.mark.parametrize("n_shared", [0, 8, 32, 40])
def test_attention_with_rows_from_a_shared_slot(pkg, n_shared):
    """score_continuations' columns: rows j < n_shared come from slot 2, the rest from the column's own slot (0 or 1).  The own slots' first n_shared rows and the
    shared slot's rows from n_shared on are NaN: a read of either shows.  n_shared = 0: the bits of the plain form."""
    H, P, N = 3, 96, 8
    counts = [41, 42, 45, 64, 65, 73, 90, 96]
    slot_of = [0, 1, 0, 1, 0, 1, 0, 1]
    q, _, _ = AC.attn_inputs(H, N, P, seed=n_shared)
    rng = np.random.default_rng(900 + n_shared)
    K, V = rng.standard_normal((3, H, P, 64)).astype(F32), rng.standard_normal((3, H, P, 64)).astype(F32)
    for a in (K, V):
        a[:2, :, :n_shared] = np.nan
        a[2, :, n_shared:] = np.nan
    nan_beyond(K[:2], {0: 90, 1: 96}); nan_beyond(V[:2], {0: 90, 1: 96})
    st = states([(c - 1, s, c, n_shared, 2) for c, s in zip(counts, slot_of)])
    got = pkg.schain_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, seq_states=st, col_mode=1, shared=1)
    want = S.attn_columns(q, K, V, st, col_mode=1, shared=1)
    assert np.isfinite(want).all()
    assert (bits(got["out"][:N]) == bits(want)).all() and untouched(got["out"][N])
    if n_shared == 0:
        plain = pkg.schain_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, seq_states=st, col_mode=1, shared=0)
        assert (bits(plain["out"]) == bits(got["out"])).all()
