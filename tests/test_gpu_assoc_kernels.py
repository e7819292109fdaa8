"""Each kernel of the SIMD association (csrc/kernels_assoc.hip.h) alone, through biogpt_hip_assoc_device -- the launch functions of a context in mode 1 -- bit for
bit against tests/assoc_ref.py (the mat-vec, the Q8 rows) and the oracle's bo_attn_head with assoc = 1 (the attention), guard bytes intact.
tests/test_assoc_restatement.py holds assoc_ref.py to the oracle on the CPU and shows that every mat-vec case here tells the two associations apart."""
import numpy as np
import pytest

import assoc_cases as AC
import assoc_ref as A
import chain_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
TYPE_IDS = [R.NAMES[t] for t in R.TYPES]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def untouched(a):
    """Every byte as the probe preset it."""
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


# ---- the Q8 rows ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [32, 64, 1024])
@pytest.mark.parametrize("q81", [False, True], ids=["q8_0", "q8_1"])
def test_q8_rows(pkg, K, q81):
    x = AC.q8_rows(K)                     # rows 0 / 1 / 2 start with the tie block, the 127 / amax block, an all-zero block
    got = pkg.assoc_device("Q8", wtype=R.Q4_1 if q81 else R.Q4_0, K=K, x=x)
    q, d, s = A.quantize_q8(x, q81)
    assert (got["q"][:8] == q).all()
    assert (bits(got["d"][:8]) == bits(d)).all()
    assert (got["s"][:8] == s).all()
    assert untouched(got["q"][8]) and untouched(got["d"][8]) and untouched(got["s"][8])
    assert got["launched"][1] == 8


@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("q81", [False, True], ids=["q8_0", "q8_1"])
def test_q8_rows_behind_the_layer_norm(pkg, K, q81):
    x = AC.sturdy_columns(K, 5, seed=9)
    lw, lb = AC.ln_params(K, 9)
    got = pkg.assoc_device("Q8", wtype=R.Q5_1 if q81 else R.Q8_0, K=K, x=x, ln_w=lw, ln_b=lb)
    q, d, s = A.lnq(x, lw, lb, q81)
    assert (got["q"][:5] == q).all() and (bits(got["d"][:5]) == bits(d)).all() and (got["s"][:5] == s).all()
    assert untouched(got["q"][5]) and untouched(got["d"][5]) and untouched(got["s"][5])


# ---- the mat-vec ----------------------------------------------------------------------------------------------------------------------------------------------

def run_matvec(pkg, case, partials=False):
    kw = dict(wtype=case.wtype, M=case.M, K=case.K, w_rows=case.w, x=case.x, ln_w=case.ln_w, ln_b=case.ln_b, epi=case.epi, bias=case.bias, resid=case.resid,
              partials=partials)
    if case.epi != "QKV":
        got = pkg.assoc_device("MATVEC", **kw)
        want = case.expected()
        out = got["out"]
        assert (bits(out[:case.N, :case.M]) == bits(want)).all(), case.name
        assert untouched(out[case.N]) and untouched(out[:, case.M:]), case.name
        return got
    P, n_past, H = 16, 5, case.K // 64
    rng = np.random.default_rng(case.K + case.N)
    k0, v0 = rng.standard_normal((H, P, 64)).astype(F32), rng.standard_normal((H, P, 64)).astype(F32)
    got = pkg.assoc_device("MATVEC", dev_state=[n_past, 0, 0, 0], P=P, k_slots=k0, v_slots=v0, **kw)
    q, k, v = case.expected()
    assert (bits(got["out"][:case.N]) == bits(q)).all() and untouched(got["out"][case.N]), case.name
    for name, before, rows in (("k", k0, k), ("v", v0, v)):
        want = before.copy()
        want[:, n_past:n_past + case.N, :] = rows.reshape(case.N, H, 64).transpose(1, 0, 2)      # head-major: [H][P][64]
        assert (bits(got[name]) == bits(want)).all(), case.name
    return got


@pytest.mark.parametrize("wtype", R.TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("epi", ["QKV", "RESID", "GELU", "LOGITS"])
def test_mat_vec(pkg, wtype, epi):
    cases = [c for c in AC.matvec_cases(wtype) if c.epi == epi]
    assert cases
    for case in cases:
        got = run_matvec(pkg, case, partials=(epi == "LOGITS" and case.N == 1))
        threads, gx, gy, lds, nc, rows = (int(v) for v in got["launched"][:6])
        assert gx * rows >= case.M and gy * nc >= case.N and lds <= 65536, case.name
        if epi == "LOGITS" and case.N == 1:
            val, idx = AC.partials_of(case.expected()[0], rows)
            assert gx == val.size
            assert (bits(got["pmax_val"][:gx]) == bits(val)).all() and (got["pmax_idx"][:gx] == idx).all(), case.name
            assert untouched(got["pmax_val"][gx:]) and untouched(got["pmax_idx"][gx:]), case.name


def test_lm_head_of_the_whole_vocabulary(pkg):
    case = AC.lm_head_case()
    got = run_matvec(pkg, case, partials=True)
    gx, rows = int(got["launched"][1]), int(got["launched"][5])
    val, idx = AC.partials_of(case.expected()[0], rows)
    assert gx == val.size and gx > 1
    assert (bits(got["pmax_val"][:gx]) == bits(val)).all() and (got["pmax_idx"][:gx] == idx).all()
    assert untouched(got["pmax_val"][gx:]) and untouched(got["pmax_idx"][gx:])


# ---- the attention --------------------------------------------------------------------------------------------------------------------------------------------

def attn_expected(oracle, q, K, V, T):
    N, H = q.shape[0], K.shape[0]
    out = np.zeros((N, H * 64), F32)
    for i in range(N):
        for h in range(H):
            out[i, h * 64:(h + 1) * 64] = oracle.attn_head(q[i, h * 64:(h + 1) * 64], K[h], V[h], int(T[i]), assoc=1)
    return out


@pytest.mark.parametrize("T", AC.ATTN_T)
def test_attention_one_column(pkg, oracle, T):
    H, P = 2, max(T + 3, 8)
    q, K, V = AC.attn_inputs(H, 1, P, seed=T)
    K[:, T:], V[:, T:] = AC.SENTINEL, AC.SENTINEL            # rows beyond the visible keys: a read of one shows
    got = pkg.assoc_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, dev_state=[T - 1, 0, 0, 0])
    want = attn_expected(oracle, q, K, V, [T])
    assert (bits(got["out"][:1]) == bits(want)).all()
    assert untouched(got["out"][1])
    assert list(got["launched"][:4]) == [17, 256, H, 1]


@pytest.mark.parametrize("state,name", [((25, 0, 1, 0), "causal"), ((60, 0, 0, 3), "chunks of 3"), ((249, 0, 0, 0), "one eval")], ids=["causal", "chunk3", "plain"])
def test_attention_eight_columns_with_their_own_visible_counts(pkg, oracle, state, name):
    H, N, P = 3, 8, 300
    n_past, _, causal, chunk = state
    T = [n_past + i + 1 if causal else n_past + (min((i // chunk + 1) * chunk, N) if chunk else N) for i in range(N)]
    q, K, V = AC.attn_inputs(H, N, P, seed=n_past)
    K[:, max(T):], V[:, max(T):] = AC.SENTINEL, AC.SENTINEL
    got = pkg.assoc_device("ATTN", H=H, P=P, q=q, k_slots=K, v_slots=V, dev_state=list(state))
    want = attn_expected(oracle, q, K, V, T)
    if causal or chunk:
        assert len(set(T)) > 1
    assert (bits(got["out"][:N]) == bits(want)).all()
    assert untouched(got["out"][N])
