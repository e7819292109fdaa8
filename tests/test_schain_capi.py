"""The SIMD chain's C ABI without a GPU: the switch (biogpt_hip_assoc_chain / biogpt_hip_get_assoc_chain), the counter (biogpt_hip_simd_chain_launches) and the
probe of its kernels (biogpt_hip_schain_device) are declared, exported and bound; a null context and a value outside {0, 1} are refused; every refusal of the
probe comes before any HIP call and names the field (there is no device here: a HIP call would make the result -2).  And the attention probe's reference
(tests/schain_ref.py) is tests/assoc_ref.py's where the gathering of a column's rows is the identity."""
import ctypes
import os
import re

import numpy as np
import pytest

import assoc_cases as AC
import assoc_ref as A
import schain_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
Q4_0 = 2


@pytest.mark.parametrize("name", ["biogpt_hip_assoc_chain", "biogpt_hip_get_assoc_chain", "biogpt_hip_simd_chain_launches", "biogpt_hip_schain_device",
                                  "biogpt_hip_schain_bench"])
def test_symbols_exported_and_bound(pkg, name):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in {n for n, _, _ in pkg.SYMBOLS}
    assert getattr(ctypes.CDLL(pkg.LIB_PATH), name) is not None
    assert getattr(pkg.lib(), name).restype is (ctypes.c_int64 if name.endswith("launches") else ctypes.c_int)


def test_python_surface(pkg):
    assert callable(pkg.schain_device) and callable(pkg.schain_bench) and callable(pkg.BiogptModel.set_assoc_chain)
    assert callable(pkg.BiogptModel.simd_chain_launches) and isinstance(pkg.BiogptModel.assoc_chain, property)
    assert pkg.SCHAIN_STAGES == {"Q8": 0, "STAGE": 1, "ATTN": 2}
    import inspect
    assert "assoc_chain" in inspect.signature(pkg.BiogptModel.load).parameters


def test_the_chain_kind_comment_names_the_fourth_kind():
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    at = hdr.index("int biogpt_hip_chain_kind(")
    assert "4 the SIMD chain" in hdr[at - 1500:at]


def test_null_context_is_refused(pkg):
    for on in (0, 1):
        assert pkg.lib().biogpt_hip_assoc_chain(None, on) == -1
        assert b"null context" in pkg.lib().biogpt_hip_last_error()
    assert pkg.lib().biogpt_hip_get_assoc_chain(None) == -1
    assert pkg.lib().biogpt_hip_simd_chain_launches(None) == -1


def test_on_outside_0_1_is_refused_with_a_message(pkg):
    # (no device, so no context: the arguments are checked in front of everything a context holds, and a block of zeros stands in for the handle)
    buf = ctypes.create_string_buffer(1 << 16)
    for on in (-1, 2, 7):
        assert pkg.lib().biogpt_hip_assoc_chain(ctypes.cast(buf, ctypes.c_void_p), on) == -1
        msg = pkg.lib().biogpt_hip_last_error()
        assert b"on must be 0 or 1" in msg and str(on).encode() in msg


def states(rows):
    """[N][8] SeqState words from (n_past, seq_id, t_vis, n_shared, shared_slot)."""
    return np.array([[n_past, 0, 0, seq_id, t_vis, n_shared, slot, 0] for n_past, seq_id, t_vis, n_shared, slot in rows], dtype=np.int32)


x32 = np.zeros((1, 32), F32)
w1 = np.zeros(18, np.uint8)
q1 = np.zeros((1, 64), F32)
kv8 = np.zeros((2, 1, 8, 64), F32)
QKV = dict(stage="STAGE", wtype=Q4_0, M=192, K=64, x=np.zeros((2, 64), F32), w_rows=np.zeros(192 * 2 * 18, np.uint8), epi="QKV", ln_w=np.zeros(64, F32),
           ln_b=np.zeros(64, F32), bias=np.zeros(192, F32), P=4)
REFUSALS = [
    ("unknown stage", dict(stage=3, wtype=Q4_0, K=32, x=x32), "stage 3 is no stage"),
    ("negative stage", dict(stage=-1, wtype=Q4_0, K=32, x=x32), "stage -1 is no stage"),
    ("float type (Q8)", dict(stage="Q8", wtype=0, K=32, x=x32), "type 0 is no block format"),
    ("float type (STAGE)", dict(stage="STAGE", wtype=1, M=1, K=32, x=x32, w_rows=w1, epi="RESID"), "type 1 is no block format"),
    ("unknown type", dict(stage="STAGE", wtype=5, M=1, K=32, x=x32, w_rows=w1, epi="RESID"), "type 5 is no block format"),
    ("K no multiple of 32 (Q8)", dict(stage="Q8", wtype=Q4_0, K=48, x=np.zeros((1, 48), F32)), "K must be a multiple of 32"),
    ("K no multiple of 32 (STAGE)", dict(stage="STAGE", wtype=Q4_0, M=1, K=40, x=np.zeros((1, 40), F32), w_rows=w1, epi="RESID"), "K must be a multiple of 32"),
    ("K zero", dict(stage="Q8", wtype=Q4_0, K=0, N=1, x=x32), "K must be a multiple of 32"),
    ("N zero", dict(stage="Q8", wtype=Q4_0, K=32, N=0, x=x32), r"N must be in \[1, 512\]"),
    ("N 513", dict(stage="Q8", wtype=Q4_0, K=32, N=513, x=x32), r"N must be in \[1, 512\]"),
    ("x missing", dict(stage="Q8", wtype=Q4_0, K=32, N=1), "x is NULL"),
    ("ln_b missing", dict(stage="Q8", wtype=Q4_0, K=32, x=x32, ln_w=np.zeros(32, F32)), "ln_w and ln_b come together"),
    ("unknown epilogue", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi=4), "epi 4 is no epilogue of the SIMD chain"),
    ("unknown tile shape", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="LOGITS", cfg=3), r"cfg must be in \[-1, 2\]"),
    ("M zero", dict(stage="STAGE", wtype=Q4_0, M=0, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32)), "M must be in"),
    ("bias missing", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", resid=np.zeros((1, 1), F32)), "bias is NULL"),
    ("resid missing", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32)), "resid is NULL"),
    ("weights missing", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32)), "w_rows or out is NULL"),
    ("q/k/v of another shape", dict(QKV, M=64, w_rows=np.zeros(64 * 2 * 18, np.uint8), bias=np.zeros(64, F32), dev_state=[0, 0, 0, 0],
                                    k_slots=np.zeros((1, 1, 4, 64), F32), v_slots=np.zeros((1, 1, 4, 64), F32)), "q/k/v is 3 K x K"),
    ("q/k/v position outside the table", dict(QKV, dev_state=[3, 0, 0, 0], k_slots=np.zeros((1, 1, 4, 64), F32), v_slots=np.zeros((1, 1, 4, 64), F32)),
     r"position 4 outside \[0, P\)"),
    ("q/k/v with both kinds of state", dict(QKV, dev_state=[0, 0, 0, 0], seq_states=states([(0, 0, 1, 0, 0), (1, 0, 2, 0, 0)]),
                                            k_slots=np.zeros((1, 1, 4, 64), F32), v_slots=np.zeros((1, 1, 4, 64), F32)), "exactly one of dev_state and seq_states"),
    ("q/k/v slot outside the slots", dict(QKV, seq_states=states([(0, 0, 1, 0, 0), (1, 2, 2, 0, 0)]), col_mode=1, k_slots=np.zeros((2, 1, 4, 64), F32),
                                          v_slots=np.zeros((2, 1, 4, 64), F32)), r"slot 2 outside \[0, n_slots\)"),
    ("q/k/v two columns on one row", dict(QKV, seq_states=states([(1, 1, 1, 0, 0), (1, 1, 2, 0, 0)]), col_mode=1, k_slots=np.zeros((2, 1, 4, 64), F32),
                                          v_slots=np.zeros((2, 1, 4, 64), F32)), "a second column writes slot 1, position 1"),
    ("column states without q/k/v", dict(stage="STAGE", wtype=Q4_0, M=1, K=32, x=x32, w_rows=w1, epi="RESID", bias=np.zeros(1, F32), resid=np.zeros((1, 1), F32),
                                         dev_state=[0, 0, 0, 0]), "only QKV reads column states"),
    ("T beyond 1024", dict(stage="ATTN", H=1, P=2048, q=q1, k_slots=np.zeros((1, 1, 2048, 64), F32), v_slots=np.zeros((1, 1, 2048, 64), F32),
                           seq_states=states([(1024, 0, 0, 0, 0)])), r"sees T = 1025 keys: the kernel holds 1 \.\. 1024"),
    ("T zero", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(3, 0, 0, 0, 0)]), col_mode=1), r"sees T = 0 keys"),
    ("T beyond the table", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(8, 0, 0, 0, 0)])), "sees 9 keys of a table of P = 8 rows"),
    ("slot beyond the slots", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(0, 2, 1, 0, 0)]), col_mode=1),
     r"slot 2 outside \[0, n_slots\)"),
    ("shared slot beyond the slots", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(3, 0, 4, 2, 5)]), col_mode=1, shared=1),
     r"shared slot 5 outside \[0, n_slots\)"),
    ("shared rows beyond the table", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(3, 0, 4, 9, 1)]), col_mode=1, shared=1),
     r"9 shared rows outside \[0, P\]"),
    ("no heads", dict(stage="ATTN", H=0, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(0, 0, 1, 0, 0)])), r"H must be in \[1, 64\]"),
    ("col_mode 2", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8, seq_states=states([(0, 0, 1, 0, 0)]), col_mode=2), "col_mode must be 0 or 1"),
    ("states missing", dict(stage="ATTN", H=1, P=8, q=q1, k_slots=kv8, v_slots=kv8), "seq_states or out is NULL"),
]


@pytest.mark.parametrize("what,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_probe_refuses_before_any_hip_call(pkg, what, kw, text):
    with pytest.raises(pkg.BiogptError, match=text):
        pkg.schain_device(**kw)


def test_probe_refusal_returns_minus_one(pkg):
    rc = pkg.lib().biogpt_hip_schain_device(0, 9, Q4_0, 0, 1, 32, 1, -1, 0, 0, 0, 0, 0, *([None] * 16))
    assert rc == -1 and b"no stage" in pkg.lib().biogpt_hip_last_error()
    rc = pkg.lib().biogpt_hip_schain_device(0, 0, Q4_0, 0, 1, 33, 1, -1, 0, 0, 0, 0, 0, *([None] * 16))
    assert rc == -1 and b"K must be a multiple of 32" in pkg.lib().biogpt_hip_last_error()


def test_bench_refuses_before_any_hip_call(pkg):
    for kw, text in ((dict(which="stage", wtype=0, M=64, K=64, N=8), "no block format"), (dict(which="stage", wtype=Q4_0, M=64, K=64, N=8, cfg=5), "cfg must be in"),
                     (dict(which="q8", wtype=Q4_0, M=64, K=48, N=8), "K must be a multiple of 32"), (dict(which="matvec", wtype=Q4_0, M=64, K=64, N=0), "N must be in")):
        with pytest.raises(pkg.BiogptError, match=text):
            pkg.schain_bench(**kw)


# ---- the attention probe's reference: gathering a column's rows, then assoc_ref.attn_head ----

def test_gathering_from_one_slot_is_the_identity():
    """A column whose rows all lie in its own slot: schain_ref.attn_columns is assoc_ref.attn_head on that slot, whatever n_shared = 0 names as the shared slot."""
    H, P, N = 2, 40, 3
    rng = np.random.default_rng(11)
    q = (0.35 * rng.standard_normal((N, H * 64))).astype(F32)
    K, V = rng.standard_normal((2, H, P, 64)).astype(F32), rng.standard_normal((2, H, P, 64)).astype(F32)
    st = states([(4, 1, 5, 0, 0), (32, 0, 33, 0, 1), (39, 1, 40, 0, 0)])
    got = S.attn_columns(q, K, V, st, col_mode=1, shared=1)
    for i, (slot, T) in enumerate(((1, 5), (0, 33), (1, 40))):
        for h in range(H):
            want = A.attn_head(q[i, h * 64:(h + 1) * 64], K[slot, h], V[slot, h], T)
            assert (got[i, h * 64:(h + 1) * 64].view(np.uint32) == want.view(np.uint32)).all()
    # col_mode 0: column i is slot i with n_past + 1 keys
    st0 = states([(4, 7, 0, 0, 0), (32, 7, 0, 0, 0)])
    got0 = S.attn_columns(q[:2], K, V, st0, col_mode=0, shared=0)
    assert (got0[0, :64].view(np.uint32) == A.attn_head(q[0, :64], K[0, 0], V[0, 0], 5).view(np.uint32)).all()
    assert (got0[1, 64:].view(np.uint32) == A.attn_head(q[1, 64:], K[1, 1], V[1, 1], 33).view(np.uint32)).all()


def test_shared_rows_come_from_the_shared_slot():
    """Rows j < n_shared are the shared slot's: the result is attn_head on the spliced rows, and differs from the column's own slot alone."""
    H, P = 1, 48
    rng = np.random.default_rng(12)
    q = (0.35 * rng.standard_normal((1, 64))).astype(F32)
    K, V = rng.standard_normal((2, H, P, 64)).astype(F32), rng.standard_normal((2, H, P, 64)).astype(F32)
    got = S.attn_columns(q, K, V, states([(40, 0, 41, 8, 1)]), col_mode=1, shared=1)
    Ks, Vs = np.concatenate([K[1, 0, :8], K[0, 0, 8:]]), np.concatenate([V[1, 0, :8], V[0, 0, 8:]])
    assert (got[0].view(np.uint32) == A.attn_head(q[0], Ks, Vs, 41).view(np.uint32)).all()
    assert (got[0].view(np.uint32) != A.attn_head(q[0], K[0, 0], V[0, 0], 41).view(np.uint32)).any()


def test_the_oracle_agrees_where_gathering_is_the_identity(oracle):
    q, K, V = AC.attn_inputs(2, 1, 70, seed=3)
    st = states([(64, 0, 65, 0, 0)])
    got = S.attn_columns(q, K[None], V[None], st, col_mode=1, shared=0)
    for h in range(2):
        want = oracle.attn_head(q[0, h * 64:(h + 1) * 64], K[h], V[h], 65, assoc=1)
        assert (got[0, h * 64:(h + 1) * 64].view(np.uint32) == np.asarray(want, dtype=F32).view(np.uint32)).all()
