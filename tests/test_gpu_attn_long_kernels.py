"""The two long-context attention kernels (csrc/kernels_attn_long.hip.h: attn_long_col_kernel, attn_long_tile_kernel), alone, against the oracle's attention
(oracle/biogpt_oracle.c, bo_attn_head) at 1025 .. 2048 keys.  biogpt_hip_attn_long_device launches them through the helper the engine's passes use; the content,
the layout of the table and the oracle's rows are those of tests/attn_cases.py (H = 3 heads of 64; SENTINEL in every row no column may see).

Every visible column's outputs equal the oracle's as uint32; the Q8 codes, d and s equal the oracle's quantizer on the oracle's row; rows from N on and the guard
row still hold 0xff; the launch is the expected one.  The kernels differ from the oracle only in how they associate the double sums: the seeds below were chosen
so that the restatement (tests/attn_ref.py) finds no fragile row in any case, so no tolerance is owed -- attn_ref is looked up only to word a
failure."""
import numpy as np
import pytest

import attn_cases as A
from test_gpu_attn_kernels import oracle_q8

pytestmark = pytest.mark.gpu

STATES = dict(A.DEV_STATES[:3])      # chunk0, chunk8, causal
# (form, keys of the last column, N, state form, family, q8 form, P, seed)
CASES = [
    (0, 1025, 1, "chunk0", "plain", 1, 2048, 0), (0, 1088, 2, "causal", "peak_first", 2, 2048, 0), (0, 1537, 8, "causal", "tie2", 0, 2048, 0),
    (0, 2047, 2, "chunk8", "wide", 1, 2048, 0), (0, 2048, 1, "chunk0", "peak_last", 2, 2048, 0), (0, 2048, 8, "chunk8", "v_alt", 1, 2048, 0),
    (0, 1030, 2, "causal", "plain", 2, 1030, 0),                                   # a table that is no multiple of 4 (nor of 64: t_cap = P)
    (1, 1025, 9, "chunk0", "plain", 2, 2048, 0), (1, 1088, 16, "chunk8", "peak_last", 1, 2048, 0), (1, 1537, 17, "causal", "wide", 0, 2048, 0),
    (1, 2047, 33, "chunk8", "tie2", 2, 2048, 0), (1, 2048, 33, "causal", "v_alt", 1, 2048, 0), (1, 2048, 16, "chunk0", "peak_first", 1, 2048, 0),
    (1, 1033, 33, "causal", "plain", 2, 2048, 0),                                  # n_past = 1000: the columns' own key counts straddle 1024, the first tile is short
    (1, 1030, 17, "chunk8", "plain", 1, 1030, 0),
]
IDS = ["%s-T%d-N%d-%s-%s-q8%d-P%d" % ((("col", "tile")[c[0]],) + c[1:7]) for c in CASES]


def case_of(form, T, N, state, family, q8, P, seed):
    q, K, V = A.content(family, T, seed=seed)
    q = np.tile(q, (2, 1))      # 34 query rows
    # the route only says how t_cap follows from t_max: whole waves of keys for the column form, the keys as they are for the tile form
    return A.dev_case("long %s" % family, A.TILE if form else A.FAST_4, N, P, q, K, V, STATES[state](N, T - N), q8=q8, family=family)


@pytest.mark.parametrize("form,T,N,state,family,q8,P,seed", CASES, ids=IDS)
def test_kernel_equals_the_oracle(pkg, oracle, form, T, N, state, family, q8, P, seed):
    c = case_of(form, T, N, state, family, q8, P, seed)
    assert c.t_max == T
    k, v = c.slots()
    rc, out, oq, od, os_, launched = pkg.attn_long_device(form, A.H, N, P, T, c.q, k[0], v[0], c.states()[0], q8=q8)
    assert rc == 0, pkg._err()
    assert tuple(launched[:4]) == (form, 1024, A.H, (N + 15) // 16 if form else N) and launched[5] == c.t_cap, list(launched)
    assert launched[4] >= (16 * c.t_cap * 4 if form else 2048 * 4), list(launched)
    ref = A.oracle_rows(c)
    bad = np.argwhere(out[:N].view(np.uint32) != ref.view(np.uint32))
    if bad.size:
        rr = A.ref_rows(c)
        msgs = ["column %d head %d dim %d: kernel %r oracle %r (T %d, fragile %s)" % (i, j // 64, j % 64, float(out[i, j]), float(ref[i, j]), int(c.T[i]),
                                                                                    bool(rr[i][j // 64]["fragile"][j % 64])) for i, j in bad[:6]]
        assert False, (len(bad), msgs)
    assert (out[N:].view(np.uint8) == 0xff).all(), "a store beyond column N"
    if not q8:
        return
    for i in range(N):
        q_ref, d_ref, s_ref = oracle_q8(oracle, ref[i], q8)
        assert (oq[i] == q_ref).all(), ("Q8 codes", i, np.flatnonzero(oq[i] != q_ref)[:6])
        assert (od[i].view(np.uint32) == d_ref.view(np.uint32)).all(), ("Q8 d", i, od[i], d_ref)
        assert (os_[i] == s_ref).all(), ("Q8 s", i, os_[i], s_ref)
    for name, x in (("codes", oq), ("d", od), ("s", os_)):
        assert (x[N:].view(np.uint8) == 0xff).all(), ("a Q8 store beyond column N", name)


def test_probe_refuses_what_the_engine_never_launches(pkg):
    """Every refusal is made before the device is touched, so small arrays serve."""
    z = np.zeros((16, A.H * 64), np.float32)
    state = lambda n_past, causal=0, chunk=0: np.array([n_past, 0, causal, chunk], dtype=np.int32)
    big = np.zeros((A.H, 2048, 64), np.float32)
    for kw, msg in ((dict(form=0, N=1, P=2048, t_max=1024, dev_state=state(1023)), "t_max must be in"), (dict(form=0, N=1, P=4096, t_max=2049, dev_state=state(2048)), "t_max must be in"),
                    (dict(form=1, N=8, P=2048, t_max=1100, dev_state=state(1092)), "tile form"), (dict(form=0, N=9, P=2048, t_max=1100, dev_state=state(1091)), "column form"),
                    (dict(form=0, N=2, P=2048, t_max=1100, dev_state=state(1200)), "visible keys"), (dict(form=0, N=2, P=2048, t_max=1100, dev_state=state(-1, 1)), "negative"),
                    (dict(form=1, N=16, P=2048, t_max=1100, dev_state=state(1090)), "visible keys"), (dict(form=2, N=1, P=2048, t_max=1100, dev_state=state(1099)), "form must be"),
                    (dict(form=0, N=1, P=1090, t_max=1100, dev_state=state(1099)), "at most P"), (dict(form=0, N=1, P=2048, t_max=1100, dev_state=None), "NULL"),
                    (dict(form=0, N=1, P=2048, t_max=1100, dev_state=state(1099), q8=3), "q8 must be")):
        kv = big if kw["P"] <= 2048 else np.zeros((A.H, kw["P"], 64), np.float32)
        rc, out = pkg.attn_long_device(H=A.H, q=z, k_slot=kv, v_slot=kv, **kw)[:2]
        assert rc == -1 and msg in pkg._err(), (kw, rc, pkg._err())
        assert (out == 0).all()
