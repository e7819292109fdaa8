"""The two long attention kernels over column states (csrc/kernels_attn_long_cols.hip.h: attn_long_seq_kernel<SHARED>, attn_long_runs_kernel), alone, against
the oracle's attention (oracle/biogpt_oracle.c, bo_attn_head) at 1025 .. 2048 keys.  biogpt_hip_attn_long_cols_device launches them through the helper the
engine's passes use; layouts and the oracle's rows are those of tests/attn_cases.py (H = 3 heads of 64; SENTINEL in every row no column may see).

Every column's outputs equal the oracle's as uint32; the Q8 codes, d and s equal the oracle's quantizer on the oracle's row; rows from N on and the guard row
still hold 0xff; the launch is the expected one.  The kernels differ from the oracle only in how they associate the double sums: the seeds below were chosen so
that the restatement (tests/attn_ref.py) finds no fragile row in any case, so no tolerance is owed -- attn_ref is looked up only to word a failure."""
import numpy as np
import pytest

import attn_cases as A
from test_gpu_attn_kernels import oracle_q8

pytestmark = pytest.mark.gpu


def causal(last, n):
    return list(range(last - n + 1, last + 1))


def run_case(name, P, runs, q8):
    """Packed columns in runs that share a slot: runs = [(visible keys per column, shared rows, seed)]; run r lives in slot order[r] with content of its own."""
    N = sum(len(ts) for ts, _, _ in runs)
    order = np.random.default_rng(N).permutation(N)
    q, tables, T, perm, ns = [], [], [], [], []
    for r, (ts, shared, seed) in enumerate(runs):
        qr, K, V = A.content("plain", max(ts), seed=seed)
        for i, t in enumerate(ts):
            q.append(qr[i]); tables.append((K[:, :t], V[:, :t])); T.append(t); perm.append(order[r]); ns.append(shared)
    return A.Case(name, A.TILE, N, P, np.array(q), tables, "seq", T=T, col_mode=1, perm=perm, n_shared=ns if any(ns) else None, q8=q8)


# name -> (form, case, run plans to evaluate: None = the planner's)
CASES = {
    # columns of 5, 1025 and 2048 keys in one launch; slot = column index
    "col-mixed": lambda: (0, A.seq_case("mixed", A.FAST_4, 3, 2048, *A.content("plain", 2048, seed=1), [5, 1025, 2048], q8=1), [None]),
    # packed: a slot permutation, n_past != t_vis - 1
    "col-packed": lambda: (0, A.distinct_seq_case("packed", A.FAST_4, 3, 2048, [2048, 5, 1025], None, 41, col_mode=1, q8=2), [None]),
    "col-shared": lambda: (0, A.distinct_seq_case("shared", A.FAST_4, 3, 2048, [2048, 1025, 1100], [8, 1024, 1099], 42, q8=0), [None]),
    "col-shared-packed": lambda: (0, A.distinct_seq_case("shared packed", A.FAST_4, 2, 2048, [1025, 2048], [1024, 2047], 43, col_mode=1, q8=1), [None]),
    "col-P1030": lambda: (0, A.seq_case("P1030", A.FAST_4, 2, 1030, *A.content("plain", 1030, seed=2), [1030, 1026], q8=2), [None]),
    # runs of 16 (causal, straddling 1024 keys), 7 (the largest t_vis first) and 1 column, each in a slot of its own
    "runs-16-7-1": lambda: (1, run_case("16-7-1", 2048, [(causal(1032, 16), 0, 3), ([2048, 1500, 1100, 1026, 900, 30, 5], 0, 4), ([1025], 0, 5)], 1), [None]),
    # a run of 8 behind 1500 shared rows beside a run of 16 by chunks of 8 without any
    "runs-shared": lambda: (1, run_case("shared", 2048, [(causal(1508, 8), 1500, 6), ([1292] * 8 + [1300] * 8, 0, 7)], 2), [None]),
    "runs-P1030": lambda: (1, run_case("P1030", 1030, [(causal(1030, 16), 0, 8), (causal(1028, 3), 0, 9)], 0), [None]),
    # one pass cut into runs two ways: identical bytes per column
    "runs-cuts": lambda: (1, run_case("cuts", 2048, [(causal(1036, 17), 0, 10)], 1), [[(0, 16), (16, 1)], [(0, 9), (9, 8)]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_oracle(pkg, oracle, name):
    form, c, plans = CASES[name]()
    N, q8 = c.N, c.q8
    k, v = c.slots()
    ref = A.oracle_rows(c)
    outs = []
    for plan in plans:
        rc, out, oq, od, os_, launched = pkg.attn_long_cols_device(form, A.H, c.P, c.t_max, c.n_slots, c.q, k, v, c.states()[1], col_mode=c.col_mode,
                                                                   shared=c.n_shared is not None, runs=plan, q8=q8)
        assert rc == 0, pkg._err()
        n_runs = len(plan if plan is not None else pkg.long_runs_plan(c.states()[1]))
        assert tuple(launched[:4]) == (form, 1024, A.H, n_runs if form else N) and launched[5] == c.t_cap, list(launched)
        assert (launched[4] >= 16 * c.t_cap * 4 and launched[6] == n_runs) if form else launched[4] == 16576, list(launched)
        bad = np.argwhere(out[:N].view(np.uint32) != ref.view(np.uint32))
        if bad.size:
            rr = A.ref_rows(c)
            msgs = ["column %d head %d dim %d: kernel %r oracle %r (T %d, fragile %s)" % (i, j // 64, j % 64, float(out[i, j]), float(ref[i, j]), int(c.T[i]),
                                                                                        bool(rr[i][j // 64]["fragile"][j % 64])) for i, j in bad[:6]]
            assert False, (len(bad), msgs)
        assert (out[N:].view(np.uint8) == 0xff).all(), "a store beyond column N"
        for i in range(N if q8 else 0):
            q_ref, d_ref, s_ref = oracle_q8(oracle, ref[i], q8)
            assert (oq[i] == q_ref).all(), ("Q8 codes", i, np.flatnonzero(oq[i] != q_ref)[:6])
            assert (od[i].view(np.uint32) == d_ref.view(np.uint32)).all(), ("Q8 d", i, od[i], d_ref)
            assert (os_[i] == s_ref).all(), ("Q8 s", i, os_[i], s_ref)
        for what, x in (("codes", oq), ("d", od), ("s", os_)):
            assert not q8 or (x[N:].view(np.uint8) == 0xff).all(), ("a Q8 store beyond column N", what)
        outs.append((out, oq, od, os_))
    for other in outs[1:]:      # a column's bytes do not depend on the run it sits in
        assert all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(outs[0], other))


def test_probe_refuses_what_the_engine_never_launches(pkg):
    """Every refusal is made before the device is touched, so small arrays serve."""
    kv = np.zeros((2, A.H, 2048, 64), np.float32)

    def st(t_vis, slot=0, ns=0, shr=0):
        return [[t - 1, 0, 0, slot, t, ns, shr, 0] for t in t_vis]
    for kw, states, msg in ((dict(form=0, t_max=1024), st([1024]), "t_max must be in"), (dict(form=0, t_max=2049), st([2049]), "t_max must be in"),
                            (dict(form=2, t_max=1100), st([1100]), "form must be"), (dict(form=1, t_max=1100, col_mode=0), st([1100]), "packed columns"),
                            (dict(form=0, t_max=1100), st([1200]), "visible keys"), (dict(form=0, t_max=1100), st([1100], slot=2), "slot"),
                            (dict(form=0, t_max=1100, shared=True), st([1100], ns=1101), "shared rows"), (dict(form=1, t_max=1100), st([1100], shr=2), "shared slot"),
                            (dict(form=1, t_max=1100, runs=[(0, 17)]), st([1100] * 17), "outside [1, 16]"), (dict(form=1, t_max=1100, runs=[(0, 1)]), st([1100] * 2), "cover"),
                            (dict(form=1, t_max=1100, runs=[(0, 2)]), st([1100]) + st([1100], slot=1), "another slot"),
                            (dict(form=0, t_max=1100, P=1090), st([1090]), "at most P"), (dict(form=0, t_max=1100, q8=3), st([1100]), "q8 must be")):
        kw = dict(dict(H=A.H, P=2048, n_slots=2, q=np.zeros((32, A.H * 64), np.float32), k_slots=kv, v_slots=kv), **kw)
        rc, out = pkg.attn_long_cols_device(seq_states=states, **kw)[:2]
        assert rc == -1 and msg in pkg._err(), (kw["form"], msg, rc, pkg._err())
        assert (out == 0).all()
