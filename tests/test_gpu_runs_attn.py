"""attn_runs_kernel<8>, alone, against the oracle's attention (bo_attn_head) through its probe (biogpt_hip_attn_runs_device, which launches through the
engine's own helper).  The cases are those of tests/runs_ref.py, which tests/test_runs_restatement.py examines on the CPU (no committed case has a fragile row,
so bit equality is owed everywhere): every column's outputs equal the oracle's bit for bit; the Q8 codes, d and s equal the oracle's quantizer on the oracle's
row; the rows from N on and the guard row still hold 0xff; every row no column may see holds SENTINEL, so a load on the wrong side of a border shows.
Then the property the call's promises rest on -- a column's bits do not depend on the run it sits in -- and the probe's refusals of a bad run table."""
import numpy as np
import pytest

import attn_cases as A
import runs_ref as R
from test_gpu_attn_kernels import oracle_q8

pytestmark = pytest.mark.gpu


def launch(pkg, c, runs=None, st=None):
    k, v = c.slots()
    return pkg.attn_runs_device(A.H, c.P, c.t_max, c.n_slots, c.q, k, v, c.st if st is None else st, runs=runs, q8=c.q8)


def check(pkg, oracle, c):
    what = "%s [N %d, P %d, t_max %d]" % (c.name, c.N, c.P, c.t_max)
    rc, out, oq, od, os_, launched = launch(pkg, c)
    assert rc == 0, (what, pkg._err())
    n_runs = len(R.plan(c.st))
    assert tuple(launched[:5]) == (16, 512, A.H, n_runs, 0) and launched[5] == min(c.P, (c.t_max + 63) // 64 * 64) and launched[6] == n_runs, (what, list(launched))
    ref = R.oracle_rows(c)
    got, N = out[:c.N], c.N
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    if bad.size:
        rr = R.ref_rows(c)
        msgs = []
        for i, j in bad:
            h, d = int(j) // 64, int(j) % 64
            r = rr[i][h]
            if r["fragile"][d] and abs(float(got[i, j]) - float(ref[i, j])) <= float(np.spacing(np.abs(ref[i, j]))):
                continue        # the association decides this float32: one ulp is owed, no more
            msgs.append("column %d head %d dim %d: kernel %r oracle %r (T %d, fragile %s)" % (i, h, d, float(got[i, j]), float(ref[i, j]), int(c.T[i]), bool(r["fragile"][d])))
        assert not msgs, (what, len(msgs), msgs[:6])
    assert (out[N:].view(np.uint8) == 0xff).all(), (what, "a store beyond column N", np.argwhere(out[N:].view(np.uint32) != 0xffffffff)[:4])
    if not c.q8:
        return
    for i in range(N):
        q_ref, d_ref, s_ref = oracle_q8(oracle, ref[i], c.q8)
        assert (oq[i] == q_ref).all(), (what, "Q8 codes", i)
        assert (od[i].view(np.uint32) == d_ref.view(np.uint32)).all(), (what, "Q8 d", i, od[i], d_ref)
        assert (os_[i] == s_ref).all(), (what, "Q8 s", i, os_[i], s_ref)
    for name, x in (("codes", oq), ("d", od), ("s", os_)):
        assert (x[N:].view(np.uint8) == 0xff).all(), (what, "a Q8 store beyond column N", name)


def _groups():
    g = {}
    for c in R.kernel_cases():
        key = "family" if c.family != "plain" else "%s P %d" % (c.name.split()[0], c.P)
        g.setdefault(key, []).append(c)
    return g


@pytest.mark.parametrize("group", sorted(_groups()))
def test_kernel_equals_the_oracle(pkg, oracle, group):
    for c in _groups()[group]:
        check(pkg, oracle, c)


def association_case():
    """24 columns: 13 consecutive tokens of a prompt (rows 40 .. 52), then 11 candidates behind 37 shared rows with 1 .. 40 rows of their own."""
    return R.RunCase("association", 100, [("pre", 40, 13), ("cont", 37, [1, 40, 7, 8, 15, 16, 17, 2, 1, 40, 9])], seed=9, q8=2)


def test_a_columns_bits_do_not_depend_on_its_run(pkg):
    c = association_case()
    assert c.N == 24
    st = c.st
    singles = [(i, 1, int(st[i, 4]) if st[i, 5] == 0 else int(st[i, 5]), int(st[i, 3]) if st[i, 5] == 0 else int(st[i, 6])) for i in range(24)]
    planned = R.plan(st)
    assert planned == [(0, 8, 40, 0), (8, 5, 48, 0), (13, 8, 37, 1), (21, 3, 37, 1)]
    # cut at odd places: the prompt's columns with a smaller legal R (1, 0 and 7 rows shared instead of 40 and more), the candidates 3 + 1 + 7
    odd = [(0, 3, 1, 0), (3, 7, 7, 0), (10, 3, 0, 0), (13, 3, 37, 1), (16, 1, 37, 1), (17, 7, 37, 1)]
    for t in (singles, planned, odd):
        R.check_invariants(st, t)
    results = []
    for t in (singles, planned, odd, None):
        rc, out, oq, od, os_, launched = launch(pkg, c, runs=None if t is None else np.asarray(t, dtype=np.int32))
        assert rc == 0, pkg._err()
        assert launched[3] == (len(planned) if t is None else len(t))
        results.append((out, oq, od, os_))
    for name, other in zip(("the planner's table", "odd cuts", "no table"), results[1:]):
        for a, b in zip(results[0], other):
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), name


def test_probe_refuses_a_bad_run_table(pkg):
    c = association_case()
    good = np.asarray(R.plan(c.st), dtype=np.int32)

    def refused(field, runs=None, st=None, **over):
        rc, out = launch(pkg, c, runs=None if runs is None else np.asarray(runs, dtype=np.int32), st=st)[:2]
        assert rc == -1 and field in pkg._err(), (field, rc, pkg._err())
        assert (out == 0).all()

    edit = lambda row, col, val: [tuple(val if (r == row and k == col) else int(x) for k, x in enumerate(t)) for r, t in enumerate(good)]
    refused("exactly one run", edit(1, 0, 7))                                 # overlap: column 7 in two runs
    refused("exactly one run", edit(1, 0, 9))                                 # a column in no run
    refused("n = 9", [(0, 9, 40, 0), (9, 4, 49, 0)] + [tuple(int(x) for x in t) for t in good[2:]])
    refused("n = 0", edit(3, 1, 0))
    refused("not all 24", [tuple(int(x) for x in t) for t in good[:3]])
    refused("beyond N", edit(3, 1, 4))
    refused("do not lie in slot", edit(0, 2, 41))                             # column 0 sees 40 rows only
    refused("do not lie in slot", edit(0, 3, 1))                              # the prompt's rows are in slot 0
    refused("do not lie in slot", edit(2, 2, 36))                             # row 36 of a candidate is a shared row, not its own
    refused("do not lie in slot", edit(2, 2, 38))                             # row 37 is the candidate's own
    refused("do not lie in slot", edit(2, 3, 0))
    refused("outside the slots", edit(2, 3, c.n_slots))
    st = c.st.copy()
    st[5, 4] = 101
    refused("visible keys", st=st)
    st = c.st.copy()
    st[20, 6] = c.n_slots
    refused("shared slot", st=st)
    rc = launch(pkg, c, runs=good)[0]
    assert rc == 0, pkg._err()
