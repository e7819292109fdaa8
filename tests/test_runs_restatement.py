"""attn_runs_kernel's planner and cases on the CPU (tests/runs_ref.py): the Python restatement of the planner against biogpt_hip_attn_runs_plan on hand-made
passes and on every kernel case, the invariants of a run table, and what the oracle (bo_attn_head) and the restatement of its arithmetic (tests/attn_ref.py)
say about the cases of tests/test_gpu_runs_attn.py: no row is fragile, so that test owes bit equality with the oracle on every row."""
import numpy as np
import pytest

import attn_cases as A
import runs_ref as R


def both_plans(pkg, st):
    want = R.plan(st)
    got = [tuple(int(x) for x in r) for r in pkg.attn_runs_plan(st)]
    assert got == want, (got[:8], want[:8])
    R.check_invariants(st, want)
    return want


def test_hand_made_passes(pkg):
    # a prefix crossing a pass border: the pass starts at token 509 of prompt 0 (rows 510 ..), then prompt 1 whole
    st, _ = R.column_states([("pre", 510, 11), ("pre", 1, 3)])
    assert both_plans(pkg, st) == [(0, 8, 510, 0), (8, 3, 518, 0), (11, 3, 1, 1)]
    # two groups adjacent: a run never spans two groups, even of equal pad[0]
    st, _ = R.column_states([("cont", 40, [1, 1, 1]), ("cont", 40, [1, 1])])
    assert both_plans(pkg, st) == [(0, 3, 40, 0), (3, 2, 40, 1)]
    # n_prefix = 1: pad[0] = 0, every candidate a slot of its own -> lone prefix runs of its own rows
    st, _ = R.column_states([("cont", 0, [1, 1, 1])])
    assert both_plans(pkg, st) == [(0, 1, 1, 1), (1, 1, 1, 2), (2, 1, 1, 3)]
    # a 40-token continuation: 40 columns of one (pad[0], pad[1]) in five runs; its own rows differ per column
    st, n_slots = R.column_states([("cont", 300, [1])])
    st = np.repeat(st, 40, axis=0)
    st[:, 4] = 301 + np.arange(40)
    assert both_plans(pkg, st) == [(8 * k, 8, 300, 0) for k in range(5)]
    # 9 candidates: 8 + 1;  a lone column
    st, _ = R.column_states([("cont", 7, [1] * 9)])
    assert both_plans(pkg, st) == [(0, 8, 7, 0), (8, 1, 7, 0)]
    st, _ = R.column_states([("pre", 5, 1)])
    assert both_plans(pkg, st) == [(0, 1, 5, 0)]
    # prefix columns, then candidates, in one pass (the mixed pass of a call)
    st, _ = R.column_states([("pre", 1, 9), ("cont", 9, [1, 2, 3])])
    assert both_plans(pkg, st) == [(0, 8, 1, 0), (8, 1, 9, 0), (9, 3, 9, 1)]
    # a column that sees fewer rows than pad[0] stands alone
    st, _ = R.column_states([("cont", 9, [1, 2, 3])])
    st[1, 4] = 4
    assert both_plans(pkg, st) == [(0, 1, 9, 0), (1, 1, 4, 0), (2, 1, 9, 0)]


def test_planner_on_every_kernel_case_and_random_passes(pkg):
    for c in R.kernel_cases():
        both_plans(pkg, c.st)
    rng = np.random.default_rng(5)
    for _ in range(200):
        groups = []
        for g in range(int(rng.integers(1, 6))):
            if rng.integers(0, 2):
                groups.append(("pre", int(rng.integers(1, 50)), int(rng.integers(1, 20))))
            else:
                groups.append(("cont", int(rng.integers(0, 50)), [int(v) for v in rng.integers(1 if len(groups) % 2 else 0, 41, int(rng.integers(1, 12)))]))
        st, _ = R.column_states(groups)
        st = st[st[:, 4] > 0]
        if len(st):
            both_plans(pkg, st)


def test_plan_refuses_null_and_bad_counts(pkg):
    st = np.zeros((1, 8), dtype=np.int32)
    out = np.zeros((1, 4), dtype=np.int32)
    f = pkg.lib().biogpt_hip_attn_runs_plan
    assert f(None, 1, out.ctypes.data) == -1 and f(st.ctypes.data, 1, None) == -1 and f(st.ctypes.data, 0, out.ctypes.data) == -1


def test_the_case_list_covers_what_the_kernel_can_get_wrong():
    cs = R.kernel_cases()
    plain = [c for c in cs if c.family == "plain"]
    assert {c.N for c in plain if len(c.groups) == 1} >= {1, 7, 8, 9, 17, 33} and {c.P for c in cs} == {100, 1024}
    assert {g[1] for c in cs for g in c.groups if g[0] == "cont"} >= {1, 2, 63, 64, 65, 127, 128, 129, 1016, 1023}
    assert {o for c in cs for g in c.groups if g[0] == "cont" for o in g[2]} >= set(R.OWN)
    assert any(len({g[0] for g in c.groups}) == 2 for c in cs) and {c.family for c in cs} >= set(R.FAMILIES)
    assert {c.q8 for c in cs} == {0, 1, 2}


def test_no_kernel_case_has_a_fragile_row_and_the_sentinel_stays_out(oracle):
    fragile, near, bad, rows = [], [], [], 0
    for c in R.kernel_cases():
        ref, orc = R.ref_rows(c), R.oracle_rows(c)
        assert np.isfinite(orc).all(), c.name
        k, v = c.slots()
        seen = np.zeros(k.shape[:3], dtype=bool)
        for i in range(c.N):
            T, ns, sh, own = int(c.st[i, 4]), int(c.st[i, 5]), int(c.st[i, 6]), int(c.st[i, 3])
            seen[sh, :, :ns] = True
            seen[own, :, ns:T] = True
            for h in range(A.H):
                K = np.concatenate([k[sh, h, :ns], k[own, h, ns:T]])
                V = np.concatenate([v[sh, h, :ns], v[own, h, ns:T]])
                Kl, Vl = c.gather(i, h)
                assert K.shape == Kl.shape and (K == Kl).all() and (V == Vl).all(), (c.name, i, h, "the layout does not hold the case's rows")
                r, o = ref[i][h], orc[i, h * 64:(h + 1) * 64]
                rows += 1
                if r["fragile"].any():
                    fragile.append((c.name, i, h))
                if r["inv_near_tie"]:
                    near.append((c.name, i, h, r["sum"]))
                ne = (r["out"].view(np.uint32) != o.view(np.uint32)) & ~r["fragile"]
                if ne.any():
                    bad.append((c.name, i, h, int(np.argmax(ne))))
        assert (k[~seen] == A.SENTINEL).all() and (v[~seen] == A.SENTINEL).all(), (c.name, "a row no column may see holds something else")
        assert (k[seen] != A.SENTINEL).any(axis=-1).all(), c.name
    assert not bad, (len(bad), bad[:6])
    assert not fragile, ("a seed gives a fragile row: choose another seed", fragile[:6])
    assert not near, near[:6]
    assert rows > 1500
