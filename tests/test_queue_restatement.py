"""The scheduler of generation over a queue without a GPU: biogpt_hip_queue_plan (the host struct biogpt_hip_generate_queue drives) equals the restatement
tests/queue_ref.py exactly over seeded cases, and its schedules have the properties a caller relies on."""
import numpy as np
import pytest

import queue_ref


def cases():
    """(label, gen_lens, max_columns, group): R 1 .. 200, C 1 .. 16, group 1 .. 9; lengths with zeros, ones, all equal, and spread from 1 to 128."""
    out = []
    rng = np.random.default_rng(0x51554555)
    for i in range(300):
        R = int(rng.integers(1, 201))
        C = int(rng.integers(1, 17))
        g = int(rng.integers(1, 10))
        kind = i % 6
        if kind == 0:
            lens = rng.integers(0, 40, R)
        elif kind == 1:
            lens = np.full(R, int(rng.integers(1, 30)))                      # all equal
        elif kind == 2:
            lens = rng.integers(0, 2, R)                                     # zeros and ones
        elif kind == 3:
            lens = np.minimum(128, 1 + rng.geometric(1.0 / 30.0, R))        # long tail
        elif kind == 4:
            lens = np.where(rng.random(R) < 0.3, 0, rng.integers(1, 9, R))   # many that never run
        else:
            lens = np.ones(R, dtype=np.int64)
        out.append(("seeded %d" % i, [int(v) for v in lens], C, g))
    out += [("one request", [5], 1, 4), ("one request, wide", [5], 16, 9), ("nobody eligible", [0, 0, 0], 4, 4), ("R = 200, C = 16", list(range(200)), 16, 9),
            ("R = C", [7] * 16, 16, 3), ("single token each", [1] * 50, 7, 5)]
    return out


CASES = cases()


def test_case_table_covers_the_ranges():
    Rs, Cs, gs = {len(c[1]) for c in CASES}, {c[2] for c in CASES}, {c[3] for c in CASES}
    assert len(CASES) >= 300 and min(Rs) == 1 and max(Rs) == 200 and Cs >= set(range(1, 17)) and gs >= set(range(1, 10))
    assert any(0 in c[1] for c in CASES) and any(1 in c[1] for c in CASES) and any(len(set(c[1])) == 1 and len(c[1]) > 1 for c in CASES)


def test_plan_equals_the_restatement(pkg):
    for label, lens, C, g in CASES:
        assert pkg.queue_plan(lens, C, g) == queue_ref.plan(lens, C, g), (label, lens, C, g)


def test_schedule_properties(pkg):
    for label, lens, max_columns, g in CASES:
        got = pkg.queue_plan(lens, max_columns, g)
        st, adm, col = got["stats"], got["admit_step"], got["column"]
        eligible = [r for r, n in enumerate(lens) if n > 0]
        C = min(max_columns, len(eligible))
        assert st["columns"] == C, label
        # every eligible request is admitted exactly once, in index order; the others never
        assert all((adm[r] >= 0 and 0 <= col[r] < C) for r in eligible) and all(adm[r] == -1 and col[r] == -1 for r in range(len(lens)) if lens[r] == 0), label
        assert [adm[r] for r in eligible] == sorted(adm[r] for r in eligible), label
        # no column holds two requests at a step: the tenures [admit_step, admit_step + length) of a column's requests do not overlap
        for c in range(C):
            mine = sorted((adm[r], adm[r] + lens[r]) for r in eligible if col[r] == c)
            assert all(a[1] <= b[0] for a, b in zip(mine, mine[1:])), (label, c)
        assert all(adm[r] + lens[r] <= st["steps"] for r in eligible), label
        assert st["busy_column_steps"] == sum(lens) <= st["column_steps"] == C * st["steps"], label
        if C:
            assert st["steps"] >= -(-sum(lens) // C), label
            assert st["groups"] >= -(-st["steps"] // g) and st["admissions"] >= 1, label
        else:
            assert st["steps"] == st["groups"] == st["admissions"] == 0, label
        if 0 < len(eligible) <= max_columns:      # everybody runs at once: one admission, as many steps as the longest takes
            assert st["admissions"] == 1 and st["steps"] == max(lens) and all(adm[r] == 0 for r in eligible), label
            assert [col[r] for r in eligible] == list(range(len(eligible))), label


def test_plan_by_hand(pkg):
    """Two columns, group 2, lengths 3 1 2 4: requests 0 and 1 start; the look behind steps 2 finds 1 finished (it idled one step) -> 2 takes column 1 at
    step 2; the look behind step 4 finds 0 and 2 finished -> 3 takes column 0 at step 4 and runs two groups alone."""
    got = pkg.queue_plan([3, 1, 2, 4], 2, 2)
    assert got["admit_step"] == [0, 0, 2, 4] and got["column"] == [0, 1, 1, 0]
    assert got["stats"] == dict(columns=2, steps=8, groups=4, admissions=3, prompt_columns=0, busy_column_steps=10, column_steps=16)
    # the last group is cut to what the only running column may still generate
    assert pkg.queue_plan([5], 4, 4)["stats"] == dict(columns=1, steps=5, groups=2, admissions=1, prompt_columns=0, busy_column_steps=5, column_steps=5)


@pytest.mark.parametrize("args, field", [
    (dict(lens=None), "gen_lens"), (dict(adm=False), "admit_step"), (dict(col=False), "column"), (dict(n=0), "n_requests"), (dict(n=-2), "n_requests"),
    (dict(C=0), "max_columns"), (dict(C=513), "max_columns"), (dict(g=0), "group"), (dict(g=65), "group"), (dict(lens=[3, -1]), "gen_lens[1]"),
])
def test_plan_argument_errors(pkg, args, field):
    lens = args.get("lens", [3, 1])
    gl = None if lens is None else np.asarray(lens, dtype=np.int32)
    adm, col = np.zeros(2, np.int32), np.zeros(2, np.int32)
    rc = pkg.lib().biogpt_hip_queue_plan(None if gl is None else gl.ctypes.data, args.get("n", 2), args.get("C", 2), args.get("g", 2),
                                         adm.ctypes.data if args.get("adm", True) else None, col.ctypes.data if args.get("col", True) else None, None)
    assert rc == -1 and field in pkg._err(), (rc, pkg._err())
