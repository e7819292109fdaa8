"""The schedule of a queue session without a GPU: biogpt_hip_queue_plan_script -- the scheduler struct the session itself drives -- is held to the Python
restatement tests/queue_session_ref.py on random scripts of submits, polls and cancels (of pending, running, finished and unknown requests, and polls of an
idle session), and a script of all submits followed by polls to the end is held to biogpt_hip_queue_plan_limits, item for item.  Every comparison is exact."""
import numpy as np
import pytest

import queue_session_ref as ref
from queue_session_ref import CANCEL, POLL, SUBMIT


def random_script(rng, max_columns, group):
    """A script and its requests' lengths and limits.  Cancels name requests in every state: the script tracks nothing, it draws ids around the ones submitted so
    far (some not submitted yet or negative: unknown), early ones (finished by then), recent ones (pending or running)."""
    ops, gen_lens, limits = [], [], []
    n = 0
    for _ in range(int(rng.integers(4, 40))):
        what = rng.random()
        if what < 0.45:
            burst = int(rng.integers(1, 6)) if rng.random() < 0.3 else 1
            for _ in range(burst):
                gl = int(rng.integers(0, 13))
                gen_lens.append(gl)
                limits.append(gl + (int(rng.integers(0, 5)) if gl > 0 and rng.random() < 0.5 else 0))
                ops.append((SUBMIT,))
                n += 1
        elif what < 0.8:
            ops.append((POLL, int(rng.integers(0, 4))))
        else:
            pick = rng.random()
            r = int(rng.integers(-2, n + 3)) if pick < 0.3 else int(rng.integers(0, max(n, 1))) if pick < 0.6 else max(n - 1 - int(rng.integers(0, max_columns + 2)), 0)
            ops.append((CANCEL, r))
            if rng.random() < 0.2:
                ops.append((CANCEL, r))      # twice: the second changes nothing
    for _ in range(int(rng.integers(0, 3))):
        ops.append((POLL, 1000))             # to the end, then on an idle session
    return ops, gen_lens, limits


@pytest.mark.parametrize("max_columns", [1, 2, 3, 8])
@pytest.mark.parametrize("group", [1, 4, 16])
def test_plan_script_equals_the_restatement(pkg, max_columns, group):
    rng = np.random.default_rng(1000 * max_columns + group)
    seen = dict(cancel_running=0, cancel_pending=0, idle_poll=0, zero=0)
    for trial in range(40):
        ops, gen_lens, limits = random_script(rng, max_columns, group)
        want = ref.plan_script(ops, gen_lens, limits, max_columns, group)
        got = pkg.queue_plan_script(ops, gen_lens, limits, max_columns, group)
        assert got == want, (trial, ops, gen_lens, limits, got, want)
        for r in range(len(gen_lens)):
            if limits[r] == 0:
                seen["zero"] += 1
            elif want["finish_group"][r] >= 0 and want["column"][r] < 0:
                seen["cancel_pending"] += 1
            elif 0 < want["lens"][r] < gen_lens[r]:
                seen["cancel_running"] += 1
        seen["idle_poll"] += 1 if ops and ops[-1] == (POLL, 1000) and len(ops) > 1 and ops[-2] == (POLL, 1000) else 0
    if max_columns <= 3:      # (with 8 columns few requests ever wait)
        assert seen["cancel_pending"] > 0, seen
    if group < 16:            # (no limit here exceeds 16: with group 16 a request ends in the group of its admission, and nothing is ever found running)
        assert seen["cancel_running"] > 0, seen
    assert seen["idle_poll"] > 0 and seen["zero"] > 0, seen


def test_a_few_scripts_by_hand(pkg):
    # two columns, group 4; request 2 waits, is cancelled while pending; request 0 is cancelled while running after one group of 4
    ops = [(SUBMIT,), (SUBMIT,), (SUBMIT,), (SUBMIT,), (POLL, 1), (CANCEL, 2), (CANCEL, 0), (POLL, 1), (POLL, 100), (POLL, 1)]
    got = pkg.queue_plan_script(ops, [10, 6, 5, 3], [10, 6, 5, 3], 2, 4)
    assert got["admit_step"] == [0, 0, -1, 4] and got["column"] == [0, 1, -1, 0]
    assert got["lens"] == [4, 6, 0, 3] and got["finish_group"] == [1, 2, 1, 2]
    assert got["stats"] == dict(columns=2, steps=7, groups=2, admissions=2, prompt_columns=0, busy_column_steps=13, column_steps=14)
    # nothing submitted: polls launch nothing
    got = pkg.queue_plan_script([(POLL, 5), (POLL, 0)], [], [], 3, 4)
    assert got["stats"] == dict(columns=3, steps=0, groups=0, admissions=0, prompt_columns=0, busy_column_steps=0, column_steps=0)
    # a request without room for a token is finished at the next poll and takes no column; cancelling it is refused and changes nothing
    got = pkg.queue_plan_script([(SUBMIT,), (CANCEL, 0), (SUBMIT,), (POLL, 1)], [0, 2], [0, 2], 1, 4)
    assert got["column"] == [-1, 0] and got["finish_group"] == [0, 1] and got["lens"] == [0, 2]


@pytest.mark.parametrize("max_columns, group", [(1, 1), (3, 4), (8, 16), (2, 64)])
def test_all_up_front_is_the_closed_plan(pkg, max_columns, group):
    rng = np.random.default_rng(77 + max_columns)
    for trial in range(20):
        R = int(rng.integers(max_columns, max_columns + 20))
        gen_lens = [int(v) for v in rng.integers(1, 13, R)]
        limits = [g + int(e) for g, e in zip(gen_lens, rng.integers(0, 4, R))]
        for r in rng.integers(0, R, 2):      # some never take a column -- but at least max_columns requests do
            if R - sum(1 for g in gen_lens if g == 0) > max_columns:
                gen_lens[int(r)] = limits[int(r)] = 0
        closed = pkg.queue_plan(gen_lens, max_columns, group, limits=limits)
        for polls in ([(POLL, 10000)], [(POLL, 1)] * 400, [(POLL, 3)] * 150):
            got = pkg.queue_plan_script([(SUBMIT,)] * R + polls, gen_lens, limits, max_columns, group)
            assert got["admit_step"] == closed["admit_step"] and got["column"] == closed["column"] and got["stats"] == closed["stats"], (trial, gen_lens, limits)
            assert got["lens"] == gen_lens and all(f >= 0 for f in got["finish_group"])


def test_plan_script_argument_errors(pkg):
    for kw, field in ((dict(max_columns=0), "max_columns must be in [1, 512]"), (dict(max_columns=513), "max_columns"), (dict(group=0), "group must be in [1, 64]"),
                      (dict(group=65), "group"), (dict(ops=[(3, 0)]), "ops[0]: kind 3"), (dict(ops=[(POLL, -1)]), "POLL -1"),
                      (dict(ops=[(SUBMIT,)], gen_lens=[5], limits=[4]), "limits[0] (4) is below gen_lens[0] (5)"),
                      (dict(ops=[(SUBMIT,)], gen_lens=[0], limits=[4]), "gen_lens[0] is 0 under a limit of 4"),
                      (dict(ops=[(SUBMIT,)], gen_lens=[-1], limits=[4]), "gen_lens[0] (-1) is negative")):
        args = dict(dict(ops=[(POLL, 1)], gen_lens=[], limits=[], max_columns=2, group=4), **kw)
        with pytest.raises(pkg.BiogptError) as e:
            pkg.queue_plan_script(args["ops"], args["gen_lens"], args["limits"], args["max_columns"], args["group"])
        assert field in str(e.value), (kw, str(e.value))
