"""A restatement of a queue session's schedule (biogpt_hip_queue_plan_script; include/biogpt_hip.h, "queue sessions") in plain Python, written from the
contract and not from the C++: a waiting list instead of a cursor, one dict per column.  Used by tests/test_queue_session_restatement.py and, for the group
counts of the arrival scripts, by tools/queue_session_bench.py."""

SUBMIT, POLL, CANCEL = 0, 1, 2


def plan_script(ops, gen_lens, limits, max_columns, group):
    """ops: (SUBMIT,), (POLL, n), (CANCEL, r).  Returns admit_step, column, finish_group, lens (per request) and stats, as the binding does."""
    cols = [dict(req=None, since=0, used=False) for _ in range(max_columns)]
    waiting = []                # pending requests, in submission order
    where = {}                  # request -> "waiting" | "running" | "done"
    news, asked = [], []        # since the last poll: requests without room for a token; cancels in the order asked
    n = 0
    admit_step, column, finish_group, lens = [], [], [], []
    st = dict(columns=max_columns, steps=0, groups=0, admissions=0, prompt_columns=0, busy_column_steps=0, column_steps=0)

    def leave(c, had):
        r = c["req"]
        c["req"] = None
        where[r] = "done"
        finish_group[r], lens[r] = st["groups"], had
        st["busy_column_steps"] += had

    for op in ops:
        kind = op[0]
        if kind == SUBMIT:
            r, n = n, n + 1
            admit_step.append(-1); column.append(-1); finish_group.append(-1); lens.append(0)
            if limits[r] > 0:
                where[r] = "waiting"
                waiting.append(r)
            else:
                where[r] = "done"
                news.append(r)
        elif kind == CANCEL:
            r = op[1]
            if r in where and where[r] != "done" and r not in asked:
                asked.append(r)
        else:
            for r in news:
                finish_group[r] = st["groups"]
            news = []
            for r in asked:
                if where[r] == "waiting":
                    waiting.remove(r)
                    where[r] = "done"
                    finish_group[r] = st["groups"]
                else:
                    c = next(c for c in cols if c["req"] == r)
                    leave(c, c["since"])
            asked = []
            for _ in range(op[1]):
                if not waiting and all(c["req"] is None for c in cols):
                    break
                took = False
                for i, c in enumerate(cols):
                    if c["req"] is None and waiting:
                        r = waiting.pop(0)
                        c["req"], c["since"], c["used"] = r, 0, True
                        where[r] = "running"
                        admit_step[r], column[r] = st["steps"], i
                        took = True
                st["admissions"] += 1 if took else 0
                g = min(group, max(limits[c["req"]] - c["since"] for c in cols if c["req"] is not None))
                for c in cols:
                    if c["used"]:
                        c["since"] += g
                st["steps"] += g
                st["column_steps"] += g * max_columns
                st["groups"] += 1
                for c in cols:
                    if c["req"] is not None and c["since"] >= gen_lens[c["req"]]:
                        leave(c, gen_lens[c["req"]])
    return dict(stats=st, admit_step=admit_step, column=column, finish_group=finish_group, lens=lens)
