"""The schedule of generation over a queue (biogpt_hip_generate_queue / biogpt_hip_queue_plan), restated in plain Python from its description,
not from the C++:

  1. eligible requests (length > 0) are admitted in index order, the first C = min(max_columns, eligible) into columns 0 .. C - 1;
  2. steps run in groups of min(group, the most tokens any running column may still generate);
  3. behind each group the host looks at the columns: a column whose request has generated all its tokens is finished;
  4. finished columns are refilled in ascending column order with the next pending requests in ascending request order;
  5. the run ends when a look shows no running column and nothing pending.

admit_step[r]: the steps run before r's first step; column[r]: its column; both -1 for a request that never ran.  Stats: steps, groups, admissions (refill
rounds that admitted somebody, the first included), busy_column_steps = the sum of the lengths, column_steps = C * steps; the plan knows no prompts, so
prompt_columns is 0."""


def plan(gen_lens, max_columns, group):
    lens = [int(v) for v in gen_lens]
    waiting = [r for r, n in enumerate(lens) if n > 0]
    C = min(int(max_columns), len(waiting))
    admit_step, column = [-1] * len(lens), [-1] * len(lens)
    holder = [None] * C          # column -> the request that runs there (None: free)
    left = {}                    # running request -> tokens it still generates
    steps = groups = admissions = 0
    while waiting or left:
        took = False
        for col in range(C):
            if holder[col] is None and waiting:
                r = waiting.pop(0)
                holder[col], left[r] = r, lens[r]
                admit_step[r], column[r] = steps, col
                took = True
        admissions += 1 if took else 0
        g = min(int(group), max(left.values()))
        steps += g
        groups += 1
        for col in range(C):
            r = holder[col]
            if r is not None:
                left[r] -= g
                if left[r] <= 0:
                    del left[r]
                    holder[col] = None
    stats = dict(columns=C, steps=steps, groups=groups, admissions=admissions, prompt_columns=0, busy_column_steps=sum(lens), column_steps=C * steps)
    return dict(stats=stats, admit_step=admit_step, column=column)
