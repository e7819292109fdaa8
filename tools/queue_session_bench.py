#!/usr/bin/env python3
"""Queue sessions (BiogptModel.queue_session) on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed), on the workload of
tools/queue_requests_bench.py: 512 requests with 32-token prompts, greedy, no EOS, n_batch 8, every request with its own n_predict (the same draw).
Milliseconds by host wall clock, the routes of one row in turn, round after round: `--warmup` rounds thrown away, then `--reps` rounds (median, min, max).
Prints one JSON line with, per max_columns (64, 256):

  upfront    all 512 requests submitted before the first poll, then polls of one group to the end: `session` against `closed` = generate_queue(params=) of the
             same requests.  What the resumable form and the per-poll drain cost.
  stream     the `upfront` script with stream off and on: `plain` against `stream`, and per look what the extra launch and the larger copy add
             (us_per_look = the difference over the groups run).
  arrivals   the requests arrive k per group (`--rate`): `session` = submit what has arrived, poll one group, repeat; `batches` = what a caller can do with the
             closed call: collect max_columns arrivals, run generate_queue(params=) on them, repeat.  Total time, and per request the groups from its arrival to
             its first token and to its completion (median, worst): counts, not wall clock -- a group is the clock's tick in both routes, a batch starts at the
             later of its last member's arrival and the end of the batch before -- taken from the run (session) and from queue_plan_script (batches), and the
             session's are checked against queue_plan_script.

  python tools/queue_session_bench.py [--reps 9] [--warmup 2] [--columns 64,256] [--rows upfront,stream,arrivals] [--rate 8]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x42494F47
N_REQUESTS, N_PROMPT, GROUP = 512, 32, 4
LEN_SEED, LEN_MIN, LEN_MAX, LEN_SCALE = 20261019, 4, 128, 38.0


def summary(ts, extra):
    return dict(ms=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3), n=len(ts), **extra)


def timed_in_turn(routes, reps, warmup):
    ts, extra = {name: [] for name in routes}, {}
    for rd in range(warmup + reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            extra[name] = fn()
            if rd >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(v, extra[name]) for name, v in ts.items()}


def spread(v):
    return dict(median=float(np.median(v)), worst=int(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="upfront,stream,arrivals")
    ap.add_argument("--columns", default="64,256")
    ap.add_argument("--rate", type=int, default=8)
    a = ap.parse_args()
    want = a.rows.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    rng = np.random.default_rng(LEN_SEED)
    limits = [int(v) for v in np.clip(LEN_MIN + np.floor(rng.exponential(LEN_SCALE, N_REQUESTS)), LEN_MIN, LEN_MAX)]
    res = {"metric": "queue_session_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_requests": N_REQUESTS, "n_prompt": N_PROMPT, "n_batch": 8, "group": GROUP,
           "rate": a.rate, "reps": a.reps, "warmup": a.warmup, "rows": want}
    prng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in prng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(N_REQUESTS)]
        seeds = [1 + r for r in range(N_REQUESTS)]
        greedy = m.request_params(top_k=1)
        max_len = N_PROMPT + LEN_MAX

        def closed(columns, idx):
            ids, info, _ = g.generate_queue([prompts[r] for r in idx], max(limits), max_columns=columns, group=GROUP, seeds=[seeds[r] for r in idx], n_batch=8,
                                            n_predicts=[limits[r] for r in idx], params=greedy)
            assert [len(i) for i in ids] == [limits[r] for r in idx]
            return info["stats"]

        def session(columns, rate, stream=False):
            """rate 0: everything up front.  Returns (stats, per request: arrival tick, first-token tick, completion tick, the planner's ops)."""
            arrive, done, admit, ops, steps_at = {}, {}, {}, [], [0]
            with g.queue_session(max_columns=columns, group=GROUP, n_predict=max(limits), stream=stream, max_len=max_len) as s:
                at = 0
                while at < N_REQUESTS or not s.idle():
                    for r in range(at, N_REQUESTS if rate == 0 else min(at + rate, N_REQUESTS)):
                        s.submit(prompts[r], limits[r], seeds[r], greedy)
                        arrive[r] = len(steps_at) - 1
                        ops.append((m.SUBMIT,))
                    at = N_REQUESTS if rate == 0 else min(at + rate, N_REQUESTS)
                    events = s.poll(1)
                    ops.append((m.POLL, 1))
                    st = s.stats()
                    steps_at.append(st["stats"]["steps"])
                    for e in events:
                        if e["kind"] == "finished":
                            assert len(e["ids"]) == limits[e["id"]]
                            done[e["id"]], admit[e["id"]] = len(steps_at) - 1, e["admit_step"]
                stats = s.stats()["stats"]
            first = {r: 1 + max(t for t, n in enumerate(steps_at) if n <= admit[r]) for r in admit}
            return stats, arrive, first, done, ops

        for columns in [int(v) for v in a.columns.split(",")]:
            out = {}
            if "upfront" in want:
                out["upfront"] = r = timed_in_turn({"session": lambda: dict(groups=session(columns, 0)[0]["groups"]), "closed": lambda: dict(groups=closed(columns, range(N_REQUESTS))["groups"])},
                                                   a.reps, a.warmup)
                r["closed/session"] = round(r["closed"]["ms"] / r["session"]["ms"], 4)
            if "stream" in want:
                out["stream"] = r = timed_in_turn({"plain": lambda: dict(groups=session(columns, 0)[0]["groups"]), "stream": lambda: dict(groups=session(columns, 0, True)[0]["groups"])},
                                                  a.reps, a.warmup)
                r["us_per_look"] = round((r["stream"]["ms"] - r["plain"]["ms"]) * 1e3 / r["plain"]["groups"], 2)
            if "arrivals" in want:
                k = a.rate
                # the session's counts, from one run, checked against the planner
                stats, arrive, first, done, ops = session(columns, k)
                plan = m.queue_plan_script(ops, limits, limits, columns, GROUP)
                assert plan["stats"] == dict(stats, prompt_columns=0) and [done[r] for r in range(N_REQUESTS)] == plan["finish_group"]
                ses = dict(first_token=spread([first[r] - arrive[r] for r in range(N_REQUESTS)]), completion=spread([done[r] - arrive[r] for r in range(N_REQUESTS)]),
                           groups=stats["groups"])
                # the batches', from the planner: a batch of `columns` requests is one closed call with a column for each
                tick, b_first, b_done = 0, [], []
                for b0 in range(0, N_REQUESTS, columns):
                    idx = list(range(b0, min(b0 + columns, N_REQUESTS)))
                    p = m.queue_plan_script([(m.SUBMIT,)] * len(idx) + [(m.POLL, 1 << 20)], [limits[r] for r in idx], [limits[r] for r in idx], columns, GROUP)
                    start = max(tick, idx[-1] // k)
                    b_first += [start + 1 - r // k for r in idx]
                    b_done += [start + p["finish_group"][i] - r // k for i, r in enumerate(idx)]
                    tick = start + p["stats"]["groups"]
                bat = dict(first_token=spread(b_first), completion=spread(b_done), groups=tick)

                def batches():
                    for b0 in range(0, N_REQUESTS, columns):
                        closed(columns, range(b0, min(b0 + columns, N_REQUESTS)))
                    return bat

                out["arrivals"] = r = timed_in_turn({"session": lambda: (session(columns, k), ses)[1], "batches": batches}, a.reps, a.warmup)
                r["batches/session"] = round(r["batches"]["ms"] / r["session"]["ms"], 4)
            for name, r in out.items():
                print("max_columns %d %s: %s" % (columns, name, json.dumps(r)), file=sys.stderr, flush=True)
            res["columns_%d" % columns] = out
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
