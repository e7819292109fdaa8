#!/usr/bin/env python3
"""Generation over a queue on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per run by host wall clock (every call returns
after its stream has drained).  512 requests with 16-token prompts, top_k = 1, no EOS, n_batch 8; every request has its own n_predict, drawn once from a
fixed seed (4 + an exponential of mean 38, cut at 128: mean about 40, range 4 .. 128; the histogram is printed).  The routes of one column count run in
turn, round after round -- `--warmup` rounds thrown away, then `--reps` rounds (median, min, max) -- so a drift of the machine meets every route alike.
Prints one JSON line with, per max_columns (8, 64, 256):

  queue         (a) generate_queue(max_columns, group = the default)
  chunks        (b) what a caller does without it: consecutive chunks of max_columns prompts through generate_sample(top_k=1), each with its chunk's
                    largest n_predict, truncated on the host
  sorted        (c) route (b) with the requests sorted by n_predict first -- knowledge a caller only has without an EOS: the best a closed batch can do
  group_G       (d) route (a) with group = 1 / 2 / 4 / 8 / 16
  and the ratios chunks / queue, sorted / queue; beside every time `busy`, the share of column steps that generated a token somebody asked for
  (busy_column_steps / column_steps).

and a second case, `equal_64`: 64 requests of 64 tokens each at max_columns = 64 against ONE generate_sample call -- the queue's overhead where it has
nothing to gain.

  python tools/queue_bench.py [--reps 9] [--warmup 2] [--routes queue,chunks,sorted,groups,equal] [--columns 8,64,256] [--groups 1,2,4,8,16]

--routes chunks,sorted uses nothing this tool's commit added: the file runs unchanged in a checkout of the parent commit.
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
N_REQUESTS, N_PROMPT = 512, 16
LEN_SEED, LEN_MIN, LEN_MAX, LEN_SCALE = 20261019, 4, 128, 38.0


def summary(ts, busy):
    return dict(ms=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3), n=len(ts), busy=round(busy, 4))


def timed_in_turn(routes, reps, warmup):
    """{name: summary}: every round runs each route once, in the order given; a route returns its busy share."""
    ts, busy = {name: [] for name in routes}, {}
    for rd in range(warmup + reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            busy[name] = fn()
            if rd >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(v, busy[name]) for name, v in ts.items()}


def chunked(g, prompts, limits, order, columns):
    """Closed calls over consecutive chunks of `order`; returns the busy share (the ids are cut to each request's own length on the host)."""
    used = 0
    for at in range(0, len(order), columns):
        idx = order[at:at + columns]
        n = max(limits[r] for r in idx)
        ids, _ = g.generate_sample([prompts[r] for r in idx], n, top_k=1, seed=1, eos_id=-1, n_batch=8)
        cut = [ids[j][:limits[r]] for j, r in enumerate(idx)]
        assert all(len(c) == limits[r] for c, r in zip(cut, idx))
        used += len(idx) * n
    return sum(limits) / used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default="queue,chunks,sorted,groups,equal")
    ap.add_argument("--columns", default="8,64,256")
    ap.add_argument("--groups", default="1,2,4,8,16")
    a = ap.parse_args()
    want = a.routes.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    rng = np.random.default_rng(LEN_SEED)
    limits = [int(v) for v in np.clip(LEN_MIN + np.floor(rng.exponential(LEN_SCALE, N_REQUESTS)), LEN_MIN, LEN_MAX)]
    hist = np.histogram(limits, bins=[4, 8, 16, 32, 64, 96, 129])[0]
    res = {"metric": "queue_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_requests": N_REQUESTS, "n_prompt": N_PROMPT, "n_batch": 8, "top_k": 1,
           "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "routes": want,
           "n_predicts": dict(mean=round(float(np.mean(limits)), 2), min=min(limits), max=max(limits), sum=sum(limits),
                              histogram={"4-7": int(hist[0]), "8-15": int(hist[1]), "16-31": int(hist[2]), "32-63": int(hist[3]), "64-95": int(hist[4]), "96-128": int(hist[5])})}
    print("n_predicts: %s" % json.dumps(res["n_predicts"]), file=sys.stderr)
    prng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in prng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(N_REQUESTS)]
        in_order, by_length = list(range(N_REQUESTS)), sorted(range(N_REQUESTS), key=lambda r: limits[r])

        def queued(columns, group=None, ps=prompts, ls=limits):
            kw = {} if group is None else dict(group=group)
            ids, info, _ = g.generate_queue(ps, max(ls), max_columns=columns, top_k=1, seed=1, eos_id=-1, n_batch=8, n_predicts=ls, **kw)
            assert [len(i) for i in ids] == ls
            return info["stats"]["busy_column_steps"] / info["stats"]["column_steps"]

        for columns in [int(v) for v in a.columns.split(",")]:
            table = {}
            if "queue" in want:
                table["queue"] = lambda: queued(columns)
            if "chunks" in want:
                table["chunks"] = lambda: chunked(g, prompts, limits, in_order, columns)
            if "sorted" in want:
                table["sorted"] = lambda: chunked(g, prompts, limits, by_length, columns)
            if "groups" in want:
                for grp in [int(v) for v in a.groups.split(",")]:
                    table["group_%d" % grp] = lambda grp=grp: queued(columns, grp)
            if not table:
                continue
            r = timed_in_turn(table, a.reps, a.warmup)
            for num in ("chunks", "sorted"):
                if num in r and "queue" in r:
                    r["%s/queue" % num] = round(r[num]["ms"] / r["queue"]["ms"], 4)
            res["columns_%d" % columns] = r
            print("max_columns %d: %s" % (columns, json.dumps(r)), file=sys.stderr)
        if "equal" in want:
            ps, ls = prompts[:64], [64] * 64

            def closed():
                ids, _ = g.generate_sample(ps, 64, top_k=1, seed=1, eos_id=-1, n_batch=8)
                assert all(len(i) == 64 for i in ids)
                return 1.0

            r = timed_in_turn({"closed": closed, "queue": lambda: queued(64, None, ps, ls), "closed_again": closed}, a.reps, a.warmup)
            r["queue/closed"] = round(r["queue"]["ms"] / r["closed"]["ms"], 4)
            r["closed_again/closed"] = round(r["closed_again"]["ms"] / r["closed"]["ms"], 4)
            res["equal_64"] = r
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
