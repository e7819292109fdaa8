#!/usr/bin/env python3
"""Beam search over a queue on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per run by host wall clock (every call returns
after its stream has drained).  510 requests with 16-token prompts, five beams, no EOS, n_batch 8; every request has its own n_predict, drawn once from a
fixed seed (tools/queue_bench.py's draw: 4 + an exponential of mean 38, cut at 128; the histogram is printed).  Without an EOS a search runs to its limit, so
the lengths of the searches are those limits.  The routes of one column count run in turn, round after round -- `--warmup` rounds thrown away, then
`--reps` rounds (median, min, max) -- so a drift of the machine meets every route alike.  Prints one JSON line with, per max_columns (40, 160, 510: 8, 32 and
102 slots):

  queue         (a) generate_beam_queue(max_columns, group = the default)
  chunks        (b) what a caller does without it: consecutive chunks of max_columns / 5 prompts through generate_beam_batch, each with its chunk's
                    largest n_predict
  the ratio chunks / queue; beside every time `busy`, the share of slot steps that some search asked for (busy_column_steps / column_steps)

and a second case, `equal_S`: S requests of 64 steps each on S slots against ONE generate_beam_batch call -- the cost of the looks at the header where the
queue has nothing to gain.

  python tools/beam_queue_bench.py [--reps 9] [--warmup 2] [--routes queue,chunks,equal] [--columns 40,160,510] [--equal-slots 32]

--routes chunks uses nothing this tool's commit added: the file runs unchanged in a checkout of the parent commit.
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
N_REQUESTS, N_PROMPT, N_BEAMS = 510, 16, 5
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


def chunked(g, prompts, limits, slots):
    """Closed calls over consecutive chunks of `slots` prompts; returns the busy share.  (A caller who needs request r's own result cannot cut a longer search
    short on the host as greedy ids are cut: they pay the chunk's steps and take what a search of that length found.)"""
    used = 0
    for at in range(0, len(prompts), slots):
        n = max(limits[at:at + slots])
        hyps, _ = g.generate_beam_batch(prompts[at:at + slots], n, n_beams=N_BEAMS, eos_id=-1, n_batch=8)
        assert all(len(h) == N_BEAMS for h in hyps)
        used += len(hyps) * n
    return sum(limits) / used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default="queue,chunks,equal")
    ap.add_argument("--columns", default="40,160,510")
    ap.add_argument("--equal-slots", type=int, default=32)
    a = ap.parse_args()
    want = a.routes.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    rng = np.random.default_rng(LEN_SEED)
    limits = [int(v) for v in np.clip(LEN_MIN + np.floor(rng.exponential(LEN_SCALE, N_REQUESTS)), LEN_MIN, LEN_MAX)]
    hist = np.histogram(limits, bins=[4, 8, 16, 32, 64, 96, 129])[0]
    res = {"metric": "beam_queue_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_requests": N_REQUESTS, "n_prompt": N_PROMPT, "n_beams": N_BEAMS,
           "n_batch": 8, "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "routes": want,
           "n_predicts": dict(mean=round(float(np.mean(limits)), 2), min=min(limits), max=max(limits), sum=sum(limits),
                              histogram={"4-7": int(hist[0]), "8-15": int(hist[1]), "16-31": int(hist[2]), "32-63": int(hist[3]), "64-95": int(hist[4]), "96-128": int(hist[5])})}
    print("n_predicts: %s" % json.dumps(res["n_predicts"]), file=sys.stderr, flush=True)
    prng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in prng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(N_REQUESTS)]

        def queued(columns, ps=prompts, ls=limits):
            hyps, info, _ = g.generate_beam_queue(ps, max(ls), n_beams=N_BEAMS, max_columns=columns, eos_id=-1, n_batch=8, n_predicts=ls)
            assert info["steps"] == ls and all(len(h) == N_BEAMS for h in hyps)
            return info["stats"]["busy_column_steps"] / info["stats"]["column_steps"]

        for columns in [int(v) for v in a.columns.split(",")]:
            table = {}
            if "queue" in want:
                table["queue"] = lambda: queued(columns)
            if "chunks" in want:
                table["chunks"] = lambda: chunked(g, prompts, limits, columns // N_BEAMS)
            if not table:
                continue
            r = timed_in_turn(table, a.reps, a.warmup)
            if "chunks" in r and "queue" in r:
                r["chunks/queue"] = round(r["chunks"]["ms"] / r["queue"]["ms"], 4)
            res["columns_%d" % columns] = r
            print("max_columns %d: %s" % (columns, json.dumps(r)), file=sys.stderr, flush=True)
        if "equal" in want:
            S = a.equal_slots
            ps, ls = prompts[:S], [64] * S

            def closed():
                hyps, _ = g.generate_beam_batch(ps, 64, n_beams=N_BEAMS, eos_id=-1, n_batch=8)
                assert all(len(h) == N_BEAMS for h in hyps)
                return 1.0

            r = timed_in_turn({"closed": closed, "queue": lambda: queued(S * N_BEAMS, ps, ls), "closed_again": closed}, a.reps, a.warmup)
            r["queue/closed"] = round(r["queue"]["ms"] / r["closed"]["ms"], 4)
            r["closed_again/closed"] = round(r["closed_again"]["ms"] / r["closed"]["ms"], 4)
            res["equal_%d" % S] = r
            print("equal_%d: %s" % (S, json.dumps(r)), file=sys.stderr, flush=True)
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
