#!/usr/bin/env python3
"""Queued generation behind a shared prefix on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per run by host wall clock
(every call returns after its stream has drained).  The workload of tools/queue_bench.py behind one few-shot block: 512 requests, each a 16-token suffix
behind the same 384-token prefix, top_k = 1, no EOS, n_batch 8; every request has its own n_predict (4 + an exponential of mean 38, cut at 128: mean about
40, range 4 .. 128, the same draw as queue_bench.py).  The routes of one column count run in turn, round after round -- `--warmup` rounds thrown away, then
`--reps` rounds (median, min, max) -- so a drift of the machine meets every route alike.  Prints one JSON line with, per max_columns (64, 256):

  prefix_queue     generate_queue(suffixes, prefix=prefix): the shared rows once, every refill its 8 + 16 own columns
  concat_queue     (a) what a caller had for the queue: generate_queue on the concatenations, 400 prompt columns per request
  prefix_chunks    (b) what a caller had for the prefix: consecutive chunks of max_columns suffixes through generate_sample(prefix=prefix, top_k=1), each
                       with its chunk's largest n_predict, truncated on the host
  prefix_queue_lp0 / prefix_queue_lp5   prefix_queue with logprobs=0 / logprobs=5
  concat_queue+score   (a), then the confidences the way a caller got them: score_batch of every concatenation ++ its ids, in chunks of max_columns
                       sequences (a sequence of a scoring call has a K / V cache of its own)
  and the ratios concat_queue / prefix_queue, prefix_chunks / prefix_queue, prefix_queue_lp0 / prefix_queue, prefix_queue_lp5 / prefix_queue,
  concat_queue+score / prefix_queue_lp0; beside every time `busy`, the share of column steps that generated a token somebody asked for.

  python tools/queue_prefix_bench.py [--reps 9] [--warmup 2] [--columns 64,256] [--routes prefix_queue,concat_queue,prefix_chunks,lp,score]

--routes concat_queue,prefix_chunks,score uses nothing this tool's commit added: the file runs unchanged in a checkout of the parent commit.
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
N_REQUESTS, N_SUFFIX, N_PREFIX = 512, 16, 384
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default="prefix_queue,concat_queue,prefix_chunks,lp,score")
    ap.add_argument("--columns", default="64,256")
    a = ap.parse_args()
    want = a.routes.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    rng = np.random.default_rng(LEN_SEED)
    limits = [int(v) for v in np.clip(LEN_MIN + np.floor(rng.exponential(LEN_SCALE, N_REQUESTS)), LEN_MIN, LEN_MAX)]
    res = {"metric": "queue_prefix_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_requests": N_REQUESTS, "n_prefix": N_PREFIX, "n_suffix": N_SUFFIX,
           "n_batch": 8, "top_k": 1, "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "routes": want,
           "n_predicts": dict(mean=round(float(np.mean(limits)), 2), min=min(limits), max=max(limits), sum=sum(limits))}
    prng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prefix = [2] + [int(v) for v in prng.integers(4, g.n_vocab, N_PREFIX - 1)]
        suffixes = [[int(v) for v in prng.integers(4, g.n_vocab, N_SUFFIX)] for _ in range(N_REQUESTS)]
        concats = [prefix + s for s in suffixes]
        last_ids = {}

        def queued(columns, prompts, **kw):
            ids, info, _ = g.generate_queue(prompts, max(limits), max_columns=columns, top_k=1, seed=1, eos_id=-1, n_batch=8, n_predicts=limits, **kw)
            assert [len(i) for i in ids] == limits
            if "logprobs" in kw:
                assert all(len(e[0]) == n for e, n in zip(info["logprobs"], limits))
            last_ids[0] = ids
            return info["stats"]["busy_column_steps"] / info["stats"]["column_steps"]

        def chunked(columns):
            used = 0
            for at in range(0, N_REQUESTS, columns):
                idx = list(range(at, min(at + columns, N_REQUESTS)))
                n = max(limits[r] for r in idx)
                ids, _ = g.generate_sample([suffixes[r] for r in idx], n, top_k=1, seed=1, eos_id=-1, n_batch=8, prefix=prefix)
                cut = [ids[j][:limits[r]] for j, r in enumerate(idx)]
                assert all(len(c) == limits[r] for c, r in zip(cut, idx))
                used += len(idx) * n
            return sum(limits) / used

        def queued_then_scored(columns):
            busy = queued(columns, concats)
            ids = last_ids[0]
            for at in range(0, N_REQUESTS, columns):
                idx = range(at, min(at + columns, N_REQUESTS))
                out = g.score_batch([concats[r] + [int(t) for t in ids[r]] for r in idx])
                assert len(out) == len(idx)
            return busy

        for columns in [int(v) for v in a.columns.split(",")]:
            table = {}
            if "prefix_queue" in want:
                table["prefix_queue"] = lambda: queued(columns, suffixes, prefix=prefix)
            if "concat_queue" in want:
                table["concat_queue"] = lambda: queued(columns, concats)
            if "prefix_chunks" in want:
                table["prefix_chunks"] = lambda: chunked(columns)
            if "lp" in want:
                table["prefix_queue_lp0"] = lambda: queued(columns, suffixes, prefix=prefix, logprobs=0)
                table["prefix_queue_lp5"] = lambda: queued(columns, suffixes, prefix=prefix, logprobs=5)
            if "score" in want:
                table["concat_queue+score"] = lambda: queued_then_scored(columns)
            if not table:
                continue
            r = timed_in_turn(table, a.reps, a.warmup)
            for num, den in (("concat_queue", "prefix_queue"), ("prefix_chunks", "prefix_queue"), ("prefix_queue_lp0", "prefix_queue"),
                             ("prefix_queue_lp5", "prefix_queue"), ("concat_queue+score", "prefix_queue_lp0")):
                if num in r and den in r:
                    r["%s/%s" % (num, den)] = round(r[num]["ms"] / r[den]["ms"], 4)
            if "prefix_queue" in want:
                r["prefix_stats"] = (queued(columns, suffixes, prefix=prefix), g.prefix_stats())[1]
            res["columns_%d" % columns] = r
            print("max_columns %d: %s" % (columns, json.dumps(r)), file=sys.stderr, flush=True)
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
