#!/usr/bin/env python3
"""Queued generation with request parameters (generate_queue(params=)) on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per
run by host wall clock (every call returns after its stream has drained).  The workload of tools/queue_bench.py: 512 requests with 32-token prompts, no EOS,
n_batch 8, every request with its own n_predict (4 + an exponential of mean 38, cut at 128: the same draw as queue_bench.py).  The routes of one row run in
turn, round after round -- `--warmup` rounds thrown away, then `--reps` rounds (median, min, max) -- so a drift of the machine meets every route alike.
Every row runs the new call against unchanged routes of the same build.  Prints one JSON line with, per max_columns (64, 256):

  same       512 requests with identical parameters (top_k 1), no rules, no stop: `requests` = generate_queue(params=one entry) against `plain` =
             generate_queue(top_k=1).  What the form costs.
  rules      the same requests with repetition_penalty 1.2 and no_repeat_ngram_size 3 on all of them: `requests` against `chunks`, the only route there was:
             consecutive chunks of max_columns prompts through generate_sample(top_k=1, <rules>) with the chunk's largest n_predict, truncated on the host.
  mixed      four parameter sets x 128 requests (request r has set r % 4: greedy; top_k 40 / top_p 0.95 / temp 6; greedy with the rules above; the hot sampler
             with repetition_penalty 1.2): `requests` = one call with a list of params against `per_set` = one call per set, the sets without rules through
             generate_queue, those with rules through the chunked route.
  stop       the `same` requests, every second one with a stop sequence that fires within its first four tokens (a token of its own free run): `requests_stop`
             against `requests`, the same requests without it.
  and per row the ratio second route / first route (above 1: the first, the new call or the call with stop sequences, is faster); beside every time `busy`, the share of column steps that generated a token
  somebody asked for.

  python tools/queue_requests_bench.py [--reps 9] [--warmup 2] [--columns 64,256] [--rows same,rules,mixed,stop]
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
N_REQUESTS, N_PROMPT = 512, 32
LEN_SEED, LEN_MIN, LEN_MAX, LEN_SCALE = 20261019, 4, 128, 38.0
HOT = dict(top_k=40, top_p=0.95, temp=6.0)
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)
SETS = [dict(top_k=1), dict(HOT), dict(top_k=1, **RULES), dict(HOT, repetition_penalty=1.2)]


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


def has_rules(par):
    return any(k in par for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="same,rules,mixed,stop")
    ap.add_argument("--columns", default="64,256")
    a = ap.parse_args()
    want = a.rows.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    rng = np.random.default_rng(LEN_SEED)
    limits = [int(v) for v in np.clip(LEN_MIN + np.floor(rng.exponential(LEN_SCALE, N_REQUESTS)), LEN_MIN, LEN_MAX)]
    res = {"metric": "queue_requests_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_requests": N_REQUESTS, "n_prompt": N_PROMPT, "n_batch": 8,
           "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "rows": want,
           "n_predicts": dict(mean=round(float(np.mean(limits)), 2), min=min(limits), max=max(limits), sum=sum(limits))}
    prng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in prng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(N_REQUESTS)]
        seeds = [1 + r for r in range(N_REQUESTS)]
        everyone = list(range(N_REQUESTS))

        def busy_of(info):
            return info["stats"]["busy_column_steps"] / info["stats"]["column_steps"]

        def plain(columns, idx, par):
            ids, info, _ = g.generate_queue([prompts[r] for r in idx], max(limits), max_columns=columns, seeds=[seeds[r] for r in idx], eos_id=-1, n_batch=8,
                                            n_predicts=[limits[r] for r in idx], **par)
            assert [len(i) for i in ids] == [limits[r] for r in idx]
            return ids, info["stats"]

        def requests(columns, idx, pars, lens=None):
            ids, info, _ = g.generate_queue([prompts[r] for r in idx], max(limits), max_columns=columns, seeds=[seeds[r] for r in idx], n_batch=8,
                                            n_predicts=[limits[r] for r in idx], params=pars)
            assert [len(i) for i in ids] == (lens if lens is not None else [limits[r] for r in idx])
            return ids, info["stats"]

        def chunked(columns, idx, par):
            """(tokens somebody asked for, column steps) of the chunked route"""
            used = 0
            for at in range(0, len(idx), columns):
                part = idx[at:at + columns]
                n = max(limits[r] for r in part)
                ids, _ = g.generate_sample([prompts[r] for r in part], n, seeds=[seeds[r] for r in part], eos_id=-1, n_batch=8, **par)
                cut = [ids[j][:limits[r]] for j, r in enumerate(part)]
                assert all(len(c) == limits[r] for c, r in zip(cut, part))
                used += len(part) * n
            return sum(limits[r] for r in idx), used

        def share(stats):
            return stats["busy_column_steps"] / stats["column_steps"]

        def per_set(columns):
            asked = steps = 0
            for k, par in enumerate(SETS):
                idx = everyone[k::4]
                if has_rules(par):
                    t, s = chunked(columns, idx, par)
                else:
                    st = plain(columns, idx, par)[1]
                    t, s = st["busy_column_steps"], st["column_steps"]
                asked, steps = asked + t, steps + s
            return asked / steps

        greedy = m.request_params(top_k=1)
        ruled = m.request_params(top_k=1, **RULES)
        mixed = [m.request_params(**SETS[r % 4]) for r in everyone]
        free = plain(256, everyone, dict(top_k=1))[0]
        stops = [m.request_params(top_k=1, stop=[[int(free[r][min(3, limits[r] - 1)])]]) if r % 2 else greedy for r in everyone]
        stop_lens = [min(limits[r], 1 + [int(t) for t in free[r]].index(int(free[r][min(3, limits[r] - 1)]))) if r % 2 else limits[r] for r in everyone]
        res["stop_lens_sum"] = sum(stop_lens)

        for columns in [int(v) for v in a.columns.split(",")]:
            out = {}
            rows = {
                "same": {"requests": lambda: share(requests(columns, everyone, greedy)[1]), "plain": lambda: share(plain(columns, everyone, dict(top_k=1))[1])},
                "rules": {"requests": lambda: share(requests(columns, everyone, ruled)[1]),
                          "chunks": lambda: (lambda t, s: t / s)(*chunked(columns, everyone, dict(top_k=1, **RULES)))},
                "mixed": {"requests": lambda: share(requests(columns, everyone, mixed)[1]), "per_set": lambda: per_set(columns)},
                "stop": {"requests_stop": lambda: share(requests(columns, everyone, stops, stop_lens)[1]), "requests": lambda: share(requests(columns, everyone, greedy)[1])},
            }
            for name in want:
                r = timed_in_turn(rows[name], a.reps, a.warmup)
                first, other = list(rows[name])
                r["%s/%s" % (other, first)] = round(r[other]["ms"] / r[first]["ms"], 4)
                out[name] = r
                print("max_columns %d %s: %s" % (columns, name, json.dumps(r)), file=sys.stderr, flush=True)
            res["columns_%d" % columns] = out
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
