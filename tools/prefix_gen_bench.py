#!/usr/bin/env python3
"""Generation behind a shared prefix on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): generate_greedy_batch / generate_sample with
prefix= against the same calls on the concatenations, which give the same ids.  Milliseconds per call by host wall clock (every call returns after its
stream has drained), warm-up 2, median of 9, spread = (max - min) / median; the two routes alternate call by call in one process, so both see the same
clocks and the same cache state of the other.  64 new tokens, n_batch 8.

  greedy   prefix 64 / 384 / 896 tokens x 16-token suffixes, 1 / 8 / 16 / 64 / 256 columns
  sample   8 / 64 samples of the prefix alone (one empty suffix)

One JSON line per case: the medians and spreads of both routes, ratio = prefix / concatenation, the call's prefix_stats() and the prompt columns of
the concatenation route.  The yardstick calls are unchanged on the parent commit.

  python tools/prefix_gen_bench.py [--reps 9] [--warmup 2] [--prefix 64,384,896] [--cols 1,8,16,64,256] [--samples 8,64]
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
N_SUFFIX, N_PREDICT = 16, 64


def timed_pair(fa, fb, reps, warmup):
    """fa and fb alternating: warm-up calls of both, then reps timed calls of each."""
    ta, tb = [], []
    for r in range(warmup + reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
    return ta, tb


def stats(ts):
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "spread": round((max(ts) - min(ts)) / med, 4)}


def ints(s):
    return [int(v) for v in s.split(",") if v]


def kernel_level(m, reps):
    """The decode attention launch alone through biogpt_hip_attn_prefix_bench: the existing attn_fast_kernel<4, false, true> against attn_prefix_kernel<8>, 16 heads,
    one layer.  A repeated stand-alone launch keeps its K / V rows in cache: these figures say what the kernels do with cached rows, not what a decode step
    of 24 layers pays for them."""
    Hh = 16
    rng = np.random.default_rng(1)
    for n_sh in (64, 256, 384, 896):
        for own in (8, 64):
            T = n_sh + own
            P = t_cap = (T + 63) // 64 * 64
            for N in (8, 16, 48, 64, 256):
                q = rng.standard_normal((N, Hh * 64)).astype(np.float32)
                blk = rng.standard_normal((Hh, P, 64)).astype(np.float32)
                k = np.ascontiguousarray(np.broadcast_to(blk, (N + 1, Hh, P, 64)))
                v = np.ascontiguousarray(k[:, :, ::-1])
                st = np.zeros((N, 8), dtype=np.int32)
                st[:, 0] = T - 1; st[:, 3] = np.arange(N); st[:, 5] = n_sh; st[:, 6] = N
                out = np.zeros((N, Hh * 64), dtype=np.float32)
                oq = np.zeros((N, Hh * 64), dtype=np.int8); od = np.zeros((N, Hh * 2), dtype=np.float32); osum = np.zeros((N, Hh * 2), dtype=np.uint32)
                res = {"mode": "kernel", "columns": N, "shared_rows": n_sh, "own_rows": own}
                for which, name in ((0, "fast_shared"), (1, "prefix_grouped")):
                    us = np.zeros(reps, dtype=np.float32)
                    rc = m.lib().biogpt_hip_attn_prefix_bench(0, Hh, N, P, t_cap, q.ctypes.data, k.ctypes.data, v.ctypes.data, st.ctypes.data, which, 1, out.ctypes.data,
                                                              oq.ctypes.data, od.ctypes.data, osum.ctypes.data, reps, us.ctypes.data)
                    assert rc == 0, m._err()
                    us = us[2:]
                    res[name + "_us"] = {"median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}
                res["ratio"] = round(res["prefix_grouped_us"]["median"] / res["fast_shared_us"]["median"], 3)
                print(json.dumps(res), flush=True)


def ab_level(m, path, a):
    """The prefix call with the grouped attention kernel never / always taken for its in-place steps: one context per arm (the switch is read when a
    model is loaded), the two alternating call by call."""
    arms = []
    for val in ("0", "1"):
        os.environ["BIOGPT_HIP_PREFIX_ATTN"] = val
        arms.append(m.BiogptModel.load(path, device=0))
    del os.environ["BIOGPT_HIP_PREFIX_ATTN"]
    V = arms[0].hparams.n_vocab
    for n_prefix in a.prefix:
        rng = np.random.default_rng(n_prefix)
        prefix = [2] + [int(v) for v in rng.integers(4, V, n_prefix - 1)]
        for cols in [c for c in a.cols if c >= 9]:
            suffixes = [[int(v) for v in rng.integers(4, V, N_SUFFIX)] for _ in range(cols)]
            ids = [g.generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix)[0] for g in arms]
            assert (ids[0] == ids[1]).all(), "the two attention kernels give different ids"
            t0, t1 = timed_pair(lambda: arms[0].generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix),
                                lambda: arms[1].generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix), a.reps, a.warmup)
            out = {"mode": "ab", "n_prefix": n_prefix, "columns": cols, "fast_shared": stats(t0), "prefix_grouped": stats(t1)}
            out["ratio"] = round(out["prefix_grouped"]["median_ms"] / out["fast_shared"]["median_ms"], 4)
            print(json.dumps(out), flush=True)
    for g in arms:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prefix", type=ints, default=[64, 384, 896])
    ap.add_argument("--cols", type=ints, default=[1, 8, 16, 64, 256])
    ap.add_argument("--samples", type=ints, default=[8, 64])
    ap.add_argument("--kernel", action="store_true", help="the kernel-level grid only")
    ap.add_argument("--ab", action="store_true", help="call level: BIOGPT_HIP_PREFIX_ATTN=0 against =1 (two contexts, alternating), greedy, 9 columns or more")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    if a.kernel:
        kernel_level(m, a.reps + 2)
        return
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED, **{k: v for k, v in m.BIOGPT_BASE.items() if k != "ftype"})
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        if a.ab:
            ab_level(m, q40, a)
            return
        g = m.BiogptModel.load(q40, device=0)
        V = g.hparams.n_vocab
        for n_prefix in a.prefix:
            rng = np.random.default_rng(n_prefix)
            prefix = [2] + [int(v) for v in rng.integers(4, V, n_prefix - 1)]
            for cols in a.cols:
                suffixes = [[int(v) for v in rng.integers(4, V, N_SUFFIX)] for _ in range(cols)]
                whole = [prefix + s for s in suffixes]
                got, _ = g.generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix)
                st = g.prefix_stats()
                want, _ = g.generate_greedy_batch(whole, N_PREDICT)
                assert (got == want).all(), "ids differ from those of the concatenations"
                tp, tc = timed_pair(lambda: g.generate_greedy_batch(suffixes, N_PREDICT, prefix=prefix), lambda: g.generate_greedy_batch(whole, N_PREDICT), a.reps, a.warmup)
                out = {"mode": "greedy", "n_prefix": n_prefix, "n_suffix": N_SUFFIX, "columns": cols, "n_predict": N_PREDICT, "stats": st,
                       "concat_prompt_columns": cols * (n_prefix + N_SUFFIX), "prefix": stats(tp), "concat": stats(tc)}
                out["ratio"] = round(out["prefix"]["median_ms"] / out["concat"]["median_ms"], 4)
                print(json.dumps(out), flush=True)
            for n_samples in a.samples:
                kw = dict(n_samples=n_samples, seed=7)
                got, _ = g.generate_sample([[]], N_PREDICT, prefix=prefix, **kw)
                st = g.prefix_stats()
                want, _ = g.generate_sample([prefix], N_PREDICT, **kw)
                assert len(got) == len(want) and all((x == y).all() for x, y in zip(got, want)), "ids differ from those of the concatenation"
                tp, tc = timed_pair(lambda: g.generate_sample([[]], N_PREDICT, prefix=prefix, **kw), lambda: g.generate_sample([prefix], N_PREDICT, **kw), a.reps, a.warmup)
                out = {"mode": "sample", "n_prefix": n_prefix, "n_suffix": 0, "columns": n_samples, "n_predict": N_PREDICT, "stats": st,
                       "concat_prompt_columns": n_prefix, "prefix": stats(tp), "concat": stats(tc)}
                out["ratio"] = round(out["prefix"]["median_ms"] / out["concat"]["median_ms"], 4)
                print(json.dumps(out), flush=True)
        g.close()


if __name__ == "__main__":
    main()
