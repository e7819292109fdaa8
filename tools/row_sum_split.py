"""Where the q/k/v (own rows of the head, <= 128 keys), fc1 and fc2 stages of the pipelined decode launch spend their time: block dots against in-order row sums.
usage: BIOGPT_HIP_DBG=128 BIOGPT_HIP_LIB=<build with -DBIOGPT_HIP_PROFILE_HOOKS> python tools/row_sum_split.py MODEL [n_past ...]
Reads the XP_WALL stamps of the last timed step and the XP_WALLX stamps ("block terms in LDS, the sums start") kernels_xpipe.hip.h leaves behind them."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import _pkg
m = _pkg.load()
g = m.BiogptModel.load(sys.argv[1])
nl = g.hparams.n_layer
# stage: (stamp before the dots, XP_WALLX index, stamp behind the sums)
stages = [("q/k/v  (LayerNorm + Q8 done -> rows stored)", 6, 0, 1), ("fc1    (LayerNorm + Q8 done -> rows + GELU done)", 10, 1, 11),
          ("fc1    (rows + GELU done -> activations published)", 11, None, 4), ("fc2    (fc1 activations arrived -> layer output published)", 12, 2, 5)]
for n_past in [int(a) for a in sys.argv[2:]] or [40, 103]:
    us = g.bench_decode(n_past, 30) * 1e6
    w = g.debug_stamps(0, nl * 16).reshape(nl, 16).astype(np.int64)[1:]
    x = g.debug_stamps(2048, nl * 8).reshape(nl, 8).astype(np.int64)[1:]
    print("n_past %d: %.1f us per token; us, mean over layers 1..%d" % (n_past, us, nl - 1))
    for name, a, k, b in stages:
        tot = float((w[:, b] - w[:, a]).mean()) * 0.01
        if k is None or not (x[:, k] > 0).all():
            print("   %-58s %5.2f" % (name, tot))
        else:
            print("   %-58s %5.2f = dots %5.2f + sums %5.2f" % (name, tot, float((x[:, k] - w[:, a]).mean()) * 0.01, float((w[:, b] - x[:, k]).mean()) * 0.01))
