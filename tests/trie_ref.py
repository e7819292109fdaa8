"""Scalar restatement of trie-constrained generation (include/biogpt_hip.h, biogpt_hip_trie; INTEGRATION.md, "Constrained decoding"): transformers'
PrefixConstrainedLogitsProcessor over a trie of token sequences, in plain Python -- pinned to transformers on the CPU (test_trie_restatement.py),
then the engine is held to it (test_trie_capi.py, test_gpu_trie.py).

    Let g be the tokens generated so far (the prompt excluded).  Walk g from the root.  If the walk ends at node u, the allowed set is the tokens of
    u's edges, and eos where an entry ends at u; if it leaves the trie, the allowed set is {eos}.  The masked row is the row's value at the allowed
    ids and -inf elsewhere.

Not a test module: a helper the tests import."""
import numpy as np

import beam_ref
import sample_ref
from oracle import sampler


class RefTrie:
    def __init__(self, seqs):
        self.root = {"end": False, "next": {}}
        self.entries = set()
        for q in seqs:
            q = tuple(int(t) for t in q)
            assert len(q) >= 1
            self.entries.add(q)
            node = self.root
            for t in q:
                node = node["next"].setdefault(t, {"end": False, "next": {}})
            node["end"] = True

    def node(self, gen):
        node = self.root
        for t in gen:
            node = node["next"].get(int(t))
            if node is None:
                return None
        return node

    def allowed(self, gen, eos):
        """The allowed ids after the generated tokens `gen`, ascending."""
        node = self.node(gen)
        if node is None:
            return [int(eos)]
        return sorted(set(node["next"]) | ({int(eos)} if node["end"] else set()))

    def mask(self, row, gen, eos):
        """The masked copy of `row` (float32 [n_vocab]): scores + mask of PrefixConstrainedLogitsProcessor."""
        r = np.asarray(row, dtype=np.float32)
        out = np.full_like(r, -np.inf)
        ids = self.allowed(gen, eos)
        out[ids] = r[ids]
        return out

    def info(self):
        nodes, edges, depth, fan = 0, 0, 0, 0
        level = [self.root]
        d = 0
        while level:
            nodes += len(level)
            depth = d
            nxt = []
            for n in level:
                edges += len(n["next"])
                fan = max(fan, len(n["next"]))
                nxt.extend(n["next"].values())
            level = nxt
            d += 1
        return dict(entries=len(self.entries), nodes=nodes, edges=edges, max_depth=depth, max_fanout=fan)


# ---- tries that cover the shapes a build and a walk can go wrong on (shared by the C-ABI and the GPU tests) ----

def shape_tries(V, seed=11):
    """{name: entries} over a vocabulary of V >= 33 tokens: duplicates, an entry that is a prefix of another, fan-out 1 / 255 / 256 / 257 / 4097 (as far as
    V holds them: one probe round, its boundary, two rounds), depth 1 and 63, tokens 0 and V - 1 (in "dup_prefix" alone).  unused_token() gives an EOS id."""
    rng = np.random.default_rng([seed, V])
    out = {}
    out["dup_prefix"] = [[3, 4, 5], [3, 4], [3, 4, 5], [3, 9], [0], [V - 1, 0, V - 1], [3, 4, 5, 6, 7]]
    inner = np.arange(1, V - 1)      # (0 and V - 1 stay free in the tries below: they serve as EOS ids there)
    out["depth1"] = [[int(t)] for t in rng.choice(inner, min(inner.size, 20), replace=False)]
    deep = [int(t) for t in rng.choice(inner, 63)]
    out["depth63"] = [deep, deep[:40], deep[:62] + [1 + deep[62] % (V - 2)], [deep[0]]]
    for fan in (1, 255, 256, 257, 4097):
        if fan + 3 > V:
            continue
        toks = sorted(int(t) for t in rng.choice(inner, fan, replace=False))
        # fan edges at the root, and again below the root's middle edge (a node that is not the first of the arrays)
        mid = toks[len(toks) // 2]
        out["fan%d" % fan] = [[t, 1 + (t % 7)] for t in toks if t != mid] + [[mid, t] for t in toks] + [[mid]]
    return out


def unused_token(entries, V, which):
    """An id that occurs in no entry: which = "first" (0 where it is free), "last" (V - 1 where it is free) or "mid"."""
    used = set(int(t) for e in entries for t in e)
    order = {"first": range(V), "last": range(V - 1, -1, -1), "mid": list(range(V // 2, V)) + list(range(V // 2))}[which]
    return next(t for t in order if t not in used)


def probe_histories(entries, V, rng, n=12):
    """Histories for a trie of `entries`: empty, inside the trie, at a leaf, at an inner node where an entry ends, leaving the trie at the first and at the
    last token, behind a leaf -- and the first and last edge of every wide node."""
    t = RefTrie(entries)
    es = sorted(t.entries)
    hs = [[]]
    picks = [es[int(i)] for i in rng.choice(len(es), min(n, len(es)), replace=False)] + [max(es, key=len), es[0], es[-1]]
    for e in picks:
        e = list(e)
        hs.append(e)                                   # an entry's end: a leaf, or an inner node where an entry ends
        hs.append(e[:max(1, len(e) // 2)])             # inside
        hs.append(e[:-1] + [(e[-1] + 1) % V])          # leaves (or not) at the last token
        hs.append([(e[0] + 1) % V] + e[1:])            # ... at the first
        hs.append(e + [e[-1]])                         # behind the end
    return hs


# ---- beam search over masked rows ----

def trie_logprobs(fn, trie, eos, record=None):
    """A beam_ref `logprobs` callback with the trie's mask on every row (transformers: log_probs = logits_processor(running sequences, log_probs), the
    log-softmax taken over the unmasked row).  record: a list that receives every step's masked rows."""
    def wrapped(prefixes):
        rows = np.asarray(fn(prefixes), dtype=np.float32)
        out = np.stack([trie.mask(rows[b], p, eos) for b, p in enumerate(prefixes)])
        if record is not None:
            record.append(out)
        return out
    return wrapped


def _gap(a, b):
    """|a - b|, None for two values at -inf: that tie is exact by construction and decides nothing a rounding could change."""
    a, b = float(a), float(b)
    if a == -np.inf and b == -np.inf:
        return None
    return abs(a - b)


def beam_search_trie(logprobs, trie, n_beams, n_predict, eos, length_penalty=1.0, early_stopping=True):
    """beam_ref's search over the masked rows.  Returns (hyps, margins): hyps as beam_ref.beam_search returns them (scores may be -inf); margins = per step
    the smallest gap of the step's decisions as beam_ref defines them, gaps between two values at -inf ignored (inf where nothing else was decided)."""
    B = int(n_beams)
    record, trace = [], []
    hyps, _, _ = beam_ref._search(trie_logprobs(logprobs, trie, eos, record), B, n_predict, eos, length_penalty, early_stopping, None, trace)
    run_scores, pool, heur, margins = [np.float32(0.0)], [], True, []
    for k, (rows, tr) in enumerate(zip(record, trace), 1):
        cand = tr["cand"]

        def hit(c):
            return c[2] == eos or k >= n_predict

        nonhit = [c for c in cand if not hit(c)]
        new_running = nonhit[:B]
        gaps = []
        if len(nonhit) >= B:      # the B-th running beam against the best candidate left out that does not stop
            sc = np.stack([(np.float32(s) + rows[b]).astype(np.float32) for b, s in enumerate(run_scores)])
            sc[:, eos] = -np.inf
            for c in new_running:
                sc[c[1], c[2]] = -np.inf      # (a kept candidate at -inf leaves a value at -inf: the gap to it is ignored either way)
            gaps.append(_gap(new_running[-1][0], sc.max()))
        if not (len(pool) == B and early_stopping) and heur:
            for c in cand[:B]:
                if not hit(c):
                    continue
                ns = beam_ref.normalize(c[0], k, length_penalty)
                pos = 0
                while pos < len(pool) and pool[pos] >= ns:
                    pos += 1
                if len(pool) == B:
                    gaps.append(_gap(ns, pool[-1]))
                if pos < B:
                    pool.insert(pos, ns)
                    del pool[B:]
        if heur and len(pool) == B and new_running:
            best = beam_ref.normalize(new_running[0][0], k, length_penalty)
            gaps.append(_gap(best, pool[-1]))
            heur = bool(best > pool[-1])
        gaps = [g for g in gaps if g is not None]
        margins.append(min(gaps) if gaps else float("inf"))
        run_scores = [c[0] for c in new_running]
    assert sorted(float(s) for _, s in hyps) == sorted(float(s) for s in pool)      # the replay above followed the search
    return hyps, margins


def finite(hyps):
    """The hypotheses a caller keeps: isfinite(score)."""
    return [(list(ids), s) for ids, s in hyps if np.isfinite(s)]


# ---- sampled / greedy generation over masked rows ----

def reference_loop_trie(oracle_model, prompt, n_batch, n_predict, top_k, top_p, temp, seed, trie, eos):
    """sample_ref.reference_loop with the trie's mask on the oracle's row in front of oracle.sampler.sample_top_k_top_p (a candidate at -inf weighs
    exp(-inf) = 0).  Returns (ids, the smallest sample_ref.decision_margin over the masked rows)."""
    rng = sample_ref.RecordingRng(sampler.Mt19937(seed))
    lg = None
    for at in range(0, len(prompt), n_batch):
        lg = oracle_model.eval(list(prompt[at:at + n_batch]), at)
    n_past, ids, margin = len(prompt), [], float("inf")
    n_predict = min(int(n_predict), oracle_model.n_positions - len(prompt))
    for k in range(n_predict):
        row = trie.mask(lg, ids, eos)
        before = len(rng.out)
        t = sampler.sample_top_k_top_p(row, top_k, top_p, temp, rng)
        margin = min(margin, sample_ref.decision_margin(row, top_k, top_p, temp, rng.out[before:]))
        ids.append(int(t))
        if t == eos:
            break
        if k + 1 < n_predict:
            lg = oracle_model.eval([t], n_past)
            n_past += 1
    return ids, margin
