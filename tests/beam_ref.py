"""Scalar restatement of beam search as biogpt_hip_generate_beam defines it ("Beam search"): transformers'
GenerationMixin._beam_search for one prompt with do_sample=False, one EOS id or none, no logits processors, early_stopping True / False,
any length_penalty -- with its unspecified tie orders made explicit.  Driven by a callback, so that the same code can be pinned to
transformers on the CPU (test_beam_restatement.py) and then hold the engine to it (test_gpu_beam.py).

    logprobs(prefixes) -> float32 [len(prefixes)][n_vocab]: the log-softmax row after the prompt + each prefix of generated ids.

Not a test module: a helper the tests import."""
import numpy as np


def normalize(score, gen_len, length_penalty):
    """The engine's normalized score: (float)((double)score / pow((double)gen_len, (double)length_penalty))."""
    return np.float32(float(score) / (float(gen_len) ** float(length_penalty)))


def log_softmax_rows(rows):
    """The arithmetic of logprob_rows_kernel up to the order of the exponential sum: (l - m) - log(S) in double, rounded once to f32."""
    r = np.asarray(rows, dtype=np.float32)
    m = r.max(axis=-1, keepdims=True)
    s = np.exp((r - m).astype(np.float32)).astype(np.float64).sum(axis=-1, keepdims=True)
    return ((r.astype(np.float64) - m.astype(np.float64)) - np.log(s)).astype(np.float32)


def beam_search(logprobs, n_beams, n_predict, eos_id=-1, length_penalty=1.0, early_stopping=True):
    """Returns (hyps, margins): hyps = [(ids list, normalized score float32), ...] best first; margins = per step the smallest gap of
    the step's decisions (float, inf where a step decides nothing): between the n_beams-th running beam kept and the best candidate
    rejected, at the border of the finished pool, and at the early-stop comparison."""
    hyps, margins, _ = _search(logprobs, n_beams, n_predict, eos_id, length_penalty, early_stopping, None, None)
    return hyps, margins


def running_beams(logprobs, n_beams, n_predict, max_steps, eos_id=-1, length_penalty=1.0, early_stopping=True, trace=None):
    """The running beams after max_steps steps of beam_search (fewer if the search stops first), in rank order: [(ids list, float32 score), ...].
    trace: a list that receives one dict per step -- cand (the 2 * n_beams candidates (score, parent rank, id) in order), parents (the parent
    rank of each new running beam), evicted (hypotheses pushed out of a full pool), done."""
    return _search(logprobs, n_beams, n_predict, eos_id, length_penalty, early_stopping, max_steps, trace)[2]


def _leading(sc, n):
    """Flat indices into sc [rows][V] that hold every row's first n entries by (value descending, id ascending), and possibly more: all a step looks
    at (its 2B candidates and the first candidate left out are within the first 2B + 1 of the global order, so within these of their rows).  Sorting
    these instead of all rows x V values changes no result."""
    V = sc.shape[1]
    if V <= n:
        return np.arange(sc.size)
    keep = []
    for b in range(sc.shape[0]):
        nth = np.partition(sc[b], V - n)[V - n]      # the n-th largest value: ties with it stay in
        keep.append(b * V + np.nonzero(sc[b] >= nth)[0])
    return np.concatenate(keep)


def _search(logprobs, n_beams, n_predict, eos_id, length_penalty, early_stopping, max_steps, trace):
    B = int(n_beams)
    running = [([], np.float32(0.0))]      # step 1 expands beam 0 alone (the others start at -1e9)
    pool = []                              # [(normalized score, ids)], best first, earlier entries first on ties
    heur_unsat = True
    margins = []
    for k in range(1, n_predict + 1):      # k: generated tokens, this step's included
        rows = np.asarray(logprobs([r[0] for r in running]), dtype=np.float32)
        V = rows.shape[1]
        sc = np.stack([(np.float32(s) + rows[b]).astype(np.float32) for b, (_, s) in enumerate(running)])
        flat = sc.reshape(-1)
        lead = _leading(sc, 2 * B + 1)
        order = lead[np.lexsort((lead % V, lead // V, -flat[lead].astype(np.float64)))]     # score descending, parent rank, token id
        cand = [(flat[i], int(i // V), int(i % V)) for i in order[:2 * B]]

        def hit(c):
            return (eos_id >= 0 and c[2] == eos_id) or k >= n_predict

        gaps = []
        evicted = 0
        nonhit = [c for c in cand if not hit(c)]
        new_running = nonhit[:B]
        if len(nonhit) >= B:     # the B-th running beam against the best non-stopping candidate left out (over all B x V)
            kept = set((c[1], c[2]) for c in new_running)
            for i in order:
                c = (flat[i], int(i // V), int(i % V))
                if (c[1], c[2]) not in kept and not hit(c):
                    gaps.append(float(new_running[-1][0]) - float(c[0]))
                    break
        # the finished pool (_update_finished_beams)
        if not (len(pool) == B and early_stopping) and heur_unsat:
            for c in cand[:B]:
                if not hit(c):
                    continue
                ns = normalize(c[0], k, length_penalty)
                hyp = list(running[c[1]][0]) + [c[2]]
                pos = 0
                while pos < len(pool) and pool[pos][0] >= ns:
                    pos += 1
                if len(pool) == B:
                    gaps.append(abs(float(ns) - float(pool[-1][0])))
                if pos < B:
                    pool.insert(pos, (ns, hyp))
                    evicted += len(pool[B:])
                    del pool[B:]
        # _check_early_stop_heuristic: a full pool only
        if heur_unsat and len(pool) == B and new_running:
            best = normalize(new_running[0][0], k, length_penalty)
            gaps.append(abs(float(best) - float(pool[-1][0])))
            heur_unsat = bool(best > pool[-1][0])
        margins.append(min(gaps) if gaps else float("inf"))
        done = (not heur_unsat) or (len(pool) == B and early_stopping) or len(nonhit) < B or k >= n_predict
        running = [(list(running[c[1]][0]) + [c[2]], c[0]) for c in new_running]
        if trace is not None:
            trace.append(dict(cand=cand, parents=[c[1] for c in new_running], evicted=evicted, done=done))
        if done or (max_steps is not None and k >= max_steps):
            break
    return [(ids, s) for s, ids in pool], margins, running


class OracleLogprobs:
    """logprobs() from the CPU oracle in the engine's order: the prompt in chunks of n_batch (the reference's unmasked chunk), then each
    prefix of generated tokens one at a time from n_past = n_prompt.  Prompt rows stay put; a prefix is re-fed from where it leaves the
    one fed before it (rows of a common prefix are identical)."""

    def __init__(self, oracle_model, prompt, n_batch):
        self.o = oracle_model
        self.n_prompt = len(prompt)
        row = None
        for at in range(0, len(prompt), n_batch):
            row = self.o.eval(list(prompt[at:at + n_batch]), at)
        self.first = log_softmax_rows(row[None, :])[0]
        self.fed = []
        self.cache = {(): self.first}
        self.evals = 0

    def row(self, prefix):
        prefix = tuple(prefix)
        if prefix in self.cache:
            return self.cache[prefix]
        common = 0
        while common < min(len(self.fed), len(prefix)) and self.fed[common] == prefix[common]:
            common += 1
        if common == len(prefix):    # (a prefix of what was fed: its row is cached already)
            common -= 1
        self.fed = list(self.fed[:common])
        out = None
        for j in range(common, len(prefix)):
            out = self.o.eval([prefix[j]], self.n_prompt + j)
            self.fed.append(prefix[j])
            self.evals += 1
            self.cache[tuple(self.fed)] = log_softmax_rows(out[None, :])[0]
        return self.cache[prefix]

    def __call__(self, prefixes):
        return np.stack([self.row(p) for p in prefixes])
