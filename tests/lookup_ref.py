"""Host restatement of prompt-lookup decoding (csrc/kernels_lookup.hip.h): the draft rule, the packed column states, the acceptance, and a simulator of a
whole call.  Acceptance depends only on the draft and the true greedy ids, so the simulator needs no model."""
import numpy as np


def draft(text, max_ngram, max_draft, room):
    """The draft for a sequence whose text (corpus ++ prompt ++ generated) is `text`: for n = max_ngram .. 1 the smallest i in [0, L - n - 1] with
    text[i : i + n] == text[L - n :]; the first n with a match wins.  room = n_predict - n_gen - 1.  Returns (draft ids, n, i); no match: ([], 0, -1)."""
    T = np.asarray(text, dtype=np.int64)
    L = T.size
    if max_draft <= 0 or room <= 0:
        return [], 0, -1
    for n in range(min(max_ngram, L - 1), 0, -1):
        win = np.lib.stride_tricks.sliding_window_view(T[:L - 1], n)      # rows i = 0 .. L - n - 1
        hit = (win == T[L - n:]).all(axis=1)
        if hit.any():
            i = int(hit.argmax())
            d = max(0, min(max_draft, L - (i + n), room))
            return [int(v) for v in T[i + n:i + n + d]], n, i
    return [], 0, -1


def column_states(token, n_past, seq_id, drafted, max_draft):
    """The 1 + max_draft packed column states [token, n_past, seq_id, t_vis] of a sequence: its token, its draft, then copies of column 0."""
    col0 = [int(token), int(n_past), int(seq_id), int(n_past) + 1]
    out = [col0]
    for j, t in enumerate(drafted):
        out.append([int(t), n_past + 1 + j, int(seq_id), n_past + 2 + j])
    while len(out) < 1 + max_draft:
        out.append(list(col0))
    return np.asarray(out, dtype=np.int32)


def argmax_low(row):
    """arg-max with the lowest id on ties (np.argmax's rule, argmax_rows_kernel's)"""
    return int(np.argmax(np.asarray(row)))


def accept(am, drafted, n_gen, n_past, n_predict, eos_id=-1):
    """One acceptance: am[j] is the arg-max of row j (only rows 0 .. m are looked at).  Returns (emitted ids, token, n_past, n_gen, finished, accepted):
    the longest m with drafted[j] == am[j] for j < m; am[0 .. m] appended, cut at n_predict and behind the first eos_id."""
    m = 0
    while m < len(drafted) and drafted[m] == am[m]:
        m += 1
    out = []
    fin = False
    for j in range(m + 1):
        if n_gen + len(out) >= n_predict:
            break
        out.append(int(am[j]))
        if eos_id >= 0 and out[-1] == eos_id:
            fin = True
            break
    fin = fin or n_gen + len(out) >= n_predict
    token = out[-1] if out else -1
    return out, token, n_past + len(out), n_gen + len(out), fin, max(len(out) - 1, 0)


def simulate(prompt, corpus, greedy_ids, max_draft, max_ngram, eos_id=-1):
    """A whole call for one sequence whose greedy continuation is greedy_ids (n_predict = len(greedy_ids)).  Returns (stats dict, [emitted ids of each pass])."""
    n_predict = len(greedy_ids)
    text = [int(t) for t in (corpus or [])] + [int(t) for t in prompt]
    n_gen, n_past = 0, len(prompt) - 1
    stats = dict(passes=0, drafted=0, accepted=0)
    passes = []
    fin = n_predict == 0
    while not fin:
        dr, _, _ = draft(text, max_ngram, max_draft, n_predict - n_gen - 1)
        am = greedy_ids[n_gen:n_gen + len(dr) + 1]      # row j's arg-max is only asked for while the drafts before it were right: then it is the greedy id
        out, _, n_past, n_gen2, fin, acc = accept(am, dr, n_gen, n_past, n_predict, eos_id)
        stats["passes"] += 1
        stats["drafted"] += len(dr)
        stats["accepted"] += acc
        text += out
        n_gen = n_gen2
        passes.append(out)
    return stats, passes
