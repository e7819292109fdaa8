"""The host restatement of prompt-lookup decoding (tests/lookup_ref.py) against a brute-force statement of the draft rule, on random texts over a 4-symbol
alphabet (many matches, several n, ties on i), and its edges; the simulator's bookkeeping.  No GPU."""
import numpy as np
import pytest

import lookup_ref


def draft_brute(text, max_ngram, max_draft, room):
    """the rule as the three loops of its definition"""
    L = len(text)
    if max_draft <= 0 or room <= 0:
        return [], 0, -1
    for n in range(max_ngram, 0, -1):
        for i in range(0, L - n):                   # i in [0, L - n - 1]
            same = True
            for k in range(n):
                if text[i + k] != text[L - n + k]:
                    same = False
                    break
            if same:
                d = min(max_draft, L - (i + n), room)
                return [int(t) for t in text[i + n:i + n + d]], n, i
    return [], 0, -1


@pytest.mark.parametrize("seed", range(8))
def test_draft_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    seen_n, ties, short, none = set(), 0, 0, 0
    for _ in range(300):
        L = int(rng.integers(1, 40))
        text = [int(v) for v in rng.integers(0, 4, L)]
        max_ngram, max_draft, room = int(rng.integers(1, 9)), int(rng.integers(0, 16)), int(rng.integers(0, 20))
        got = lookup_ref.draft(text, max_ngram, max_draft, room)
        want = draft_brute(text, max_ngram, max_draft, room)
        assert got == want, (text, max_ngram, max_draft, room)
        dr, n, i = got
        seen_n.add(n)
        if n > 0:
            later = [j for j in range(i + 1, L - n) if text[j:j + n] == text[L - n:]]
            ties += 1 if later else 0
            short += 1 if len(dr) < min(max_draft, room) else 0
            assert dr == text[i + n:i + n + len(dr)] and len(dr) >= 1
        else:
            none += 1
    assert {1, 2, 3} <= seen_n and ties > 20 and short > 5 and none > 5, (seen_n, ties, short, none)


def test_draft_edges():
    d = lookup_ref.draft
    assert d([5, 6, 7, 8], 3, 7, 10) == ([], 0, -1)                          # no match
    assert d([9], 3, 7, 10) == ([], 0, -1)                                   # a text of one token
    assert d([1, 2, 3, 9, 4, 3], 3, 7, 10) == ([9, 4, 3], 1, 2)              # a match only at n = 1; the continuation runs to the end of the text
    assert d([1, 2, 3, 1, 2], 3, 7, 10) == ([3, 1, 2], 2, 0)                 # a continuation shorter than max_draft
    assert d([1, 2, 3, 1, 2], 3, 2, 10) == ([3, 1], 2, 0)                    # max_draft cuts it
    assert d([1, 2, 3, 1, 2], 3, 7, 0) == ([], 0, -1)                        # n_predict - n_gen - 1 = 0: nothing may be drafted
    assert d([1, 2, 3, 1, 2], 3, 7, 1) == ([3], 2, 0)                        # ... = 1
    assert d([1, 2, 3, 1, 2], 3, 0, 5) == ([], 0, -1)                        # max_draft = 0
    assert d([7, 7, 7, 7], 2, 7, 10) == ([7, 7], 2, 0)                       # ties on i: the smallest, which has the longest continuation
    assert d([1, 2, 0, 2, 5, 1, 2], 1, 7, 10) == ([0, 2, 5, 1, 2], 1, 1)     # max_ngram = 1 ignores the longer match at 0
    assert d([1, 2, 0, 2, 5, 1, 2], 8, 7, 10) == ([0, 2, 5, 1, 2], 2, 0)     # max_ngram longer than the text


def test_column_states():
    c = lookup_ref.column_states(11, 40, 3, [12, 13], 4)
    assert c.tolist() == [[11, 40, 3, 41], [12, 41, 3, 42], [13, 42, 3, 43], [11, 40, 3, 41], [11, 40, 3, 41]]
    assert lookup_ref.column_states(11, 0, 0, [], 0).tolist() == [[11, 0, 0, 1]]


def test_accept_cases():
    a = lookup_ref.accept
    assert a([4, 5, 6, 7], [4, 5, 6], 2, 10, 20) == ([4, 5, 6, 7], 7, 14, 6, False, 3)        # all drafts right: one more token than drafted
    assert a([9, 5, 6, 7], [4, 5, 6], 2, 10, 20) == ([9], 9, 11, 3, False, 0)                 # first draft wrong
    assert a([4, 5, 1, 7], [4, 5, 6], 2, 10, 20) == ([4, 5, 1], 1, 13, 5, False, 2)           # wrong in the middle
    assert a([4], [], 2, 10, 20) == ([4], 4, 11, 3, False, 0)                                 # d = 0
    assert a([4, 5, 6, 7], [4, 5, 6], 2, 10, 20, eos_id=5) == ([4, 5], 5, 12, 4, True, 1)     # EOS inside the accepted run
    assert a([4, 5, 6, 7], [4, 5, 6], 17, 10, 20) == ([4, 5, 6], 6, 13, 20, True, 2)          # n_predict reached inside the run
    assert a([4, 5], [4], 18, 10, 20) == ([4, 5], 5, 12, 20, True, 1)                         # ... exactly at its end


@pytest.mark.parametrize("seed", range(4))
def test_simulator_bookkeeping(seed):
    rng = np.random.default_rng(100 + seed)
    prompt = [int(v) for v in rng.integers(0, 4, 12)]
    greedy = [int(v) for v in rng.integers(0, 4, 30)]
    for corpus in ([], greedy, greedy[5:20]):
        for md, mn in ((1, 1), (7, 3), (15, 8)):
            st, passes = lookup_ref.simulate(prompt, corpus, greedy, md, mn)
            assert sum(passes, []) == greedy
            assert st["passes"] == len(passes) and st["passes"] + st["accepted"] == len(greedy) and st["accepted"] <= st["drafted"]
            assert all(1 <= len(p) <= 1 + md for p in passes)
    st, passes = lookup_ref.simulate(prompt, [], greedy, 0, 3)
    assert st == dict(passes=30, drafted=0, accepted=0)
    eos = greedy[7]
    st, passes = lookup_ref.simulate(prompt, greedy, greedy, 7, 3, eos_id=eos)
    out = sum(passes, [])
    assert out == greedy[:greedy.index(eos) + 1] and st["passes"] + st["accepted"] == len(out)


def test_own_continuation_as_corpus_halves_the_passes():
    """corpus = the continuation itself: once the tail n-gram is unique in it, every pass copies max_draft tokens"""
    prompt = [2, 50, 51, 52]
    greedy = list(range(100, 148))
    st, _ = lookup_ref.simulate(prompt, greedy, greedy, 7, 3)
    assert st["passes"] <= 48 // 2 and st["passes"] + st["accepted"] == 48
