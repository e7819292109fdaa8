"""The stop rule of queued generation with request parameters (tests/queue_requests_ref.py) against cases written out by hand.  The generated tokens are what
the closed call of the request alone returns; the prompt is never part of them, so a match cannot reach into it."""
from queue_requests_ref import stop_cut


def test_no_stop_sequence_is_the_closed_call():
    assert stop_cut([5, 6, 7], []) == ([5, 6, 7], 0)
    assert stop_cut([], [[5]]) == ([], 0)
    assert stop_cut([5, 6, 2], [], eos=2) == ([5, 6, 2], 1)


def test_a_match_at_the_last_token():
    assert stop_cut([5, 6, 7, 8], [[7, 8]]) == ([5, 6, 7, 8], 2)


def test_a_match_in_the_middle_cuts_behind_it():
    assert stop_cut([5, 6, 7, 8, 9], [[6, 7]]) == ([5, 6, 7], 2)
    assert stop_cut([5, 6, 7, 6, 7], [[9], [6, 7]]) == ([5, 6, 7], 3)


def test_a_match_that_would_need_a_prompt_token_is_no_match():
    # the prompt ended with 4: [4, 5] lies across the border and does not count; its second occurrence lies inside
    assert stop_cut([5, 6, 7], [[4, 5]]) == ([5, 6, 7], 0)
    assert stop_cut([5, 6, 4, 5, 9], [[4, 5]]) == ([5, 6, 4, 5], 2)
    # a sequence longer than everything generated so far
    assert stop_cut([5, 6], [[4, 5, 6]]) == ([5, 6], 0)


def test_one_stop_sequence_is_the_suffix_of_another():
    # both complete at the same token: the lower index is reported, whichever is the longer
    assert stop_cut([5, 6, 7, 8], [[6, 7], [7]]) == ([5, 6, 7], 2)
    assert stop_cut([5, 6, 7, 8], [[7], [6, 7]]) == ([5, 6, 7], 2)
    # the shorter completes alone where the longer's first token is missing
    assert stop_cut([5, 9, 7, 8], [[6, 7], [7]]) == ([5, 9, 7], 3)


def test_a_stop_of_length_one_equal_to_the_eos_id():
    # the EOS is checked first, as in the kernel
    assert stop_cut([5, 6, 2], [[2]], eos=2) == ([5, 6, 2], 1)
    assert stop_cut([5, 6, 2, 9], [[2]], eos=-1) == ([5, 6, 2], 2)


def test_a_limit_reached_on_the_matching_token():
    # the closed call stopped at its limit of 3 tokens; the stop sequence completes on that token and is what is reported
    assert stop_cut([5, 6, 7], [[6, 7]]) == ([5, 6, 7], 2)
    assert stop_cut([5, 6, 7], [[6, 8]]) == ([5, 6, 7], 0)
