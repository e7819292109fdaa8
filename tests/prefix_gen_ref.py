"""Host restatement of how a generation call behind a shared prefix lays out its prompt work (biogpt_hip_generate_greedy_prefix /
biogpt_hip_generate_sample_prefix): which prefix rows are shared, what every sequence still evaluates itself, how many prompt columns
that makes, and where the n_batch chunks of the reference's prompt loop fall.  No GPU, no package: plain integers."""


def n_shared(n_prefix, n_batch):
    """The largest multiple of n_batch that is <= n_prefix - 1: the shared rows end on a chunk border, and the last prefix token is never shared."""
    return (n_prefix - 1) // n_batch * n_batch


def effective_prompts(prefix, suffixes, n_batch):
    """What sequence s evaluates itself: prefix[n_shared:] + suffix_s, never empty."""
    k = n_shared(len(prefix), n_batch)
    return [list(prefix[k:]) + list(s) for s in suffixes]


def prompt_columns(n_prefix, n_batch, suffix_lens):
    """Prompt columns of the whole call: the shared rows once, then every sequence's own."""
    k = n_shared(n_prefix, n_batch)
    return k + sum(n_prefix - k + n for n in suffix_lens)


def chunks(length, n_batch, start=0):
    """[begin, end) of the reference's prompt chunks over positions [start, start + length)."""
    return [(start + at, start + min(at + n_batch, length)) for at in range(0, length, n_batch)]


def layout(n_prefix, n_batch, suffix_lens):
    """The call's numbers, and per sequence the chunks of its own columns in absolute positions."""
    k = n_shared(n_prefix, n_batch)
    return dict(n_shared=k, prompt_columns=prompt_columns(n_prefix, n_batch, suffix_lens), columns=len(suffix_lens),
                shared_chunks=chunks(k, n_batch), own_chunks=[chunks(n_prefix - k + n, n_batch, k) for n in suffix_lens])
