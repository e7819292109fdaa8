"""The stop rule of generate_queue(params=) (biogpt_hip_generate_queue_requests; INTEGRATION.md, "Generation over a queue"), restated on the output of the
closed call of a request alone.  Not a test module: a helper the tests import."""


def stop_cut(gen, stops, eos=-1):
    """gen: what the closed call of the request alone generated (it ends with its EOS or at its limit).  Returns (the request's ids, why it ended: 0 its limit,
    1 its EOS id, 2 + i stop sequence i): cut just behind the first token at which a stop sequence lies complete inside the generated tokens -- the EOS is
    looked at first, the lowest index wins among the stop sequences."""
    gen = [int(t) for t in gen]
    for t in range(len(gen)):
        if eos >= 0 and gen[t] == eos:
            return gen[:t + 1], 1
        for i, s in enumerate(stops):
            if 0 < len(s) <= t + 1 and gen[t + 1 - len(s):t + 1] == [int(v) for v in s]:
                return gen[:t + 1], 2 + i
    return gen, 0
