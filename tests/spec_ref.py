"""The specification of lookup-drafted speculative decoding (DESIGN.md "Speculative decoding") in
plain Python: the drafting rule, and a replay of the loop on a row whose true continuation is
known.  A helper of tests/test_spec_cpu.py and tests/test_gpu_spec.py, not a test."""


def draft(S, k, n_max, n_min):
    """The draft for the sequence ``S`` (lookup ++ prompt ++ emitted): for n = min(n_max, E - 1)
    down to n_min, the largest j in [0, E - n - 1] with S[j : j + n] == S[E - n : E]; at the first
    n that has one, S[j + n : min(j + n + k, E)].  Empty when nothing matches or k == 0."""
    S = [int(x) for x in S]
    E = len(S)
    if k <= 0:
        return []
    for n in range(min(n_max, E - 1), n_min - 1, -1):
        tail = S[E - n:]
        for j in range(E - n - 1, -1, -1):
            if S[j:j + n] == tail:
                return S[j + n:min(j + n + k, E)]
    return []


def simulate(lookup, prompt, true_ids, draft_len, n_max, n_min, stop_ids=()):
    """The loop on one row whose ordinary decoding emits ``true_ids`` (all R of them, stop ids
    ignored): (ids, row_steps, drafted, accepted).  The token chosen at a chunk position whose
    inputs so far were the true ones is the next true id, which is all the loop ever looks at."""
    true = [int(x) for x in true_ids]
    stops = {int(x) for x in stop_ids}
    R = len(true)
    if R == 0:
        return [], 0, 0, 0
    out = [true[0]]  # from the prefill
    steps = drafted = accepted = 0
    fin = true[0] in stops or R == 1
    while not fin:
        m = len(out)
        S = [int(x) for x in lookup] + [int(x) for x in prompt] + out
        d = draft(S, min(draft_len, R - m - 1), n_max, n_min)
        chunk = [out[-1]] + d
        chosen = true[m:m + len(chunk)]
        a = 0
        while a < len(d) and chunk[a + 1] == chosen[a]:
            a += 1
        steps += 1
        drafted += len(d)
        accepted += a
        for t in range(a + 1):
            out.append(chosen[t])
            if chosen[t] in stops:
                fin = True
                break
        fin = fin or len(out) >= R
    return out, steps, drafted, accepted
