"""The sampling rule (DESIGN.md "Sampling") restated in NumPy, Philox4x32-10, and the rule by which
a device pick is judged.  A helper for test_sampling_cpu.py and test_gpu_sampling.py.

The rule, for one logits row z[0..n), temperature T > 0, top_k >= 0, 0 < top_p <= 1 and a uniform
u in [0, 1):
  1. a NaN in the row, or a maximum that is not finite: the argmax rule (first NaN, else first
     maximum); T == 0 is greedy too;
  2. m = max z, w_i = exp((z_i - m) / T);
  3. rank order: z descending, ties by lower index;
  4. K = the first top_k ranks if 0 < top_k < n, else all;
  5. top_p < 1: S = the shortest prefix of K in rank order whose mass reaches top_p * sum_K w (at
     least one token); else S = K;
  6. walk S in ascending index order with a running sum c_i: the first i with c_i > u * sum_S w,
     else the last index of S.

Acceptance.  Device exp and summation round differently from float64, so a pick g is judged by
where u falls: with S_hi the rule's set for top_p + D and its float64 CDF in index order, g is
accepted iff g is in S_hi and u lies within TOL of g's CDF interval.  D = 2e-4, TOL = 1e-3: a
float32 restatement with a sequential cumsum (the loosest order a kernel could pick) stays within
3.75e-4 of the float64 rule over 300 draws of each configuration in CONFIGS; TOL is about 2.7
times that, because a device's exp and reduction tree are not NumPy's.

Where a prefix's mass falls inside [top_p, top_p + D) of the kept mass, S_hi holds a token more
than the rule's own set S, and the CDF of S_hi alone would reject the float64 rule's exact pick
(at top_k = 40 a boundary token carries about 1 % of the mass, ten times TOL).  The slack D exists
because a device may land on either side of such a boundary, so there every set from S to S_hi
(they are nested prefixes in rank order) is a set the device may have cut, and g is accepted iff
it passes on one of them.  Everywhere else S = S_hi and this is the rule above, D and TOL as given.
"""

import numpy as np

D = 2e-4
TOL = 1e-3

# (n, logit scale, T, top_k, top_p)
CONFIGS = [
    (32000, 3.0, 0.8, 0, 0.9),
    (32000, 3.0, 0.7, 40, 0.95),
    (512, 2.0, 1.0, 0, 0.9),
    (32000, 1.0, 1.5, 0, 0.9),
    (128256, 3.0, 0.8, 0, 0.9),
    (40001, 3.0, 1.0, 0, 1.0),
    (7, 2.0, 1.0, 3, 0.8),
]

_M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123): 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in ctr)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def uniform(seed, row, pos):
    """u of a sampling step: key = the seed's halves, counter = (row, pos, 0, 0)."""
    x = philox4x32_10((row, pos, 0, 0), (seed & _M32, (seed >> 32) & _M32))
    return (x[0] >> 8) * 2.0 ** -24


def argmax_rule(z):
    z = np.asarray(z)
    nan = np.flatnonzero(np.isnan(z))
    return int(nan[0]) if nan.size else int(np.argmax(z))


def _ranked(z, T, top_k, dtype):
    """(K in rank order, the weights of the whole row), or None where the rule is the argmax."""
    z = np.asarray(z).astype(dtype)
    n = z.size
    if T == 0 or np.isnan(z).any() or not np.isfinite(z.max()):
        return None
    w = np.exp((z - z.max()) / dtype(T))
    order = np.argsort(-z, kind="stable")  # z descending, ties by lower index
    return (order[:top_k] if 0 < top_k < n else order), w


def _prefix(K, w, top_p, dtype):
    """How many ranks of K the nucleus keeps."""
    if not top_p < 1:
        return K.size
    c = np.cumsum(w[K])
    cnt = int(np.searchsorted(c, dtype(top_p) * c[-1], side="left")) + 1  # first prefix with c >= target
    return max(1, min(cnt, K.size))


def kept_set(z, T, top_k, top_p, dtype=np.float64):
    """(indices of S ascending, their weights), or None where the rule is the argmax."""
    r = _ranked(z, T, top_k, dtype)
    if r is None:
        return None
    K, w = r
    idx = np.sort(K[:_prefix(K, w, top_p, dtype)])
    return idx, w[idx]


def draw(idx, w, u, dtype=np.float64):
    """Step 6 on a kept set (kept_set's pair): many uniforms may share one set."""
    c = np.cumsum(w)  # sequential, in dtype
    hit = np.flatnonzero(c > dtype(u) * c[-1])
    return int(idx[hit[0]]) if hit.size else int(idx[-1])


def sample(z, T, top_k, top_p, u, dtype=np.float64):
    s = kept_set(z, T, top_k, top_p, dtype)
    if s is None:
        return argmax_rule(z)
    return draw(s[0], s[1], u, dtype)


def distance(z, T, top_k, top_p, u, g, d=D):
    """How far u lies outside the CDF interval of g (0 inside; inf when g is not in S_hi, or is not
    the argmax where the rule is the argmax): the least over the sets from S to S_hi."""
    r = _ranked(z, T, top_k, np.float64)
    if r is None:
        return 0.0 if g == argmax_rule(z) else float("inf")
    K, w = r
    best = float("inf")
    for cnt in range(_prefix(K, w, top_p, np.float64), _prefix(K, w, min(1.0, top_p + d), np.float64) + 1):
        idx = np.sort(K[:cnt])
        j = int(np.searchsorted(idx, g))
        if j >= idx.size or idx[j] != g:
            continue
        c = np.cumsum(w[idx])
        lo = (c[j - 1] if j else 0.0) / c[-1]
        hi = c[j] / c[-1]
        best = min(best, float(max(lo - u, u - hi, 0.0)))
    return best


def accept(z, T, top_k, top_p, u, g, tol=TOL, d=D):
    return distance(z, T, top_k, top_p, u, g, d) <= tol
