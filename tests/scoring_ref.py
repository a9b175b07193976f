"""Reference side of the scoring tests (CPU, float64): every position's logits from the oracle's
public pieces, and the scoring rule of DESIGN.md "Scoring" restated in NumPy.

The rule for one row of logits z[0..N) and a target t:
  lse = m + log sum_i exp(z_i - m), m = max z (a -inf logit adds 0 to the sum);
  logprob = z_t - lse; t = -1 is "no target" and scores 0.0;
  a row whose maximum is NaN or +inf, or whose logits are all -inf, scores NaN;
  argmax = the first NaN, else the first maximum (np.argmax's rule, llama3.py:320).
"""

import numpy as np

import llama3_oracle as orc


def all_logits(model: "orc.OracleModel", ids, start_pos: int) -> np.ndarray:
    """OracleModel.__call__ (llama3.py:285-308) with every position's logits kept: float64
    [B, L, VS].  Writes the oracle's KV caches exactly as the call does."""
    ids = np.asarray(ids)
    L = ids.shape[1]
    h = model.emb[ids]
    cos = model.cos[start_pos:start_pos + L]
    sin = model.sin[start_pos:start_pos + L]
    mask = orc.causal_mask(L, start_pos)
    for layer in model.layers:
        h = layer(h, start_pos, mask, cos, sin)
    h = orc.rmsnorm(h, model.final_norm, model.args.norm_eps)
    return np.asarray(h @ model.lm_head.T, dtype=np.float64)


def logprobs64(z, targets):
    """The rule in float64 over the last axis of z; targets int of z.shape[:-1].
    Returns (logprob, lse, argmax, margin): margin = top-1 minus top-2 logit (inf for a one-column
    row, NaN where the row holds a NaN)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64)
    N = z.shape[-1]
    if t.shape != z.shape[:-1]:
        raise ValueError(f"targets {t.shape} for logits {z.shape}")
    if ((t < -1) | (t >= N)).any():
        raise ValueError("target outside [0, N) and not -1")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(z, axis=-1)  # NaN if the row holds one
        bad = np.isnan(m) | np.isinf(m)
        sub = np.where(bad, 0.0, m)
        s = np.sum(np.exp(z - sub[..., None]), axis=-1)
        lse = sub + np.log(s)
        lse = np.where(np.isnan(m) | (m == np.inf), np.nan, lse)  # all -inf: -inf
        zt = np.take_along_axis(z, np.maximum(t, 0)[..., None], axis=-1)[..., 0]
        lp = np.where(bad, np.nan, zt - lse)
        lp = np.where(t < 0, 0.0, lp)
    am = np.argmax(z, axis=-1)  # the first NaN, else the first maximum
    if N > 1:
        top2 = np.partition(z, N - 2, axis=-1)[..., N - 2:]
        with np.errstate(invalid="ignore"):
            margin = top2[..., 1] - top2[..., 0]
    else:
        margin = np.full(z.shape[:-1], np.inf)
    return lp, lse, am, margin
