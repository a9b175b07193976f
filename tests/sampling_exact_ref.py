"""Rows on which the sample kernel's pick is one specific index, and the integer arithmetic that
names it.  A helper for test_sampling_exact_cpu.py and test_gpu_sampling_exact.py.

sample.hip turns every weight into a 32-bit fixed-point integer and adds integers only.  An element
equal to the row's maximum weighs exactly W = 2^32 - 256; an element at -inf, or at most -1e30 with
T <= 100, weighs exactly 0.  On a row made of such elements the select, the tie cut and the index
searches decide the pick alone, so a test may ask for equality.  ExactRow restates the kernel's
integer steps (DESIGN.md "Sampling"; the rule itself is sampling_ref's):
  f      = int(float32(top_p) * 2^32)
  target = max(1, ceil(mass(K) * f / 2^32))      nucleus: the shortest rank-order prefix reaching it
  frac   = int(float32(u) * 2^32)
  target = floor(mass(S) * frac / 2^32) + 1      draw: the first index of S, ascending, reaching it
with rank order = value descending, then lower index (-0 == +0).

The builders below make the tables of both test modules: plateau rows, two-plateau rows, and
top-k rows of adversarial bit patterns.  geometry() and bucket_shift() restate how the kernel
spreads a row over its 16 waves and how wide an index bucket of the search is.
"""

import itertools
import math
from collections import namedtuple

import numpy as np

NT, NW, R, NB = 1024, 16, 32, 4096  # sample.hip's constants
W = 2 ** 32 - 256
_M32 = 0xFFFFFFFF
U_LAST = 1.0 - 2.0 ** -24

TEMPERATURES = (0.5, 1.0, 100.0)
TOP_PS = (1.0, 0.5, 0.75, 0.9, 1e-9)
PLATEAU_VALUES = (0.0, 3.5, -2.25, "zeros")  # "zeros": -0.0 and +0.0 alternating, -0.0 first
LOWS = (-np.inf, -1e30, -3e38, -2.5e33)  # all weigh exactly 0 below a finite maximum, T <= 100
REG_SIZES = (7, 2048, 2049, 32000, 32768)
LONG_SIZES = (32769, 40001, 65537, 131073, 262145)


def geometry(n):
    """(register form?, indices per wave ch, non-empty waves): wave w holds [w * ch, (w + 1) * ch)."""
    reg = n <= R * NT
    ch = R * 64 if reg else (((n + NW - 1) // NW + 63) & ~63)
    return reg, ch, (n + ch - 1) // ch


def bucket_shift(length):
    """s of index_search's first histogram over a wave of `length` indices: buckets of 2^s."""
    s = 0
    while ((length + (1 << s) - 1) >> s) > NB:
        s += 1
    return s


def search_shift(n):
    """The widest s a search of the row starts with (its full waves')."""
    return bucket_shift(min(geometry(n)[1], n))


def mul_frac_floor(a, f):
    return (a >> 32) * f + (((a & _M32) * f) >> 32)


def mul_frac_ceil(a, f):
    return (a >> 32) * f + (((a & _M32) * f + _M32) >> 32)


def frac_of(u):
    uf = float(np.float32(u)) * 4294967296.0
    return (int(uf) if uf < 4294967295.0 else _M32) if uf > 0.0 else 0


class ExactRow:
    """A row with its elements' integer weights: the kept set and the pick in exact integers."""

    def __init__(self, z, wint, order=None):
        self.z = np.asarray(z, np.float32)
        self.w = np.asarray(wint, np.int64)
        # z descending, ties by lower index; -(-0.0) and -(+0.0) compare equal
        self.order = np.argsort(-self.z.astype(np.float64), kind="stable") if order is None else order

    def kept(self, top_k, top_p):
        """The indices of S, ascending."""
        K = self.order[:top_k] if 0 < top_k < self.z.size else self.order
        p32 = float(np.float32(top_p))
        if p32 < 1.0:
            cw = np.cumsum(self.w[K])
            target = max(1, mul_frac_ceil(int(cw[-1]), int(p32 * 4294967296.0)))
            K = K[:int(np.searchsorted(cw, target, side="left")) + 1]
        return np.sort(K)

    def pick(self, S, u):
        cw = np.cumsum(self.w[S])
        target = mul_frac_floor(int(cw[-1]), frac_of(u)) + 1
        return int(S[int(np.searchsorted(cw, target, side="left"))])


def lows(n, phase=0):
    """A weightless row: runs of each of LOWS."""
    return np.asarray(LOWS, np.float32)[((np.arange(n) + phase) // 61) % len(LOWS)]


def boundary_uniforms(members, ch):
    """u = 0, the largest u, and j / c rounded to 24 bits with its two neighbours for the first, the
    last and the wave-crossing members j of a final set of c weighted members (ascending)."""
    c = len(members)
    js = {1, c - 1}
    cross = np.flatnonzero(np.diff(np.asarray(members) // ch)) + 1
    if cross.size:
        js |= {int(cross[0]), int(cross[cross.size // 2]), int(cross[-1])}
    q = {0, (1 << 24) - 1}
    for j in js:
        if 0 < j < c:
            u0 = (j * (1 << 25) + c) // (2 * c)
            q |= {v for v in (u0 - 1, u0, u0 + 1) if 0 <= v < 1 << 24}
    return np.array(sorted(q), np.float32) * np.float32(2.0 ** -24)


# ---- 1. plateau rows -----------------------------------------------------------------------

Call = namedtuple("Call", "label z T top_k top_p u want meta")


def plateau_positions(n):
    """[(kind, member indices ascending)] of size n's table."""
    _, ch, waves = geometry(n)
    rng = np.random.default_rng(4000 + n)
    kinds = [("ends", [0, n - 1])]
    if waves > 1:
        kinds.append(("waves", sorted({i for w in (1, waves // 2, waves - 1) for i in (w * ch - 1, w * ch)})))
    if n >= 64:
        # a wave the search has to walk to, and full (so that its buckets are the widest)
        lo = ch if waves > 2 else 0
        B = 1 << bucket_shift(min(ch, n - lo))
        # both sides of a bucket boundary, and two members inside one bucket (a bucket is one
        # index where s = 0)
        kinds.append(("buckets", [lo + 37 * B - 1, lo + 37 * B, lo + 42 * B, lo + 42 * B + max(B - 1, 1)]))
    last = (waves - 1) * ch
    kinds.append(("single", [last + (n - last) // 2]))
    if n in (7, 2049, 65537):
        kinds.append(("dense", list(range(n))))
    kinds.append(("scattered", np.sort(rng.choice(n, min(1000, max(3, n // 2)), replace=False)).tolist()))
    return kinds


def plateau_row(n, members, value, phase=0):
    z = lows(n, phase)
    members = np.asarray(members)
    if isinstance(value, str):
        z[members] = np.where(np.arange(members.size) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    else:
        z[members] = value
    return z


def plateau_weights(z):
    z = np.asarray(z)
    top = z == z.max()
    assert np.isfinite(z.max()) and (z[~top] <= -1e30).all()
    return np.where(top, W, 0).astype(np.int64)


def plateau_calls(n):
    """The calls of size n: one row tiled over its uniforms, with the integer model's picks."""
    _, ch, _ = geometry(n)
    t = (REG_SIZES + LONG_SIZES).index(n)
    tied = 0
    for si, (kind, members) in enumerate(plateau_positions(n)):
        si += n  # the rotations start elsewhere at every size
        # the rows of more than one member take the values in turn, from a start that leaves the
        # mixed zeros on one of them at every size (the smallest sizes have three such rows)
        value = PLATEAU_VALUES[(tied + 3 - t) % 4 if len(members) > 1 else t % 3]
        tied += len(members) > 1
        z = plateau_row(n, members, value, phase=si)
        row = ExactRow(z, plateau_weights(z))
        M = len(members)
        ks = sorted({k for k in (0, 1, M - 1, M, M + 1, n - 1, n) if k >= 0})
        for (ik, k), (ip, p) in itertools.product(enumerate(ks), enumerate(TOP_PS)):
            if (ik + ip + si) % 3:  # a third of the pairs per row; three rows in a row cover all
                continue
            T = TEMPERATURES[(ik + si // 3) % 3]
            S = row.kept(k, p)
            u = boundary_uniforms(S[row.w[S] > 0], ch)
            yield Call(f"n={n} {kind} M={M} m={value} T={T} top_k={k} top_p={p}", z, T, k, p, u,
                       [row.pick(S, float(v)) for v in u], {"kind": kind, "M": M, "kept": S, "value": value})


# ---- 2. two plateaus -----------------------------------------------------------------------

def two_plateau_calls(n):
    """[(Call, candidates)] of size n: M1 elements at the maximum m and M2 at m - T ln 2, top_p cutting
    inside the second plateau.  The device's weight of the second plateau is one integer near W / 2
    that is not known exactly, so a case (one u of a call) is kept only if the exact integers give
    the same set and pick for W / 2 * (1 + e), e in {-1e-4, 0, 1e-4}.  Call.meta: `third` of the
    second plateau the cut falls in, `crosses` (the kept part of it spans a wave boundary)."""
    _, ch, waves = geometry(n)
    rng = np.random.default_rng(7000 + n)
    out = []
    for ci, (M1, M2, layout) in enumerate(itertools.product((4, 37), (30, 301), ("scattered", "boundary"))):
        T = TEMPERATURES[ci % 3]
        m = (3.5, -2.25)[(ci // 2) % 2]
        z2 = np.float32(np.float32(m) - np.float32(T * math.log(2.0)))
        if layout == "scattered":
            pos = rng.choice(n, M1 + M2, replace=False)
            p1, p2 = pos[:M1], np.sort(pos[M1:])
        else:  # the second plateau contiguous across a wave boundary
            start = (waves // 2) * ch - M2 // 2
            p1, p2 = rng.choice(start, M1, replace=False), np.arange(start, start + M2)
        z = lows(n, ci)
        z[p1] = m
        z[p2] = z2
        params = []
        for k, m2k in ((0, M2), (M1 + M2 - 2, M2 - 2)):
            for t in (1 / 6, 1 / 2, 5 / 6) if k == 0 else (1 / 2,):
                params.append((k, (M1 + 0.5 * (math.floor(t * m2k) + 0.5)) / (M1 + 0.5 * m2k)))
        params += [(0, 0.5), (0, 0.75)]
        order = ExactRow(z, np.zeros(n, np.int64)).order
        rows = []
        for e in (-1e-4, 0.0, 1e-4):
            w = np.zeros(n, np.int64)
            w[p1] = W
            w[p2] = round(W / 2 * (1 + e))
            rows.append(ExactRow(z, w, order))
        in2 = np.zeros(n, bool)
        in2[p2] = True
        for k, p in params:
            sets = [r.kept(k, p) for r in rows]
            kept2 = sets[1][in2[sets[1]]]
            if kept2.size == 0 or sets[1].size < M1 + kept2.size:
                continue  # the cut is not inside the second plateau: no candidate
            us = np.concatenate([[0, (1 << 24) - 1], rng.integers(0, 1 << 24, 6)]).astype(np.float32)
            us *= np.float32(2.0 ** -24)
            same = all(np.array_equal(s, sets[1]) for s in sets)
            picks = [[r.pick(s, float(v)) for v in us] for r, s in zip(rows, sets)]
            ok = np.array([same and picks[0][j] == picks[1][j] == picks[2][j] for j in range(us.size)])
            m2k = M2 if k == 0 else M2 - 2
            meta = {"third": min(2, 3 * (kept2.size - 1) // m2k), "crosses": bool(kept2[0] // ch != kept2[-1] // ch),
                    "kept": sets[1]}
            call = Call(f"n={n} M1={M1} M2={M2} {layout} m={m} T={T} top_k={k} top_p={p!r}", z, T, k, p, us[ok],
                        [v for v, o in zip(picks[1], ok) if o], meta)
            out.append((call, us.size))
    return out


# ---- 3. top-k on adversarial keys ------------------------------------------------------------

def order_key(z):
    """sample.hip's order-preserving key of a float (no NaN; -0 == +0)."""
    z = np.asarray(z, np.float32).copy()
    z[z == 0] = 0.0
    b = z.view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def _from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def topk_rows(n):
    """[(name, row, ks)]: rows of bit patterns on which the first 12 key bits decide little.  Every k
    is at most 8 and every row's first 8 ranks lie within 2 of each other, so at T = 100 each kept
    member has at least a tenth of the mass and 256 stratified uniforms reach every one."""
    _, ch, _ = geometry(n)
    rng = np.random.default_rng(9000 + n)
    rows = []

    def places(cnt):
        return rng.choice(n, cnt, replace=False)

    # all of the row in one level-0 bin ([1, 1.125)): four ranks alone in their level-1 bins, the
    # next ranks crowded into one level-1 bin, so levels 1 and 2 hold the thresholds
    off = rng.choice(1000 << 10, n, replace=False)
    at = places(4)
    off[at] = [(1023 << 10) + 5, (1022 << 10) + 9, (1021 << 10) + 1, (1020 << 10) + 7]
    rows.append(("share12", _from_bits(0x3F800000 + off), (1, 2, 4, 6, 8)))

    # twelve distinct values sharing their top 22 key bits above a background in the same level-0 bin
    off = rng.choice(1 << 19, n, replace=False)
    off[places(12)] = 0xFFC00 + rng.choice(1 << 10, 12, replace=False)
    rows.append(("share22", _from_bits(0x3F800000 + off), (1, 2, 5, 8)))

    # all negative ((-1.125, -1]): inverted keys; four ranks alone in their level-1 bins, then six
    # sharing 22 key bits
    off = (24 << 10) + rng.choice(900 << 10, n, replace=False)
    at = places(10)
    off[at[:4]] = [5, (1 << 10) + 9, (2 << 10) + 1, (3 << 10) + 7]
    off[at[4:]] = (8 << 10) + rng.choice(1 << 10, 6, replace=False)
    rows.append(("negative", _from_bits(0xBF800000 + off), (1, 3, 4, 5, 7, 8)))

    # two positives, five zeros of both signs (the lowest index a -0.0), the rest negative
    z = (-1 - rng.random(n)).astype(np.float32)
    at = places(7)
    z[at[:2]] = [1e-3, 1e-40]
    z[np.sort(at[2:])] = [-0.0, 0.0, -0.0, 0.0, -0.0]
    rows.append(("zeros", z, (2, 3, 4, 6, 8)))

    # denormals of both signs
    bits = rng.choice(np.arange(1, 1 << 23), n, replace=False).astype(np.uint32)
    bits[rng.random(n) < 0.5] |= 0x80000000
    rows.append(("denormal", _from_bits(bits), (1, 4, 8)))

    # six equal values, three on each side of a wave boundary, below two higher ones
    off = rng.choice(1000 << 10, n, replace=False)
    tie = 7 * ch + np.arange(-3, 3)
    off[tie] = 1019 << 10
    at = rng.choice(np.setdiff1d(np.arange(n), tie), 2, replace=False)
    off[at] = [(1023 << 10) + 5, (1022 << 10) + 9]
    rows.append(("tie6", _from_bits(0x3F800000 + off), (3, 5, 7)))
    return rows
