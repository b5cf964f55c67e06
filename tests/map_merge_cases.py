"""Inputs and references of the map merge's tests (include/obvi_map_merge.h): shared by tests/test_map_merge_abi.py (CPU: the yardstick is itself held) and
tests/test_gpu_map_merge.py (the device against the yardstick).  Nothing here touches the product.

The device evaluates  mu' = mu - Y W (H mu - d),  C' = Cs - Y Y^T  (G = Cs H^T, T = H G + R = L L^T, W = L^-1, Y = G W^T) on the objects that are not dropped.
The yardstick shares no step with it, in long double:
  exact merge (no noise) -- the null-space form: every x that satisfies the constraint is x = E z + c, z the survivors, E copying each survivor into its
      duplicates, c holding d in the dropped rows; then  C' = (E^T Cs^-1 E)^-1,  mu' = C' E^T Cs^-1 (mu - c);
  with noise -- the information form:  (Cs^-1 + H^T R^-1 H)^-1  and its mean  C (Cs^-1 mu + H^T R^-1 d),  restricted to the survivors.

Maps and inverses: those of tests/map_update_cases.py (24 objects: 168 / 216 rows; 70 objects: 490 / 630 rows).  Groups come from a seeded permutation --
scattered, the survivor of a group any of its members, so `keep` lies both before and after `drop`; offsets are 0.1 N(0, 1); noise blocks
1e-3 (A A^T + od I) plus a small antisymmetric part (the entry symmetrises them).

Not used: one group of 24, or two groups of 12.  There the survivors' covariance collapses to 1e-2 and numpy's own fp64 evaluation of the formula sits at
3e-12 .. 8e-12 of the yardstick -- at the bar the device is held to, which measures the inputs then and not the device."""
import functools

import numpy as np

from map_update_cases import LD, inverse, map_information, map_of, rows_of, sym
from test_gpu_map_pair_priors import inv_ld

# (map, od, group sizes, with noise too).  Q rows | rows left --
#   small, 7: 7 | 161;  63, 70 | 105, 98 (T across one tile);  105, 98 | 63, 70 (the result across one tile)
#   small, 9: 9, 63, 72 | 207, 153, 144;  153, 144 | 63, 72
#   large: 210 | 280 and 270 | 360: several tiles both ways
GROUPS = [
    ("small", 7, (2,), True), ("small", 7, (2,) * 9, False), ("small", 7, (2,) * 10, False), ("small", 7, (3,) * 6 + (2,) * 3, True), ("small", 7, (3,) * 4 + (2,) * 6, False),
    ("small", 9, (2,), False), ("small", 9, (2,) * 7, False), ("small", 9, (2,) * 8, False), ("small", 9, (4, 4, 4, 3, 3, 3, 3), True), ("small", 9, (3,) * 8, False),
    ("large", 7, (3,) * 10 + (2,) * 10, True), ("large", 9, (3,) * 15, False),
]
# two by hand: object 0 dropped into the last one, the last one dropped into object 0
HAND = [("small", 7, "first_into_last"), ("small", 7, "last_into_first")]


def _name(sizes):
    out, i = [], 0
    while i < len(sizes):
        j = i
        while j < len(sizes) and sizes[j] == sizes[i]:
            j += 1
        out.append("%dx%d" % (sizes[i], j - i))
        i = j
    return "+".join(out)


_SIZES = {_name(s): s for _, _, s, _ in GROUPS}
CASES = [(w, od, _name(s), False) for w, od, s, _ in GROUPS] + [(w, od, _name(s), True) for w, od, s, noisy in GROUPS if noisy] + [(w, od, k, False) for w, od, k in HAND]


def pairs_of(rng, n, sizes):
    """(drop, keep) of groups of the given sizes among n objects: a seeded permutation cut into groups, the survivor a random member."""
    perm = rng.permutation(n)
    drop, keep, at = [], [], 0
    for m in sizes:
        grp = perm[at:at + m]
        at += m
        k = int(grp[rng.integers(m)])
        for o in grp:
            if int(o) != k:
                drop.append(int(o)); keep.append(k)
    return np.array(drop, np.uint32), np.array(keep, np.uint32)


@functools.lru_cache(maxsize=None)
def merge_case(which, od, key, noisy):
    """(drop [q], keep [q], offset [q][od], noise [q][od][od] or None) of one case; computed once."""
    mean, _ = map_of(which, od)
    n = len(mean)
    rng = np.random.default_rng(5000 + 10 * od + (3 if which == "large" else 0) + sum(map(ord, key)))
    if key == "first_into_last":
        drop, keep = np.array([0], np.uint32), np.array([n - 1], np.uint32)
    elif key == "last_into_first":
        drop, keep = np.array([n - 1], np.uint32), np.array([0], np.uint32)
    else:
        drop, keep = pairs_of(rng, n, _SIZES[key])
    q = len(drop)
    offset = 0.1 * rng.normal(size=(q, od))
    noise = None
    if noisy:
        A = rng.normal(size=(q, od, od))
        S = rng.normal(size=(q, od, od))
        noise = 1e-3 * (A @ A.transpose(0, 2, 1) + od * np.eye(od)) + 1e-6 * (S - S.transpose(0, 2, 1))
        noise.setflags(write=False)
    for a in (drop, keep, offset):
        a.setflags(write=False)
    return drop, keep, offset, noise


def new_index(n, drop, keep):
    """The contract restated: survivors keep their old relative order, a dropped object gets its keep's new number.  Returns (new_index [n], kept [n - q])."""
    dropped = np.zeros(n, bool)
    dropped[drop] = True
    kept = np.flatnonzero(~dropped)
    idx = np.full(n, -1, np.int64)
    idx[kept] = np.arange(len(kept))
    idx[drop] = idx[keep]
    assert (idx >= 0).all()
    return idx.astype(np.uint32), kept


def constraint(n, od, drop, keep):
    H = np.zeros((len(drop) * od, n * od), dtype=LD)
    for r, (b, k) in enumerate(zip(drop, keep)):
        H[od * r:od * r + od, od * b:od * b + od] = np.eye(od)
        H[od * r:od * r + od, od * k:od * k + od] = -np.eye(od)
    return H


def noise_blocks(noise, dtype):
    q, od, _ = noise.shape
    R = np.zeros((q * od, q * od), dtype=dtype)
    for r in range(q):
        R[od * r:od * r + od, od * r:od * r + od] = sym(np.asarray(noise[r], dtype=dtype))
    return R


def yardstick(mean, cov, Lam, drop, keep, offset, noise, od):
    """(mean [n - q][od], cov) in long double from the map, its information Lam = Cs^-1 (long double), and the pairs."""
    n = len(mean)
    mu = np.asarray(mean, dtype=LD).ravel()
    idx, kept = new_index(n, drop, keep)
    if noise is None:
        E = np.zeros((n * od, len(kept) * od), dtype=LD)
        for o in range(n):
            E[od * o:od * o + od, od * idx[o]:od * idx[o] + od] = np.eye(od)
        c = np.zeros(n * od, dtype=LD)
        c[rows_of(drop, od)] = np.asarray(offset, dtype=LD).ravel()
        EtL = E.T @ Lam
        C = inverse(sym(EtL @ E))
        return (C @ (EtL @ (mu - c))).reshape(-1, od), C
    H = constraint(n, od, drop, keep)
    q = len(drop)
    Ri = np.zeros((q * od, q * od), dtype=LD)
    for r in range(q):
        Ri[od * r:od * r + od, od * r:od * r + od] = inv_ld(sym(np.asarray(noise[r], dtype=LD)))
    HtRi = H.T @ Ri
    C = inverse(sym(Lam + HtRi @ H))
    m = C @ (Lam @ mu + HtRi @ np.asarray(offset, dtype=LD).ravel())
    rows = rows_of(kept, od)
    return m[rows].reshape(-1, od), C[np.ix_(rows, rows)]


@functools.lru_cache(maxsize=None)
def merge_reference(which, od, key, noisy):
    mean, cov = map_of(which, od)
    drop, keep, offset, noise = merge_case(which, od, key, noisy)
    return yardstick(mean, cov, map_information(which, od), drop, keep, offset, noise, od)


def merge_formula(mean, cov, drop, keep, offset, noise, od, dtype=np.float64):
    """mu' = mu - Y W (H mu - d), C' = Cs - Y Y^T on the survivors, with explicit inverses -- what the device evaluates.  fp64: numpy's own evaluation (the round
    trip a session needs without the device entry); long double: held against the yardstick on the CPU."""
    inv = np.linalg.inv if dtype == np.float64 else inv_ld
    n = len(mean)
    Cs = sym(np.asarray(cov, dtype=dtype))
    mu = np.asarray(mean, dtype=dtype).ravel()
    H = constraint(n, od, drop, keep).astype(dtype)
    d = np.zeros(len(drop) * od, dtype=dtype) if offset is None else np.asarray(offset, dtype=dtype).ravel()
    G = Cs @ H.T
    T = H @ G
    if noise is not None:
        T = T + noise_blocks(noise, dtype)
    Ti = inv(sym(T))
    new_mu = mu - G @ (Ti @ (H @ mu - d))
    new_C = sym(Cs - G @ Ti @ G.T)
    rows = rows_of(new_index(n, drop, keep)[1], od)
    return new_mu[rows].reshape(-1, od), new_C[np.ix_(rows, rows)]
