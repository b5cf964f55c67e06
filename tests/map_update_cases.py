"""Inputs and references of the map update's tests (include/obvi_map_update.h): shared by tests/test_map_update_abi.py (CPU: the yardstick is itself held)
and tests/test_gpu_map_update.py (the device against the yardstick).  Nothing here touches the product.

The yardstick is conditioning in INFORMATION form, in long double:
      C' = (Cs^-1 + E_A (Ps^-1 - Cs_AA^-1) E_A^T)^-1        mu' = C' (Cs^-1 mu + E_A (Ps^-1 m - Cs_AA^-1 mu_A))
which shares no step with the update formula the device evaluates (mu' = mu + K (m - mu_A), C' = Cs - K (Cs_AA - Ps) K^T, K = Cs[:, A] Cs_AA^-1).

Maps: spd(cond = 1e3) plus a small antisymmetric part (the symmetrisation is exercised) -- a 24-object map whose 168 / 216 rows put a tile boundary on either
side of every split, and the 70-object map of test_gpu_map_resident.py.  Selections are scattered and out of order.  The posterior of a window is
P = (Cs_AA^-1 + J^T J)^-1, m = mu_A + P b from a seeded random J with 2 N_A rows, in long double, rounded to fp64: it is below its prior, as a real one is.

Inverses: inv_ld of test_gpu_map_pair_priors.py (the fp64 inverse refined by Newton-Schulz steps in long double) for everything of a window's size and for the
small map; inv_big for the 490- and 630-row matrices, the same algorithm with ONE step and products whose right operand is column-major (numpy's long-double
product is three plain loops: 2.5 s at 630 rows, 0.9 s column-major).  One step is enough there: the matrices have condition numbers below 2e4, the fp64 inverse
is good to 1e-11, a step squares that (a second step changes nothing), and the result is probed: |M (X z) - z| <= 5e-15 |z| on random z -- the probe's own
rounding leaves 4e-16 there, the fp64 inverse without the step 3e-14."""
import functools

import numpy as np

from test_gpu_map_pair_priors import inv_ld, spd
from test_gpu_map_resident import the_map

LD = np.longdouble
N_SMALL = 24


def sym(M):
    return 0.5 * (M + M.T)


def rows_of(sel, od):
    return np.concatenate([np.arange(od * o, od * o + od) for o in sel])


@functools.lru_cache(maxsize=None)
def small_map(od):
    """24 objects: 168 rows at od 7, 216 at od 9.  Computed once, never changed."""
    rng = np.random.default_rng(300 + od)
    n = N_SMALL * od
    R = rng.normal(size=(n, n))
    cov = spd(rng, n, cond=1e3) + 1e-4 * 1e-2 * (R - R.T)
    mean = rng.normal(size=(N_SMALL, od))
    assert np.abs(cov - cov.T).max() > 0
    mean.setflags(write=False); cov.setflags(write=False)
    return mean, cov


def map_of(which, od):
    return small_map(od) if which == "small" else the_map(od)


def selection(rng, n, k):
    """k of n objects, scattered and out of order (k = n: a permutation that is not the identity)."""
    sel = rng.permutation(n)[:k]
    if k > 1 and (np.diff(sel) > 0).all():
        sel = sel[::-1].copy()
    return sel


def mm(A, B):
    return A @ np.asfortranarray(B)


def inv_big(M):
    M = np.asarray(M, dtype=LD)
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    X = mm(X, 2 * np.eye(len(M), dtype=LD) - mm(M, X))
    X = 0.5 * (X + X.T)
    z = np.random.default_rng(len(M)).normal(size=(len(M), 3)).astype(LD)
    assert np.abs(M @ (X @ z) - z).max() <= 5e-15 * np.abs(z).max()
    return X


def inverse(M):
    return inv_ld(M) if len(M) <= 300 else inv_big(M)


@functools.lru_cache(maxsize=None)
def map_information(which, od):
    mean, cov = map_of(which, od)
    L = inverse(sym(np.asarray(cov, dtype=LD)))
    L.setflags(write=False)
    return L


def posterior(prior_mean, prior_cov, seed):
    """(m [N_A], P [N_A][N_A]) in fp64 from the window's prior N(prior_mean, prior_cov) and seeded random measurements J x = b."""
    NA = len(prior_cov)
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(2 * NA, NA)).astype(LD)
    b = rng.normal(size=NA).astype(LD)
    P = inv_ld(inv_ld(prior_cov) + J.T @ J)
    m = np.asarray(prior_mean, dtype=LD).ravel() + P @ b
    return m.astype(np.float64), P.astype(np.float64)


def yardstick(which, od, windows):
    """The information form, long double.  windows: [(sel, m, P, prior_cov)], prior_cov = the sub-block the window's prior was cut from (None: the map's own, for
    one window or the first of several).  Returns (mean [N], cov [N][N]) as long double."""
    mean, cov = map_of(which, od)
    Lam = np.array(map_information(which, od))
    eta = Lam @ np.asarray(mean, dtype=LD).ravel()
    Cs = sym(np.asarray(cov, dtype=LD))
    for sel, m, P, prior in windows:
        idx = rows_of(sel, od)
        if prior is None:
            prior_cov, prior_mean = Cs[np.ix_(idx, idx)], np.asarray(mean, dtype=LD).ravel()[idx]
        else:
            prior_cov, prior_mean = prior
        Li, Lp = inv_ld(sym(np.asarray(P, dtype=LD))), inv_ld(prior_cov)
        Lam[np.ix_(idx, idx)] += Li - Lp
        eta[idx] += Li @ np.asarray(m, dtype=LD).ravel() - Lp @ np.asarray(prior_mean, dtype=LD)
    C = inverse(sym(Lam))
    return C @ eta, C


def update_formula(mean, cov, sel, m, P, od, dtype=np.float64):
    """mu' = mu + K (m - mu_A), C' = Cs - K (Cs_AA - Ps) K^T with the A rows and columns set to the posterior -- what the device evaluates; fp64: numpy's own
    evaluation (the round trip a session needs without the device entry), long double: held against the yardstick on the CPU."""
    inv = np.linalg.inv if dtype == np.float64 else inv_ld
    Cs = sym(np.asarray(cov, dtype=dtype))
    mu = np.asarray(mean, dtype=dtype).ravel()
    idx = rows_of(sel, od)
    Ps = sym(np.asarray(P, dtype=dtype))
    Caa = Cs[np.ix_(idx, idx)]
    K = Cs[:, idx] @ inv(Caa)
    new_mu = mu + K @ (np.asarray(m, dtype=dtype).ravel() - mu[idx])
    new_C = sym(Cs - K @ (Caa - Ps) @ K.T)
    new_C[np.ix_(idx, idx)] = Ps
    new_mu[idx] = np.asarray(m, dtype=dtype).ravel()
    return new_mu.reshape(-1, od), new_C


# the host-pointer form's cases: (map, od, k).  Window rows 7 63 70 98 105 161 168 | 9 63 72 144 153 216 around the tile edges of 168 / 216 map rows, the rest
# 161 ... 0 | 207 ... 0; and several tiles on both sides: 30 of the 70 objects.
EDGE_CASES = [("small", 7, k) for k in (1, 9, 10, 14, 15, 23, 24)] + [("small", 9, k) for k in (1, 7, 8, 16, 17, 24)] + [("large", 7, 30), ("large", 9, 30)]


@functools.lru_cache(maxsize=None)
def edge_case(which, od, k):
    """(sel, m [k][od], P) of one case; computed once."""
    mean, cov = map_of(which, od)
    n = len(mean)
    rng = np.random.default_rng(1000 * od + k + (7 if which == "large" else 0))
    sel = selection(rng, n, k)
    idx = rows_of(sel, od)
    Caa = sym(np.asarray(cov))[np.ix_(idx, idx)]
    m, P = posterior(mean[sel], Caa, seed=17 * k + od)
    R = rng.normal(size=P.shape)
    P = P + 1e-6 * np.abs(P).max() * (R - R.T)            # the caller's P need not be symmetric: the entry symmetrises it
    m = m.reshape(k, od)
    for a in (sel, m, P):
        a.setflags(write=False)
    return sel, m, P


@functools.lru_cache(maxsize=None)
def edge_reference(which, od, k):
    sel, m, P = edge_case(which, od, k)
    mu, C = yardstick(which, od, [(sel, m, P, None)])
    return mu.reshape(-1, od), C
