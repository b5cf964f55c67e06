"""Inputs and references of the tests of a map that grows (include/obvi_map_extend.h): shared by tests/test_map_extend_abi.py (CPU: the yardstick is itself
held) and tests/test_gpu_map_extend.py (the device against the yardstick).  Nothing here touches the product.  Maps, selections and inverses are those of
tests/map_update_cases.py, which this module imports and does not change.

The window held A (k_old objects of the map, prior = the map's marginal) and B (k_new objects the map lacks, no prior).  The yardstick is the INFORMATION form
in long double over the rows (old map, B):
      Lam' = pad(Cs^-1) + E (Ps^-1 - pad(Cs_AA^-1)) E^T            eta' = pad(Cs^-1 mu) + E (Ps^-1 m - pad(Cs_AA^-1 mu_A))
      C' = Lam'^-1                                                  mu' = C' eta'
(E picks the rows of (A, B); pad fills the rows of B with zeros), which shares no step with the formula the device evaluates:
      mu'[old] = mu + K (m_A - mu_A), C'[old, old] = Cs - K (Cs_AA - Ps_AA) K^T, C'[old, B] = K Ps_AB, C'[B, B] = Ps_BB, mu'[B] = m_B,  K = Cs[:, A] Cs_AA^-1.

The posterior of a window is P = (pad(Cs_AA^-1) + J^T J)^-1, m = (mu_A, 0) + P b from a seeded random J with 2 (N_A + N_B) rows, in long double, rounded to
fp64 -- B is observable through J alone, as a new object is through its measurements -- plus the small antisymmetric part edge_case gives its P."""
import functools

import numpy as np

import map_update_cases as base
from map_update_cases import LD, map_of, mm, rows_of, selection, sym
from test_gpu_map_pair_priors import inv_ld

# (map, od, k_old, k_new).  od 7: window rows 14 70 133 133 196 21 119 around 64 / 128 / 192, the small map's 168 rows grow to 175 175 231 238 196 189 189;
# od 9: 18 135 135 261 36 180, 216 rows grow to 225 288 279 261 252 252.  B starts inside a tile in every case.  And several tiles everywhere: the 70-object map.
EXTEND_CASES = ([("small", 7, a, b) for a, b in ((1, 1), (9, 1), (10, 9), (9, 10), (24, 4), (0, 3), (14, 3))]
                + [("small", 9, a, b) for a, b in ((1, 1), (7, 8), (8, 7), (24, 5), (0, 4), (16, 4))]
                + [("large", 7, 30, 12), ("large", 9, 30, 8)])


def inverse(M):
    """inv_ld up to 300 rows; above, the algorithm of map_update_cases.inv_big (the fp64 inverse, ONE Newton-Schulz step in long double with column-major right
    operands) with the probe's bound set for the matrices of this module.  |M (X z) - z| / |z| estimates |M X - I|, which bounds the relative error of X; 1e-13 is
    a hundred times below the 1e-11 bar the references serve.  The probe's own rounding grows with the condition number: 1.4e-14 at the worst matrix here (648
    rows, condition 2.9e4 -- the grown information matrix of the od 9 handle-form window, whose new objects carry only a weak prior), where further steps change
    nothing and the fp64 inverse without the step leaves 5e-13: the bound still tells the two apart."""
    if len(M) <= 300:
        return inv_ld(M)
    M = np.asarray(M, dtype=LD)
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    X = mm(X, 2 * np.eye(len(M), dtype=LD) - mm(M, X))
    X = 0.5 * (X + X.T)
    z = np.random.default_rng(len(M)).normal(size=(len(M), 3)).astype(LD)
    assert np.abs(M @ (X @ z) - z).max() <= 1e-13 * np.abs(z).max()
    return X


def window_posterior(prior_mean, prior_cov, n_new_rows, seed):
    """(m [N_A + N_B], P) in fp64: the window's prior N(prior_mean, prior_cov) over A, none over B, and seeded random measurements J x = b of all of (A, B)."""
    NA = len(prior_cov)
    NP = NA + n_new_rows
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(2 * NP, NP)).astype(LD)
    b = rng.normal(size=NP).astype(LD)
    info = J.T @ J
    if NA:
        info[:NA, :NA] += inverse(np.asarray(prior_cov, dtype=LD))
    P = inverse(info)
    m = np.concatenate([np.asarray(prior_mean, dtype=LD).ravel(), np.zeros(n_new_rows, dtype=LD)]) + P @ b
    return m.astype(np.float64), P.astype(np.float64)


def extend_information(Lam, eta, idx, n_new_rows, m, P, prior):
    """One window added in information form.  Lam, eta: long double, over the rows so far; idx: the rows of A; prior: (cov, mean) the window's prior over A was cut
    from.  Returns the grown (Lam, eta)."""
    N, NB = len(Lam), n_new_rows
    big = np.zeros((N + NB, N + NB), dtype=LD)
    big[:N, :N] = Lam
    e = np.concatenate([eta, np.zeros(NB, dtype=LD)])
    rows = np.concatenate([np.asarray(idx, dtype=np.int64), np.arange(N, N + NB)])
    Li = inverse(sym(np.asarray(P, dtype=LD)))
    big[np.ix_(rows, rows)] += Li
    e[rows] += Li @ np.asarray(m, dtype=LD).ravel()
    if len(idx):
        Lp = inverse(np.asarray(prior[0], dtype=LD))
        big[np.ix_(idx, idx)] -= Lp
        e[idx] -= Lp @ np.asarray(prior[1], dtype=LD).ravel()
    return big, e


def yardstick(which, od, windows):
    """The information form, long double.  windows: [(sel, k_new, m, P, prior)], sel: the window's old objects in the numbering of the map as grown so far,
    prior = (cov, mean) its prior was cut from (None: the map's own marginal, for the first window).  which None: no map at all.  Returns (mean, cov)."""
    if which is None:
        Lam, eta, Cs, mu = np.zeros((0, 0), dtype=LD), np.zeros(0, dtype=LD), None, None
    else:
        mean, cov = map_of(which, od)
        Lam = np.array(base.map_information(which, od))
        mu = np.asarray(mean, dtype=LD).ravel()
        eta = Lam @ mu
        Cs = sym(np.asarray(cov, dtype=LD))
    for sel, k_new, m, P, prior in windows:
        idx = rows_of(sel, od) if len(sel) else np.zeros(0, dtype=np.int64)
        if prior is None and len(sel):
            prior = (Cs[np.ix_(idx, idx)], mu[idx])
        Lam, eta = extend_information(Lam, eta, idx, k_new * od, m, P, prior)
    C = inverse(sym(Lam))
    return C @ eta, C


def extension_formula(mean, cov, sel, k_new, m, P, od, dtype=np.float64):
    """What the device evaluates; fp64: numpy's own evaluation (the round trip a session needs without the device entry), long double: held against the yardstick
    on the CPU.  mean / cov None: no map yet."""
    inv = np.linalg.inv if dtype == np.float64 else inverse
    NB = k_new * od
    Ps = sym(np.asarray(P, dtype=dtype))
    mv = np.asarray(m, dtype=dtype).ravel()
    if mean is None:
        return mv.reshape(-1, od), Ps
    Cs = sym(np.asarray(cov, dtype=dtype))
    mu = np.asarray(mean, dtype=dtype).ravel()
    N, NA = len(mu), len(sel) * od
    new_C = np.zeros((N + NB, N + NB), dtype=dtype)
    new_mu = np.concatenate([mu, mv[NA:]])
    new_C[:N, :N] = Cs
    if NA:
        idx = rows_of(sel, od)
        Caa = Cs[np.ix_(idx, idx)]
        K = Cs[:, idx] @ inv(Caa)
        new_mu[:N] = mu + K @ (mv[:NA] - mu[idx])
        new_C[:N, :N] = sym(Cs - K @ (Caa - Ps[:NA, :NA]) @ K.T)
        new_C[:N, N:] = K @ Ps[:NA, NA:]
        new_C[N:, :N] = new_C[:N, N:].T
        rows = np.concatenate([idx, np.arange(N, N + NB)])
        new_mu[idx] = mv[:NA]
    else:
        rows = np.arange(N, N + NB)
    new_C[np.ix_(rows, rows)] = Ps
    return new_mu.reshape(-1, od), new_C


@functools.lru_cache(maxsize=None)
def extend_case(which, od, k_old, k_new):
    """(sel [k_old], m [k_old + k_new][od], P) of one case; computed once."""
    mean, cov = map_of(which, od)
    rng = np.random.default_rng(5000 + 1000 * od + 37 * k_old + k_new + (7 if which == "large" else 0))
    sel = selection(rng, len(mean), k_old) if k_old else np.zeros(0, dtype=np.int64)
    idx = rows_of(sel, od) if k_old else np.zeros(0, dtype=np.int64)
    Caa = sym(np.asarray(cov))[np.ix_(idx, idx)]
    m, P = window_posterior(mean[sel], Caa, k_new * od, seed=17 * k_old + 3 * k_new + od)
    R = rng.normal(size=P.shape)
    P = P + 1e-6 * np.abs(P).max() * (R - R.T)            # the caller's P need not be symmetric: the entry symmetrises it
    m = m.reshape(k_old + k_new, od)
    for a in (sel, m, P):
        a.setflags(write=False)
    return sel, m, P


@functools.lru_cache(maxsize=None)
def extend_reference(which, od, k_old, k_new):
    sel, m, P = extend_case(which, od, k_old, k_new)
    mu, C = yardstick(which, od, [(sel, k_new, m, P, None)])
    return mu.reshape(-1, od), C


def grown_rows(sel, n, k_new, od):
    """Rows of the window's (A, B) in the grown map: A at its map rows, B behind the n old objects."""
    return np.concatenate([rows_of(sel, od) if len(sel) else np.zeros(0, dtype=np.int64), np.arange(n * od, (n + k_new) * od)]).astype(np.int64)
