"""Inputs and references of the map match's tests (include/obvi_map_match.h): shared by tests/test_map_match_abi.py (CPU: the yardstick is itself held) and
tests/test_gpu_map_match.py (the device against the formula in long double).  Nothing here touches the product.

The device evaluates, for every pair a < b,  s = d^T T^-1 d  on the rows m of a mask, d = mu_b[m] - mu_a[m] (row 3 wrapped by a yaw period),
T = Cs_bb[m,m] - Cs_ba[m,m] - Cs_ab[m,m] + Cs_aa[m,m].  `formula` restates that: in long double with inv_ld (the reference of the GPU tests), in fp64 with numpy
(the round trip a session needs without the device entry).  The yardstick shares no step with it: the same quantity as a constrained least squares,
      s = min over {x: x_b[m] - x_a[m] = w} of (x - mu)^T Cs^-1 (x - mu),
in null-space form -- every x that satisfies the constraint is x = E z + c, z all rows but b's masked ones, E copying a's masked rows into b's (the E of
tests/map_merge_cases.py, restricted to the mask), c holding w -- with the map's information Lam = Cs^-1 of tests/map_update_cases.py:
      z* solves (E^T Lam E) z = E^T Lam (mu - c),   s = r^T Lam r,  r = E z* + c - mu.
E is applied by index (its products with Lam are row and column sums), and the system is solved by numpy's fp64 inverse with three steps of iterative refinement
whose residuals are long double; s is at a minimum in z, so what is left of the solve's error enters s squared.

Maps: the 24- and 70-object maps of tests/map_update_cases.py; every leading sub-map of the large one (objects 0 .. n - 1, n = 1 .. 33: its pairs are the large
map's pairs with b < n, so their reference is a slice of the large map's); the small map grown by five noisy copies of five of its objects (`planted`), one of
them turned by pi + 0.05 in a variant (od 7); a 258-object map whose leading sub-maps of 257 and 258 objects stand at the edge of the scatter's 256-wide sweep
(`sweep`); and a map with two exact copies, E Cr E^T copied entry by entry, whose pairs (2, 6) and (4, 7) have T = 0.

A gate or a distance is never a literal: `midpoint` puts it midway between two neighbours of the sorted long-double reference where their relative gap is at
least 1e-9, so membership never hangs on a rounding."""
import collections
import functools

import numpy as np

from map_update_cases import LD, N_SMALL, map_information, map_of, sym
from test_gpu_map_pair_priors import inv_ld, spd

N_SWEEP = 33                     # leading sub-maps 1 .. 33: across the pair kernel's blocks of 9 (od 7) and 7 (od 9) objects at B, B + 1, 2 B + 1 and beyond
N_EDGE = 258                    # the scatter's sweep of 256 candidates of a row: row 0 of 257 objects fills one exactly, of 258 objects starts a second
N_COPIES = 5
YAW_TURN = np.pi + 0.05
MASKS = ("all", "centre", "row", "no_yaw")
COPIES_SRC = np.array([0, 1, 2, 3, 4, 5, 2, 4])
COPIES_SINGULAR = [(2, 6), (4, 7)]


def mask_of(name, od):
    """row_mask of a named mask: 0 reads all rows; `row` is the single row 4, `no_yaw` all rows but row 3 (the yaw of the 7-parameter block)."""
    return {"all": 0, "centre": 0b111, "row": 1 << 4, "no_yaw": ((1 << od) - 1) & ~(1 << 3)}[name]


def mask_rows(mask, od):
    return [c for c in range(od) if ((mask or (1 << od) - 1) >> c) & 1]


def all_pairs(n):
    """(a [p], b [p]) of every pair a < b, in (a, b) order."""
    return np.triu_indices(n, 1)


# ---- the maps ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_sources(od):
    return np.sort(np.random.default_rng(700 + od).permutation(N_SMALL)[:N_COPIES])


@functools.lru_cache(maxsize=None)
def planted_map(od, yaw=False):
    """The small map grown by N_COPIES copies x_S + e, e ~ N(0, R_i) per copy, R_i = 1e-2 (A A^T + od I): cov = [[C, C[:, S]], [C[S, :], C_SS + R]]."""
    mean, cov = map_of("small", od)
    S = planted_sources(od)
    rng = np.random.default_rng(710 + od)
    rows = np.concatenate([np.arange(od * o, od * o + od) for o in S])
    R = np.zeros((len(rows), len(rows)))
    e = np.zeros((N_COPIES, od))
    for i in range(N_COPIES):
        A = rng.normal(size=(od, od))
        Ri = 1e-2 * (A @ A.T + od * np.eye(od))
        R[od * i:od * i + od, od * i:od * i + od] = Ri
        e[i] = np.linalg.cholesky(Ri) @ rng.normal(size=od)
    N = len(cov)
    big = np.zeros((N + len(rows), N + len(rows)))
    big[:N, :N] = cov
    big[:N, N:] = cov[:, rows]
    big[N:, :N] = cov[rows, :]
    big[N:, N:] = cov[np.ix_(rows, rows)] + R
    mu = np.concatenate([mean, mean[S] + e])
    if yaw:
        assert od == 7
        mu[N_SMALL + 2, 3] += YAW_TURN
    mu.setflags(write=False); big.setflags(write=False)
    return mu, big


def planted_pairs(od):
    return [(int(s), N_SMALL + i) for i, s in enumerate(planted_sources(od))]


def planted_labels(od):
    """The copies share their source's label; all other labels are distinct."""
    lab = np.arange(N_SMALL + N_COPIES, dtype=np.int32)
    lab[N_SMALL:] = planted_sources(od)
    return lab


@functools.lru_cache(maxsize=None)
def copies_map(od):
    rng = np.random.default_rng(720 + od)
    rows = np.concatenate([np.arange(od * o, od * o + od) for o in COPIES_SRC])
    Cr = spd(rng, 6 * od)
    mean, cov = rng.normal(size=(6, od))[COPIES_SRC], Cr[np.ix_(rows, rows)]
    mean.setflags(write=False); cov.setflags(write=False)
    return mean, cov


@functools.lru_cache(maxsize=None)
def sweep_map(od):
    """N_EDGE objects: row 0 of the leading sub-maps of N_EDGE - 1 and N_EDGE objects has exactly one 256-wide sweep of candidates, and one more than a sweep."""
    rng = np.random.default_rng(740 + od)
    mean, cov = rng.normal(size=(N_EDGE, od)), spd(rng, N_EDGE * od)
    mean.setflags(write=False); cov.setflags(write=False)
    return mean, cov


def case_map(name, od):
    if name in ("small", "large"):
        return map_of(name, od)
    if name == "sweep":
        return sweep_map(od)
    if name == "copies":
        return copies_map(od)
    return planted_map(od, yaw=(name == "planted_yaw"))


# ---- the formula ---------------------------------------------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "a b stat yaw singular dist")   # per pair, in (a, b) order: stat is NaN where the pair is singular


def singular_pairs(T):
    """The pivot rule of the entry on T [p][k][k] in fp64: a pivot of L that is not positive and finite, or p_min^2 <= 1e-13 p_max^2."""
    A = np.array(T, dtype=np.float64)
    p, k = A.shape[:2]
    bad, piv = np.zeros(p, bool), np.ones((p, k))
    with np.errstate(all="ignore"):
        for j in range(k):
            pj = A[:, j, j]
            ok = (pj > 0) & np.isfinite(pj)
            bad |= ~ok
            piv[:, j] = np.sqrt(np.where(ok, pj, 1.0))
            col = A[:, j + 1:, j] / piv[:, j, None]
            A[:, j + 1:, j + 1:] -= col[:, :, None] * col[:, None, :]
    return bad | ~(piv.min(axis=1) ** 2 > 1e-13 * piv.max(axis=1) ** 2)


def formula(mean, cov, od, mask=0, yaw_period=0.0, dtype=LD):
    """The entry's statistic of every pair, as the header states it.  Long double: inv_ld pair by pair; fp64: numpy's batched solve."""
    mu = np.asarray(mean, dtype=dtype).reshape(-1, od)
    n = len(mu)
    a, b = all_pairs(n)
    d = mu[b] - mu[a]
    w = np.zeros(len(a))
    if yaw_period > 0:                                            # the wrap is an fp64 number the entry reports: formed in fp64 whatever the rest is formed in
        m64 = np.asarray(mean, dtype=np.float64).reshape(-1, od)
        w = yaw_period * np.rint((m64[b, 3] - m64[a, 3]) / yaw_period)
        d[:, 3] = d[:, 3] - w.astype(dtype)
    blocks = sym(np.asarray(cov, dtype=dtype)).reshape(n, od, n, od).transpose(0, 2, 1, 3)
    T = blocks[b, b] - blocks[b, a] - blocks[a, b] + blocks[a, a]
    T = np.tril(T) + np.tril(T, -1).transpose(0, 2, 1)
    rows = mask_rows(mask, od)
    T, dm = T[:, rows][:, :, rows], d[:, rows]
    singular = singular_pairs(T) if len(a) else np.zeros(0, bool)
    stat = np.full(len(a), np.nan, dtype=dtype)
    good = np.flatnonzero(~singular)
    if dtype == np.float64:
        if len(good):
            stat[good] = np.einsum("pi,pi->p", dm[good], np.linalg.solve(T[good], dm[good][:, :, None])[:, :, 0])
    else:
        for i in good:
            stat[i] = dm[i] @ inv_ld(T[i]) @ dm[i]
    c = mu[b, :3] - mu[a, :3]
    dist = np.sqrt((c * c).sum(axis=1))
    return Reference(a, b, stat, np.asarray(w, dtype=np.float64), singular, dist)


@functools.lru_cache(maxsize=None)
def reference(name, od, mask_name="all", yaw_period=0.0):
    mean, cov = case_map(name, od)
    return formula(mean, cov, od, mask_of(mask_name, od), yaw_period)


def leading(ref, n):
    """The reference of the leading sub-map of n objects: the pairs with b < n, which keep their order."""
    sel = ref.b < n
    return Reference(*(x[sel] for x in ref))


def leading_map(mean, cov, n, od):
    return np.ascontiguousarray(mean[:n]), np.ascontiguousarray(cov[:n * od, :n * od])


def tested(ref, labels=None, max_centre_distance=np.inf):
    """[p] bool: the pairs the label and distance tests let through."""
    ok = np.ones(len(ref.a), bool)
    if labels is not None:
        lab = np.asarray(labels)
        ok &= (lab[ref.a] == lab[ref.b]) & (lab[ref.a] >= 0)
    if np.isfinite(max_centre_distance):
        ok &= ref.dist <= LD(max_centre_distance)
    return ok


def expected(ref, gate, labels=None, max_centre_distance=np.inf):
    """(found [p] bool, counts) of a call."""
    t = tested(ref, labels, max_centre_distance)
    found = t & ~ref.singular & (ref.stat <= LD(gate))
    return found, (int(found.sum()), int(t.sum()), int((t & ref.singular).sum()))


def midpoint(values, count):
    """(threshold, count): a threshold that exactly `count` of `values` do not exceed -- midway between the two neighbours of the sorted values (below the first:
    0; above the last: three times the last), moved up while their relative gap is under 1e-9.  NaNs are not values."""
    v = np.sort(np.asarray(values, dtype=LD)[~np.isnan(np.asarray(values, dtype=LD))])
    count = min(count, len(v))
    while True:
        below = v[count - 1] if count > 0 else LD(0)
        above = v[count] if count < len(v) else (3 * v[-1] if len(v) else LD(2))
        if above - below >= LD(1e-9) * above:
            return float(0.5 * (below + above)), count
        count += 1


def gates(ref):
    """Thresholds that report none, one, about twenty and all of the reference's pairs."""
    k = int((~np.isnan(ref.stat)).sum())
    return [midpoint(ref.stat, c)[0] for c in sorted({0, min(1, k), min(20, k), k})]


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------------------
def yardstick(mean, Lam, od, a, b, mask=0, w=0.0):
    """s of one pair as the constrained least squares of the module's docstring, long double, from the map's information Lam."""
    mu = np.asarray(mean, dtype=LD).ravel()
    N = len(mu)
    m = mask_rows(mask, od)
    ra, rb = [od * a + c for c in m], [od * b + c for c in m]
    keep = np.setdiff1d(np.arange(N), rb)
    col = np.full(N, -1)
    col[keep] = np.arange(len(keep))
    EtL = np.array(Lam[keep, :])                                  # E^T Lam: the rows of b fold into the rows of a
    for i in range(len(m)):
        EtL[col[ra[i]], :] += Lam[rb[i], :]
    M = np.array(EtL[:, keep])                                    # (E^T Lam) E: the same for the columns
    for i in range(len(m)):
        M[:, col[ra[i]]] += EtL[:, rb[i]]
    c = np.zeros(N, dtype=LD)
    if 3 in m:
        c[od * b + 3] = w
    rhs = EtL @ (mu - c)
    Mi = np.linalg.inv(M.astype(np.float64))
    z = (Mi @ rhs.astype(np.float64)).astype(LD)
    for _ in range(3):
        z = z + (Mi @ (rhs - M @ z).astype(np.float64)).astype(LD)
    assert np.abs(rhs - M @ z).max() <= 1e-15 * np.abs(rhs).max()
    x = np.zeros(N, dtype=LD)
    x[keep] = z
    x[rb] = z[col[ra]] + c[rb]
    r = x - mu
    return r @ (Lam @ r)


@functools.lru_cache(maxsize=None)
def yardstick_pairs(name, od):
    """Indices into all_pairs(n) of the pairs the yardstick is evaluated on: all of the small map, a seeded sample of 40 of the large one."""
    n = len(map_of(name, od)[0])
    p = n * (n - 1) // 2
    return np.arange(p) if name == "small" else np.sort(np.random.default_rng(730 + od).permutation(p)[:40])


@functools.lru_cache(maxsize=None)
def yardstick_reference(name, od, mask_name):
    mean, _ = map_of(name, od)
    Lam = map_information(name, od)
    a, b = all_pairs(len(mean))
    idx = yardstick_pairs(name, od)
    return np.array([yardstick(mean, Lam, od, int(a[i]), int(b[i]), mask_of(mask_name, od)) for i in idx], dtype=LD)
