"""Inputs and references of the tests of the entry that locates one device-resident map in another (include/obvi_map_locate.h): shared by
tests/test_map_locate_abi.py (CPU: the reference is itself held) and tests/test_gpu_map_locate.py (the device against the reference).  Nothing here touches the
product.

Maps.  A is the 24-object map of tests/map_update_cases.py (and its leading 12 objects for the small exhaustive cases; the 70-object map for one planted
case) with its centres re-spread on a seeded square (20 m; 40 m for the 70 objects) and z in [0, 3] m, and its covariance scaled so that the mean centre sigma is
3 cm: baselines differ by far more than the centres are uncertain.  B holds 8 of A's first 12 objects seen from T_A<-B = (-4, 2.5, 0.3, -1.1), each estimate
drawn with the independent noise of an spd covariance with eigenvalues 1e-4 .. 1e-2, and 4 objects only B has.  Labels: none; four seeded classes; one class
an object (B's own objects carry classes A does not have).  Every leading sub-map of B with 1 .. 10 objects.  A symmetric constellation: four objects of one
label on a 4 m square whose heights differ by centimetres and whose height variances differ, B's centres = A's -- with only the diagonals long enough for a seed there are 8 seeds, every one with all four
objects as inliers, and those that give bit-identical transforms (the identity twice, the half turn twice) tie exactly in cost: the planted ties.

Reference (`evaluate`, dtype long double): the definition of the header, hypothesis by hypothesis, vectorised over hypotheses; the same code with dtype float64
is numpy's fp64 evaluation.  tests/test_map_locate_abi.py holds it against a plain-Python restatement.

Yardstick of the refinement (`newton`): the minimiser of sum e^T S(psi)^-1 e over the hypothesis's inliers, partners fixed, found by Newton steps in long
double on the FULL objective -- S's dependence on psi included, derivatives by central differences -- started from the true transform.  It shares no step with
the Gauss-Newton iteration.  Gauss-Newton's fixed point is not that minimiser: it drops d S / d psi from the gradient.  The bar on their difference is
therefore derived, not fitted (`gauss_newton_gap`): to first order the fixed point is off by (Hessian / 2)^-1 (0 0 0 q), q = 1/2 sum e^T S^-1 S' S^-1 e, and
twice that first-order figure (room for the second order) plus 1e-9 is the bar.  The covariance is compared with the inverse of the central-difference
Hessian / 2: the Gauss-Newton matrix leaves out the terms of the Hessian that are linear in the residuals, which are of the order of the whitened residual over
the whitened lever arm; the bar is `hessian_gap`, twice the largest |y_i| / |L_i^-1 Rz' p_b|.

Thresholds are never literals: `thresholds` puts pair_min_distance, pair_tolerance and the gate midway into the gap of the deciding quantities that lies at
the wanted value (or, for pair_tolerance, behind a wanted number of compatible seeds), and `conditions` asserts, on the CPU, that no deciding quantity lies
within 1e-9 relative of its threshold, that no object has two partners within 1e-9, and that no two hypotheses that qualify and have equal inliers have costs
within 1e-9 relative unless their transforms are bit-identical (the planted ties)."""
import collections
import functools

import numpy as np

from map_update_cases import LD, map_of, sym
from test_gpu_map_pair_priors import spd

T_TRUE = np.array([-4.0, 2.5, 0.3, -1.1])          # T_A<-B
N_SHARED, N_EXTRA = 8, 4
LABELLINGS = ("none", "classes", "objects")
MIN_INLIERS = 3
Case = collections.namedtuple("Case", "name od mean_a cov_a mean_b cov_b label_a label_b shared truth_extra")
Params = collections.namedtuple("Params", "dmin tol gate min_inliers")
Result = collections.namedtuple("Result", "counts seeds hyp T0 inliers cost partner order margins")


def rz(psi, dtype):
    c, s = np.cos(dtype(psi)), np.sin(dtype(psi))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=dtype)


# ---- the maps ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def map_a(od, n):
    """(mean [n][od], cov): the 24- or 70-object map, centres re-spread, covariance scaled.  n = 12: the leading sub-map of the 24."""
    if n == 12:
        mean, cov = map_a(od, 24)
        return np.ascontiguousarray(mean[:12]), np.ascontiguousarray(cov[:12 * od, :12 * od])
    mean, cov = map_of("small" if n == 24 else "large", od)
    rng = np.random.default_rng(900 + od + n)
    side = 20.0 if n == 24 else 40.0
    mean = np.array(mean)
    mean[:, :2] = rng.uniform(-side / 2, side / 2, size=(n, 2))
    mean[:, 2] = rng.uniform(0.0, 3.0, size=n)
    centre = np.concatenate([np.arange(od * o, od * o + 3) for o in range(n)])
    cov = np.array(cov) * (0.03 ** 2 / np.diag(cov)[centre].mean())
    assert np.abs(cov - cov.T).max() > 0
    mean.setflags(write=False); cov.setflags(write=False)
    return mean, cov


@functools.lru_cache(maxsize=None)
def map_b(od, n):
    """(mean_b [12][od], cov_b, shared [8], truth_extra [4][3]) for A = map_a(od, n): the shared objects come first, in ascending order of their A numbers."""
    mean_a, _ = map_a(od, n)
    rng = np.random.default_rng(940 + od + n)
    shared = np.sort(rng.permutation(12)[:N_SHARED])
    side = 20.0 if n <= 24 else 40.0
    truth_extra = np.column_stack([rng.uniform(-side / 2, side / 2, size=(N_EXTRA, 2)), rng.uniform(0.0, 3.0, size=N_EXTRA)])
    nb = N_SHARED + N_EXTRA
    truth = rng.normal(size=(nb, od))
    truth[:N_SHARED, 3:] = mean_a[shared, 3:]
    if od == 7:
        truth[:N_SHARED, 3] -= T_TRUE[3]                                             # the yaw as B's frame sees it (the chain matches whole blocks)
    truth[:, :3] = (np.concatenate([mean_a[shared, :3], truth_extra]) - T_TRUE[:3]) @ rz(T_TRUE[3], np.float64)      # Rz(-psi) (p - t), row by row
    R = rng.normal(size=(nb * od, nb * od))
    cov_b = spd(rng, nb * od, cond=1e2, scale=1e-4)
    mean_b = truth + (np.linalg.cholesky(cov_b) @ rng.normal(size=nb * od)).reshape(nb, od)
    cov_b = cov_b + 1e-6 * (R - R.T)
    for x in (mean_b, cov_b, shared, truth_extra):
        x.setflags(write=False)
    return mean_b, cov_b, shared, truth_extra


@functools.lru_cache(maxsize=None)
def case(od, n_a, labelling, n_b=N_SHARED + N_EXTRA):
    mean_a, cov_a = map_a(od, n_a)
    mean_b, cov_b, shared, extra = map_b(od, 24 if n_a == 12 else n_a)
    rng = np.random.default_rng(970 + n_a)
    if labelling == "none":
        la = lb = None
    elif labelling == "classes":
        la = rng.integers(0, 4, size=n_a).astype(np.int32)
        lb = np.concatenate([la[shared], rng.integers(0, 4, size=N_EXTRA)]).astype(np.int32)
    else:
        la = np.arange(n_a, dtype=np.int32)
        lb = np.concatenate([shared, 1000 + np.arange(N_EXTRA)]).astype(np.int32)
    if lb is not None:
        lb = lb[:n_b]
    return Case("%d x %d, od %d, labels: %s" % (n_a, n_b, od, labelling), od, mean_a, cov_a, np.ascontiguousarray(mean_b[:n_b]),
                np.ascontiguousarray(cov_b[:n_b * od, :n_b * od]), la, lb, shared, extra)


@functools.lru_cache(maxsize=None)
def square():
    od = 7
    mean = np.zeros((4, od))
    mean[:, :3] = [[0, 0, 0.0], [4, 0, 0.02], [4, 4, 0.05], [0, 4, 0.09]]
    cov, cov_b = 0.0025 * np.eye(4 * od), 0.0025 * np.eye(4 * od)
    for o in range(4):                                                  # unequal height variances, and not the same in B: without them the quarter turns' costs are equal in exact arithmetic only
        cov[od * o + 2, od * o + 2] *= (1.0, 2.0, 3.0, 5.0)[o]
        cov_b[od * o + 2, od * o + 2] *= (7.0, 1.0, 4.0, 2.0)[o]
    mean.setflags(write=False); cov.setflags(write=False); cov_b.setflags(write=False)
    return Case("the square", od, mean, cov, mean, cov_b, None, None, np.arange(4), np.zeros((0, 3)))


# ---- the definition of the header, in any float type -------------------------------------------------------------------------------------------------------
def records(mean, cov, od, dtype):
    """(centres [n][3], blocks [n][3][3]) of a map, symmetrised entry by entry."""
    n = len(mean)
    Cs = sym(np.asarray(cov, dtype=dtype))
    return np.asarray(mean, dtype=dtype)[:, :3].copy(), np.array([Cs[od * o:od * o + 3, od * o:od * o + 3] for o in range(n)], dtype=dtype).reshape(n, 3, 3)


def all_seeds(na, nb):
    """[seeds][4] in lexicographic order of (a1 < a2, b1 != b2)."""
    a1, a2 = np.triu_indices(na, 1)
    b1, b2 = np.divmod(np.arange(nb * nb), nb)
    keep = b1 != b2
    b1, b2 = b1[keep], b2[keep]
    return np.column_stack([np.repeat(a1, len(b1)), np.repeat(a2, len(b1)), np.tile(b1, len(a1)), np.tile(b2, len(a1))]).astype(np.int64).reshape(-1, 4)


def seed_quantities(c, dtype):
    """(seeds, tested, |u|, |v|, | |u| - |v| |, |dz_A - dz_B|) over every seed."""
    pa, _ = records(c.mean_a, c.cov_a, c.od, dtype)
    pb, _ = records(c.mean_b, c.cov_b, c.od, dtype)
    sd = all_seeds(len(pa), len(pb))
    la = np.zeros(len(pa), np.int64) if c.label_a is None else np.asarray(c.label_a, np.int64)
    lb = np.zeros(len(pb), np.int64) if c.label_b is None else np.asarray(c.label_b, np.int64)
    a1, a2, b1, b2 = sd.T
    tested = (la[a1] >= 0) & (la[a1] == lb[b1]) & (la[a2] >= 0) & (la[a2] == lb[b2])
    u, v = pa[a2, :2] - pa[a1, :2], pb[b2, :2] - pb[b1, :2]
    nu, nv = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]), np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
    dz = np.abs((pa[a2, 2] - pa[a1, 2]) - (pb[b2, 2] - pb[b1, 2]))
    return sd, tested, nu, nv, np.abs(nu - nv), dz


def hypotheses(c, sd, dtype):
    """T [h][4] of the seeds sd."""
    pa, _ = records(c.mean_a, c.cov_a, c.od, dtype)
    pb, _ = records(c.mean_b, c.cov_b, c.od, dtype)
    a1, a2, b1, b2 = sd.T
    u, v = pa[a2, :2] - pa[a1, :2], pb[b2, :2] - pb[b1, :2]
    psi = np.arctan2(v[:, 0] * u[:, 1] - v[:, 1] * u[:, 0], v[:, 0] * u[:, 0] + v[:, 1] * u[:, 1])
    cs, sn = np.cos(psi), np.sin(psi)
    ma, mb = (pa[a1] + pa[a2]) / 2, (pb[b1] + pb[b2]) / 2
    return np.column_stack([ma[:, 0] - (cs * mb[:, 0] - sn * mb[:, 1]), ma[:, 1] - (sn * mb[:, 0] + cs * mb[:, 1]), ma[:, 2] - mb[:, 2], psi]).astype(dtype).reshape(-1, 4)


def pair_statistics(c, T, dtype):
    """s [h][nb][na] of the transforms T: +inf where the labels differ or the pair is singular."""
    pa, A = records(c.mean_a, c.cov_a, c.od, dtype)
    pb, B = records(c.mean_b, c.cov_b, c.od, dtype)
    la = np.zeros(len(pa), np.int64) if c.label_a is None else np.asarray(c.label_a, np.int64)
    lb = np.zeros(len(pb), np.int64) if c.label_b is None else np.asarray(c.label_b, np.int64)
    out = np.full((len(T), len(pb), len(pa)), np.inf, dtype=dtype)
    for h0 in range(0, len(T), 128):
        t = T[h0:h0 + 128]
        cs, sn = np.cos(t[:, 3]), np.sin(t[:, 3])
        R = np.zeros((len(t), 3, 3), dtype=dtype)
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = cs, -sn, sn, cs, 1
        moved = np.einsum("hij,bj->hbi", R, pb) + t[:, None, :3]
        RB = np.einsum("hij,bjk,hlk->hbil", R, B, R)
        e = pa[None, None] - moved[:, :, None]                                       # [h][nb][na][3]
        S = A[None, None] + RB[:, :, None]                                           # [h][nb][na][3][3]
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = np.ones(S.shape[:3], bool)
            d = []
            p0 = S[..., 0, 0]
            ok &= (p0 > 0) & np.isfinite(p0)
            d.append(np.sqrt(np.where(ok, p0, 1)))
            l10, l20 = S[..., 1, 0] / d[0], S[..., 2, 0] / d[0]
            p1 = S[..., 1, 1] - l10 * l10
            g1 = (p1 > 0) & np.isfinite(p1)
            d.append(np.sqrt(np.where(g1, p1, 1)))
            l21 = (S[..., 2, 1] - l20 * l10) / d[1]
            p2 = (S[..., 2, 2] - l20 * l20) - l21 * l21
            g2 = (p2 > 0) & np.isfinite(p2)
            d.append(np.sqrt(np.where(g2, p2, 1)))
            pmin, pmax = np.minimum(np.minimum(d[0], d[1]), d[2]), np.maximum(np.maximum(d[0], d[1]), d[2])
            ok &= g1 & g2 & (pmin * pmin > dtype(1e-13) * pmax * pmax)
            y0 = e[..., 0] / d[0]
            y1 = (e[..., 1] - l10 * y0) / d[1]
            y2 = ((e[..., 2] - l20 * y0) - l21 * y1) / d[2]
            s = (y0 * y0 + y1 * y1) + y2 * y2
        ok &= (lb[None, :, None] >= 0) & (lb[None, :, None] == la[None, None, :])
        out[h0:h0 + 128] = np.where(ok, s, np.inf)
    return out


def evaluate(c, p, dtype=LD):
    """Everything up to the ranking, in `dtype`.  order: the qualifying hypotheses' numbers (positions among the compatible seeds), best first."""
    sd, tested, nu, nv, dn, dz = seed_quantities(c, dtype)
    base = tested & (nu >= dtype(p.dmin)) & (nv >= dtype(p.dmin))
    compatible = base & (dn <= dtype(p.tol)) & (dz <= dtype(p.tol))
    hyp = np.flatnonzero(compatible)
    T = hypotheses(c, sd[hyp], dtype)
    s = pair_statistics(c, T, dtype)
    nb = s.shape[1] if len(T) else len(c.mean_b)
    if len(T):
        partner = np.argmin(s, axis=2)                                               # the smallest a on ties
        best = np.take_along_axis(s, partner[..., None], axis=2)[..., 0]
    else:
        partner, best = np.zeros((0, nb), np.int64), np.zeros((0, nb), dtype)
    inlier = best <= dtype(p.gate)
    partner = np.where(inlier, partner, -1).astype(np.int32)
    inliers = inlier.sum(axis=1).astype(np.int32)
    cost = np.zeros(len(T), dtype=dtype)
    for b in range(nb):                                                              # ascending b
        cost = cost + np.where(inlier[:, b], best[:, b], 0)
    qualify = np.flatnonzero(inliers >= p.min_inliers)
    order = qualify[np.lexsort((qualify, cost[qualify], -inliers[qualify]))]
    counts = (int(tested.sum()), int(compatible.sum()), len(qualify))
    second = np.sort(s, axis=2)[..., :2] if len(T) and s.shape[2] > 1 else None
    margins = dict(nu=nu[tested], nv=nv[tested], dn=dn[base], dz=dz[base], best=best, second=second)
    return Result(counts, sd[hyp], hyp, T, inliers, cost, partner, order, margins)


def normal_equations(c, T, partner, dtype):
    """(H [4][4], g [4], per-inlier (y, whitened Rz' p_b)) of one hypothesis at T with its partner row."""
    pa, A = records(c.mean_a, c.cov_a, c.od, dtype)
    pb, B = records(c.mean_b, c.cov_b, c.od, dtype)
    R = rz(T[3], dtype)
    cs, sn = R[0, 0], R[1, 0]
    H, g, parts = np.zeros((4, 4), dtype=dtype), np.zeros(4, dtype=dtype), []
    for b in np.flatnonzero(np.asarray(partner) >= 0):
        a = partner[b]
        S = A[a] + R @ B[b] @ R.T
        L = np.linalg.cholesky(S.astype(np.float64)).astype(dtype) if dtype == np.float64 else chol3(S)
        G = np.zeros((3, 4), dtype=dtype)
        G[:, :3] = np.eye(3, dtype=dtype)
        G[:, 3] = [-sn * pb[b, 0] - cs * pb[b, 1], cs * pb[b, 0] - sn * pb[b, 1], 0]
        e = pa[a] - (R @ pb[b] + T[:3])
        Z, y = forward(L, G), forward(L, e[:, None])[:, 0]
        H += Z.T @ Z
        g += Z.T @ y
        parts.append((y, Z[:, 3]))
    return H, g, parts


def chol3(S):
    L = np.zeros((3, 3), dtype=S.dtype)
    for j in range(3):
        L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, 3):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def forward(L, M):
    X = np.zeros_like(M)
    for i in range(len(L)):
        X[i] = (M[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def inv_spd(H):
    """H^-1 of a small SPD matrix by its Cholesky factor, in H's type."""
    n = len(H)
    L = np.zeros_like(H)
    for j in range(n):
        L[j, j] = np.sqrt(H[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    W = forward(L, np.eye(n, dtype=H.dtype))
    return W.T @ W


def refine(c, T0, partner, iterations, dtype=LD):
    """(T [4], cov [4][4]): the Gauss-Newton steps of the header."""
    T = np.array(T0, dtype=dtype)
    for it in range(iterations + 1):
        H, g, _ = normal_equations(c, T, partner, dtype)
        Hi = inv_spd(H)
        if it < iterations:
            T = T + Hi @ g
    return T, Hi


def report(c, p, iterations, capacity=None, dtype=LD):
    """(Result, k, T [k][4], cov [k][4][4]) of the first `capacity` (None: all) ranked hypotheses."""
    r = evaluate(c, p, dtype)
    k = len(r.order) if capacity is None else min(capacity, len(r.order))
    out = [refine(c, r.T0[h], r.partner[h], iterations, dtype) for h in r.order[:k]]
    return r, k, np.array([o[0] for o in out], dtype=dtype).reshape(k, 4), np.array([o[1] for o in out], dtype=dtype).reshape(k, 4, 4)


# ---- the yardstick of the refinement ---------------------------------------------------------------------------------------------------------------------------
def objective(c, T, partner):
    _, _, parts = normal_equations(c, np.asarray(T, dtype=LD), partner, LD)
    return sum((y @ y for y, _ in parts), LD(0))


def derivatives(f, x, h):
    """(gradient, Hessian) of f at x by central differences, long double."""
    n = len(x)
    E = np.eye(n, dtype=LD) * h
    g = np.array([(f(x + E[i]) - f(x - E[i])) / (2 * h) for i in range(n)], dtype=LD)
    Hs = np.zeros((n, n), dtype=LD)
    f0 = f(x)
    for i in range(n):
        Hs[i, i] = (f(x + E[i]) - 2 * f0 + f(x - E[i])) / (h * h)
        for j in range(i):
            Hs[i, j] = Hs[j, i] = (f(x + E[i] + E[j]) - f(x + E[i] - E[j]) - f(x - E[i] + E[j]) + f(x - E[i] - E[j])) / (4 * h * h)
    return g, Hs


def newton(c, partner, start=T_TRUE, steps=8):
    """(T*, (Hessian / 2)^-1 at T*): the minimiser of the full objective.  h = 1e-5: truncation 1e-10 of the derivatives' own size, long-double round-off below."""
    f = functools.partial(objective, c, partner=partner)
    x = np.asarray(start, dtype=LD)
    for _ in range(steps):
        g, Hs = derivatives(lambda t: f(t), x, LD(1e-5))
        x = x - np.linalg.solve(Hs.astype(np.float64), g.astype(np.float64)).astype(LD)
    g, Hs = derivatives(lambda t: f(t), x, LD(1e-5))
    return x, inv_spd(Hs / 2), float(np.abs(g).max())


def gauss_newton_gap(c, T_star, cov_star, partner):
    """The first-order distance of Gauss-Newton's fixed point from the minimiser T*, per component: |cov* (0 0 0 q)|, q = 1/2 sum e^T S^-1 S' S^-1 e."""
    pa, A = records(c.mean_a, c.cov_a, c.od, LD)
    pb, B = records(c.mean_b, c.cov_b, c.od, LD)
    R = rz(T_star[3], LD)
    dR = np.array([[-R[1, 0], -R[0, 0], 0], [R[0, 0], -R[1, 0], 0], [0, 0, 0]], dtype=LD)
    q = LD(0)
    for b in np.flatnonzero(np.asarray(partner) >= 0):
        a = partner[b]
        S = A[a] + R @ B[b] @ R.T
        dS = dR @ B[b] @ R.T + R @ B[b] @ dR.T
        w = np.linalg.solve(S.astype(np.float64), (pa[a] - (R @ pb[b] + T_star[:3])).astype(np.float64)).astype(LD)
        q += w @ dS @ w / 2
    return np.abs(cov_star[:, 3] * q)


def hessian_gap(c, T_star, partner):
    """Twice the largest whitened residual over its whitened lever arm: the relative size of what the Gauss-Newton matrix leaves out of the Hessian / 2."""
    _, _, parts = normal_equations(c, np.asarray(T_star, dtype=LD), partner, LD)
    return 2 * max(float(np.sqrt(y @ y) / np.sqrt(z @ z)) for y, z in parts)


# ---- thresholds, and the conditions on the inputs ----------------------------------------------------------------------------------------------------------
def gap_mid(values, target):
    """The middle of the gap of `values` that holds `target` (below all: half the first; above all: the last and a half)."""
    v = np.unique(np.asarray(values, dtype=LD)[np.isfinite(np.asarray(values, dtype=LD))])
    i = int(np.searchsorted(v, LD(target)))
    below = v[i - 1] if i > 0 else LD(0)
    above = v[i] if i < len(v) else (below * 3 if i > 0 else LD(2 * target))
    return float((below + above) / 2)


def nth_mid(values, count):
    """A threshold that exactly `count` of `values` do not exceed: midway between the two neighbours."""
    v = np.sort(np.asarray(values, dtype=LD))
    assert 0 < count < len(v) and v[count] > v[count - 1], (count, len(v))
    return float((v[count - 1] + v[count]) / 2)


_THRESHOLDS = {}


def thresholds(c, dmin=2.0, tol=0.25, gate=16.0, n_compatible=None, min_inliers=MIN_INLIERS):
    key = (c.name, dmin, tol, gate, n_compatible, min_inliers)
    if key not in _THRESHOLDS:
        _THRESHOLDS[key] = _thresholds(c, dmin, tol, gate, n_compatible, min_inliers)
    return _THRESHOLDS[key]


def _thresholds(c, dmin, tol, gate, n_compatible, min_inliers):
    sd, tested, nu, nv, dn, dz = seed_quantities(c, LD)
    dmin = gap_mid(np.concatenate([nu, nv]), dmin)
    base = tested & (nu >= dmin) & (nv >= dmin)
    worst = np.maximum(dn, dz)[base]
    tol = gap_mid(worst, tol) if n_compatible is None else nth_mid(worst, n_compatible)
    r = evaluate(c, Params(dmin, tol, 1.0, min_inliers), LD)
    gate = gap_mid(r.margins["best"].ravel(), gate) if r.margins["best"].size else gate
    return Params(dmin, tol, gate, min_inliers)


def apart(values, threshold, rel=1e-9):
    v = np.asarray(values, dtype=LD).ravel()
    v = v[np.isfinite(v)]
    return bool((np.abs(v - LD(threshold)) > LD(rel) * LD(threshold)).all())


def conditions(c, p, r=None):
    """The conditions on the inputs of the module's docstring; returns the planted ties: pairs of adjacent ranks whose transforms are bit-identical."""
    r = evaluate(c, p, LD) if r is None else r
    m = r.margins
    assert apart(m["nu"], p.dmin) and apart(m["nv"], p.dmin) and apart(m["dn"], p.tol) and apart(m["dz"], p.tol) and apart(m["best"], p.gate), c.name
    if m["second"] is not None:
        s1, s2 = m["second"][..., 0], m["second"][..., 1]
        with np.errstate(invalid="ignore"):
            close = np.isfinite(s2) & (s1 <= p.gate) & ~(s2 - s1 > LD(1e-9) * s2)
        assert not close.any(), c.name
    ties = []
    for i, j in zip(r.order[:-1], r.order[1:]):
        if r.inliers[i] == r.inliers[j] and not abs(r.cost[j] - r.cost[i]) > LD(1e-9) * max(r.cost[i], r.cost[j]):
            assert np.array_equal(r.T0[i], r.T0[j]), (c.name, i, j)
            ties.append((int(i), int(j)))
    return ties


def errors(cost, T, cov, cost_ref, T_ref, cov_ref, cost_scale=None):
    """(cost, transform, covariance): per hypothesis the largest difference over the largest entry of the reference -- for the transform at least 1 -- (cost_scale: over that instead, where a
    reference cost is zero by construction); the worst hypothesis."""
    if len(cost_ref) == 0:
        return 0.0, 0.0, 0.0
    ec = np.abs(np.asarray(cost, dtype=LD) - cost_ref) / (np.abs(cost_ref) if cost_scale is None else LD(cost_scale))
    et = np.abs(np.asarray(T, dtype=LD) - T_ref).max(axis=1) / np.maximum(np.abs(T_ref).max(axis=1), 1)       # (the square's identity is all zeros)
    ev = np.abs(np.asarray(cov, dtype=LD) - cov_ref).reshape(len(cov_ref), -1).max(axis=1) / np.abs(cov_ref).reshape(len(cov_ref), -1).max(axis=1)
    return float(ec.max()), float(et.max()), float(ev.max())


# (od, n_a, labelling) of the exhaustive cases
EXHAUSTIVE = [(od, n_a, lab) for od in (7, 9) for n_a in (12, 24) for lab in LABELLINGS]


def square_thresholds():
    return thresholds(square(), dmin=5.0, tol=0.5)


# numpy's fp64 evaluation of the definition against the long-double one, the worst figure over every case (tests/test_map_locate_abi.py measures and holds it);
# the GPU bar is three orders over it, the rule of tests/test_gpu_map_match.py
FP64_WORST = 4e-14   # measured: cost 3.44e-14, transform 3.80e-16, covariance 1.57e-15
GPU_BAR = 1e3 * FP64_WORST


# ---- the chain: locate, move, join, match, resolve, merge ------------------------------------------------------------------------------------------------------
WIDE_SIGMA = np.diag([1e-2, 1e-2, 1e-2, 1e-4])       # 10 cm and 0.01 rad (10 cm at 10 m): several times the located transform's own sigmas, so the merge decides, and
                                                     # well under the metres that separate neighbouring objects, so the match still tells them apart


@functools.lru_cache(maxsize=None)
def chain():
    """(case, thresholds, the Chain of tests/map_frame_cases.py with the LOCATED transform as T_est, its long-double reference): nobody supplies a transform."""
    import map_frame_cases as frame
    c = case(7, 24, "classes")
    p = thresholds(c)
    r, k, T, cov = report(c, p, 3, capacity=1)
    extra = np.zeros((N_EXTRA, c.od))
    extra[:, :3] = c.truth_extra
    ch = frame.Chain(c.od, c.mean_a, c.cov_a, c.mean_b, c.cov_b, c.shared, extra, T_TRUE, T[0].astype(np.float64), WIDE_SIGMA)
    return c, p, ch, frame.run_chain(ch)
