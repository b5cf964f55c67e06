"""Designed cases for the tile Cholesky solve of an LM step (chol_kernels.hip: k_potrf, k_trsm, k_update, k_update_potrf, k_backward, k_backward_det), the
reference they are judged by and the metric.  CPU only; touches nothing in the product.

Metric.  For a system S y = b in the order of the tile grid (real rows only; padding rows are identity and decoupled), L* the Cholesky factor of S by a plain
column loop in numpy.longdouble:

    omega(y) = max_i |S y - b|_i / ((|L*| |L*^T|) |y| + |b|)_i          (everything in long double)

the componentwise backward error in the form of Higham's bound for a Cholesky solve, |dA| <= gamma_{3m+1} |L| |L^T| (Accuracy and Stability of Numerical
Algorithms, 2nd ed., theorem 10.4).

Bar.  max((3 m + 1) 2^-53, 8 omega(y_emu)), y_emu from emulate(): this project's algorithm in numpy float64 on the same S, b -- 64 x 64 tiles with padding
rows as identity, L_ik = S_ik inv(L_kk)^T through an explicit inverse, updates and right-hand side tile by tile, backward substitution through inv(L_kk)^T.
The first term is derived; the second is there because multiplying by explicit inverses is not backward stable in the textbook sense (its error grows with
the condition of a diagonal tile's factor, and the emulation carries that dependence); the factor 8 is the allowance for the device's other summation order
(MFMA k-blocks of 4, sliced products, atomics over at most 64 nt terms).  The bar is never taken from the device's own value.

Cases (CASES; each declares in `expect` the structure it must reach, which the GPU test reads back from obvi_ba_get_problem_stats):

  pad57    6 variable poses + 3 objects: one tile with 7 padding rows (k_potrf alone; the look-ahead loop ends on a padded panel)
  full64   6 poses + 4 objects: one tile, no padding row
  over65   5 poses + 5 objects: a second tile with one real row and 63 padding rows; a 7-row block across the tile edge
  od9_63   6 poses + 3 objects of 9: the other block size, one tile with one padding row
  od9_72   6 poses + 4 objects of 9: a 9-row block across the tile edge
  wide     44 variable poses + 8 objects in ONE dissection leaf (default OBVI_ND_LEAF): 320 rows, five full tiles, a dense chain of levels inside one node,
           several products per update target (OBVI_UPD_CHUNK 1 / 2, OBVI_PRE_MAX 0 / 2 / 8)
  deep     24 variable poses under OBVI_ND_LEAF=4 / OBVI_ND_G=1, every feature seen from two consecutive frames only (both cameras), objects seen from two or
           three neighbouring frames and two objects seen from both ends of the trajectory: every node starts on a tile boundary, so tiles of 6 to 24 real
           rows and 40 or more padding rows, four or more levels, ancestor tiles that do not exist (presence bits clear), objects on separators and in the
           root: four levels, so with OBVI_BACKWARD_LEVELS 1 / 3 / 4 / 8 the chains of k_backward are 0 to 3 long (prefetch path)
  deeper   the same problem under OBVI_ND_LEAF=2: five or more levels, so that a leaf has four or more ancestors and, with OBVI_BACKWARD_LEVELS 8 (the
           default of a tree this shallow), walks them on the long path of k_backward (chains of 4 - 7)"""
import functools

import numpy as np

import synth

LD = np.longdouble
TILE = 64
RADII = (100.0, 1e300)
U = 2.0 ** -53
REJECT_POS = (0, 1, 2, 3, 4, 59, 60, 63)      # 0-3: the four roles p, det, p2, det2 of a 4 x 4 block (potrf_factor_block)

# stats of obvi_ba_get_problem_stats a case must reach ("min_*": at least); filled from the plan these problems get (plan.cpp is deterministic)
EXPECT = {
    "pad57": dict(reduced_rows=57, tiles_per_dim=1, tiles_nonzero=1, trsm_jobs=0, update_jobs=0, chol_levels=1),
    "full64": dict(reduced_rows=64, tiles_per_dim=1, tiles_nonzero=1, trsm_jobs=0, update_jobs=0, chol_levels=1),
    "over65": dict(reduced_rows=65, tiles_per_dim=2, tiles_nonzero=3, trsm_jobs=1, update_jobs=1, chol_levels=2),
    "od9_63": dict(reduced_rows=63, tiles_per_dim=1, tiles_nonzero=1, trsm_jobs=0, update_jobs=0, chol_levels=1),
    "od9_72": dict(reduced_rows=72, tiles_per_dim=2, tiles_nonzero=3, trsm_jobs=1, update_jobs=1, chol_levels=2),
    "wide": dict(reduced_rows=320, tiles_per_dim=5, tiles_nonzero=15, trsm_jobs=10, update_jobs=20, chol_levels=5),
    "deep": dict(reduced_rows=207, tiles_per_dim=15, tiles_nonzero=41, trsm_jobs=26, update_jobs=38, chol_levels=4),
    "deeper": dict(reduced_rows=207, tiles_per_dim=17, tiles_nonzero=47, trsm_jobs=30, update_jobs=44, chol_levels=5),
}
KNOBS = {"deep": {"OBVI_ND_LEAF": "4", "OBVI_ND_G": "1"}, "deeper": {"OBVI_ND_LEAF": "2", "OBVI_ND_G": "1"}}
MULTI_TILE = ("over65", "od9_72", "wide", "deep", "deeper")
SAME_PROBLEM = {"deeper": "deep"}             # cases that differ in the handle's knobs only: one system on the CPU


# ------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------
def _problem(P, O, od, seed, L, **kw):
    prob = synth.make_problem(P=P, L=L, O=O, seed=seed, const_poses=1, min_obj_obs=2, object_classes=("bench",), bbox_noise=5.0, **kw)
    assert len(prob["objects"]) == O
    return prob


def _finish(name, prob, od):
    if od == 9:
        prob = synth.nine_dof(prob, tilt=0.1, seed=7)
    var_pose = prob["pose_const"] == 0
    assert np.all(np.bincount(prob["rp_pose"], minlength=len(var_pose))[var_pose] > 0)
    assert np.all(np.bincount(prob["bb_obj"][var_pose[prob["bb_pose"]]], minlength=len(prob["objects"])) >= 1), "an object no variable pose sees"
    m = 6 * int(var_pose.sum()) + od * len(prob["objects"])
    return dict(name=name, od=od, prob=prob, m=m, knobs=KNOBS.get(name, {}), expect=EXPECT[name])


def _deep(name="deep"):
    """make_problem's scene, its incidence cut down by hand (the values stay measurements of the same scene)"""
    prob = _problem(25, 9, 7, 31, 900, stereo=True)
    P = 25
    # features: the two consecutive frames of the track picked by the feature's id
    keep = np.zeros(len(prob["rp_pose"]), bool)
    pt, fr = prob["rp_point"].astype(np.int64), prob["rp_pose"].astype(np.int64)
    for l in range(len(prob["points"])):
        idx = np.flatnonzero(pt == l)
        frames = np.unique(fr[idx])
        pairs = [f for f in frames if f + 1 in frames]
        if not pairs:
            continue
        f0 = pairs[l % len(pairs)]
        keep[idx[(fr[idx] == f0) | (fr[idx] == f0 + 1)]] = True
    for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_is_outlier"):
        prob[k] = prob[k][keep]
    seen = np.bincount(prob["rp_point"], minlength=len(prob["points"]))
    assert (np.bincount(prob["rp_pose"], minlength=P)[1:] >= 8).all()
    prob["point_const"] = (seen == 0).astype(np.uint8)      # (a feature that lost its track: constant and unused)
    # objects: two or three neighbouring frames; the two seen from most frames keep their first and last one
    bo, bp = prob["bb_obj"].astype(np.int64), prob["bb_pose"].astype(np.int64)
    spans = [np.flatnonzero((bo == o) & (bp >= 1)) for o in range(9)]
    wide2 = sorted(range(9), key=lambda o: -(bp[spans[o]].max() - bp[spans[o]].min()))[:2]
    keepb = np.zeros(len(bo), bool)
    for o in range(9):
        idx = spans[o][np.argsort(bp[spans[o]])]
        if o in wide2:
            keepb[idx[[0, 1, -2, -1]]] = True
            assert bp[idx[-1]] - bp[idx[0]] >= 16, "no object seen from both ends"
        else:
            n = 2 + o % 2
            s = (5 * o) % max(1, len(idx) - n + 1)
            keepb[idx[s:s + n]] = True
    for k in ("bb_obj", "bb_pose", "bb_cam", "bb_corners", "bb_cov"):
        prob[k] = prob[k][keepb]
    return _finish(name, prob, 7)


CASES = {
    "pad57": lambda: _finish("pad57", _problem(7, 3, 7, 11, 160), 7),
    "full64": lambda: _finish("full64", _problem(7, 4, 7, 12, 160), 7),
    "over65": lambda: _finish("over65", _problem(6, 5, 7, 13, 140), 7),
    "od9_63": lambda: _finish("od9_63", _problem(7, 3, 7, 14, 160), 9),
    "od9_72": lambda: _finish("od9_72", _problem(7, 4, 7, 15, 160), 9),
    "wide": lambda: _finish("wide", _problem(45, 8, 7, 16, 900), 7),
    "deep": _deep,
    "deeper": lambda: _deep("deeper"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def upload(ba, c):
    synth.upload(ba, c["prob"])


# ------------------------------------------------------------------------------------------
# order of the tile grid
# ------------------------------------------------------------------------------------------
def grid(grid_row):
    """(perm, rows, nt): canonical indices in grid order, their rows of the tile grid, tiles per dimension"""
    grid_row = np.asarray(grid_row, np.int64)
    perm = np.argsort(grid_row, kind="stable")
    rows = grid_row[perm]
    assert len(np.unique(rows)) == len(rows), "grid_row is no permutation"
    return perm, rows, int(rows.max()) // TILE + 1


def tile_mask(S, grid_row):
    """lower-triangular tile pattern of S in the grid's order, closed under the fill of a tile Cholesky (a Python restatement of the structural mask:
    tile (i, j) fills if a column k < j holds both (i, k) and (j, k))"""
    perm, rows, nt = grid(grid_row)
    t = rows // TILE
    M = np.zeros((nt, nt), bool)
    nz = np.asarray(S)[np.ix_(perm, perm)] != 0
    for a in range(nt):
        for b in range(a + 1):
            M[a, b] = nz[np.ix_(t == a, t == b)].any()
    M[np.arange(nt), np.arange(nt)] = True
    for k in range(nt):
        col = np.flatnonzero(M[:, k])
        col = col[col > k]
        for i in col:
            for j in col:
                if j <= i:
                    M[i, j] = True
    return M


def tile_levels(M):
    """level of every tile column in the elimination tree of the pattern M: 0 without a tile to its left, else one more than the deepest of them"""
    nt = len(M)
    lvl = np.zeros(nt, int)
    for k in range(nt):
        left = np.flatnonzero(M[k, :k])
        lvl[k] = 0 if len(left) == 0 else 1 + lvl[left].max()
    return lvl


def inside_mask(S, grid_row, M):
    perm, rows, nt = grid(grid_row)
    t = rows // TILE
    nz = np.asarray(S)[np.ix_(perm, perm)] != 0
    return all(M[max(a, b), min(a, b)] or not nz[np.ix_(t == a, t == b)].any() for a in range(nt) for b in range(nt))


# ------------------------------------------------------------------------------------------
# reference and metric
# ------------------------------------------------------------------------------------------
def chol_ld(S):
    """Cholesky factor by a plain column loop in long double; a pivot that is not positive raises"""
    A = np.array(S, dtype=LD)
    m = len(A)
    Lf = np.zeros((m, m), LD)
    for j in range(m):
        p = A[j, j] - Lf[j, :j] @ Lf[j, :j]
        if not p > 0:
            raise np.linalg.LinAlgError("pivot %d is %g" % (j, float(p)))
        Lf[j, j] = np.sqrt(p)
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def solve_ld(Lf, b):
    m = len(Lf)
    z = np.array(b, dtype=LD)
    for i in range(m):
        z[i] = (z[i] - Lf[i, :i] @ z[:i]) / Lf[i, i]
    for i in range(m - 1, -1, -1):
        z[i] = (z[i] - Lf[i + 1:, i] @ z[i + 1:]) / Lf[i, i]
    return z


class System:
    """S y = b with its grid order and L* (computed once, shared, never modified)"""

    def __init__(self, S, b, grid_row):
        self.S, self.b, self.grid_row = np.array(S, np.float64), np.array(b, np.float64), np.asarray(grid_row, np.int64)
        self.perm, self.rows, self.nt = grid(self.grid_row)
        self.m = len(self.b)
        self.Sg, self.bg = self.S[np.ix_(self.perm, self.perm)].astype(LD), self.b[self.perm].astype(LD)
        self.L = chol_ld(self.Sg)
        self.E = np.abs(self.L) @ np.abs(self.L.T)

    def omega(self, y):
        yg = np.asarray(y, np.float64)[self.perm].astype(LD)
        if not np.isfinite(yg.astype(np.float64)).all():
            return float("inf")
        w = np.abs(self.Sg @ yg - self.bg) / (self.E @ np.abs(yg) + np.abs(self.bg))
        return float(w.max())

    def bar(self, y_emu=None):
        return max((3 * self.m + 1) * U, 8.0 * self.omega(self.emulate() if y_emu is None else y_emu))

    @functools.lru_cache(maxsize=None)
    def emulate(self, fault=None):
        return emulate(self.S, self.b, self.grid_row, fault)

    def lapack(self):
        import scipy.linalg
        Sg, bg = self.Sg.astype(np.float64), self.bg.astype(np.float64)
        y = np.zeros(self.m)
        y[self.perm] = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Sg, lower=True), bg)
        return y


# ------------------------------------------------------------------------------------------
# the project's algorithm in numpy float64
# ------------------------------------------------------------------------------------------
def _potrf64(A):
    """column loop on one tile, no exception: a zero or negative pivot poisons what follows, as on the device"""
    Lf = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(TILE):
            p = A[j, j] - Lf[j, :j] @ Lf[j, :j]
            Lf[j, j] = np.sqrt(p)
            Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def _trtri64(Lf):
    X = np.zeros_like(Lf)
    with np.errstate(all="ignore"):
        for i in range(TILE):
            e = np.zeros(TILE); e[i] = 1.0
            X[i] = (e - Lf[i, :i] @ X[:i]) / Lf[i, i]
    return X


FAULTS = ("drop_update", "skip_rhs", "skip_backward", "pad_zero", "inv_entry")


def fault_applies(sys_, fault):
    M = tile_mask(sys_.S, sys_.grid_row)
    n_off = int(M.sum()) - sys_.nt
    if fault in ("drop_update", "skip_rhs", "skip_backward"):
        return n_off > 0
    if fault == "pad_zero":
        return sys_.m < sys_.nt * TILE
    return True


FACTOR_FAULTS = ("drop_update", "pad_zero", "inv_entry")


def factor_tiles(S, grid_row, fault=None):
    """(A, inv, M): the padded grid with the factor tiles L_ik (i >= k; L_kk with a zero upper part) where the mask M holds, the explicit inverses L_kk^-1, and
    the fill-closed tile mask -- the part of the tile algorithm the solve and the covariance pass (tests/cov_cases.py) share; fault: one of FACTOR_FAULTS"""
    perm, rows, nt = grid(grid_row)
    n = nt * TILE
    A = np.eye(n)
    A[np.ix_(rows, rows)] = np.asarray(S, np.float64)[np.ix_(perm, perm)]
    todo = fault
    if todo == "pad_zero":
        pad = np.setdiff1d(np.arange(n), rows)
        A[pad[0], pad[0]] = 0.0
        todo = None
    M = tile_mask(S, grid_row)
    T = lambda i, j: (slice(i * TILE, (i + 1) * TILE), slice(j * TILE, (j + 1) * TILE))  # noqa: E731
    inv = [None] * nt
    with np.errstate(all="ignore"):
        for k in range(nt):
            Lkk = _potrf64(A[T(k, k)])
            inv[k] = _trtri64(Lkk)
            if todo == "inv_entry" and k == nt - 1:
                r = int(rows[-1]) % TILE                      # the diagonal entry of the last real row of the last tile
                inv[k][r, r] *= 1.0 + 1e-9
                todo = None
            A[T(k, k)] = Lkk
            col = [i for i in range(k + 1, nt) if M[i, k]]
            for i in col:
                A[T(i, k)] = A[T(i, k)] @ inv[k].T
            for i in col:
                for j in col:
                    if j > i:
                        continue
                    if todo == "drop_update":
                        todo = None
                        continue
                    A[T(i, j)] -= A[T(i, k)] @ A[T(j, k)].T
    assert todo is None, "the fault %r found no place in this system" % (fault,)
    return A, inv, M


def emulate(S, b, grid_row, fault=None):
    """y of S y = b (canonical order) by the tile algorithm; fault: one of FAULTS, planted once"""
    perm, rows, nt = grid(grid_row)
    n = nt * TILE
    A, inv, M = factor_tiles(S, grid_row, fault if fault in FACTOR_FAULTS else None)
    todo = None if fault in FACTOR_FAULTS else fault
    z = np.zeros(n)
    z[rows] = np.asarray(b, np.float64)[perm]
    T = lambda i, j: (slice(i * TILE, (i + 1) * TILE), slice(j * TILE, (j + 1) * TILE))  # noqa: E731
    V = lambda i: slice(i * TILE, (i + 1) * TILE)  # noqa: E731
    with np.errstate(all="ignore"):
        for k in range(nt):                                   # (tile row i takes its terms in the order of k, as when this ran inside the factorisation)
            z[V(k)] = inv[k] @ z[V(k)]
            for i in range(k + 1, nt):
                if not M[i, k]:
                    continue
                if todo == "skip_rhs":
                    todo = None
                    continue
                z[V(i)] -= A[T(i, k)] @ z[V(k)]
        yg = np.zeros(n)
        for k in range(nt - 1, -1, -1):
            t = z[V(k)].copy()
            for i in range(k + 1, nt):
                if not M[i, k]:
                    continue
                if todo == "skip_backward":
                    todo = None
                    continue
                t -= A[T(i, k)].T @ yg[V(i)]
            yg[V(k)] = inv[k].T @ t
    assert todo is None, "the fault %r found no place in this system" % (fault,)
    y = np.zeros(len(perm))
    y[perm] = yg[rows]
    return y


# ------------------------------------------------------------------------------------------
# given-values sets
# ------------------------------------------------------------------------------------------
def _mirror(A):
    """exactly symmetric: the lower triangle and its mirror image"""
    Lw = np.tril(A)
    return Lw + np.tril(A, -1).T


def jacobi_scaled(S, b):
    d = 1.0 / np.sqrt(np.diag(S))
    return _mirror(S * d[:, None] * d[None, :]), b * d


def random_on_pattern(S, grid_row, seed):
    """B B^T + I, B random lower triangular on the tile pattern of tril(S) in the grid's order; the right-hand side random"""
    rng = np.random.Generator(np.random.MT19937(seed))
    perm, rows, nt = grid(grid_row)
    m = len(perm)
    t = rows // TILE
    nz = np.asarray(S)[np.ix_(perm, perm)] != 0
    P = np.zeros((nt, nt), bool)
    for a in range(nt):
        for c in range(a + 1):
            P[a, c] = nz[np.ix_(t == a, t == c)].any()
    B = np.tril(rng.uniform(-1.0, 1.0, (m, m))) * P[np.ix_(t, t)] / np.sqrt(m)
    Ag = _mirror(B @ B.T + np.eye(m))
    A = np.zeros((m, m))
    A[np.ix_(perm, perm)] = Ag
    return A, rng.uniform(-1.0, 1.0, m)


def with_pivot(sys_, g, factor):
    """the system with S_gg (g: a row of the tile grid) changed so that the pivot of that row becomes factor * S_gg exactly (the rows in front of it are as
    they were, so the sign of the new pivot does not depend on round-off): -0.5 must be rejected, +0.5 accepted.
    Lowering a pivot that was above 0.5 S_gg takes more out of every later pivot, and on a reduced system of the project -- rows of one pose block are
    strongly coupled -- the twin is then often no longer positive definite (the long double factorisation itself refuses it): both sets are built on the
    B B^T + I system of random_on_pattern(), whose coupling is weak enough that every twin stays positive definite (tests/test_chol_reference.py holds the
    oracle's mirror to that)."""
    at = int(np.flatnonzero(sys_.rows == g)[0])
    c = int(sys_.perm[at])
    pivot = sys_.L[at, at] ** 2
    S = sys_.S.copy()
    S[c, c] = float(LD(sys_.S[c, c]) - pivot + LD(factor) * LD(sys_.S[c, c]))
    return S, c


def reject_rows(sys_, M=None):
    """{label: grid row}: the positions REJECT_POS of a first-level tile, a mid-level tile and the root tile where those are real rows, and the last real
    row in front of padding"""
    M = tile_mask(sys_.S, sys_.grid_row) if M is None else M
    lvl = tile_levels(M)
    real = set(int(r) for r in sys_.rows)
    tiles = {"first": 0, "root": sys_.nt - 1}
    mid = [k for k in range(sys_.nt) if 0 < lvl[k] < lvl.max()]
    if mid:
        tiles["mid"] = max(mid, key=lambda k: sum(k * TILE + p in real for p in REJECT_POS))
    out = {}
    for where, k in tiles.items():
        for p in REJECT_POS:
            if k * TILE + p in real:
                out["%s+%d" % (where, p)] = k * TILE + p
    edge = [r for r in sorted(real) if r + 1 not in real and (r + 1) % TILE != 0]
    if edge:
        out["before_padding"] = edge[len(edge) // 2]
    return out
