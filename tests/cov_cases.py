"""Designed cases for the covariance kernels (cov_kernels.hip: k_selinv_y, k_selinv_off, k_selinv_diag, k_cov_gather, k_cov_seed_rows, k_cov_forward,
k_cov_rhs_pairs; at the end of the file k_cov_points and k_cov_point_cross), the reference they are judged by and the measure.  CPU only; touches nothing in the product.

The system is the one the pass itself inverts (obvi_cov_debug_compute_pairs returns it): S in canonical order and the row of the tile grid of every index.

Reference.  Sigma* = L*^-T L*^-1 in numpy.longdouble, L* = chol_cases.chol_ld(S) in the grid's order; kept per system, never modified.

Measure, for any block of poses and objects, on or off the tile pattern of the factor:

    omega(block) = max_ij |Sigma - Sigma*|_ij / (|Sigma*| E |Sigma*|)_ij,        E = |L*| |L*^T|

the forward-error form of the bound behind chol_cases' omega: a computed inverse X of A satisfies X - A^-1 = -A^-1 dA X with |dA| <= gamma_{3m+1} |L| |L^T|
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 10.4 and section 14.1), so |X - A^-1| <= gamma |A^-1| E |A^-1| to first order.

Bar.  max((3 m + 1) 2^-53, 8 omega(emulation)): the first term derived, the second from emulate_selinv() / emulate_off_pattern(), this project's algorithm
in numpy float64 on the same S and grid_row on top of chol_cases.factor_tiles (explicit L_kk^-1 products are not backward stable in the textbook sense, and
the emulation carries that dependence); 8 is chol_cases' allowance for the MFMA's other summation order.  The bar is never taken from the device's value.

  emulate_selinv        the Takahashi recursion on the fill-closed tile mask: levels root-down, per level the Y_jk = L_jk L_kk^-1 of every column through a
                        scratch, then Sigma_ik = -sum_j Sigma_ij Y_jk in list order (Sigma_ij = Sigma_ji^T where i < j), then Sigma_kk, symmetrised
  emulate_off_pattern   Yt = (L^-1 E)^T tile row by tile row, the unit vectors of the distinct blocks sorted by row, 64 to a slab, a slab skipping the tiles
                        in front of its first right-hand side; then Yt_a Yt_b^T over the columns from the tile of the later block on

Cases: the eight of chol_cases.CASES with their knobs and expect tables, and deep9: the `deep` incidence with 9-parameter objects (m = 225), the only
od = 9 case with tiles that do not exist, hence with pairs off the pattern.

On the CPU there is no plan, so no grid order: cpu_grid_row() gives the multi-level cases a nested dissection of the pose chain in which every node starts
on a tile boundary (leaf tiles of a few poses under 40 and more padding rows, separators, ancestors that do not exist); the fill closure is computed from the
values whatever the order is.  The GPU test uses the grid order the device reports.

FAULTS, each planted once in the emulation, fault_applies() saying where one can occur:
  off_drop          drop the product with the farthest ancestor in one off-diagonal target
  off_no_transpose  read Sigma_ji untransposed where i < j
  diag_drop         drop one Y^T Sigma term of a diagonal target
  y_in_place        form one column's Y after a neighbour has overwritten its L tile (the hazard the scratch exists for)
  pad_as_data       clear one padding row's identity entry
  fwd_skip          drop one j term of a forward row
  slab_first_late   skip one tile too many in a slab
  rhs_first_late    start a pair's product one tile late"""
import functools

import numpy as np

import chol_cases as cc
import synth

LD = cc.LD
TILE = cc.TILE
U = cc.U
POSE, POINT, OBJECT = 0, 1, 2

# deep9's plan is read back by the GPU test; what the case is there for: rows, several levels, more tiles than a dense grid of its rows would have
EXPECT_DEEP9 = dict(reduced_rows=225, min_tiles_per_dim=8, min_chol_levels=4)
KNOBS = dict(cc.KNOBS, deep9=cc.KNOBS["deep"])
CASES = tuple(sorted(cc.CASES)) + ("deep9",)
MULTI_TILE = cc.MULTI_TILE + ("deep9",)
GIVEN_ON = ("wide", "deep", "deeper", "deep9")
OFF_PATTERN_ON = ("deep", "deeper", "deep9")
SAME_PROBLEM = cc.SAME_PROBLEM


@functools.lru_cache(maxsize=None)
def case(name):
    if name != "deep9":
        return cc.case(name)
    base = cc.case("deep")
    prob = synth.nine_dof(base["prob"], tilt=0.1, seed=7)
    m = base["m"] + 2 * len(prob["objects"])
    assert m == 225
    return dict(name="deep9", od=9, prob=prob, m=m, knobs=KNOBS["deep9"], expect=EXPECT_DEEP9)


def upload(ba, c):
    synth.upload(ba, c["prob"])


# ------------------------------------------------------------------------------------------
# blocks: canonical order is variable poses by index, then objects
# ------------------------------------------------------------------------------------------
class Blocks:
    """canonical first index and size of every pose and object block of a case"""

    def __init__(self, c):
        prob = c["prob"]
        self.od = c["od"]
        self.var_pose = np.flatnonzero(prob["pose_const"] == 0)
        self.const_pose = np.flatnonzero(prob["pose_const"] != 0)
        self.nP, self.nO = len(prob["pose_const"]), len(prob["objects"])
        self.start = {}
        for r, p in enumerate(self.var_pose):
            self.start[(POSE, int(p))] = (6 * r, 6)
        for o in range(self.nO):
            self.start[(OBJECT, o)] = (6 * len(self.var_pose) + self.od * o, self.od)
        self.keys = sorted(self.start)
        assert 6 * len(self.var_pose) + self.od * self.nO == c["m"]

    def idx(self, key):
        s, d = self.start[key]
        return np.arange(s, s + d)


def cpu_grid_row(c, leaf=4):
    """a grid order for the CPU: single-node cases keep the canonical order; the `deep` family gets a nested dissection of the chain of variable poses
    (separator: the middle pose; leaves of at most `leaf` poses), every node starting on a tile boundary, an object in the lowest node that holds all the
    poses it is seen from (the separator of that node where they lie on both sides of it)"""
    if c["name"] not in ("deep", "deeper", "deep9"):
        return np.arange(c["m"])
    prob, od = c["prob"], c["od"]
    var = np.flatnonzero(prob["pose_const"] == 0)
    rank = {int(p): r for r, p in enumerate(var)}
    seen = [sorted({rank[int(p)] for p in prob["bb_pose"][prob["bb_obj"] == o] if int(p) in rank}) for o in range(len(prob["objects"]))]
    nodes = []                                                   # post-order: (poses, objects)

    def split(lo, hi, objs):
        if hi - lo <= (2 if c["name"] == "deeper" else leaf):
            nodes.append((list(range(lo, hi)), objs))
            return
        mid = (lo + hi) // 2
        left = [o for o in objs if seen[o][-1] < mid]
        right = [o for o in objs if seen[o][0] > mid]
        split(lo, mid, left)
        split(mid + 1, hi, right)
        nodes.append(([mid], [o for o in objs if o not in left and o not in right]))
    split(0, len(var), list(range(len(seen))))
    grid_row = np.zeros(c["m"], np.int64)
    at = 0
    for poses, objs in nodes:
        for r in poses:
            grid_row[6 * r:6 * r + 6] = at + np.arange(6)
            at += 6
        for o in objs:
            s = 6 * len(var) + od * o
            grid_row[s:s + od] = at + np.arange(od)
            at += od
        at = -(-at // TILE) * TILE
    return grid_row


# ------------------------------------------------------------------------------------------
# reference and measure
# ------------------------------------------------------------------------------------------
def _inv_lower_ld(Lf):
    m = len(Lf)
    X = np.zeros((m, m), LD)
    for i in range(m):
        X[i] = -(Lf[i, :i] @ X[:i])
        X[i, i] += LD(1)
        X[i] /= Lf[i, i]
    return X


class CovSystem:
    """S (canonical) with its grid order, Sigma* and the denominator of the measure in canonical order (computed once, shared, never modified)"""

    def __init__(self, S, grid_row):
        self.sys = cc.System(S, np.zeros(len(S)), grid_row)
        self.S, self.grid_row, self.m, self.nt = self.sys.S, self.sys.grid_row, self.sys.m, self.sys.nt
        Li = _inv_lower_ld(self.sys.L)
        Sg = Li.T @ Li
        back = np.argsort(self.sys.perm)                         # canonical index -> position in the grid's order
        self.Sigma = Sg[np.ix_(back, back)]
        aS = np.abs(Sg)
        self.D = (aS @ self.sys.E @ aS)[np.ix_(back, back)]
        self.M = cc.tile_mask(self.S, self.grid_row)
        r = self.grid_row
        self.on = self.M[np.maximum.outer(r, r) // TILE, np.minimum.outer(r, r) // TILE]      # entries of the canonical matrix on the mask
        self.floor = (3 * self.m + 1) * U

    def omega(self, X, ia, ib):
        """of a block X of rows ia, columns ib (canonical indices)"""
        X = np.asarray(X, np.float64)
        if X.shape != (len(ia), len(ib)) or not np.isfinite(X).all():
            return float("inf")
        return float((np.abs(X.astype(LD) - self.Sigma[np.ix_(ia, ib)]) / self.D[np.ix_(ia, ib)]).max())

    def on_pattern(self, ia, ib):
        """every tile the two blocks' rows touch is in the fill-closed mask"""
        ta, tb = np.unique(self.grid_row[ia] // TILE), np.unique(self.grid_row[ib] // TILE)
        return all(self.M[max(a, b), min(a, b)] for a in ta for b in tb)

    def canon(self, G):
        """a padded grid with lower tiles (diagonal tiles holding both triangles) -> canonical m x m, NaN off the mask: entry by entry as k_cov_gather reads"""
        r = self.grid_row
        hi, lo = np.maximum.outer(r, r), np.minimum.outer(r, r)
        same = hi // TILE == lo // TILE
        rr, ccol = np.where(same, r[:, None], hi), np.where(same, r[None, :], lo)
        out = G[rr, ccol].astype(np.float64)
        out[~self.on] = np.nan
        return out

    @functools.lru_cache(maxsize=None)
    def selinv(self, fault=None):
        return self.canon(emulate_selinv(self.S, self.grid_row, fault))

    def omega_all(self, X):
        """largest omega over the entries of a canonical matrix that lie on the mask (NaN elsewhere)"""
        on = self.on
        if not np.isfinite(np.where(on, X, 0.0)).all():
            return float("inf")
        return float((np.abs(np.where(on, X, 0.0).astype(LD) - np.where(on, self.Sigma, LD(0))) / self.D).max())

    @functools.lru_cache(maxsize=None)
    def bar(self):
        return max(self.floor, 8.0 * self.omega_all(self.selinv()))

    def off_pattern(self, blocks, pairs, fault=None):
        """blocks: [(canonical first index, size)]; pairs: [(x, y)] indices into blocks -> the emulated blocks"""
        rows = [(int(self.grid_row[s]), d) for s, d in blocks]
        return emulate_off_pattern(self.S, self.grid_row, rows, pairs, fault)

    def bar_off(self, blocks, pairs):
        emu = self.off_pattern(blocks, pairs)
        w = max(self.omega(X, np.arange(blocks[x][0], sum(blocks[x])), np.arange(blocks[y][0], sum(blocks[y]))) for X, (x, y) in zip(emu, pairs))
        return max(self.floor, 8.0 * w), w


# ------------------------------------------------------------------------------------------
# the project's algorithm in numpy float64
# ------------------------------------------------------------------------------------------
FAULTS = ("off_drop", "off_no_transpose", "diag_drop", "y_in_place", "pad_as_data", "fwd_skip", "slab_first_late", "rhs_first_late")
RECURSION_FAULTS = FAULTS[:5]
_T = lambda i, j: (slice(i * TILE, (i + 1) * TILE), slice(j * TILE, (j + 1) * TILE))  # noqa: E731
_V = lambda i: slice(i * TILE, (i + 1) * TILE)  # noqa: E731


def fault_applies(s, fault, rows=None, pairs=None):
    """s: a CovSystem; rows / pairs: the request of the off-pattern route (the last three faults)"""
    M, nt = s.M, s.nt
    deg = [int(M[k + 1:, k].sum()) for k in range(nt)]
    if fault in ("off_drop", "diag_drop"):
        return max(deg) >= 1
    if fault in ("off_no_transpose", "y_in_place"):
        return max(deg) >= 2
    if fault == "pad_as_data":
        return s.m < nt * TILE
    if rows is None or not pairs:
        return False
    try:                                                         # the route itself says whether the fault finds a place in this request
        emulate_off_pattern(s.S, s.grid_row, rows, pairs, fault)
    except AssertionError:
        return False
    return True


def emulate_selinv(S, grid_row, fault=None):
    """the padded grid after the selected inversion: Sigma in the lower tiles of the mask, diagonal tiles symmetric; fault: one of RECURSION_FAULTS"""
    A, inv, M = cc.factor_tiles(S, grid_row, "pad_zero" if fault == "pad_as_data" else None)
    todo = None if fault == "pad_as_data" else fault
    nt = len(M)
    lvl = cc.tile_levels(M)
    with np.errstate(all="ignore"):
        for level in range(int(lvl.max()), -1, -1):
            cols = [k for k in range(nt) if lvl[k] == level]
            rows_of = {k: [j for j in range(k + 1, nt) if M[j, k]] for k in cols}
            Y = {(j, k): A[_T(j, k)] @ inv[k] for k in cols for j in rows_of[k]}
            for k in cols:
                for i in rows_of[k]:
                    acc = np.zeros((TILE, TILE))
                    for j in rows_of[k]:
                        if todo == "off_drop" and j == rows_of[k][-1]:
                            todo = None
                            continue
                        Sij = A[_T(i, j)] if i >= j else A[_T(j, i)].T
                        if todo == "off_no_transpose" and i < j:
                            Sij = A[_T(j, i)]
                            todo = None
                        acc += Sij @ Y[(j, k)]
                    A[_T(i, k)] = -acc
                    if todo == "y_in_place" and len(rows_of[k]) >= 2 and i == rows_of[k][0]:
                        Y[(i, k)] = A[_T(i, k)] @ inv[k]         # the next target of this column reads the tile its neighbour has just written
                        todo = None
            for k in cols:
                D = inv[k].T @ inv[k]
                sub = np.zeros((TILE, TILE))
                for j in rows_of[k]:
                    if todo == "diag_drop":
                        todo = None
                        continue
                    sub += Y[(j, k)].T @ A[_T(j, k)]
                D = D - sub
                A[_T(k, k)] = 0.5 * (D + D.T)
    assert todo is None, "the fault %r found no place in this system" % (fault,)
    return A


def rhs_layout(rows):
    """(rhs_row, col_of): the unit vectors of the distinct blocks (first grid row, size), ascending, and the first column of every block"""
    rhs_row, col_of = [], {}
    for r, d in sorted(set(rows)):
        col_of[r] = len(rhs_row)
        rhs_row += list(range(r, r + d))
    return np.array(rhs_row, np.int64), col_of


def emulate_off_pattern(S, grid_row, rows, pairs, fault=None):
    """rows: [(first grid row, size)] of the blocks; pairs: [(x, y)] indices into rows -> [block x, block y] of Sigma, by forward substitution"""
    A, inv, M = cc.factor_tiles(S, grid_row)
    nt = len(M)
    rhs_row, col_of = rhs_layout(rows)
    nslabs = -(-len(rhs_row) // TILE)
    Yt = np.zeros((nslabs * TILE, nt * TILE))
    Yt[np.arange(len(rhs_row)), rhs_row] = 1.0
    todo = fault
    with np.errstate(all="ignore"):
        for sl in range(nslabs):
            first = int(rhs_row[sl * TILE]) // TILE
            if todo == "slab_first_late" and sl == nslabs - 1:
                first += 1
                todo = None
            for k in range(first, nt):
                acc = np.zeros((TILE, TILE))
                for j in range(first, k):
                    if not M[k, j]:
                        continue
                    if todo == "fwd_skip" and Yt[_V(sl), _V(j)].any():
                        todo = None
                        continue
                    acc += Yt[_V(sl), _V(j)] @ A[_T(k, j)].T
                Yt[_V(sl), _V(k)] = (Yt[_V(sl), _V(k)] - acc) @ inv[k].T
        out = []
        for x, y in pairs:
            (ra, da), (rb, db) = rows[x], rows[y]
            first = max(ra, rb) // TILE * TILE
            late = slice(first, first + TILE)
            if todo == "rhs_first_late" and Yt[col_of[ra]:col_of[ra] + da, late].any() and Yt[col_of[rb]:col_of[rb] + db, late].any():
                first += TILE
                todo = None
            out.append(Yt[col_of[ra]:col_of[ra] + da, first:] @ Yt[col_of[rb]:col_of[rb] + db, first:].T)
    assert todo is None, "the fault %r found no place in this request" % (fault,)
    return out


# ------------------------------------------------------------------------------------------
# requests off the pattern, aimed at the slab edges
# ------------------------------------------------------------------------------------------
def _star(s, B, keys, n_pose, n_obj):
    """[(hub, k)]: n_pose poses and n_obj objects in all, every pair off the pattern -- a hub block and blocks off the pattern with it; None: no such set"""
    for hub in keys:
        nb = [k for k in keys if k != hub and not s.on_pattern(B.idx(hub), B.idx(k))]
        poses, objs = [k for k in nb if k[0] == POSE], [k for k in nb if k[0] == OBJECT]
        need_p, need_o = n_pose - (hub[0] == POSE), n_obj - (hub[0] == OBJECT)
        if need_p >= 0 and need_o >= 0 and len(poses) >= need_p and len(objs) >= need_o and need_p + need_o > 0:
            return [(hub, k) for k in poses[:need_p] + objs[:need_o]]
    return None


def rhs_count(B, pairs):
    """right-hand sides of a request whose pairs are all off the pattern: the rows of its distinct blocks"""
    return sum(B.start[k][1] for k in {k for p in pairs for k in p})


def sixty_fourth_column_inside_a_block(s, B, pairs):
    edges = np.cumsum([d for _, d in sorted({(int(s.grid_row[B.start[k][0]]), B.start[k][1]) for p in pairs for k in p})])
    return edges[-1] > 2 * TILE and TILE not in edges


def off_pattern_sets(s, B):
    """{label: [(key a, key b)]} (a set that cannot be built is missing or empty): the requests of the GPU test and of the CPU test of the faults, all pairs off the pattern of s (a CovSystem), B the case's Blocks.
    6 a + 9 b is a multiple of 3: with 9-parameter objects no request has exactly 64 or 65 right-hand sides, and the sets `rhs63` and `rhs66` stand on both
    sides of the slab edge instead."""
    keys, od = B.keys, B.od
    tile = lambda k: int(s.grid_row[B.start[k][0]]) // TILE  # noqa: E731
    off = [(a, b) for x, a in enumerate(keys) for b in keys[x + 1:] if not s.on_pattern(B.idx(a), B.idx(b))]
    assert off, "no pair off the pattern"
    sets = {}
    if od == 7:
        sets["rhs64"] = _star(s, B, keys, 6, 4)
        sets["rhs65"] = _star(s, B, keys, 5, 5)
    else:
        sets["rhs63"] = _star(s, B, keys, 6, 3)
        sets["rhs66"] = _star(s, B, keys, 5, 4)
    order = sorted(off, key=lambda p: (abs(tile(p[0]) - tile(p[1])), p))
    for n in range(1, len(order) + 1):                           # over 128, the 64th column inside a block: the nearest pairs first, until both hold
        if sixty_fourth_column_inside_a_block(s, B, order[:n]):
            sets["over128"] = order[:n]
            break
    sets["past_tile0"] = _star(s, B, [k for k in keys if tile(k) > 0], 3, 2)
    far = max(off, key=lambda p: abs(tile(p[0]) - tile(p[1])))
    sets["ends"] = [far] + [p for p in off if tile(p[0]) == 0 and tile(p[1]) >= s.nt - 2][:3]
    rows_of = lambda k: set(s.grid_row[B.idx(k)] // TILE)  # noqa: E731
    sets["share_tile"] = [p for p in off if rows_of(p[0]) & rows_of(p[1])][:4]
    if not sets["share_tile"]:
        # every node of these grids starts on a tile boundary and no block straddles one, so two blocks of one tile are always on the pattern: the pairs here
        # are (a, c) and (b, c) with a and b in one tile instead -- two right-hand-side blocks whose columns of Yt start in the same tile
        for x, (a, c) in enumerate(off):
            twin = [(b, c2) for b, c2 in off[x + 1:] if c2 == c and b != a and tile(b) == tile(a)]
            if twin:
                sets["share_tile"] = [(a, c), twin[0]]
                break
    groups = []
    for ka, kb in ((POSE, POSE), (POSE, OBJECT), (OBJECT, OBJECT)):
        groups += [p for p in off if {p[0][0], p[1][0]} == {ka, kb}][:3]
    sets["groups"] = groups
    return sets


def request(s, B, pairs):
    """(blocks, index pairs) of a list of key pairs, as CovSystem.off_pattern takes them"""
    ks = sorted({k for p in pairs for k in p})
    return [B.start[k] for k in ks], [(ks.index(a), ks.index(b)) for a, b in pairs]


# ------------------------------------------------------------------------------------------
# blocks with a feature (k_cov_points, k_cov_point_cross)
# ------------------------------------------------------------------------------------------
# Reference: the formulas in the header comments of the two kernels in long double, H_ll and W_a = J_pose^T J_point of every record from the oracle's
# debug_linearize(0), robustified, Sigma* of the reduced blocks from the system the device returns:
#     C_ll = H_l^-1 + H_l^-1 (sum_ab W_a^T Sigma*_{p(a)p(b)} W_b) H_l^-1       C_lx = -H_l^-1 sum_a W_a^T Sigma*_{p(a)x}
#     C_lm = H_l^-1 (sum_ab W_a^T Sigma*_{p(a)p(b)} W_b) H_m^-1
# Error: max_ij |C - C*|_ij / sqrt(C*_ii C*_jj), the diagonals those of the two own blocks.  Bar: max(8 max(e_emu, d), n_terms 2^-53) with
#     e_emu    the float64 restatement of the kernel's own order (C = chol(H), Z_a = W_a C^-T; lane x takes items x, x + 64, ...; a butterfly sum) against C*
#     d        the same long double formula on Sigma* of the ORACLE's system: what a rounding-level change of the inputs does to the answer
#     n_terms  the products summed into one entry of the block: 36 per pair of records (6 per record of a block with a pose or an object), and the 9 of the
#              two triangular products
# In this case d, not e_emu, sets the bar: two poses near the end of the path are held weakly at the start point (the Jacobi-scaled reduced system has a
# condition number of 6e11), the covariance of every feature is dominated by that mode, and a change of the system in its last bits moves every block by 1e-5
# of its scale -- the device's blocks differ from the reference by 4e-6 on every feature alike, the forward error of a backward stable inverse.  A dropped
# pair of records of a 9-record feature (1 / 81 of the sum) stands two orders above the bar; one of a 65-record feature (1 / 4225) only about twice.
# FEATURE_TABLE, per feature of the case (FEATURE_GROUPS) and kind of block (its own block, its blocks with a pose or an object, its block with another feature):
# the largest e_emu, measured on the CPU on the oracle's system (tests/test_cov_reference.py), and the largest d, measured with the system a deterministic
# handle returned on an MI355X (tests/test_gpu_cov_edges.py); each test prints its figures and fails if one drifts from the table by more than a factor 2.
KINDS = ("own", "reduced", "feature")
FEATURE_TABLE = {
    "n2": dict(e_emu=(6.3e-11, 2.2e-12, 3e-12), d=(1.3e-05, 1.3e-05, 1.4e-05)),
    "n8": dict(e_emu=(6.7e-13, 2.1e-13, 3.6e-13), d=(1.4e-05, 1.4e-05, 1.4e-05)),
    "n9": dict(e_emu=(1.6e-13, 6.4e-14, 1.4e-13), d=(1.5e-05, 1.4e-05, 1.5e-05)),
    "n63": dict(e_emu=(2e-14, 1.4e-14, 2.1e-14), d=(1.6e-05, 1.5e-05, 1.5e-05)),
    "n64": dict(e_emu=(3.9e-15, 4.2e-15, 1.1e-14), d=(1.5e-05, 1.5e-05, 1.4e-05)),
    "n65": dict(e_emu=(1.7e-14, 2.7e-15, 1.2e-13), d=(1.4e-05, 1.4e-05, 1.4e-05)),
    "stereo": dict(e_emu=(1.9e-12, 1.6e-14, 2.8e-12), d=(1.3e-05, 1.3e-05, 1.3e-05)),
    "masked": dict(e_emu=(3.3e-12, 2.5e-12, 8.7e-13), d=(1.4e-05, 1.3e-05, 8.5e-06)),
    "const_pose": dict(e_emu=(6.3e-13, 5.6e-13, 5.7e-12), d=(3e-06, 8.6e-06, 7.9e-06)),
}
FEATURE_GROUPS = ("n2", "n8", "n9", "n63", "n64", "n65", "stereo", "masked", "const_pose")


@functools.lru_cache(maxsize=None)
def feature_case():
    """one fixed incidence in the scene of tests/schur_cases.py, stereo: features with 2, 8 (64 pairs of records: one full stride of k_cov_points), 9, 63, 64
    and 65 records, a stereo feature with two records per frame, one with a masked sighting, one seen from a constant pose, a constant and an unobserved one;
    two objects seen from six poses each, so that (feature, object) pairs exist.  pack_a / pack_b themselves have no object."""
    import schur_cases as sc
    b = sc._Builder("cov_features", 72, True, 7301, const_poses=(0, 70, 71))
    b.track("n65", 2, 65); b.track("n2", 5, 2); b.track("n8", 8, 8); b.track("n9", 20, 9); b.track("n63", 3, 63); b.track("n64", 4, 64)
    b.track("stereo", 30, 3, cams=(0, 1))
    b.point("masked", [(40, 0), (41, 0, "m0"), (42, 0), (43, 0)])
    b.track("const_pose", 0, 4)
    b.point("const_point", [(10, 0), (11, 0), (12, 0)], const=True)
    b.gap(1)
    for j in range(10):                                         # (the fillers thin out towards the last frames)
        b.frames("tail", list(range(61 + j % 4, b.n_frames)))
    b.fillers(180)                                              # (every pose held by a dozen features: the undamped system is full rank)
    case = b.finish()
    prob = case["prob"]
    rng = np.random.Generator(np.random.MT19937(7302))
    dims = np.array(synth.SHAPE_CLASSES["bench"][0], np.float64)
    gt = np.array([[1.5, 11.0, 0.0, 0.3], [4.5, 13.0, 0.0, -0.8]])
    gt = np.concatenate([gt, np.stack([dims, dims])], axis=1)
    bb_obj = np.repeat([0, 1], 6).astype(np.uint32)
    bb_pose = np.array([6, 7, 8, 9, 10, 11, 38, 39, 40, 41, 42, 43], np.uint32)
    px, valid, depth = synth.project_ellipsoids(gt[bb_obj], prob["gt_poses"][bb_pose], prob["K"][0], prob["ext"][0])
    assert valid.all() and (depth > 1.5).all()
    corners = np.stack([px[:, 0:2].min(axis=1), px[:, 0:2].max(axis=1), px[:, 2:4].min(axis=1), px[:, 2:4].max(axis=1)], axis=1) + rng.normal(size=(12, 4)) * 2.0
    objects = gt.copy()
    objects[:, 0:3] += rng.normal(size=(2, 3)) * 0.05
    cov = np.zeros((12, 4, 4)); cov[:, np.arange(4), np.arange(4)] = synth.RESIDUAL_PARAMS["bbox_var"]
    sp_cov = np.zeros((2, 3, 3)); sp_cov[:, np.arange(3), np.arange(3)] = np.array(synth.SHAPE_CLASSES["bench"][1], np.float64) ** 2
    prob.update(objects=objects, gt_objects=gt, object_const=np.zeros(2, np.uint8), bb_obj=bb_obj, bb_pose=bb_pose, bb_cam=np.zeros(12, np.uint16), bb_corners=corners,
                bb_cov=cov.reshape(-1, 16), bb_huber=synth.RESIDUAL_PARAMS["bbox_huber"], bb_invalid=synth.RESIDUAL_PARAMS["invalid_ellipsoid_error"],
                sp_obj=np.arange(2, dtype=np.uint32), sp_mean=np.stack([dims, dims]), sp_cov=sp_cov.reshape(-1, 9), sp_huber=synth.RESIDUAL_PARAMS["shape_huber"],
                obj_class=["bench", "bench"])
    case.update(od=7, m=6 * int((prob["pose_const"] == 0).sum()) + 14)
    counts = np.bincount(prob["rp_point"], minlength=len(prob["points"]))
    assert [int(counts[case["groups"][k][0]]) for k in FEATURE_GROUPS] == [2, 8, 9, 63, 64, 65, 6, 4, 4]
    return case


def feature_upload(ba, case):
    synth.upload(ba, case["prob"])
    ba.set_active_mask(0, case["mask0"])


def _butterfly(lanes):
    """the kernels' __shfl_xor sum over 64 lanes, as lane 0 sees it"""
    x = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[x ^ o]
    return lanes[0]


class FeatureRef:
    """H, W of every record from a linearisation (r, J_pose, J_point of debug_linearize(0)) of feature_case(), and the blocks with a feature on a given Sigma
    (canonical order, as CovSystem.Sigma) in long double and in the kernels' own order in float64"""

    def __init__(self, case, r, J0, J1):
        prob = case["prob"]
        self.B = Blocks(case)
        a = prob["rp_huber"]
        sq = (np.asarray(r, LD) ** 2).sum(axis=1)
        w = np.where(sq > a * a, a / np.sqrt(np.maximum(sq, LD(1e-300))), LD(1)) * (case["mask0"] != 0)
        self.active = case["mask0"] != 0
        J0, J1 = np.asarray(J0, LD), np.asarray(J1, LD)
        self.Hrec = w[:, None, None] * np.einsum("nri,nrj->nij", J1, J1)
        self.Wrec = w[:, None, None] * np.einsum("nri,nrj->nij", J0, J1)                  # [6][3] per record
        self.pose = prob["rp_pose"].astype(np.int64)
        self.ptr = np.searchsorted(prob["rp_point"], np.arange(len(prob["points"]) + 1))   # (records are sorted by point, pose, camera)
        self.var = prob["point_const"] == 0

    def records(self, l):
        """(record, canonical first index of its pose or -1) in the order of the point's list; a masked record or one of a constant pose: -1"""
        return [(f, self.B.start[(POSE, int(self.pose[f]))][0] if self.active[f] and (POSE, int(self.pose[f])) in self.B.start else -1) for f in range(self.ptr[l], self.ptr[l + 1])]

    def H(self, l):
        return self.Hrec[self.ptr[l]:self.ptr[l + 1]][self.active[self.ptr[l]:self.ptr[l + 1]]].sum(axis=0)

    @staticmethod
    def _inv3(H):
        Lf = cc.chol_ld(H)
        return np.array([cc.solve_ld(Lf, e) for e in np.eye(3)], LD).T

    def n_terms(self, a, b):
        na = sum(r >= 0 for _, r in self.records(a[1]))
        if b[0] != POINT:
            return 6 * na + 3
        return 36 * na * sum(r >= 0 for _, r in self.records(b[1])) + 9

    # ---- long double ----
    def block(self, a, b, Sigma):
        """C*_{ab}: a a feature, b a feature, a pose or an object (keys (kind, index)); None: a zero block"""
        l = a[1]
        if not self.var[l] or (b[0] == POINT and not self.var[b[1]]) or (b[0] != POINT and b not in self.B.start):
            return None
        Hl = self._inv3(self.H(l))
        if b[0] != POINT:
            ib = self.B.idx(b)
            acc = np.zeros((3, len(ib)), LD)
            for f, r in self.records(l):
                if r >= 0:
                    acc += self.Wrec[f].T @ Sigma[r:r + 6][:, ib]
            return -Hl @ acc
        m = b[1]
        acc = np.zeros((3, 3), LD)
        rm = [x for x in self.records(m) if x[1] >= 0]
        for f, r in self.records(l):
            if r < 0:
                continue
            t = np.zeros((6, 3), LD)
            for f2, r2 in rm:
                t += Sigma[r:r + 6, r2:r2 + 6] @ self.Wrec[f2]
            acc += self.Wrec[f].T @ t
        C = Hl @ acc @ self._inv3(self.H(m))
        return C + Hl if l == m else C

    def diag(self, key, Sigma):
        if key[0] == POINT:
            return np.diag(self.block(key, key, Sigma))
        i = self.B.idx(key)
        return np.diag(Sigma)[i]

    def error(self, X, a, b, Sigma):
        want = self.block(a, b, Sigma)
        scale = np.sqrt(np.outer(self.diag(a, Sigma), self.diag(b, Sigma)))
        return float((np.abs(np.asarray(X, np.float64).astype(LD) - want) / scale).max())

    # ---- the kernels' order in float64 ----
    def _cz(self, l):
        H = self.H(l).astype(np.float64)
        C = np.linalg.cholesky(H)
        Ci = np.zeros((3, 3))
        for i in range(3):                                       # forward substitution on the identity
            e = np.zeros(3); e[i] = 1.0
            for j in range(3):
                Ci[j, i] = (e[j] - C[j, :j] @ Ci[:j, i]) / C[j, j]
        return Ci, {f: self.Wrec[f].astype(np.float64) @ Ci.T for f, r in self.records(l) if r >= 0}

    def emulate(self, a, b, Sigma64):
        if b[0] == POINT and b[1] < a[1]:                        # the pass forms a pair of features once, the lower index first, and serves the other order transposed
            return self.emulate(b, a, Sigma64).T
        l = a[1]
        Cl, Zl = self._cz(l)
        ra = self.records(l)
        if b[0] != POINT:
            ib = self.B.idx(b)
            lanes = np.zeros((64, 3, len(ib)))
            for e, (f, r) in enumerate(ra):
                if r >= 0:
                    lanes[e % 64] += Zl[f].T @ Sigma64[r:r + 6][:, ib]
            return -(Cl.T @ _butterfly(lanes))
        Cm, Zm = (Cl, Zl) if b[1] == l else self._cz(b[1])
        rb = self.records(b[1])
        lanes = np.zeros((64, 3, 3))
        for e in range(len(ra) * len(rb)):
            (f, r), (f2, r2) = ra[e // len(rb)], rb[e % len(rb)]
            if r >= 0 and r2 >= 0:
                lanes[e % 64] += Zl[f].T @ (Sigma64[r:r + 6, r2:r2 + 6] @ Zm[f2])
        M = _butterfly(lanes)
        if b[1] != l:
            return Cl.T @ (M @ Cm)
        c = Cl.T @ ((M + np.eye(3)) @ Cl)
        return 0.5 * (c + c.T)


def feature_pairs(case):
    """[(group, a, b)]: the own block of every feature of FEATURE_GROUPS and its pairs with a pose that sees it, a far pose, both objects and the next feature of the list"""
    g, prob = case["groups"], case["prob"]
    ids = [g[k][0] for k in FEATURE_GROUPS]
    var = [int(p) for p in np.flatnonzero(prob["pose_const"] == 0)]
    out = []
    for x, l in enumerate(ids):
        seen = [int(p) for p in prob["rp_pose"][prob["rp_point"] == l] if int(p) in var]
        far = max(var, key=lambda p: min(abs(p - q) for q in seen))
        out += [(FEATURE_GROUPS[x], (POINT, l), b) for b in ((POINT, l), (POSE, seen[0]), (POSE, far), (OBJECT, 0), (OBJECT, 1), (POINT, ids[(x + 1) % len(ids)]))]
    return out


def feature_kind(a, b):
    return "own" if a == b else "feature" if b[0] == POINT else "reduced"


def feature_bar(ref, group, a, b):
    t = FEATURE_TABLE[group]
    k = KINDS.index(feature_kind(a, b))
    return max(8.0 * max(t["e_emu"][k], t["d"][k]), ref.n_terms(a, b) * U)
