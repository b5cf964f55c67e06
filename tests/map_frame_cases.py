"""Inputs and references of the tests of the map's move into another frame and of the join (include/obvi_map_frame.h): shared by tests/test_map_frame_abi.py
(CPU: the yardstick is itself held) and tests/test_gpu_map_frame.py (the device against the yardstick).  Nothing here touches the product.

The device evaluates  mu'_o = g(T, mu_o),  C' = Jt Cs Jt^T + G Sigma_s G^T  block pair by block pair.  `formula` restates that: in long double (held against the
yardstick on the CPU) and in fp64 with numpy (the round trip a session needs without the device entry).  The yardstick shares no step with it -- the
INFORMATION form in long double: z = (x', tau) = M (x, tau), M = [[Jt, G], [0, I]], so
      Lambda_z = M^-T blockdiag(Cs^-1, Sigma_s^-1) M^-1,      M^-1 = [[Jt^-1, -Jt^-1 G], [0, I]]  written analytically (Jt^-1 block by block),
and C' is the leading block of Lambda_z^-1, taken as the inverse of the Schur complement of Lambda_z's (tau, tau) block -- tau marginalised in information
form, which keeps the large inverse as well conditioned as the map itself (an exact transform: C' = (Jt^-T Cs^-1 Jt^-1)^-1).  Jt^-1 is never a numerical
inverse: Rz(-psi) for the 7-parameter block, blockdiag(R_T^T, Jl^-1(aa) R_T^T Jl(aa'), I) for the 9-parameter one.

The Jacobians here are closed forms (left Jacobians of SO(3)), where the device pushes forward-mode duals through quaternions; tests/test_map_frame_abi.py holds
them against central differences of g.

Maps: the covariances of the 24- and 70-object maps of tests/map_update_cases.py and, for od 7, their means.  For od 9 the rotation rows of the means are
replaced: angles in [1.2, 1.6] rad about seeded axes, so that every composed angle stays within [0.2, 2.6] -- the rotation log is not differentiable at pi and
the estimator's means are not drawn there -- and object 0 has aa = 0.  Every leading sub-map of the large one (1 .. 33 objects) is a slice of the large map's
reference: the moved sub-map is the marginal of the moved map.

Transforms: a generic one (od 7: psi = 0.7, t = (3, -2, 0.5); od 9: 0.9 rad about the skew axis (1, -2, 2) / 3), a pure translation, the identity and, for
od 7, psi = 3.1 (near pi).  For od 9 a transform near pi would carry composed angles to pi and is left out.  Each is used without a covariance and with
Sigma = 1e-2 (A A^T + dT I), rotation rows and columns scaled by 0.1, plus a small antisymmetric part (the entry symmetrises).  The large maps take the generic
transform only (each reference there is a 500- to 640-row inverse in long double).

The chain (od 7): B holds 8 objects of the small map A, seen from another frame with independent noise, and 4 objects only B has.  It is moved by an estimate
of the transform that is off by half a sigma of its Sigma, joined to A, matched, resolved and merged.  A's means are taken as the truth of A's objects: the
small map's covariance (sigma about 1.2) is wider than its objects are apart, so a typical draw of A could not be matched by anything."""
import collections
import functools

import numpy as np

import map_match_cases
import map_merge_cases
from map_update_cases import LD, N_SMALL, inverse, map_information, map_of, sym
from test_gpu_map_pair_priors import inv_ld, spd
from map_support import errors  # noqa: F401  (the tests call it as cases.errors)

N_SWEEP = 33
DT = {7: 4, 9: 6}
TRANSFORMS = {7: ("generic", "translation", "identity", "near_pi"), 9: ("generic", "translation", "identity")}
# (map, od, transform, with Sigma)
CASES = [("small", od, t, s) for od in (7, 9) for t in TRANSFORMS[od] for s in (False, True)] + [("large", od, "generic", s) for od in (7, 9) for s in (False, True)]


def transform_of(name, od):
    t = np.array([3.0, -2.0, 0.5])
    if od == 7:
        psi = {"generic": 0.7, "translation": 0.0, "identity": 0.0, "near_pi": 3.1}[name]
        return np.concatenate([np.zeros(3) if name == "identity" else t, [psi]])
    a = 0.9 * np.array([1.0, -2.0, 2.0]) / 3.0 if name == "generic" else np.zeros(3)
    return np.concatenate([np.zeros(3) if name == "identity" else t, a])


@functools.lru_cache(maxsize=None)
def sigma_of(od, seed=0):
    """The transform's covariance as the caller hands it over: not symmetric."""
    dT = DT[od]
    rng = np.random.default_rng(800 + od + seed)
    A = rng.normal(size=(dT, dT))
    S = 1e-2 * (A @ A.T + dT * np.eye(dT))
    s = np.ones(dT)
    s[3:] = 0.1
    S = S * s[:, None] * s[None, :]
    R = rng.normal(size=(dT, dT))
    S = S + 1e-6 * np.abs(S).max() * (R - R.T)
    S.setflags(write=False)
    return S


# ---- rotations, in any float type ------------------------------------------------------------------------------------------------------------------------------
def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=v.dtype)


def _abc(th, dtype):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3, by series below 1e-3."""
    if th < 1e-3:
        t2 = th * th
        return 1 - t2 / 6 + t2 * t2 / 120, dtype(0.5) - t2 / 24 + t2 * t2 / 720, dtype(1) / 6 - t2 / 120 + t2 * t2 / 5040
    h = np.sin(th / 2) / (th / 2)
    return np.sin(th) / th, h * h / 2, (th - np.sin(th)) / (th * th * th)


def exp_so3(a):
    dtype = a.dtype.type
    th = np.sqrt(a @ a)
    A, B, _ = _abc(th, dtype)
    H = hat(a)
    return np.eye(3, dtype=dtype) + A * H + B * (H @ H)


def log_so3(R):
    """Angle in [0, pi]; exact at the identity."""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=R.dtype) / 2
    s, c = np.sqrt(v @ v), (np.trace(R) - 1) / 2
    return v if s == 0 else (np.arctan2(s, c) / s) * v


def left_jacobian(a):
    dtype = a.dtype.type
    _, B, C = _abc(np.sqrt(a @ a), dtype)
    H = hat(a)
    return np.eye(3, dtype=dtype) + B * H + C * (H @ H)


def left_jacobian_inverse(a):
    dtype = a.dtype.type
    th = np.sqrt(a @ a)
    H = hat(a)
    k = dtype(1) / 12 + th * th / 720 if th < 1e-3 else 1 / (th * th) - (1 + np.cos(th)) / (2 * th * np.sin(th))
    return np.eye(3, dtype=dtype) - H / 2 + k * (H @ H)


def rz(psi, dtype):
    c, s = np.cos(dtype(psi)), np.sin(dtype(psi))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=dtype)


# ---- the move ------------------------------------------------------------------------------------------------------------------------------------------------------
def g(T, x, od, dtype=LD):
    """x' [od] of one object."""
    T, x = np.asarray(T, dtype=dtype), np.asarray(x, dtype=dtype)
    out = x.copy()
    if od == 7:
        out[:3] = rz(T[3], dtype) @ x[:3] + T[:3]
        out[3] = x[3] + T[3]
    else:
        R = exp_so3(T[3:])
        out[:3] = R @ x[:3] + T[:3]
        out[3:6] = log_so3(R @ exp_so3(x[3:6]))
    return out


def move_means(T, mean, od, dtype=LD):
    return np.array([g(T, m, od, dtype) for m in np.asarray(mean).reshape(-1, od)], dtype=dtype)


def jacobians(T, mean, od, dtype=LD):
    """(J [n][K][K], Ji [n][K][K], G [n][K][dT]): the K = od - 3 moving rows of J_o, of J_o^-1 and of G_o, in closed form."""
    T, mu = np.asarray(T, dtype=dtype), np.asarray(mean, dtype=dtype).reshape(-1, od)
    n, K, dT = len(mu), od - 3, DT[od]
    J, Ji, G = (np.zeros((n, K, c), dtype=dtype) for c in (K, K, dT))
    for o in range(n):
        G[o, :3, :3] = np.eye(3, dtype=dtype)
        if od == 7:
            psi = T[3]
            c, s = np.cos(psi), np.sin(psi)
            J[o, :3, :3], J[o, 3, 3] = rz(psi, dtype), 1
            Ji[o, :3, :3], Ji[o, 3, 3] = rz(-psi, dtype), 1
            G[o, :3, 3] = np.array([[-s, -c, 0], [c, -s, 0], [0, 0, 0]], dtype=dtype) @ mu[o, :3]
            G[o, 3, 3] = 1
        else:
            R, Jl_a = exp_so3(T[3:]), left_jacobian(T[3:])
            new = log_so3(R @ exp_so3(mu[o, 3:6]))
            J[o, :3, :3], J[o, 3:, 3:] = R, left_jacobian_inverse(new) @ R @ left_jacobian(mu[o, 3:6])
            Ji[o, :3, :3], Ji[o, 3:, 3:] = R.T, left_jacobian_inverse(mu[o, 3:6]) @ R.T @ left_jacobian(new)
            G[o, :3, 3:] = -hat(R @ mu[o, :3]) @ Jl_a
            G[o, 3:, 3:] = left_jacobian_inverse(new) @ Jl_a
    return J, Ji, G


def _blocks(Jk, od):
    """[n][K][K] -> [n][od][od] with the identity on the dimensions."""
    n, K = len(Jk), od - 3
    out = np.zeros((n, od, od), dtype=Jk.dtype)
    out[:, :K, :K] = Jk
    out[:, K:, K:] = np.eye(3, dtype=Jk.dtype)
    return out


def _full(G, od):
    """[n][K][dT] -> [n od][dT] with zero dimension rows."""
    n, K, dT = G.shape
    out = np.zeros((n, od, dT), dtype=G.dtype)
    out[:, :K] = G
    return out.reshape(n * od, dT)


def congruence(Jb, M, od, transposed=False):
    """blockdiag(J_o) M blockdiag(J_o)^T block pair by block pair (transposed: blockdiag(J_o)^T M blockdiag(J_o))."""
    n = len(Jb)
    B = M.reshape(n, od, n, od)
    out = np.einsum("aki,akbl,blj->aibj", Jb, B, Jb) if transposed else np.einsum("aik,akbl,bjl->aibj", Jb, B, Jb)
    return out.reshape(n * od, n * od)


def formula(mean, cov, T, Sigma, od, dtype=np.float64):
    """(mean' [n][od], C') as the header states them."""
    Cs = sym(np.asarray(cov, dtype=dtype))
    J, _, G = jacobians(T, mean, od, dtype)
    C = congruence(_blocks(J, od), Cs, od)
    if Sigma is not None:
        Gf = _full(G, od)
        C = C + Gf @ sym(np.asarray(Sigma, dtype=dtype)) @ Gf.T
    return move_means(T, mean, od, dtype), C


def yardstick(mean, Lam, T, Sigma, od):
    """C' in long double from the map's information Lam = Cs^-1 (long double): the information form of the module's docstring."""
    _, Ji, G = jacobians(T, mean, od, LD)
    N = len(Lam)
    Lp = sym(congruence(_blocks(Ji, od), np.asarray(Lam, dtype=LD), od, transposed=True))       # Jt^-T Lam Jt^-1
    if Sigma is None:
        return inverse(Lp)
    Gf = _full(G, od)
    LG = Lp @ Gf
    W = inv_ld(sym(Gf.T @ LG + inv_ld(sym(np.asarray(Sigma, dtype=LD)))))           # the inverse of Lambda_z's (tau, tau) block
    return inverse(sym(Lp - LG @ W @ LG.T))                                          # tau marginalised in information form: the Schur complement


# ---- the maps and the cases ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_map(which, od):
    mean, cov = map_of(which, od)
    if od == 9:
        rng = np.random.default_rng(810 + len(mean))
        mean = np.array(mean)
        axis = rng.normal(size=(len(mean), 3))
        mean[:, 3:6] = axis / np.linalg.norm(axis, axis=1)[:, None] * rng.uniform(1.2, 1.6, len(mean))[:, None]
        mean[0, 3:6] = 0.0
        for name in TRANSFORMS[9]:
            ang = np.linalg.norm(move_means(transform_of(name, 9), mean[1:], 9, np.float64)[:, 3:6], axis=1)
            assert ang.min() >= 0.2 and ang.max() <= 2.6, (name, ang.min(), ang.max())
        mean.setflags(write=False)
    return mean, cov


def case_inputs(which, od, tname, with_sigma):
    mean, cov = case_map(which, od)
    return mean, cov, transform_of(tname, od), (sigma_of(od) if with_sigma else None)


@functools.lru_cache(maxsize=None)
def reference(which, od, tname, with_sigma):
    """(mean' [n][od], C') of one case in long double: the means by g, the covariance by the yardstick."""
    mean, _, T, Sigma = case_inputs(which, od, tname, with_sigma)
    C = yardstick(mean, map_information(which, od), T, Sigma, od)
    mu = move_means(T, mean, od)
    C.setflags(write=False); mu.setflags(write=False)
    return mu, C


def leading(mean, cov, n, od):
    return np.ascontiguousarray(mean[:n]), np.ascontiguousarray(cov[:n * od, :n * od])


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------------------------------
N_SHARED, N_EXTRA = 8, 4
Chain = collections.namedtuple("Chain", "od mean_a cov_a mean_b cov_b shared truth_extra T_true T_est Sigma")


@functools.lru_cache(maxsize=None)
def chain(od=7):
    assert od == 7
    rng = np.random.default_rng(840 + od)
    mean_a, cov_a = map_of("small", od)
    shared = np.sort(rng.permutation(N_SMALL)[:N_SHARED])
    truth_extra = rng.normal(size=(N_EXTRA, od))
    truth_extra[:, :3] *= 3.0                                          # B's own objects lie around A's, not among them
    T_true = np.array([-4.0, 2.5, 0.3, -1.1])                          # T_A<-B
    Sigma = sym(np.array(sigma_of(od, seed=1)))
    z = rng.normal(size=DT[od])
    T_est = T_true + 0.5 * np.linalg.cholesky(Sigma) @ (z / np.linalg.norm(z))     # delta^T Sigma^-1 delta = 0.25
    back = np.concatenate([-(rz(-T_true[3], np.float64) @ T_true[:3]), [-T_true[3]]])   # T_B<-A
    in_b = move_means(back, np.concatenate([mean_a[shared], truth_extra]), od, np.float64)
    nb = N_SHARED + N_EXTRA
    cov_b = spd(rng, nb * od, cond=1e2, scale=1e-4)
    mean_b = in_b + (np.linalg.cholesky(cov_b) @ rng.normal(size=nb * od)).reshape(nb, od)
    for a in (shared, truth_extra, T_true, T_est, Sigma, mean_b, cov_b):
        a.setflags(write=False)
    return Chain(od, mean_a, cov_a, mean_b, cov_b, shared, truth_extra, T_true, T_est, Sigma)


def planted(ch):
    return [(int(s), N_SMALL + i) for i, s in enumerate(ch.shared)]


def greedy(a, b, stat):
    """The resolver's rule (include/obvi_map_match.h), restated: (drop, keep)."""
    state, drop, keep = {}, [], []
    for i in sorted(range(len(a)), key=lambda i: (stat[i], a[i], b[i], i)):
        if state.get(int(a[i]), 0) in (0, 1) and state.get(int(b[i]), 0) == 0:
            state[int(a[i])], state[int(b[i])] = 1, 2
            drop.append(int(b[i])); keep.append(int(a[i]))
    return np.array(drop, np.uint32), np.array(keep, np.uint32)


ChainReference = collections.namedtuple("ChainReference", "moved_mean moved_cov joined_mean joined_cov match gate pairs drop keep fused_mean fused_cov")


def run_chain(ch, dtype=LD):
    """move, join, match, resolve, merge by the formulas of the three case modules."""
    od = ch.od
    mu_m, C_m = formula(ch.mean_b, ch.cov_b, ch.T_est, ch.Sigma, od, dtype)
    na, nb = len(ch.mean_a) * od, len(ch.mean_b) * od
    joined = np.zeros((na + nb, na + nb), dtype=dtype)
    joined[:na, :na], joined[na:, na:] = ch.cov_a, C_m
    mu_j = np.concatenate([np.asarray(ch.mean_a, dtype=dtype), mu_m])
    match = map_match_cases.formula(mu_j, joined, od, dtype=dtype)
    gate, count = map_match_cases.midpoint(match.stat, N_SHARED)
    found = np.flatnonzero(match.stat <= gate)
    pairs = [(int(match.a[i]), int(match.b[i])) for i in found]
    drop, keep = greedy(match.a[found], match.b[found], match.stat[found])
    mu_f, C_f = map_merge_cases.merge_formula(mu_j, joined, drop, keep, None, None, od, dtype=dtype)
    return ChainReference(mu_m, C_m, mu_j, joined, match, gate, pairs, drop, keep, mu_f, C_f)


@functools.lru_cache(maxsize=None)
def chain_reference(od=7):
    return run_chain(chain(od))


def extra_distances(ch, mean_extra):
    """Centre distances of B's own objects from their true places."""
    return np.linalg.norm(np.asarray(mean_extra, dtype=np.float64)[:, :3] - ch.truth_extra[:, :3], axis=1)
