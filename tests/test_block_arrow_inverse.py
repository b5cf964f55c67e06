"""The identity a collective covariance pass rests on (include/obvi_cov.h), in plain numpy on a random block-arrow SPD matrix:
K diagonal blocks A_k (the members' own reduced systems), a dense tail T (the shared objects) and the couplings B_k between each block and
the tail -- no coupling between two blocks.

    M = [ A_1            B_1 ]
        [      ...       ... ]
        [           A_K  B_K ]
        [ B_1^T ... B_K^T  T ]

1. The tail block of M^-1 is the inverse of T minus the SUM of the members' Schur complements B_k^T A_k^-1 B_k: what collective (2) sums.
2. The Takahashi recursion over the Cholesky factor of M, run from the root (the tail) down and restricted to ONE diagonal block plus the
   tail, reproduces that block of the full inverse: a member needs its own columns of the factor and the tail's, nothing of the others."""
import numpy as np


def block_arrow(rng, sizes, tail):
    n = sum(sizes) + tail
    M = np.zeros((n, n))
    at, spans = 0, []
    for s in sizes:
        G = rng.standard_normal((s + tail + 3, s + tail))          # rows that see the block and the tail: A_k, B_k and a share of T
        H = G.T @ G
        M[at:at + s, at:at + s] += H[:s, :s]
        M[at:at + s, n - tail:] += H[:s, s:]
        M[n - tail:, at:at + s] += H[s:, :s]
        M[n - tail:, n - tail:] += H[s:, s:]
        spans.append((at, at + s))
        at += s
    M[n - tail:, n - tail:] += np.eye(tail)
    return M, spans, (n - tail, n)


def takahashi(L, rows):
    """Sigma = (L L^T)^-1 on the index set `rows` (ascending, closed under the elimination tree's ancestors) by the recursion
    Sigma_ik = -sum_{j in I(k)} Sigma_ij Y_jk, Sigma_kk = 1/L_kk^2 - sum_j Y_jk Sigma_jk, Y_jk = L_jk / L_kk, from the last column up; only entries
    inside `rows` are ever read."""
    rows = list(rows)
    pos = {r: x for x, r in enumerate(rows)}
    S = np.zeros((len(rows), len(rows)))
    for x in range(len(rows) - 1, -1, -1):
        k = rows[x]
        below = [j for j in rows[x + 1:] if L[j, k] != 0.0]
        y = np.array([L[j, k] / L[k, k] for j in below])
        b = [pos[j] for j in below]
        for i in rows[x + 1:]:
            S[pos[i], x] = S[x, pos[i]] = -S[pos[i], b] @ y if below else 0.0
        S[x, x] = 1.0 / L[k, k] ** 2 - (y @ S[b, x] if below else 0.0)
    return S


def test_the_tail_of_the_inverse_is_the_inverse_of_the_summed_schur_complements():
    rng = np.random.default_rng(7)
    M, spans, (t0, t1) = block_arrow(rng, [12, 7, 18, 6], 9)
    joint = M[t0:t1, t0:t1].copy()
    for a, b in spans:
        joint -= M[t0:t1, a:b] @ np.linalg.solve(M[a:b, a:b], M[a:b, t0:t1])
    want = np.linalg.inv(M)[t0:t1, t0:t1]
    got = np.linalg.inv(joint)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_the_recursion_on_one_block_and_the_tail_gives_that_block_of_the_full_inverse():
    rng = np.random.default_rng(11)
    M, spans, (t0, t1) = block_arrow(rng, [10, 14, 5], 8)
    L = np.linalg.cholesky(M)
    full = np.linalg.inv(M)
    for a, b in spans:
        # the factor has no entry that couples two members' blocks: a member's columns are its own
        others = [r for c, d in spans if (c, d) != (a, b) for r in range(c, d)]
        assert np.all(L[np.ix_(others, range(a, b))] == 0.0) and np.all(L[np.ix_(range(a, b), others)] == 0.0)
        rows = list(range(a, b)) + list(range(t0, t1))
        got = takahashi(L, rows)
        want = full[np.ix_(rows, rows)]
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    # and the member's columns of the joint factor are those of its OWN factor: L_kk from A_k, the tail rows B_k^T L_kk^-T
    a, b = spans[1]
    Lk = np.linalg.cholesky(M[a:b, a:b])
    assert np.abs(L[a:b, a:b] - Lk).max() <= 1e-12 * np.abs(Lk).max()
    assert np.abs(L[t0:t1, a:b] - np.linalg.solve(Lk, M[a:b, t0:t1]).T).max() <= 1e-11 * np.abs(L[t0:t1, a:b]).max()
