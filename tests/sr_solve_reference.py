"""Test systems and error measures for ``naqs_net_sr_solve`` (a plain helper module, like sr_reference.py; numpy only, seeded).

``system(M, F, shift, seed)`` builds a system with the structure of the natural-gradient step's own (include/naqs_hip.h,
naqs_net_sr_gram): a Jacobian J [M, F] of rank F < M with columns spread over decades, weights w, the centred Gram matrix
T = D (G - m 1^T - 1 m^T + c) D of G = J J^T (rank-deficient: sqrt(w) is a null vector) plus shift x the mean diagonal, and a
right-hand side y = g / (2 sqrt w).  ``pair(M, shift)`` is the (amplitude, phase) pair the tests solve in one call.

``blocked_model`` is the algorithm of csrc/naqs_sr_solve.hip in float64 numpy — 64-wide block columns, right-looking, the
right-hand side carried as one more row, then the back substitution block by block — for rehearsing the measures on the CPU.

Measures, in np.longdouble on the host, u = 2^-53:
    eta = |T x - y|_inf / (|T|_inf |x|_inf + |y|_inf)          normwise backward error of the solution
    rho = |L L^T - T|_inf / |T|_inf                            backward error of the factor (L: the returned lower triangle;
                                                               T symmetric); ``rho_rows``: the numerator on sampled rows
    fwd = |x - x_lapack|_inf / |x_lapack|_inf                  against scipy.linalg.cho_solve on the CPU
Bounds: eta, rho <= max(M, 16) u (far inside Cholesky's worst-case theory, gamma_{3M+1} M); fwd <= cond_2(T) max(M, 16) u.
LAPACK and the blocked model sit at eta <= 6.5e-17 over the tests' 33 size / shift cases; one float32 rounding anywhere in the
chain (6e-8) lands far outside.
"""
import numpy as np

U = 2.0 ** -53
NB = 64
SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 200, 333, 777)
SHIFTS = (1e-2, 1e-3, 1e-6)


def system(M, F=None, shift=1e-3, seed=0):
    """(T [M, M], y [M]) float64."""
    F = max(1, min(40, M // 2)) if F is None else F
    rs = np.random.RandomState(seed)
    J = rs.normal(size=(M, F)) * np.exp(rs.normal(0.0, 2.0, F))[None, :]
    w = rs.random_sample(M) + 0.05
    w /= w.sum()
    sw = np.sqrt(w)
    G = J @ J.T
    m = G @ w
    T = sw[:, None] * (G - m[:, None] - m[None, :] + w @ m) * sw[None, :]
    T = 0.5 * (T + T.T)
    T = T + shift * np.trace(T) / M * np.eye(M)
    y = rs.normal(size=M) / (2.0 * sw)
    return np.ascontiguousarray(T), y


def pair(M, shift):
    """The amplitude-slot and phase-slot systems of size M: ((T_a, y_a), (T_phi, y_phi))."""
    return system(M, None, shift, 1000 + M), system(M, None, shift, 5000 + M)


def bound(M):
    return max(M, 16) * U


def _inf(a):
    a = np.abs(np.asarray(a, np.longdouble))
    return a.max() if a.ndim == 1 else a.sum(1).max()


def eta(T, x, y):
    T, x, y = (np.asarray(v, np.longdouble) for v in (T, x, y))
    return float(_inf(T @ x - y) / (_inf(T) * _inf(x) + _inf(y)))


def rho(T, L):
    """L: any [M, M] array whose lower triangle (with the diagonal) is the factor; the strict upper triangle is ignored."""
    Ll, Tl = np.tril(np.asarray(L, np.longdouble)), np.asarray(T, np.longdouble)
    M, B = len(Ll), 96
    E = np.zeros((M, M), np.longdouble)
    for i in range(0, M, B):                  # both are symmetric: the lower blocks, each over the columns where L is not zero
        for j in range(0, i + 1, B):
            E[i:i + B, j:j + B] = Ll[i:i + B, :j + B] @ Ll[j:j + B, :j + B].T - Tl[i:i + B, j:j + B]
            E[j:j + B, i:i + B] = E[i:i + B, j:j + B].T
    return float(_inf(E) / _inf(Tl))


def rho_rows(T, L, rows):
    """rho on sampled rows, for sizes where the whole product is too slow in longdouble: |L[rows] L^T - T[rows]|_inf / |T|_inf
    (L as for ``rho``; the norm of the numerator is the largest row sum over ``rows``)."""
    rows = np.asarray(rows)
    worst = np.longdouble(0)
    for r in rows:                            # row r of L L^T: L[r, :r + 1] against the first r + 1 columns of every row
        lr = np.asarray(L[r, :r + 1], np.longdouble)
        Lc = np.array(L[:, :r + 1], np.longdouble)
        Lc[:r + 1] = np.tril(Lc[:r + 1])      # (the strict upper triangle is ignored)
        worst = max(worst, np.abs(Lc @ lr - np.asarray(T[r], np.longdouble)).sum())
    tnorm = max(np.abs(np.asarray(T[i:i + 256], np.longdouble)).sum(1).max() for i in range(0, len(T), 256))
    return float(worst / tnorm)


def fwd(x, x_ref):
    return float(_inf(np.asarray(x, np.longdouble) - np.asarray(x_ref, np.longdouble)) / _inf(x_ref))


def lapack_solve(T, y):
    """(x, info) by LAPACK on the CPU: dpotrf (lower) + dpotrs; info is dpotrf's."""
    from scipy.linalg import cho_solve, lapack
    c, info = lapack.dpotrf(T, lower=1)
    if info != 0:
        return np.full(len(y), np.nan), int(info)
    return cho_solve((c, True), y), 0


def _chol64(A):
    """Unblocked right-looking Cholesky of one diagonal block, column by column -> (L, first failed pivot or -1)."""
    A = A.copy()
    n = len(A)
    fail = -1
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            if not d > 0 and fail < 0:
                fail = j
            s = np.sqrt(d)
            A[j + 1:, j] /= s
            A[j, j] = s
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A), fail


def _rows_times_inv_lt(A, L):
    """A L^-T by forward substitution, column by column (times the reciprocal of the diagonal, as LAPACK's dtrsm)."""
    X = A.copy()
    for c in range(L.shape[0]):
        X[:, c] *= 1.0 / L[c, c]
        X[:, c + 1:] -= np.outer(X[:, c], L[c + 1:, c])
    return X


def blocked_model(T, y):
    """-> (x, L, info) as naqs_net_sr_solve computes them, in float64 numpy (potrf's info; x is NaN after a failure)."""
    A = np.array(T, np.float64)
    z = np.array(y, np.float64)
    M = len(z)
    nb = (M + NB - 1) // NB
    for k in range(nb):
        s = slice(k * NB, min(M, (k + 1) * NB))
        L, fail = _chol64(A[s, s])
        if fail >= 0:
            return np.full(M, np.nan), A, k * NB + fail + 1
        A[s, s] = L
        z[s] = _rows_times_inv_lt(z[None, s], L)[0]
        if s.stop < M:
            A[s.stop:, s] = _rows_times_inv_lt(A[s.stop:, s], L)
            A[s.stop:, s.stop:] -= A[s.stop:, s] @ A[s.stop:, s].T
            z[s.stop:] -= A[s.stop:, s] @ z[s]
    x = np.zeros(M)
    for k in range(nb - 1, -1, -1):
        s = slice(k * NB, min(M, (k + 1) * NB))
        L = A[s, s]
        xk = z[s].copy()
        for r in range(len(xk) - 1, -1, -1):
            xk[r] *= 1.0 / L[r, r]
            xk[:r] -= L[r, :r] * xk[r]
        x[s] = xk
        z[:s.start] -= A[s, :s.start].T @ xk
    return x, np.tril(A), 0
