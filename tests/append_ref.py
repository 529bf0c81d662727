"""NumPy restatement of pg_chol_append on the padded buffers the library keeps (include/pygpr_hip.h):

    L [n_pad x n_pad]     lower factor of K + jitter I on the first n rows, identity pad, strictly upper part scratch
    Minv [n_pad x n_pad]  L^-1, same layout
    invd [n_pad/128, 128, 128]  inverses of L's 128-blocks on the diagonal (= Minv's diagonal blocks), identity past n
    u = L^-1 y, alpha = Minv^T u  [n_pad], zero past n

`append` reads L and Minv through their lower triangles only (explicit bounds), as the kernels do, and returns the buffers of the n + k
problem, or the unchanged buffers and info = n + c + 1 when pivot c of the Schur complement is not > 0."""
import numpy as np

JITTER = 1e-7


def se_kernel(a, b, sigma=1.3, ell=0.8):
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return sigma ** 2 * np.exp(-0.5 * d2 / ell ** 2)


def lower(a):
    return np.tril(a)


def padded_fit(K, y, n_pad, garbage=None):
    """The padded state of a fit on K (already holding noise + jitter on its diagonal).  garbage: value (or None for random numbers) written
    into the strictly upper parts of L and Minv above their diagonal 128-blocks, which the library treats as scratch."""
    n = K.shape[0]
    L = np.eye(n_pad)
    L[:n, :n] = np.linalg.cholesky(K)
    M = np.linalg.inv(L)
    M = lower(M)
    invd = np.stack([M[b * 128:(b + 1) * 128, b * 128:(b + 1) * 128].copy() for b in range(n_pad // 128)])
    yp = np.zeros(n_pad)
    yp[:n] = y
    u = M @ yp
    alpha = M.T @ u
    rng = np.random.default_rng(0)
    for A in (L, M):
        for i in range(n_pad):
            c0 = (i // 128 + 1) * 128
            if c0 < n_pad:
                A[i, c0:] = rng.standard_normal(n_pad - c0) if garbage is None else garbage
    return L, invd, M, u, alpha


def grow(L, invd, M, u, alpha, n_pad):
    """blockdiag(., I) copies of the state at a larger padded size (Exact_GP.append before a block that crosses n_pad)."""
    m = L.shape[0]
    out = []
    for A in (L, M):
        B = np.eye(n_pad)
        B[:m, :m] = A
        out.append(B)
    iv = np.stack([np.eye(128)] * (n_pad // 128))
    iv[: m // 128] = invd
    uu, aa = np.zeros(n_pad), np.zeros(n_pad)
    uu[:m], aa[:m] = u, alpha
    return out[0], iv, out[1], uu, aa


def chol_info(S):
    """Unblocked Cholesky with the kernel's pivot test; (Ls, 0) or (None, c + 1)."""
    k = S.shape[0]
    A = lower(S).astype(np.float64)
    for c in range(k):
        piv = A[c, c]
        if not piv > 0:
            return None, c + 1
        d = np.sqrt(piv)
        A[c, c] = d
        A[c + 1:, c] /= d
        A[c + 1:, c + 1:] -= np.tril(np.outer(A[c + 1:, c], A[c + 1:, c]))
    return A, 0


def append(L, invd, M, u, alpha, n, Kt, Knn, yn):
    """One pg_chol_append: Kt [k x n_pad] (zero past n), Knn [k x k] (noise + jitter on the diagonal), yn [k]."""
    k = Knn.shape[0]
    n_pad = L.shape[0]
    assert 1 <= k <= 128 and n + k <= n_pad and n_pad % 256 == 0
    Ml = lower(M[:n, :n])
    Vt = Kt[:, :n] @ Ml.T
    S = Knn - Vt @ Vt.T
    Ls, c1 = chol_info(S)
    if c1:
        return L.copy(), invd.copy(), M.copy(), u.copy(), alpha.copy(), n + c1
    Lsi = lower(np.linalg.inv(Ls))
    W = -Lsi @ (Vt @ Ml)
    L2, M2, iv2, u2 = L.copy(), M.copy(), invd.copy(), u.copy()
    L2[n:n + k, :] = 0.0
    M2[n:n + k, :] = 0.0
    L2[n:n + k, :n] = Vt
    L2[n:n + k, n:n + k] = Ls
    M2[n:n + k, :n] = W
    M2[n:n + k, n:n + k] = Lsi
    for g in range(n, n + k):
        b = g // 128
        iv2[b, g % 128, :] = M2[g, b * 128:(b + 1) * 128]
    u2[n:n + k] = Lsi @ (yn - Vt @ u[:n])
    a2 = lower(M2).T @ u2
    return L2, iv2, M2, u2, a2, 0
