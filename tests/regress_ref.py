"""A numpy float64 restatement of the four estimator regressors of csrc/regress.hip (LR, EN, BR, KNR behind
a StandardScaler), for the tests and for the fixture generator: the same algorithms, not the device code.
No sklearn here."""
import numpy as np

EPS = np.finfo(np.float64).eps
LR_TAU = 1e-11


def scaler(x_tr):
    """mean / scale in the device's summation order (four interleaved row groups, added in order), sklearn's
    _is_constant_feature rule for scale 1."""
    n = len(x_tr)

    def grouped(a):
        parts = []
        for rg in range(4):
            acc = np.zeros(a.shape[1])
            for row in a[rg::4]:
                acc = acc + row
            parts.append(acc)
        return ((parts[0] + parts[1]) + parts[2]) + parts[3]

    mean = grouped(x_tr) / n
    d = x_tr - mean
    var = grouped(d * d) / n
    nm = n * mean * EPS
    constant = var <= n * EPS * var + nm * nm
    return mean, np.where(constant, 1.0, np.sqrt(var)), constant


def standardise(x, mean, scale):
    return (x - mean) * (1.0 / scale)


def gram(z, yc):
    """The augmented Gram matrix [D + 1, D + 1] of (Z, yc)."""
    za = np.concatenate([z, yc[:, None]], 1)
    return za.T @ za


def lr_from_gram(G, tau=LR_TAU, eig=None):
    """Minimum-norm least squares through the eigendecomposition of G[:D,:D]: coef, rank, min kept ratio."""
    D = len(G) - 1
    lam, V = eig if eig is not None else np.linalg.eigh(G[:D, :D])
    lam = np.maximum(lam, 0.0)
    keep = lam > tau * lam.max()
    t = np.where(keep, (V.T @ G[:D, D]) / np.where(keep, lam, 1.0), 0.0)
    return V @ t, int(keep.sum()), float((lam[keep] / lam.max()).min())


def br_from_gram(G, n, alpha_1=1e-6, alpha_2=1e-6, lambda_1=1e-6, lambda_2=1e-6, tol=1e-3, max_iter=300, eig=None):
    """sklearn's BayesianRidge.fit loop in the eigenbasis.  Returns coef, alpha, lambda, n_iter and the list
    of sum |coef_old - coef| per iteration (index 0 unused)."""
    D = len(G) - 1
    lam, V = eig if eig is not None else np.linalg.eigh(G[:D, :D])
    lam = np.maximum(lam, 0.0)
    p = V.T @ G[:D, D]
    yy = G[D, D]
    alpha, lam_ = 1.0 / (yy / n + EPS), 1.0
    coef_old, dcs = None, []
    for it in range(max_iter):
        c = p / (lam + lam_ / alpha)
        coef = V @ c
        sse = (yy - 2.0 * np.sum(c * p)) + np.sum(lam * c * c)
        gamma = np.sum((alpha * lam) / (lam_ + alpha * lam))
        lam_ = (gamma + 2 * lambda_1) / (np.sum(coef ** 2) + 2 * lambda_2)
        alpha = (n - gamma + 2 * alpha_1) / (sse + 2 * alpha_2)
        dc = np.inf if coef_old is None else float(np.sum(np.abs(coef_old - coef)))
        dcs.append(dc)
        if it != 0 and dc < tol:
            break
        coef_old = coef.copy()
    coef = V @ (p / (lam + lam_ / alpha))
    return coef, float(alpha), float(lam_), it + 1, dcs


def en_residual(Q, q, w, alpha=0.01, l1_ratio=0.5):
    """|z|_2 for the subgradient z of 1/2 w'Qw - q.w + a r |w|_1 + 1/2 a (1 - r) |w|^2 closest to zero."""
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    g = Q @ w - q + l2 * w
    z = np.where(w != 0, g + l1 * np.sign(w), np.maximum(np.abs(g) - l1, 0.0))
    return float(np.linalg.norm(z))


def en_from_gram(G, n, alpha=0.01, l1_ratio=0.5, tol_rel=1e-10, tol=0.0, max_sweeps=200000):
    """Covariance-form cyclic coordinate descent; returns coef, |z|, tol, sweeps."""
    D = len(G) - 1
    Q, q = G[:D, :D] / n, G[:D, D] / n
    l1, l2 = alpha * l1_ratio, alpha * (1 - l1_ratio)
    tol = tol if tol > 0 else tol_rel * np.abs(q).max()
    w, h = np.zeros(D), -q.copy()
    for sweep in range(max_sweeps + 1):
        if en_residual(Q, q, w, alpha, l1_ratio) <= tol:
            break
        for j in range(D):
            tmp = Q[j, j] * w[j] - h[j]
            wn = np.sign(tmp) * max(abs(tmp) - l1, 0.0) / (Q[j, j] + l2)
            if wn != w[j]:
                h += (wn - w[j]) * Q[:, j]
                w[j] = wn
    return w, en_residual(Q, q, w, alpha, l1_ratio), tol, sweep


def sqdist_direct(zq, zt):
    """Squared distances by direct differences, [n_q, n_t]."""
    out = np.empty((len(zq), len(zt)))
    for i, a in enumerate(zq):
        d = zt - a
        out[i] = np.sum(d * d, 1)
    return out


def knr_exact(d2, y_tr, k):
    """The k nearest by (distance, position); returns the sorted neighbour positions [n_q, k], the estimates
    (summed in position order) and the k-th distance."""
    n_q, n_t = d2.shape
    nbr = np.empty((n_q, k), np.int64)
    for i in range(n_q):
        order = np.lexsort((np.arange(n_t), d2[i]))[:k]
        nbr[i] = np.sort(order)
    est = np.array([sum_in_order(y_tr[nb]) / k for nb in nbr])
    dk = np.sort(d2, 1)[:, k - 1]
    return nbr, est, dk


def sum_in_order(v):
    acc = 0.0
    for a in v:
        acc += float(a)
    return acc


def knr_band(zq, zt, D):
    """beta = 2 (D + 4) eps (|a|^2 + max |b|^2): the dot-product rounding bound on |a|^2 + |b|^2 - 2 a.b."""
    return 2.0 * (D + 4) * EPS * (np.sum(zq * zq, 1) + np.sum(zt * zt, 1).max())
