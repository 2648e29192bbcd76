"""A numpy float64 restatement of the two support vector regressors of csrc/svr.hip, for the tests and for the
fixture generator: both objectives, both duals, libsvm's KKT violation and two small solvers.  The same
algorithms, not the device code.  No sklearn here.

SVR (rbf):  dual   W(beta) = 1/2 beta^T K beta - y^T beta + eps |beta|_1,  -C <= beta <= C, sum beta = 0 (minimised)
            primal P(beta, b) = 1/2 beta^T K beta + C sum_i max(0, |y_i - (K beta)_i - b| - eps)
            gap = P + W >= W(beta) - W(beta*) >= 1/2 (beta - beta*)^T K (beta - beta*) for every feasible beta, any b.
LSVR:       primal P(v) = 1/2 |v|^2 + C sum_i max(0, |y_i - v.x~_i| - eps), x~ = (z, 1)
            dual   D(beta) = -1/2 |X~^T beta|^2 + y^T beta - eps |beta|_1, |beta_i| <= C (maximised)
            gap = P(X~^T beta) - D(beta) >= P(v) - P(v*) >= 1/2 |v - v*|^2.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
TAU = 1e-12


def gamma_scale(z):
    """sklearn's gamma='scale'."""
    var = z.var()
    return 1.0 / (z.shape[1] * var) if var != 0 else 1.0


def rbf(za, zb, gamma):
    """exp(-gamma |a - b|^2) by direct differences, [n_a, n_b]."""
    out = np.empty((len(za), len(zb)))
    for i, a in enumerate(za):
        d = zb - a
        out[i] = np.exp(-gamma * np.sum(d * d, 1))
    return out


# --------------------------------------------------------------------------------------------- SVR
def svr_dual(K, y, beta, eps):
    return 0.5 * beta @ K @ beta - y @ beta + eps * np.abs(beta).sum()


def svr_primal(K, y, beta, b, C, eps):
    return 0.5 * beta @ K @ beta + C * np.maximum(np.abs(y - K @ beta - b) - eps, 0.0).sum()


def svr_gap(K, y, beta, b, C, eps):
    return float(svr_primal(K, y, beta, b, C, eps) + svr_dual(K, y, beta, eps))


def svr_up_down(K, y, beta, C, eps):
    """-u over the coordinates that can rise, -d over those that can fall (-inf / +inf elsewhere)."""
    g = K @ beta - y
    up = np.where(beta < C, -(g + np.where(beta >= 0, eps, -eps)), -np.inf)
    down = np.where(beta > -C, -(g + np.where(beta > 0, eps, -eps)), np.inf)
    return g, up, down


def svr_violation(K, y, beta, C, eps):
    """libsvm's m(beta) - M(beta)."""
    _, up, down = svr_up_down(K, y, beta, C, eps)
    return float(up.max() - down.min())


def svr_free(beta, C):
    return (beta != 0) & (np.abs(beta) < C)


def svr_intercept(K, y, beta, C, eps):
    """libsvm's rule: the mean over the free support vectors, the midpoint of [M, m] without any."""
    g, up, down = svr_up_down(K, y, beta, C, eps)
    free = svr_free(beta, C)
    if free.any():
        return float(np.mean(-(g[free] + eps * np.sign(beta[free]))))
    return float(0.5 * (up.max() + down.min()))


def svr_feasible(beta, C):
    """The residual sum moved onto the free coordinate with the most room: an exact dual point."""
    beta = beta.copy()
    free = np.nonzero(svr_free(beta, C))[0]
    s = beta.sum()
    if len(free) and s != 0.0:
        i = free[np.argmax(np.minimum(C - np.abs(beta[free]), np.abs(beta[free])))]
        assert abs(s) < min(C - abs(beta[i]), abs(beta[i]))
        beta[i] -= s
    return beta


def svr_smo(K, y, C, eps, tol=1e-12, max_iter=2000000):
    """SMO on the signed dual variable with second-order working-set selection; returns beta, b, violation,
    iterations."""
    n = len(y)
    beta, g = np.zeros(n), -y.astype(np.float64).copy()
    kd = np.diag(K).copy()
    viol, verified, it = np.inf, False, 0
    while True:
        up = np.where(beta < C, -(g + np.where(beta >= 0, eps, -eps)), -np.inf)
        dn = g + np.where(beta > 0, eps, -eps)
        i = int(np.argmax(up))
        gmax = up[i]
        low = beta > -C
        viol = gmax - np.min(np.where(low, -dn, np.inf))
        gain = np.where(low, gmax + dn, 0.0)
        if viol <= tol or not np.any(gain > 0):
            if verified:
                break
            g, verified = K @ beta - y, True
            continue
        verified = False
        if it >= max_iter:
            break
        curv = kd[i] + kd - 2.0 * K[i]
        curv = np.where(curv <= 0, TAU, curv)
        j = int(np.argmax(np.where(gain > 0, gain * gain / curv, -np.inf)))
        room_i = -beta[i] if beta[i] < 0 else C - beta[i]
        room_j = beta[j] if beta[j] > 0 else beta[j] + C
        room = min(room_i, room_j)
        delta = min(gain[j] / curv[j], room)
        nbi = (0.0 if beta[i] < 0 else C) if delta == room_i else beta[i] + delta
        nbj = (0.0 if beta[j] > 0 else -C) if delta == room_j else beta[j] - delta
        g += delta * (K[i] - K[j])
        beta[i], beta[j] = nbi, nbj
        it += 1
    return beta, svr_intercept(K, y, beta, C, eps), float(viol), it


# -------------------------------------------------------------------------------------------- LSVR
def with_bias(z):
    return np.concatenate([z, np.ones((len(z), 1))], 1)


def lsvr_primal(xt, y, v, C, eps):
    return 0.5 * v @ v + C * np.maximum(np.abs(y - xt @ v) - eps, 0.0).sum()


def lsvr_dual(xt, y, beta, eps):
    v = xt.T @ beta
    return -0.5 * v @ v + y @ beta - eps * np.abs(beta).sum()


def lsvr_gap(xt, y, beta, C, eps):
    return float(lsvr_primal(xt, y, xt.T @ beta, C, eps) - lsvr_dual(xt, y, beta, eps))


def lsvr_free(beta, C):
    return (beta != 0) & (np.abs(beta) < C)


def lsvr_cd(xt, y, C, eps, tol=0.0, tol_rel=1e-10, max_sweeps=100000, check=10):
    """Exact dual coordinate descent in natural cyclic order (soft threshold, then clip); returns beta,
    v = X~^T beta, the gap, the sweeps."""
    n = len(y)
    h = np.sum(xt * xt, 1)
    beta, v = np.zeros(n), np.zeros(xt.shape[1])
    tol = tol if tol > 0 else tol_rel * lsvr_primal(xt, y, v, C, eps)
    sweep = 0
    while True:
        if sweep % check == 0 or sweep >= max_sweeps:
            v = xt.T @ beta
            gap = lsvr_gap(xt, y, beta, C, eps)
            if gap <= tol or sweep >= max_sweeps:
                break
        for i in range(n):
            u = beta[i] - (xt[i] @ v - y[i]) / h[i]
            bn = min(max(np.sign(u) * max(abs(u) - eps / h[i], 0.0), -C), C)
            if bn != beta[i]:
                v += (bn - beta[i]) * xt[i]
                beta[i] = bn
        sweep += 1
    return beta, xt.T @ beta, gap, sweep
