"""A numpy float64 restatement of prediction from a saved SVR / KNR model (csrc/kpredict.hip), for the tests:
the same functions of (feature row, model), by direct differences, not the device code.  No sklearn here."""
import numpy as np

from tests import regress_ref as R

EPS = np.finfo(np.float64).eps


def numpy_scaler(x_tr):
    """mean / standard deviation with numpy's own sums; scale 1 for a constant column."""
    mean, scale = x_tr.mean(0), x_tr.std(0)
    return mean, np.where(np.ptp(x_tr, axis=0) == 0, 1.0, scale)


def svr_predict(feat, m):
    """sum_j beta_j exp(-gamma |z_q - z_j|^2) + intercept; m: a dict in the SVR file's layout."""
    zq = R.standardise(np.asarray(feat, np.float64), m["mean"], m["scale"])
    zs = R.standardise(m["support"], m["mean"], m["scale"])
    if len(zs) == 0:
        return np.full(len(zq), float(m["intercept"]))
    return np.exp(-m["gamma"] * R.sqdist_direct(zq, zs)) @ m["beta"] + m["intercept"]


def svr_gate(feat, m, est):
    """Per query: 2 sum_j |beta_j| (gamma band_qj + 4 eps) + 2 n_sv eps sum_j |beta_j| + 2 eps |est_q| with
    band_qj = 2 (D + 4) eps (|z_q|^2 + |z_j|^2): the rounding bound on a kernel entry computed as |a|^2 + |b|^2 -
    2 a.b and passed through exp, once for the device and once for the reference, each against exact
    arithmetic; the reordering bound of a sum of n_sv terms; the intercept add."""
    zq = R.standardise(np.asarray(feat, np.float64), m["mean"], m["scale"])
    zs = R.standardise(m["support"], m["mean"], m["scale"])
    D, a = zq.shape[1], np.abs(m["beta"])
    band = 2.0 * (D + 4) * EPS * (np.sum(zq * zq, 1)[:, None] + np.sum(zs * zs, 1)[None, :])
    return 2.0 * ((m["gamma"] * band + 4 * EPS) @ a) + 2.0 * len(a) * EPS * a.sum() + 2.0 * EPS * np.abs(est)


def knr_predict(feat, m):
    """The k nearest training rows by (distance, position): positions [B, k] ascending, the estimates summed in
    position order, the distances [B, n], the k-th distance and the band within which a neighbour set may
    differ; m: a dict in the KNR file's layout."""
    zq = R.standardise(np.asarray(feat, np.float64), m["mean"], m["scale"])
    zt = R.standardise(m["train"], m["mean"], m["scale"])
    d2 = R.sqdist_direct(zq, zt)
    nbr, est, dk = R.knr_exact(d2, m["target"], int(m["n_neighbors"]))
    return nbr, est, d2, dk, R.knr_band(zq, zt, zq.shape[1])


def check_knr(feat, m, est, nbr):
    """The device's result against the restatement: the estimate is the mean over the returned set in position
    order, exactly; the set is the exact one where no second distance lies within the band of the k-th, and
    otherwise holds everything closer than the band and nothing farther.  Returns the share of clear rows."""
    k = int(m["n_neighbors"])
    nbr_x, est_x, d2, dk, band = knr_predict(feat, m)
    assert nbr.shape == nbr_x.shape and np.all(np.diff(nbr, axis=1) > 0)
    assert nbr.min() >= 0 and nbr.max() < len(m["train"])
    clear = (np.abs(d2 - dk[:, None]) <= band[:, None]).sum(1) == 1
    for i in range(len(est)):
        assert est[i] == R.sum_in_order(m["target"][nbr[i]]) / k, i
        if clear[i]:
            assert np.array_equal(nbr[i], nbr_x[i]), i
            assert est[i] == est_x[i], i
        else:
            closer = np.nonzero(d2[i] < dk[i] - band[i])[0]
            assert np.all(np.isin(closer, nbr[i])) and np.all(d2[i][nbr[i]] <= dk[i] + band[i]), i
    return float(clear.mean())
