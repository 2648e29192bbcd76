"""regression.py's deterministic sklearn estimators on the GPU (csrc/regress.hip), every cross-validation
fold in flight: LinearRegression (LR), ElasticNet (EN), BayesianRidge (BR), KNeighborsRegressor (KNR).

Each follows fit_model (regression.py:38-77) on the flattened stage-24 features: StandardScaler fitted on
the fold's training rows, the model fitted on the standardised training rows, predictions for the training
and the validation rows.  Float64 on the device; the host only reads results back.  DESIGN.md §6b has the
algorithms and the two documented deviations (LR's eigenvalue cut tau, KNR's tie rule).

    results, info = fit_lr(features, rewards, split)            # also fit_en, fit_br, fit_knr

features [N, ...] (flattened), rewards [N] or [k, N] (per-fold targets, e.g. normalised against each fold's
training set), split (k, N) bool, True = validation.  results: per fold {train_est, val_est (float64),
train_time, val_time}; info: coef, intercept, mean, scale [k, D] for the linear models, plus per model
rank / min_ratio (LR), znorm / tol / sweeps (EN), alpha / lambda / n_iter (BR), neighbors [k, N, n_neighbors]
(KNR: positions within the fold's training rows) and train_rows (KNR: each fold's training rows as dataset
indices, the order those positions count in).  There is no CPU path.
"""
import ctypes
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

LR_TAU = 1e-11        # eigenvalues of Z^T Z at or below tau * max are treated as exact dependencies
LR_WARN_RATIO = 1e-8  # the CLI warns when the smallest kept eigenvalue ratio is below this
EIGH_MAX_SWEEPS = 60
BUILT = ("LR", "EN", "BR", "KNR")


@dataclass
class ENOpt:
    """regression.py:86-90, and the solver's stopping rule."""
    alpha: float = 0.01
    l1_ratio: float = 0.5
    tol: float = 0.0          # absolute bound on the optimality residual |z|_2; 0: tol_rel * |Z^T y / n|_inf
    tol_rel: float = 1e-10
    max_sweeps: int = 200000


@dataclass
class BROpt:
    """regression.py:102-108, and BayesianRidge's own defaults."""
    alpha_1: float = 1e-6
    alpha_2: float = 1e-6
    lambda_1: float = 1e-6
    lambda_2: float = 1e-6
    tol: float = 1e-3
    max_iter: int = 300


@dataclass
class KNROpt:
    """regression.py:205-208."""
    n_neighbors: int = 500


_ENOPT, _BROPT, _KNROPT = ENOpt(), BROpt(), KNROpt()  # the defaults a call without opts uses (regression.py's _*OPT)


class _Folds:
    """The device arrays every fit shares: features, per-fold targets, training lists, scaler statistics."""

    def __init__(self, features, rewards, split, device):
        x = np.asarray(features, dtype=np.float64)
        self.x = np.ascontiguousarray(x.reshape(len(x), -1))
        self.split = np.asarray(split, dtype=bool)
        self.k, self.N = self.split.shape
        self.D = self.x.shape[1]
        assert len(self.x) == self.N
        y = np.asarray(rewards, dtype=np.float64)
        self.y = np.array(np.broadcast_to(y, (self.k, self.N)) if y.ndim == 1 else y.reshape(self.k, self.N), order="C")
        self.tr = [np.nonzero(~m)[0].astype(np.int32) for m in self.split]
        self.tr_off = np.concatenate([[0], np.cumsum([len(a) for a in self.tr])]).astype(np.int64)
        if not 1 <= self.D <= 255:
            raise ValueError(f"edgeml_amd.regress: {self.D} features; the solvers take 1 to 255")
        if min(len(a) for a in self.tr) < 1:
            raise ValueError("edgeml_amd.regress: a fold without training rows")
        self.device = device

    def upload(self):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        k, D = self.k, self.D
        self.g_x, self.g_y = t(self.x), t(self.y)
        self.g_tr, self.g_tro = t(np.concatenate(self.tr + [np.zeros(1, np.int32)])), t(self.tr_off)
        self.tro_host = (ctypes.c_int64 * (k + 1))(*[int(o) for o in self.tr_off])
        self.mean = torch.empty((k, D), dtype=torch.float64, device=self.device)
        self.scale = torch.empty_like(self.mean)
        self.ymean = torch.empty(k, dtype=torch.float64, device=self.device)
        L, p = ops.lib(), ops._ptr
        ops.check(L.edgedet_reg_scaler(p(self.g_x), self.N, D, p(self.g_y), p(self.g_tr), self.tro_host, p(self.g_tro),
                                       k, p(self.mean), p(self.scale), p(self.ymean), ops.stream_handle()))
        return self

    def gram(self):
        Dp = (self.D + 1 + 15) // 16 * 16
        G = torch.empty((self.k, Dp, Dp), dtype=torch.float64, device=self.device)
        L, p = ops.lib(), ops._ptr
        ops.check(L.edgedet_reg_gram(p(self.g_x), self.N, self.D, p(self.g_y), p(self.g_tr), self.tro_host,
                                     p(self.g_tro), self.k, p(self.mean), p(self.scale), p(self.ymean), p(G),
                                     ops.stream_handle()))
        return G

    def eigh(self, G):
        k, D = self.k, self.D
        L, p = ops.lib(), ops._ptr
        wb = int(L.edgedet_reg_workspace_size(k, D, 0, 0))
        ws = torch.empty(wb, dtype=torch.uint8, device=self.device)
        lam = torch.empty((k, D), dtype=torch.float64, device=self.device)
        vt = torch.empty((k, D, D), dtype=torch.float64, device=self.device)
        sweeps = torch.zeros(k, dtype=torch.int32, device=self.device)
        status = torch.zeros(k, dtype=torch.int32, device=self.device)
        off = torch.zeros((k, 2), dtype=torch.float64, device=self.device)
        ops.check(L.edgedet_reg_eigh(p(G), D, k, p(ws), wb, EIGH_MAX_SWEEPS, p(lam), p(vt), p(sweeps), p(status),
                                     p(off), ops.stream_handle()))
        st = status.cpu().numpy()
        if np.any(st != 0):
            o = off.cpu().numpy()
            bad = [f"fold {f + 1}: off-diagonal norm {o[f, 0]:.3e} > {o[f, 1]:.3e}" for f in np.nonzero(st)[0]]
            raise RuntimeError(f"Jacobi eigensolver did not converge in {EIGH_MAX_SWEEPS} sweeps: " + "; ".join(bad))
        return lam, vt, {"eigh_sweeps": sweeps.cpu().numpy(), "eigh_offnorm": off.cpu().numpy()}

    def predict(self, coef, t_fit):
        """Estimates of every row under every fold's linear model, split by the fold's mask."""
        k, N = self.k, self.N
        L, p = ops.lib(), ops._ptr
        out = torch.empty((k, N), dtype=torch.float64, device=self.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.check(L.edgedet_reg_predict(p(self.g_x), N, self.D, p(self.mean), p(self.scale), p(coef), p(self.ymean), k,
                                        p(out), ops.stream_handle()))
        torch.cuda.synchronize()
        per_image = (time.perf_counter() - t0) / (k * N)
        info = {"coef": coef.cpu().numpy(), "intercept": self.ymean.cpu().numpy(), "mean": self.mean.cpu().numpy(),
                "scale": self.scale.cpu().numpy(), "fit_time": t_fit}
        return self.results(out.cpu().numpy(), per_image), info

    def results(self, est, per_image):
        return [{"train_est": est[f][~self.split[f]], "val_est": est[f][self.split[f]], "train_time": per_image,
                 "val_time": per_image} for f in range(self.k)]


def _start(features, rewards, split, device):
    ops.need_device("edgeml_amd.regress")
    fo = _Folds(features, rewards, split, device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    return fo.upload(), t0


def _fit_time(t0):
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fit_lr(features, rewards, split, opts=None, device="cuda"):
    """LinearRegression(): the minimum-norm least-squares solution through the eigendecomposition of Z^T Z
    (eigenvalues <= LR_TAU * max dropped).  The intercept is the training mean of the target: the
    standardised columns are centred by construction."""
    fo, t0 = _start(features, rewards, split, device)
    G = fo.gram()
    lam, vt, einfo = fo.eigh(G)
    k, D = fo.k, fo.D
    coef = torch.empty((k, D), dtype=torch.float64, device=device)
    rank = torch.zeros(k, dtype=torch.int32, device=device)
    ratio = torch.zeros(k, dtype=torch.float64, device=device)
    p = ops._ptr
    ops.check(ops.lib().edgedet_reg_fit_lr(p(G), D, k, p(lam), p(vt), LR_TAU, p(coef), p(rank), p(ratio),
                                           ops.stream_handle()))
    results, info = fo.predict(coef, _fit_time(t0))
    info.update(einfo, rank=rank.cpu().numpy(), min_ratio=ratio.cpu().numpy(), tau=LR_TAU)
    return results, info


def fit_br(features, rewards, split, opts=None, device="cuda"):
    """BayesianRidge(alpha_1, alpha_2, lambda_1, lambda_2): sklearn's loop on the spectrum of Z^T Z."""
    opts = opts or _BROPT
    fo, t0 = _start(features, rewards, split, device)
    if min(len(a) for a in fo.tr) <= fo.D:
        raise ValueError("edgeml_amd.regress.fit_br needs more training rows than features in every fold")
    G = fo.gram()
    lam, vt, einfo = fo.eigh(G)
    k, D = fo.k, fo.D
    coef = torch.empty((k, D), dtype=torch.float64, device=device)
    hyper = torch.zeros((k, 2), dtype=torch.float64, device=device)
    n_iter = torch.zeros(k, dtype=torch.int32, device=device)
    p = ops._ptr
    ops.check(ops.lib().edgedet_reg_fit_br(p(G), D, fo.tro_host, p(fo.g_tro), k, p(lam), p(vt), opts.alpha_1,
                                           opts.alpha_2, opts.lambda_1, opts.lambda_2, opts.tol, opts.max_iter,
                                           p(coef), p(hyper), p(n_iter), ops.stream_handle()))
    results, info = fo.predict(coef, _fit_time(t0))
    h = hyper.cpu().numpy()
    info.update(einfo, alpha=h[:, 0].copy(), n_iter=n_iter.cpu().numpy())
    info["lambda"] = h[:, 1].copy()
    return results, info


def fit_en(features, rewards, split, opts=None, device="cuda"):
    """ElasticNet(alpha, l1_ratio): coordinate descent down to an optimality residual |z|_2 <= tol, so the
    coefficients are within |z| / (alpha (1 - l1_ratio)) of the unique optimum."""
    opts = opts or _ENOPT
    fo, t0 = _start(features, rewards, split, device)
    G = fo.gram()
    k, D = fo.k, fo.D
    coef = torch.empty((k, D), dtype=torch.float64, device=device)
    res = torch.zeros((k, 2), dtype=torch.float64, device=device)
    sweeps = torch.zeros(k, dtype=torch.int32, device=device)
    status = torch.zeros(k, dtype=torch.int32, device=device)
    p = ops._ptr
    ops.check(ops.lib().edgedet_reg_fit_en(p(G), D, fo.tro_host, p(fo.g_tro), k, opts.alpha, opts.l1_ratio,
                                           opts.tol_rel, opts.tol, opts.max_sweeps, p(coef), p(res), p(sweeps),
                                           p(status), ops.stream_handle()))
    t_fit = _fit_time(t0)
    st, r = status.cpu().numpy(), res.cpu().numpy()
    if np.any(st != 0):
        bad = [f"fold {f + 1}: |z| {r[f, 0]:.3e} > tol {r[f, 1]:.3e}" for f in np.nonzero(st)[0]]
        raise RuntimeError(f"ElasticNet coordinate descent did not converge in {opts.max_sweeps} sweeps: "
                           + "; ".join(bad))
    results, info = fo.predict(coef, t_fit)
    info.update(znorm=r[:, 0].copy(), tol=r[:, 1].copy(), sweeps=sweeps.cpu().numpy(), status=st)
    return results, info


def fit_knr(features, rewards, split, opts=None, device="cuda"):
    """KNeighborsRegressor(n_neighbors): exact brute-force neighbours on the standardised rows, ties at the
    k-th distance to the lowest training position, the mean summed in position order."""
    opts = opts or _KNROPT
    ops.need_device("edgeml_amd.regress")
    fo = _Folds(features, rewards, split, device)
    kn = int(opts.n_neighbors)
    for tr in fo.tr:
        if kn > len(tr):  # sklearn's wording (neighbors/_base.py kneighbors)
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {kn}, "
                             f"n_samples_fit = {len(tr)}, n_samples = {len(tr)}")
    if kn < 1:
        raise ValueError(f"Expected n_neighbors > 0. Got {kn}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fo.upload()
    k, N, D = fo.k, fo.N, fo.D
    L, p = ops.lib(), ops._ptr
    wb = int(L.edgedet_reg_workspace_size(k, D, N, int(fo.tr_off[-1])))
    ws = torch.empty(wb, dtype=torch.uint8, device=device)
    est = torch.empty((k, N), dtype=torch.float64, device=device)
    nbr = torch.empty((k, N, kn), dtype=torch.int32, device=device)
    ops.check(L.edgedet_knn_fit_predict(p(fo.g_x), N, D, p(fo.g_y), p(fo.g_tr), fo.tro_host, p(fo.g_tro), k,
                                        p(fo.mean), p(fo.scale), kn, p(ws), wb, p(est), p(nbr), ops.stream_handle()))
    t_fit = _fit_time(t0)
    info = {"neighbors": nbr.cpu().numpy(), "mean": fo.mean.cpu().numpy(), "scale": fo.scale.cpu().numpy(),
            "fit_time": t_fit, "n_neighbors": kn, "train_rows": [a.copy() for a in fo.tr]}
    return fo.results(est.cpu().numpy(), t_fit / (k * N)), info


FITS = {"LR": fit_lr, "EN": fit_en, "BR": fit_br, "KNR": fit_knr}
NAMES = {"LR": "Linear Regression", "EN": "Elastic Net", "BR": "Bayesian Ridge", "KNR": "K Neighbors Regressor"}


def model_data(name, info, fold, features=None, targets=None):
    """What wts{k}.pickle holds for one fold: plain numpy data, not sklearn objects.  A KNR model is its
    training set: given the dataset's features [N, ...] and the targets the fit took ([N] or [k, N]), the file
    also holds train (the fold's raw training rows, float64 [n, D], training-list order) and target (their
    targets [n]), which edgeml_amd.kpredict and the offloading cascade predict from."""
    m = {"model": name, "mean": info["mean"][fold].copy(), "scale": info["scale"][fold].copy()}
    if name == "KNR":
        m["n_neighbors"] = int(info["n_neighbors"])
        if features is not None and targets is not None:
            rows = info["train_rows"][fold]
            x = np.asarray(features, dtype=np.float64).reshape(len(features), -1)
            y = np.asarray(targets, dtype=np.float64)
            m.update(train=x[rows].copy(), target=(y if y.ndim == 1 else y[fold])[rows].copy())
        return m
    m.update(coef=info["coef"][fold].copy(), intercept=float(info["intercept"][fold]))
    if name == "LR":
        m.update(rank=int(info["rank"][fold]), tau=float(info["tau"]))
    elif name == "BR":
        m.update(alpha=float(info["alpha"][fold]), n_iter=int(info["n_iter"][fold]))
        m["lambda"] = float(info["lambda"][fold])
    elif name == "EN":
        m.update(znorm=float(info["znorm"][fold]), sweeps=int(info["sweeps"][fold]))
    return m
