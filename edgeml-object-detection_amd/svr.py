"""regression.py's SVR (rbf) and LinearSVR on the GPU (csrc/svr.hip), every cross-validation fold in flight,
each solved to the optimum of its strongly convex objective.

Both follow fit_model (regression.py:38-77) on the flattened stage-24 features: StandardScaler fitted on the
fold's training rows (edgeml_amd.regress's), the model fitted on the standardised training rows, predictions for
the training and the validation rows.  Float64 on the device; the host only reads results back.

    results, info = fit_svr(features, rewards, split)      # SVR(kernel='rbf', C=0.05, epsilon=0.05), gamma='scale'
    results, info = fit_lsvr(features, rewards, split)     # LinearSVR(C=0.005, epsilon=0.005)

features, rewards, split and results are edgeml_amd.regress's.  info: mean, scale [k, D], beta (a list: each
fold's dual coefficients over its training rows), intercept [k], status; for SVR gamma, violation (libsvm's
m - M at the end), iterations; for LSVR coef [k, D], v [k, D + 1], gap, tol, sweeps.  The fitted function is
the unique optimum: sklearn stops at tol = 1e-3 (libsvm) / 1e-4 (liblinear) and liblinear shuffles, so its
estimates sit a small, measured distance away (tests/golden/g8_svr.npz).  There is no CPU path.

    python -m edgeml_amd.svr data_dir reward_path split_path save_dir --model SVR|LSVR [--normalize]
                             [--model-dir DIR] [--tol-rel 1e-4]

takes regression.py's arguments (and --tol-rel, LSVR's gap tolerance relative to P(0), for datasets where the
default 1e-10 takes too many sweeps), prints fit_model's MSE line per fold, writes estimate<k>.npz into save_dir and,
with --model-dir, wts<k>.pickle holding plain numpy data: for LSVR {model, mean, scale, coef, intercept, ...},
which edgeml_amd.offload loads as a linear model; for SVR {model, mean, scale, gamma, support (raw feature
rows), beta, intercept}, which edgeml_amd.kpredict predicts from (csrc/kpredict.hip) and the cascade loads as
kind "svr".
"""
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import estimator, ops
from .regress import _Folds

MAX_SVR_ROWS = 4000  # training rows per fold: the SMO gradient lives in LDS
NAMES = {"SVR": "Support Vector Regression", "LSVR": "Linear Support Vector Regression"}


@dataclass
class SVROpt:
    """regression.py:135-141, and the solver's stopping rule."""
    C: float = 0.05
    epsilon: float = 0.05
    kernel: str = "rbf"
    tol: float = 1e-9          # absolute bound on libsvm's maximal KKT violation m(beta) - M(beta)
    max_iter: int = 10000000


@dataclass
class LSVROpt:
    """regression.py:153-157, and the solver's stopping rule."""
    C: float = 0.005
    epsilon: float = 0.005
    tol: float = 0.0           # absolute bound on the duality gap; 0: tol_rel * P(0)
    tol_rel: float = 1e-10
    max_sweeps: int = 100000


_SVROPT, _LSVROPT = SVROpt(), LSVROpt()  # the defaults a call without opts uses (regression.py's _*OPT)


def _start(features, rewards, split, device, with_kernel):
    fo = _Folds(features, rewards, split, device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fo.upload()
    wb = int(ops.lib().edgedet_svr_workspace_size(fo.tro_host, fo.k, fo.D, int(with_kernel)))
    if wb < 0:
        raise ValueError("edgeml_amd.svr: bad fold sizes")
    ws = torch.empty(wb // 8, dtype=torch.float64, device=device)
    return fo, t0, ws, wb


def _per_fold(fo, flat):
    return [flat[fo.tr_off[f]:fo.tr_off[f + 1]].copy() for f in range(fo.k)]


def fit_svr(features, rewards, split, opts=None, device="cuda"):
    """SVR(kernel='rbf', C, epsilon), gamma='scale': SMO down to a maximal KKT violation <= tol."""
    opts = opts or _SVROPT
    if opts.kernel != "rbf":
        raise ValueError(f"edgeml_amd.svr: kernel '{opts.kernel}' is not built; only 'rbf' is")
    ops.need_device("edgeml_amd.svr")
    n_max = int((~np.asarray(split, dtype=bool)).sum(1).max())
    if n_max > MAX_SVR_ROWS:
        raise ValueError(f"edgeml_amd.svr.fit_svr: {n_max} training rows in a fold; the solver takes {MAX_SVR_ROWS}")
    fo, t0, ws, wb = _start(features, rewards, split, device, True)
    k, N, D, T = fo.k, fo.N, fo.D, int(fo.tr_off[-1])
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)  # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)  # noqa: E731
    beta, icpt, gamma, viol, iters, status = f64(T), f64(k), f64(k), f64(k), i32(k), i32(k)
    L, p = ops.lib(), ops._ptr
    ops.check(L.edgedet_svr_fit(p(fo.g_x), N, D, p(fo.g_y), p(fo.g_tr), fo.tro_host, p(fo.g_tro), k, p(fo.mean),
                                p(fo.scale), opts.C, opts.epsilon, opts.tol, opts.max_iter, p(ws), wb, p(beta), p(icpt),
                                p(gamma), p(viol), p(iters), p(status), ops.stream_handle()))
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    st, vi, it = status.cpu().numpy(), viol.cpu().numpy(), iters.cpu().numpy()
    if np.any(st != 0):
        bad = [f"fold {f + 1}: violation {vi[f]:.3e} > tol {opts.tol:.3e}" for f in np.nonzero(st)[0]]
        raise RuntimeError(f"SVR SMO did not converge in {opts.max_iter} iterations: " + "; ".join(bad))
    out = torch.empty((k, N), dtype=torch.float64, device=device)
    t1 = time.perf_counter()
    ops.check(L.edgedet_svr_predict(p(fo.g_x), N, D, p(fo.mean), p(fo.scale), fo.tro_host, p(fo.g_tro), k, p(ws), wb,
                                    p(beta), p(icpt), p(gamma), p(out), ops.stream_handle()))
    torch.cuda.synchronize()
    per_image = (time.perf_counter() - t1) / (k * N)
    info = {"mean": fo.mean.cpu().numpy(), "scale": fo.scale.cpu().numpy(), "beta": _per_fold(fo, beta.cpu().numpy()),
            "intercept": icpt.cpu().numpy(), "gamma": gamma.cpu().numpy(), "violation": vi, "iterations": it,
            "status": st, "fit_time": t_fit, "train_rows": [a.copy() for a in fo.tr]}
    return fo.results(out.cpu().numpy(), per_image), info


def fit_lsvr(features, rewards, split, opts=None, device="cuda"):
    """LinearSVR(C, epsilon): exact dual coordinate descent in natural order down to a duality gap <= tol, so
    |v - v*| <= sqrt(2 gap) for the unique optimum v* of the primal."""
    opts = opts or _LSVROPT
    ops.need_device("edgeml_amd.svr")
    fo, t0, ws, wb = _start(features, rewards, split, device, False)
    k, N, D, T = fo.k, fo.N, fo.D, int(fo.tr_off[-1])
    beta = torch.zeros(T, dtype=torch.float64, device=device)
    v = torch.zeros((k, D + 1), dtype=torch.float64, device=device)
    res = torch.zeros((k, 2), dtype=torch.float64, device=device)
    sweeps = torch.zeros(k, dtype=torch.int32, device=device)
    status = torch.zeros(k, dtype=torch.int32, device=device)
    L, p = ops.lib(), ops._ptr
    ops.check(L.edgedet_lsvr_fit(p(fo.g_x), N, D, p(fo.g_y), p(fo.g_tr), fo.tro_host, p(fo.g_tro), k, p(fo.mean),
                                 p(fo.scale), opts.C, opts.epsilon, opts.tol, opts.tol_rel, opts.max_sweeps, p(ws), wb,
                                 p(beta), p(v), p(res), p(sweeps), p(status), ops.stream_handle()))
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    st, r = status.cpu().numpy(), res.cpu().numpy()
    if np.any(st != 0):
        bad = [f"fold {f + 1}: gap {r[f, 0]:.3e} > tol {r[f, 1]:.3e}" for f in np.nonzero(st)[0]]
        raise RuntimeError(f"LinearSVR dual coordinate descent did not converge in {opts.max_sweeps} sweeps: "
                           + "; ".join(bad) + " (raise LSVROpt.max_sweeps, or loosen tol / tol_rel: the fit is "
                           "within sqrt(2 gap) of the optimum)")
    fo.ymean = v[:, D].contiguous()  # the intercept edgedet_reg_predict adds
    results, info = fo.predict(v[:, :D].contiguous(), t_fit)
    info.update(beta=_per_fold(fo, beta.cpu().numpy()), v=v.cpu().numpy(), gap=r[:, 0].copy(), tol=r[:, 1].copy(),
                sweeps=sweeps.cpu().numpy(), status=st)
    return results, info


FITS = {"SVR": fit_svr, "LSVR": fit_lsvr}


def model_data(name, info, fold, features=None):
    """What wts{k}.pickle holds for one fold: plain numpy data, not sklearn objects."""
    m = {"model": name, "mean": info["mean"][fold].copy(), "scale": info["scale"][fold].copy(),
         "intercept": float(info["intercept"][fold])}
    if name == "LSVR":
        m.update(coef=info["coef"][fold].copy(), gap=float(info["gap"][fold]), sweeps=int(info["sweeps"][fold]))
        return m
    beta = info["beta"][fold]
    sv = np.nonzero(beta)[0]
    rows = info["train_rows"][fold][sv]
    x = np.asarray(features, dtype=np.float64).reshape(len(features), -1)
    m.update(gamma=float(info["gamma"][fold]), support=x[rows].copy(), beta=beta[sv].copy(),
             violation=float(info["violation"][fold]), iterations=int(info["iterations"][fold]))
    return m


def main(opts):
    if opts.model not in FITS:
        raise SystemExit(f"edgeml_amd.svr builds --model SVR (Support Vector Regression, rbf) and LSVR (Linear "
                         f"Support Vector Regression); --model {opts.model} belongs to edgeml_amd.estimator")
    if opts.stage != 24:
        raise SystemExit("edgeml_amd.svr runs on the stage-24 output features (--stage 24); the hidden-layer "
                         "feature maps of stages 0-23 train a conv net: python -m edgeml_amd.convnet")
    features, reward, split = estimator.load_inputs(opts)
    y = estimator.fold_targets(reward, split, opts.normalize, np.float64)
    fit_opts = None
    if opts.model == "LSVR" and getattr(opts, "tol_rel", None) is not None:
        fit_opts = LSVROpt(tol_rel=opts.tol_rel)
    results, info = FITS[opts.model](features, y, split, fit_opts)
    estimator.report_folds(opts, NAMES[opts.model], y, split, results,
                           lambda fold: model_data(opts.model, info, fold, features))
    return results, info


def getargs(argv=None):
    a = estimator.base_parser("SVR", prog="python -m edgeml_amd.svr")
    a.add_argument("--tol-rel", type=float, default=None,
                   help="LSVR only: stop at a duality gap of this times P(0) (default 1e-10; large datasets want 1e-4)")
    return a.parse_args(argv)


if __name__ == "__main__":
    main(getargs())
