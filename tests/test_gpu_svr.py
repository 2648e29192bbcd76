"""SVR and LinearSVR of edgeml_amd.svr (csrc/svr.hip) against G8 (tests/golden/g8_svr.npz: regression.py's own
SVR / LSVR runs under sklearn 1.7.2 on G7's data, a certificate per model and fold, and the quantities the
bounds below are derived from; tests/golden/make_golden_svr.py).  No gate here is fitted to what the device
returns: each is a condition of the problem, a rounding bound, or follows from strong convexity:

  LSVR  P is 1-strongly convex in v, so |v - v*| <= sqrt(2 (P(v) - P*)) <= sqrt(2 gap) for any dual-feasible
        beta with v = X~^T beta; two such points are within sqrt(2 gap_1) + sqrt(2 gap_2) of each other and
        their estimates within that times |(z, 1)|.
  SVR   W(beta) - W(beta*) >= 1/2 |beta - beta*|_K^2 on the feasible set and gap >= W(beta) - W(beta*), so
        |beta_1 - beta_2|_K <= sqrt(2 gap_1) + sqrt(2 gap_2); |(K dbeta)_i| <= |dbeta|_K since K_ii = 1; at a free
        support vector both solutions share (same sign), y_i - (K beta)_i - b = +-eps up to each one's violation,
        so |b_1 - b_2| <= |dbeta|_K + viol_1 + viol_2, and the estimates differ by at most |dbeta|_K + |b_1 - b_2|.
The reference's default fits (tol 1e-3 / 1e-4) are held by the triangle inequality through the certificate,
with G8's stored max |est_cert - est_ref|.
"""
import os
import pickle

import numpy as np
import pytest

from tests import regress_ref as R
from tests import svr_ref as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def g8():
    g = {}
    for name in ("g7_regressors.npz", "g8_svr.npz"):
        with np.load(os.path.join(HERE, "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g8") or k in ("features", "reward", "split")})
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    ref = []
    for f, m in enumerate(g["split"]):  # the restatement, once
        tr = ~m
        mean, scale, _ = R.scaler(g["features"][tr])
        z = R.standardise(g["features"], mean, scale)
        gamma = float(g[f"SVR/gamma{f}"])
        ref.append({"tr": tr, "n": int(tr.sum()), "z": z, "y": g["reward"][tr], "gamma": gamma,
                    "K": S.rbf(z[tr], z[tr], gamma), "xt": S.with_bias(z[tr]), "rows": np.linalg.norm(S.with_bias(z), axis=1)})
    g["ref"] = ref
    return g


@pytest.fixture(scope="module")
def fits(g8):
    """Both models fitted once on all folds; shared, never modified."""
    from edgeml_amd import svr
    return {name: svr.FITS[name](g8["features"], g8["reward"], g8["split"]) for name in ("SVR", "LSVR")}


def all_rows(g, results, f):
    est = np.empty(len(g["reward"]))
    est[~g["split"][f]], est[g["split"][f]] = results[f]["train_est"], results[f]["val_est"]
    return est


# ---------------------------------------------------------------------------------- kernel matrix
def kernel_matrix(z, gamma_in=0.0):
    import torch
    from edgeml_amd import ops
    n, D = z.shape
    g_z = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    nrm = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    gam = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    K = torch.full((n, n), np.nan, dtype=torch.float64, device="cuda")
    ops.check(ops.lib().edgedet_svr_kernel_matrix(ops._ptr(g_z), n, D, gamma_in, ops._ptr(nrm), ops._ptr(gam), ops._ptr(K),
                                                  ops.stream_handle()))
    torch.cuda.synchronize()
    return K.cpu().numpy(), float(gam.cpu().numpy()[0]), nrm.cpu().numpy()


def check_kernel_matrix(z, what, gamma_ref=None):
    n, D = z.shape
    K, gamma, nrm = kernel_matrix(z)
    want = S.gamma_scale(z) if gamma_ref is None else gamma_ref
    print(f"{what}: gamma {gamma!r} (reference {want!r}), bound {n * D * EPS:.3e} relative")
    assert abs(gamma - want) <= n * D * EPS * want
    band = R.knr_band(z, z, D)  # the rounding bound on |a|^2 + |b|^2 - 2 a.b, per row
    err = np.abs(K - S.rbf(z, z, gamma))
    gate = gamma * band[:, None] + 4 * EPS
    print(f"{what}: max |K - K_numpy| {err.max():.3e}, max err / gate {(err / gate).max():.3f}")
    assert np.all(err <= gate)
    assert np.all(np.abs(nrm - np.sum(z * z, 1)) <= D * EPS * np.sum(z * z, 1))
    K2, gamma2, _ = kernel_matrix(z, gamma_in=0.25)
    assert gamma2 == 0.25 and np.all(np.abs(K2 - S.rbf(z, z, 0.25)) <= 0.25 * band[:, None] + 4 * EPS)


def test_kernel_matrix_19_by_34():
    """Neither size is a multiple of the 16 x 16 tile or of the k-step of four."""
    check_kernel_matrix(np.random.default_rng(8).normal(0, 1, (19, 34)), "19 x 34")


def test_kernel_matrix_of_a_fold(g8):
    r = g8["ref"][1]
    assert r["n"] % 16 != 0 and r["n"] > 64  # more than one workgroup along both axes
    check_kernel_matrix(np.ascontiguousarray(r["z"][r["tr"]]), "fold 1", gamma_ref=r["gamma"])


def test_gamma_is_sklearns(g8, fits):
    for f, r in enumerate(g8["ref"]):
        gamma = fits["SVR"][1]["gamma"][f]
        print(f"fold {f}: gamma {gamma!r}, sklearn {r['gamma']!r}")
        assert abs(gamma - r["gamma"]) <= r["n"] * g8["D"] * EPS * r["gamma"]
        assert abs(r["gamma"] - 1 / 32) <= 64 * EPS  # 32 unit-variance columns and two constant ones


# ------------------------------------------------------------------------------------------- LSVR
def test_lsvr(g8, fits):
    from edgeml_amd import svr
    results, info = fits["LSVR"]
    C, eps = svr.LSVROpt().C, svr.LSVROpt().epsilon
    assert np.all(info["status"] == 0)
    for f, r in enumerate(g8["ref"]):
        n, xt, y, beta, v = r["n"], r["xt"], r["y"], info["beta"][f], info["v"][f]
        assert r["n"] % 4 != 0 and len(beta) == n
        assert np.all(np.abs(beta) <= C)  # exactly
        free = S.lsvr_free(beta, C)
        assert free.any() and np.any(np.abs(beta) == C) and np.any(beta == 0)
        # v = X~^T beta recomputed on the device from the final beta: an n-term sum per component
        assert np.all(np.abs(v - xt.T @ beta) <= n * EPS * (np.abs(xt).T @ np.abs(beta)))
        np.testing.assert_array_equal(info["coef"][f], v[:-1])
        assert info["intercept"][f] == v[-1]
        p0 = S.lsvr_primal(xt, y, np.zeros(xt.shape[1]), C, eps)
        assert info["tol"][f] == pytest.approx(1e-10 * p0, rel=1e-9)
        gap = S.lsvr_gap(xt, y, beta, C, eps)
        print(f"fold {f}: gap device {info['gap'][f]:.3e}, numpy {gap:.3e}, tol {info['tol'][f]:.3e}, sweeps "
              f"{info['sweeps'][f]}, free / bounded / zero {free.sum()} / {(np.abs(beta) == C).sum()} / {(beta == 0).sum()}")
        assert info["gap"][f] <= info["tol"][f] and gap <= info["tol"][f]
        # distance to the certificate; numpy's own evaluation of the gap is good to n eps P
        gap_dev = max(gap, 0.0) + n * EPS * S.lsvr_primal(xt, y, xt.T @ beta, C, eps)
        bound = np.sqrt(2 * gap_dev) + np.sqrt(2 * float(g8[f"LSVR/gap_cert{f}"]))
        dv = np.linalg.norm(v - g8[f"LSVR/v_cert{f}"])
        est = all_rows(g8, results, f)
        d_cert = np.abs(est - g8[f"LSVR/est_cert{f}"])
        d_ref = np.abs(est - g8[f"LSVR/est_ref{f}"])
        print(f"   |v - v_cert| {dv:.3e} (bound {bound:.3e}), max |est - cert| {d_cert.max():.3e} (min bound "
              f"{(bound * r['rows']).min():.3e}), max |est - ref| {d_ref.max():.3e} (stored distance "
              f"{float(g8[f'LSVR/dist{f}']):.3e})")
        assert dv <= bound
        assert np.all(d_cert <= bound * r["rows"])
        assert np.all(d_ref <= bound * r["rows"] + float(g8[f"LSVR/dist{f}"]))


# -------------------------------------------------------------------------------------------- SVR
def test_svr(g8, fits):
    from edgeml_amd import svr
    results, info = fits["SVR"]
    o = svr.SVROpt()
    C, eps, tol = o.C, o.epsilon, o.tol
    assert tol == 1e-9 and np.all(info["status"] == 0)
    for f, r in enumerate(g8["ref"]):
        n, K, y, beta, b = r["n"], r["K"], r["y"], info["beta"][f], float(info["intercept"][f])
        assert len(beta) == n
        assert np.all(np.abs(beta) <= C)  # exactly
        assert abs(beta.sum()) <= (n + int(info["iterations"][f])) * EPS * C
        free = S.svr_free(beta, C)
        assert free.any() and np.any(np.abs(beta) == C) and np.any(beta == 0)
        exact = S.svr_feasible(beta, C)  # the residual sum on one free coordinate: an exact dual point
        viol = S.svr_violation(K, y, exact, C, eps)
        # one n-term gradient in numpy, on a K within gamma band + 4 eps of the device's
        kerr = r["gamma"] * R.knr_band(r["z"][r["tr"]], r["z"][r["tr"]], g8["D"]).max() + 4 * EPS
        slack = 2 * (n * EPS * (np.abs(K) @ np.abs(exact)).max() + EPS * np.abs(y).max() + kerr * np.abs(exact).sum())
        print(f"fold {f}: violation device {info['violation'][f]:.3e}, numpy {viol:.3e} (tol {tol:.1e} + {slack:.1e}), "
              f"iterations {info['iterations'][f]}, free / bounded / zero {free.sum()} / {(np.abs(beta) == C).sum()} / "
              f"{(beta == 0).sum()}")
        assert info["violation"][f] <= tol and viol <= tol + slack
        gap = S.svr_gap(K, y, exact, b, C, eps)
        gap_dev = max(gap, 0.0) + n * EPS * S.svr_primal(K, y, exact, b, C, eps)
        bound = np.sqrt(2 * gap_dev) + np.sqrt(2 * float(g8[f"SVR/gap_cert{f}"]))
        db = exact - g8[f"SVR/beta_cert{f}"]
        q = db @ K @ db
        nrm = np.sqrt(max(q, 0.0) + 2 * n * EPS * (np.abs(db) @ np.abs(K) @ np.abs(db)))
        same = free & g8[f"SVR/free_cert{f}"] & (np.sign(beta) == np.sign(g8[f"SVR/beta_cert{f}"]))
        assert same.any()  # a free support vector both solutions share
        b_gate = nrm + viol + float(g8[f"SVR/viol_cert{f}"])
        d_b = abs(b - float(g8[f"SVR/b_cert{f}"]))
        est = all_rows(g8, results, f)
        d_cert = np.abs(est - g8[f"SVR/est_cert{f}"]).max()
        d_ref = np.abs(est - g8[f"SVR/est_ref{f}"]).max()
        print(f"   gap {gap:.3e}, |dbeta|_K {nrm:.3e} (bound {bound:.3e}), |b - b_cert| {d_b:.3e} (gate {b_gate:.3e}), "
              f"max |est - cert| {d_cert:.3e} (gate {nrm + b_gate:.3e}), max |est - ref| {d_ref:.3e} (stored distance "
              f"{float(g8[f'SVR/dist{f}']):.3e}), shared free {same.sum()}")
        assert nrm <= bound
        assert d_b <= b_gate
        assert d_cert <= nrm + b_gate
        assert d_ref <= nrm + b_gate + float(g8[f"SVR/dist{f}"])


# ------------------------------------------------------------------------------------- edge cases
def test_epsilon_one_leaves_no_support_vector(g8):
    from edgeml_amd import svr
    y = g8["reward"]
    assert np.abs(y).max() < 1.0
    results, info = svr.fit_svr(g8["features"], y, g8["split"], svr.SVROpt(epsilon=1.0))
    for f, r in enumerate(g8["ref"]):
        assert np.all(info["beta"][f] == 0) and info["iterations"][f] == 0
        b = info["intercept"][f]
        assert r["y"].max() - 1.0 <= b <= r["y"].min() + 1.0
        assert np.all(all_rows(g8, results, f) == b)
    results, info = svr.fit_lsvr(g8["features"], y, g8["split"], svr.LSVROpt(epsilon=1.0))
    for f in range(g8["folds"]):
        assert np.all(info["beta"][f] == 0) and np.all(info["v"][f] == 0) and info["sweeps"][f] == 0
        assert np.all(all_rows(g8, results, f) == 0.0)


def _flat(results, info):
    keys = sorted(k for k in info if k != "fit_time" and isinstance(info[k], np.ndarray))
    return [r[p] for r in results for p in ("train_est", "val_est")] + list(info["beta"]), keys, [info[k] for k in keys]


@pytest.mark.parametrize("name", ["SVR", "LSVR"])
def test_folds_together_equal_one_at_a_time_and_reruns(g8, fits, name):
    from edgeml_amd import svr
    arrs, keys, infos = _flat(*fits[name])
    arrs2, keys2, infos2 = _flat(*svr.FITS[name](g8["features"], g8["reward"], g8["split"]))
    assert keys == keys2
    for a, b in zip(arrs + infos, arrs2 + infos2):
        np.testing.assert_array_equal(a, b)
    for f in range(g8["folds"]):
        res1, info1 = svr.FITS[name](g8["features"], g8["reward"], g8["split"][f:f + 1])
        np.testing.assert_array_equal(res1[0]["train_est"], fits[name][0][f]["train_est"])
        np.testing.assert_array_equal(res1[0]["val_est"], fits[name][0][f]["val_est"])
        np.testing.assert_array_equal(info1["beta"][0], fits[name][1]["beta"][f])
        for k_ in keys:
            np.testing.assert_array_equal(info1[k_][0], fits[name][1][k_][f])


def test_three_iterations_raise_naming_the_folds(g8):
    from edgeml_amd import svr
    with pytest.raises(RuntimeError, match=r"SMO did not converge in 3 iterations: fold 1: violation .*fold 3"):
        svr.fit_svr(g8["features"], g8["reward"], g8["split"], svr.SVROpt(max_iter=3))
    with pytest.raises(RuntimeError, match=r"did not converge in 3 sweeps: fold 1: gap .*fold 3"):
        svr.fit_lsvr(g8["features"], g8["reward"], g8["split"], svr.LSVROpt(max_sweeps=3))
    with pytest.raises(ValueError, match="kernel 'linear' is not built"):
        svr.fit_svr(g8["features"], g8["reward"], g8["split"], svr.SVROpt(kernel="linear"))


def test_launchers_refuse_bad_arguments(g8):
    import ctypes
    from edgeml_amd import ops
    L = ops.lib()
    off = (ctypes.c_int64 * 3)(0, 5, 5)  # an empty fold
    assert L.edgedet_svr_workspace_size(off, 2, 34, 1) < 0
    off = (ctypes.c_int64 * 3)(0, 5, 12)
    assert L.edgedet_svr_workspace_size(off, 2, 34, 0) == (12 * 34 + 12) * 8
    assert L.edgedet_svr_workspace_size(off, 2, 34, 1) == (12 * 34 + 12 + 25 + 49) * 8
    assert L.edgedet_svr_workspace_size(off, 2, 256, 1) < 0 and L.edgedet_svr_workspace_size(off, 2, 0, 1) < 0
    assert L.edgedet_svr_kernel_matrix(None, 4, 4, 0.0, None, None, None, None) == -1
    assert b"null pointer" in L.edgedet_last_error()


# ------------------------------------------------------------------------------------ CLI end to end
@pytest.fixture(scope="module")
def files(g8, tmp_path_factory):
    td = tmp_path_factory.mktemp("g8")
    fdir = td / "features"
    for i, x in enumerate(g8["features"]):
        (fdir / f"{i:06d}").mkdir(parents=True)
        np.save(fdir / f"{i:06d}" / "stage24_output_features.npy", x)
    np.savez(td / "reward.npz", reward=g8["reward"])
    np.save(td / "split.npy", g8["split"])
    return td


@pytest.mark.parametrize("name", ["SVR", "LSVR"])
def test_cli_round_trip(g8, fits, files, name, capsys):
    import torch
    from edgeml_amd import offload, ops, svr
    save, mdir = files / f"est_{name}", files / f"model_{name}"
    svr.main(svr.getargs([str(files / "features"), str(files / "reward.npz"), str(files / "split.npy"), str(save),
                          "--model", name, "--model-dir", str(mdir)]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("fold ")]
    assert len(lines) == g8["folds"] and all(f"Trained {svr.NAMES[name]} model with training MSE: " in ln for ln in lines)
    D = g8["D"]
    for f in range(g8["folds"]):
        with np.load(save / f"estimate{f + 1}.npz", allow_pickle=False) as z:
            assert sorted(z.files) == ["train_est", "train_time", "val_est", "val_time"]
            np.testing.assert_array_equal(z["train_est"], fits[name][0][f]["train_est"])
            np.testing.assert_array_equal(z["val_est"], fits[name][0][f]["val_est"])
        path = mdir / f"wts{f + 1}.pickle"
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        assert m["model"] == name and all(isinstance(m[k], (np.ndarray, float, int, str)) for k in m)
        if name == "SVR":
            beta = fits[name][1]["beta"][f]
            np.testing.assert_array_equal(m["beta"], beta[beta != 0])
            np.testing.assert_array_equal(m["support"], g8["features"][~g8["split"][f]][beta != 0])
            assert m["gamma"] == fits[name][1]["gamma"][f] and m["intercept"] == fits[name][1]["intercept"][f]
            with pytest.raises(ValueError, match="does not predict from them yet"):
                offload.load_estimator(str(path), D)
            continue
        est = offload.load_estimator(str(path), D)
        assert est.kind == "linear"
        d = est.device_data("cuda")
        x = torch.from_numpy(np.ascontiguousarray(g8["features"][g8["split"][f]])).cuda()
        out = torch.empty(len(x), dtype=torch.float64, device="cuda")
        ops.check(ops.lib().edgedet_reg_predict(ops._ptr(x), len(x), D, ops._ptr(d["mean"]), ops._ptr(d["scale"]),
                                                ops._ptr(d["coef"]), ops._ptr(d["intercept"]), 1, ops._ptr(out),
                                                ops.stream_handle()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), fits[name][0][f]["val_est"])
