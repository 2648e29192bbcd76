"""Host side of the support vector regressors (edgeml_amd.svr): the G8 fixture's own conditions, the numpy
restatement of both objectives and solvers (tests/svr_ref.py) against G8's stored gaps and certificates, the
option defaults, the CLI's arguments, the refusals, and the C-ABI's new exports.  No device needed."""
import os
import pickle
import re

import numpy as np
import pytest

from tests import regress_ref as R
from tests import svr_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW_EXPORTS = ("edgedet_svr_workspace_size", "edgedet_svr_kernel_matrix", "edgedet_svr_fit", "edgedet_svr_predict",
               "edgedet_lsvr_fit")
SVR_C, SVR_EPS, LSVR_C, LSVR_EPS = 0.05, 0.05, 0.005, 0.005


@pytest.fixture(scope="module")
def g8():
    g = {}
    for name in ("g7_regressors.npz", "g8_svr.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g8") or k in ("features", "reward", "split")})
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    ref = []
    for f, m in enumerate(g["split"]):
        tr = ~m
        mean, scale, _ = R.scaler(g["features"][tr])
        z = R.standardise(g["features"], mean, scale)
        ref.append({"tr": tr, "n": int(tr.sum()), "z": z, "y": g["reward"][tr],
                    "K": S.rbf(z[tr], z[tr], float(g[f"SVR/gamma{f}"])), "xt": S.with_bias(z[tr])})
    g["ref"] = ref
    return g


def test_fixture_conditions(g8):
    assert str(g8["sklearn_version"]) == "1.7.2"
    assert [r["n"] for r in g8["ref"]] == [237, 242, 241]
    for f, r in enumerate(g8["ref"]):
        assert r["n"] % 4 != 0 and r["n"] % 16 != 0
        assert abs(float(g8[f"SVR/gamma{f}"]) - 1 / 32) <= 64 * EPS
        assert abs(S.gamma_scale(r["z"][r["tr"]]) - float(g8[f"SVR/gamma{f}"])) <= r["n"] * g8["D"] * EPS / 32
        for key, C in (("SVR/beta_cert", SVR_C), ("SVR/beta_ref", SVR_C), ("LSVR/beta_cert", LSVR_C)):
            b = g8[f"{key}{f}"]
            assert len(b) == r["n"] and np.all(np.abs(b) <= C)
            assert S.svr_free(b, C).any() and np.any(np.abs(b) == C) and np.any(b == 0)
        shared = (g8[f"SVR/free_ref{f}"] & g8[f"SVR/free_cert{f}"]
                  & (np.sign(g8[f"SVR/beta_ref{f}"]) == np.sign(g8[f"SVR/beta_cert{f}"])))
        assert shared.sum() >= 1
        assert abs(g8[f"SVR/beta_cert{f}"].sum()) <= 4 * EPS * SVR_C
        # the certificates are far better than the default fits, and libsvm at tol=1e-12 is in between
        assert float(g8[f"SVR/gap_cert{f}"]) <= float(g8[f"SVR/gap_libsvm{f}"]) < 1e-8 < float(g8[f"SVR/gap_ref{f}"])
        assert float(g8[f"SVR/viol_cert{f}"]) < 1e-9 < float(g8[f"SVR/viol_ref{f}"]) < 1e-3  # sklearn's tol
        assert float(g8[f"LSVR/gap_cert{f}"]) < 1e-14
        assert float(g8[f"LSVR/primal_cert{f}"]) <= float(g8[f"LSVR/primal_ref{f}"])


def test_restatement_reproduces_the_stored_svr_figures(g8):
    for f, r in enumerate(g8["ref"]):
        K, y, n = r["K"], r["y"], r["n"]
        beta, b = g8[f"SVR/beta_cert{f}"], float(g8[f"SVR/b_cert{f}"])
        scale = n * EPS * S.svr_primal(K, y, beta, b, SVR_C, SVR_EPS)  # two evaluations of P + W
        assert abs(S.svr_gap(K, y, beta, b, SVR_C, SVR_EPS) - float(g8[f"SVR/gap_cert{f}"])) <= 4 * scale
        gslack = 4 * n * EPS * ((np.abs(K) @ np.abs(beta)).max() + np.abs(y).max())
        assert abs(S.svr_violation(K, y, beta, SVR_C, SVR_EPS) - float(g8[f"SVR/viol_cert{f}"])) <= gslack
        assert abs(S.svr_intercept(K, y, beta, SVR_C, SVR_EPS) - b) <= float(g8[f"SVR/viol_cert{f}"]) + gslack
        np.testing.assert_array_equal(S.svr_free(beta, SVR_C), g8[f"SVR/free_cert{f}"])
        est = S.rbf(r["z"], r["z"][r["tr"]], float(g8[f"SVR/gamma{f}"])) @ beta + b
        assert np.abs(est - g8[f"SVR/est_cert{f}"]).max() <= 4 * n * EPS * np.abs(beta).sum()
        assert np.abs(est - g8[f"SVR/est_ref{f}"]).max() == pytest.approx(float(g8[f"SVR/dist{f}"]), rel=1e-6)
        # the reference's default fit, on the same objective
        bref, b0 = g8[f"SVR/beta_ref{f}"], float(g8[f"SVR/b_ref{f}"])
        assert S.svr_gap(K, y, bref, b0, SVR_C, SVR_EPS) == pytest.approx(float(g8[f"SVR/gap_ref{f}"]), rel=1e-6)
        assert S.svr_violation(K, y, bref, SVR_C, SVR_EPS) == pytest.approx(float(g8[f"SVR/viol_ref{f}"]), rel=1e-6)
        est0 = S.rbf(r["z"], r["z"][r["tr"]], float(g8[f"SVR/gamma{f}"])) @ bref + b0
        assert np.abs(est0 - g8[f"SVR/est_ref{f}"]).max() <= 64 * n * EPS * np.abs(bref).sum()  # sklearn's own predict


def test_restated_smo_reaches_the_certificate(g8):
    """The numpy SMO at the device's default tolerance, held to the certificate as the device is."""
    for f, r in enumerate(g8["ref"]):
        K, y, n = r["K"], r["y"], r["n"]
        beta, b, viol, it = S.svr_smo(K, y, SVR_C, SVR_EPS, tol=1e-9)
        assert viol <= 1e-9 and it < 5000 and np.all(np.abs(beta) <= SVR_C)
        assert abs(beta.sum()) <= (n + it) * EPS * SVR_C
        exact = S.svr_feasible(beta, SVR_C)
        gap = S.svr_gap(K, y, exact, b, SVR_C, SVR_EPS) + n * EPS * S.svr_primal(K, y, exact, b, SVR_C, SVR_EPS)
        db = exact - g8[f"SVR/beta_cert{f}"]
        nrm = np.sqrt(max(db @ K @ db, 0.0))
        assert nrm <= np.sqrt(2 * gap) + np.sqrt(2 * float(g8[f"SVR/gap_cert{f}"]))
        assert abs(b - float(g8[f"SVR/b_cert{f}"])) <= nrm + 2e-9 + float(g8[f"SVR/viol_cert{f}"])


def test_restatement_reproduces_the_stored_lsvr_figures(g8):
    for f, r in enumerate(g8["ref"]):
        xt, y, n = r["xt"], r["y"], r["n"]
        beta, v = g8[f"LSVR/beta_cert{f}"], g8[f"LSVR/v_cert{f}"]
        assert np.all(np.abs(v - xt.T @ beta) <= n * EPS * (np.abs(xt).T @ np.abs(beta)))
        scale = n * EPS * S.lsvr_primal(xt, y, v, LSVR_C, LSVR_EPS)
        assert abs(S.lsvr_gap(xt, y, beta, LSVR_C, LSVR_EPS) - float(g8[f"LSVR/gap_cert{f}"])) <= 4 * scale
        assert S.lsvr_primal(xt, y, v, LSVR_C, LSVR_EPS) == pytest.approx(float(g8[f"LSVR/primal_cert{f}"]), rel=1e-12)
        assert S.lsvr_primal(xt, y, g8[f"LSVR/v_ref{f}"], LSVR_C, LSVR_EPS) == pytest.approx(
            float(g8[f"LSVR/primal_ref{f}"]), rel=1e-12)
        est = S.with_bias(r["z"]) @ v
        assert np.abs(est - g8[f"LSVR/est_cert{f}"]).max() <= 4 * g8["D"] * EPS * np.abs(est).max() + 64 * EPS
        assert np.abs(est - g8[f"LSVR/est_ref{f}"]).max() == pytest.approx(float(g8[f"LSVR/dist{f}"]), rel=1e-6)
        # the default reference fit is no optimum, but within strong convexity's reach of the certificate
        dv = np.linalg.norm(g8[f"LSVR/v_ref{f}"] - v)
        excess = float(g8[f"LSVR/primal_ref{f}"]) - float(g8[f"LSVR/primal_cert{f}"])
        assert 0 < excess and dv <= np.sqrt(2 * (excess + float(g8[f"LSVR/gap_cert{f}"])))


def test_restated_dual_cd_on_a_small_problem():
    """Sixty sweeps' worth of rows: the plain cyclic solver reaches its gap, and the strong-convexity bound holds
    between two of its own runs at different tolerances."""
    rng = np.random.default_rng(3)
    z = rng.normal(0, 1, (45, 5))
    y = z @ rng.normal(0, 0.1, 5) + 0.02 * rng.normal(0, 1, 45)
    xt = S.with_bias(z)
    b1, v1, gap1, s1 = S.lsvr_cd(xt, y, 0.05, 0.01, tol_rel=1e-4)
    b2, v2, gap2, s2 = S.lsvr_cd(xt, y, 0.05, 0.01, tol_rel=1e-12, max_sweeps=20000)
    assert 0 <= gap2 <= gap1 and s1 <= s2 < 20000
    assert np.all(np.abs(b2) <= 0.05) and np.any(np.abs(b2) == 0.05)
    assert np.linalg.norm(v1 - v2) <= np.sqrt(2 * gap1) + np.sqrt(2 * gap2)


def test_option_defaults_are_the_references():
    from edgeml_amd import regress, svr
    s, l = svr.SVROpt(), svr.LSVROpt()
    assert (s.C, s.epsilon, s.kernel, s.tol) == (0.05, 0.05, "rbf", 1e-9) and s.max_iter >= 1000000
    assert (l.C, l.epsilon, l.tol, l.tol_rel) == (0.005, 0.005, 0.0, 1e-10) and l.max_sweeps >= 100000
    assert sorted(svr.FITS) == ["LSVR", "SVR"]
    assert svr._Folds is regress._Folds and sorted(regress.FITS) == ["BR", "EN", "KNR", "LR"]


def test_cli_arguments():
    from edgeml_amd import estimator, svr
    a = svr.getargs(["d", "r", "s", "o", "--model", "LSVR", "--normalize", "--model-dir", "m"])
    assert (a.data_dir, a.reward_path, a.split_path, a.save_dir) == ("d", "r", "s", "o")
    assert a.model == "LSVR" and a.normalize and a.model_dir == "m" and a.stage == 24
    b = svr.getargs(["d", "r", "s", "o", "--model", "SVR"])
    assert b.model == "SVR" and not b.normalize and b.model_dir == "" and b.tol_rel is None
    assert svr.getargs(["d", "r", "s", "o", "--model", "LSVR", "--tol-rel", "1e-4"]).tol_rel == 1e-4
    b.model = "LR"
    with pytest.raises(SystemExit, match="--model LR belongs to edgeml_amd.estimator"):
        svr.main(b)
    for name in ("SVR", "LSVR"):  # the estimator CLI still refuses them, and now says where they are
        with pytest.raises(SystemExit) as e:
            estimator.check_model(estimator.getargs(["d", "r", "s", "o", "--model", name]))
        assert f"--model {name} is not built" in str(e.value) and "edgeml_amd.svr" in str(e.value)


def test_other_kernels_are_refused_and_there_is_no_cpu_path(g8):
    import torch
    from edgeml_amd import svr
    for kernel in ("linear", "poly", "sigmoid", "precomputed"):
        with pytest.raises(ValueError, match=f"kernel '{kernel}' is not built"):
            svr.fit_svr(g8["features"], g8["reward"], g8["split"], svr.SVROpt(kernel=kernel))
    if torch.cuda.is_available():
        return  # the refusal only exists where no device does
    for fit in svr.FITS.values():
        with pytest.raises(RuntimeError, match="no CPU path"):
            fit(g8["features"], g8["reward"], g8["split"])


def test_header_declares_and_library_exports_the_new_names():
    import ctypes
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        txt = f.read()
    assert "support vector regressors" in txt
    declared = set(re.findall(r"\b(edgedet_[a-z_0-9]+)\s*\(", txt))
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in ops.EXPORTS and hasattr(lib, name), name
    off = (ctypes.c_int64 * 3)(0, 5, 12)
    assert lib.edgedet_svr_workspace_size(off, 2, 34, 0) == (12 * 34 + 12) * 8
    assert lib.edgedet_svr_workspace_size(off, 2, 34, 1) == (12 * 34 + 12 + 25 + 49) * 8
    assert lib.edgedet_svr_workspace_size(off, 2, 256, 1) < 0 and lib.edgedet_svr_workspace_size(off, 2, 0, 1) < 0
    assert lib.edgedet_svr_workspace_size((ctypes.c_int64 * 3)(0, 5, 5), 2, 34, 1) < 0  # an empty fold
    assert lib.edgedet_svr_workspace_size(None, 2, 34, 1) < 0


def test_load_estimator_takes_lsvr_files_and_refuses_svr_files(tmp_path):
    from edgeml_amd import offload, svr
    D = 9
    rng = np.random.default_rng(1)
    info = {"mean": rng.normal(0, 1, (1, D)), "scale": rng.uniform(0.5, 2, (1, D)), "coef": rng.normal(0, 1, (1, D)),
            "intercept": np.array([0.25]), "gap": np.array([1e-12]), "sweeps": np.array([7], np.int32),
            "gamma": np.array([0.125]), "violation": np.array([1e-10]), "iterations": np.array([11], np.int32),
            "beta": [np.array([0.0, 0.05, -0.01, 0.0])], "train_rows": [np.array([0, 2, 3, 5], np.int32)]}
    feats = rng.normal(0, 1, (6, D))
    for name in ("LSVR", "SVR"):
        m = svr.model_data(name, info, 0, feats)
        with open(tmp_path / f"{name}.pickle", "wb") as f:
            pickle.dump(m, f)
    est = offload.load_estimator(str(tmp_path / "LSVR.pickle"), D)
    assert est.kind == "linear" and est.intercept == 0.25
    np.testing.assert_array_equal(est.coef, info["coef"][0])
    np.testing.assert_array_equal(est.mean, info["mean"][0])
    with open(tmp_path / "SVR.pickle", "rb") as f:
        m = pickle.load(f)
    np.testing.assert_array_equal(m["support"], feats[[2, 3]])
    np.testing.assert_array_equal(m["beta"], [0.05, -0.01])
    with pytest.raises(ValueError, match="an SVR file holds support vectors"):
        offload.load_estimator(str(tmp_path / "SVR.pickle"), D)
    with pytest.raises(ValueError, match="features, the cascade makes 10"):
        offload.load_estimator(str(tmp_path / "LSVR.pickle"), D + 1)
