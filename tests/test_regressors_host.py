"""Host side of the estimator regressors (edgeml_amd.regress, estimator --model LR | EN | BR | KNR): the G7
fixture's own invariants, the numpy restatement of the four algorithms (tests/regress_ref.py) against the
reference's results in G7, the CLI's model names, and the C-ABI's new exports.  No device needed."""
import argparse
import os
import re

import numpy as np
import pytest

from tests import regress_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW_EXPORTS = ("edgedet_reg_workspace_size", "edgedet_reg_scaler", "edgedet_reg_gram", "edgedet_reg_eigh",
               "edgedet_reg_fit_lr", "edgedet_reg_fit_en", "edgedet_reg_fit_br", "edgedet_reg_predict",
               "edgedet_knn_fit_predict")


@pytest.fixture(scope="module")
def g7():
    with np.load(os.path.join(ROOT, "tests", "golden", "g7_regressors.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    ref = []
    for m in g["split"]:
        tr = ~m
        mean, scale, const = R.scaler(g["features"][tr])
        z = R.standardise(g["features"], mean, scale)
        y = g["reward"][tr]
        ref.append({"tr": tr, "n": int(tr.sum()), "mean": mean, "scale": scale, "const": const, "z": z, "y": y,
                    "G": R.gram(z[tr], y - y.mean())})
    g["ref"] = ref
    return g


def spread(g, key):
    return max(float(g[f"{key}{f}"]) for f in range(g["folds"]))


def test_fixture_invariants(g7):
    x, split, D = g7["features"], g7["split"], g7["D"]
    nc = int(g7["num_class"])
    assert str(g7["sklearn_version"]) == "1.7.2"
    assert x.shape == (360, 34) and x.dtype == np.float64 and (D + 1) % 16 != 0
    assert split.shape == (3, 360) and np.all(split.sum(0) == 1)
    for m in split:
        n = int((~m).sum())
        assert n % 16 != 0 and n % 64 != 0 and n > D + 1
    assert len({int((~m).sum()) for m in split}) == 3  # ragged
    assert np.all(x[:, nc - 1] == 0) and np.all(x[:, nc + 2] == 0.1)
    assert int(g7["k"]) == 6 and np.all(x[:, :nc].sum(1) == 6)  # every image fills its top 6 boxes
    pairs = [(i, j) for i in range(len(x)) for j in range(i + 1, len(x)) if np.array_equal(x[i], x[j])]
    assert len(pairs) >= 2 and all(g7["reward"][i] != g7["reward"][j] for i, j in pairs)
    for i, j in pairs:  # each pair trains together in some fold
        assert any(not m[i] and not m[j] for m in split)
    for f in range(3):
        assert g7[f"KNR/inband{f}"].mean() <= 0.10
    assert int(g7["KNR/straddle"]) >= 1
    assert max(int(g7[f"BR/n_iter{f}"]) for f in range(3)) >= 3
    for f in range(3):
        assert int(g7[f"LR/rank{f}"]) == D - 3  # two constant columns and the class-count dependency
        assert np.any(g7[f"EN/coef_hi{f}"] == 0) and np.any(g7[f"EN/coef_hi{f}"] != 0)
        assert float(g7[f"EN/z_hi{f}"]) < 1e-14 < float(g7[f"EN/z_default{f}"])


def test_restated_scaler_matches_sklearns(g7):
    for f, r in enumerate(g7["ref"]):
        assert np.array_equal(r["scale"] == 1.0, g7[f"scaler/scale{f}"] == 1.0) and int(r["const"].sum()) == 2
        np.testing.assert_allclose(r["mean"], g7[f"scaler/mean{f}"], rtol=0, atol=r["n"] * EPS * np.abs(g7["features"]).max())
        np.testing.assert_allclose(r["scale"], g7[f"scaler/scale{f}"], rtol=r["n"] * EPS, atol=0)


def test_restated_lr(g7):
    for f, r in enumerate(g7["ref"]):
        coef, rank, ratio = R.lr_from_gram(r["G"])
        assert rank == int(g7[f"LR/rank{f}"]) and ratio > 1e-6
        assert np.abs(g7[f"LR/null{f}"].T @ coef).max() <= 64 * spread(g7, "LR/null_ref")
        est = r["z"] @ coef + r["y"].mean()
        bound = (float(g7[f"LR/g_gram{f}"]) + float(g7[f"LR/g_ref{f}"])) / float(g7[f"LR/sigma_min{f}"])
        assert np.abs(est - g7[f"LR/est_ref{f}"]).max() <= bound


def test_restated_br(g7):
    for f, r in enumerate(g7["ref"]):
        coef, alpha, lam, n_iter, dcs = R.br_from_gram(r["G"], r["n"])
        assert n_iter == int(g7[f"BR/n_iter{f}"])
        assert dcs[-1] < 0.5e-3 and dcs[-2] >= 2e-3  # the stopping decision is not a close call
        assert abs(alpha - float(g7[f"BR/alpha{f}"])) <= 64 * spread(g7, "BR/alpha_spread") * alpha
        assert abs(lam - float(g7[f"BR/lambda{f}"])) <= 64 * spread(g7, "BR/lambda_spread") * lam
        est = r["z"] @ coef + r["y"].mean()
        assert np.abs(est - g7[f"BR/est_ref{f}"]).max() <= 64 * spread(g7, "BR/est_spread")


def test_restated_en(g7):
    mu = 0.01 * 0.5
    for f, r in enumerate(g7["ref"]):
        w, zn, tol, sweeps = R.en_from_gram(r["G"], r["n"])
        assert zn <= tol and sweeps < 200000
        assert np.any(w == 0) and np.any(w != 0)
        est = r["z"] @ w + r["y"].mean()
        rows = np.linalg.norm(r["z"], axis=1)
        assert np.all(np.abs(est - g7[f"EN/est_hi{f}"]) <= rows * (zn + float(g7[f"EN/z_hi{f}"])) / mu)
        assert np.all(np.abs(est - g7[f"EN/est_ref{f}"]) <= rows * (zn + float(g7[f"EN/z_default{f}"])) / mu)


def test_restated_knr(g7):
    k = int(g7["n_neighbors"])
    for f, r in enumerate(g7["ref"]):
        d2 = R.sqdist_direct(r["z"], r["z"][r["tr"]])
        nbr, est, dk = R.knr_exact(d2, r["y"], k)
        beta = R.knr_band(r["z"], r["z"][r["tr"]], g7["D"])
        inband = (np.abs(d2 - dk[:, None]) <= beta[:, None]).sum(1) > 1
        assert np.array_equal(inband, g7[f"KNR/inband{f}"])
        ok = ~inband
        assert np.all(np.abs(est - g7[f"KNR/est_ref{f}"])[ok] <= 2 * k * EPS * np.abs(r["y"]).max())


def _opts(model, stage=24):
    return argparse.Namespace(model=model, stage=stage)


def test_cli_accepts_the_built_models_and_refuses_the_rest():
    from edgeml_amd import estimator
    for name in ("CNN", "LR", "EN", "BR", "KNR"):
        estimator.check_model(_opts(name))
        assert estimator.getargs(["d", "r", "s", "o", "--model", name]).model == name
    for name in ("SGD", "SVR", "LSVR", "RFR", "GBR"):
        with pytest.raises(SystemExit) as e:
            estimator.check_model(_opts(name))
        msg = str(e.value)
        assert f"--model {name} is not built" in msg
        for built in ("CNN", "LR", "EN", "BR", "KNR"):
            assert built in msg
    with pytest.raises(SystemExit, match="no model of regression.py"):
        estimator.check_model(_opts("XGB"))
    with pytest.raises(SystemExit, match="stages 0-23"):
        estimator.check_model(_opts("CNN", stage=17))
    assert estimator.getargs(["d", "r", "s", "o"]).model == "CNN"  # the default is unchanged


def test_cnn_paths_are_untouched():
    from edgeml_amd import estimator
    assert estimator.parse_path("out/est") == (os.path.join("out", "est_best"), os.path.join("out", "est_last"))
    assert estimator.parse_path("") == ("", "")
    assert estimator.parse_path("/abs/est") == (os.path.join("abs", "est_best"), os.path.join("abs", "est_last"))


def test_option_defaults_are_the_references():
    from edgeml_amd import regress
    assert (regress.ENOpt().alpha, regress.ENOpt().l1_ratio) == (0.01, 0.5)
    b = regress.BROpt()
    assert (b.alpha_1, b.alpha_2, b.lambda_1, b.lambda_2, b.tol, b.max_iter) == (1e-6, 1e-6, 1e-6, 1e-6, 1e-3, 300)
    assert regress.KNROpt().n_neighbors == 500 and regress.KNROpt(n_neighbors=7).n_neighbors == 7
    assert regress.LR_TAU == R.LR_TAU == 1e-11
    assert sorted(regress.FITS) == ["BR", "EN", "KNR", "LR"]


def test_there_is_no_cpu_path(g7):
    import torch
    from edgeml_amd import regress
    if torch.cuda.is_available():
        return  # the refusal only exists where no device does
    for fit in regress.FITS.values():
        with pytest.raises(RuntimeError, match="no CPU path"):
            fit(g7["features"], g7["reward"], g7["split"])


def test_header_declares_and_library_exports_the_regressors():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        txt = f.read()
    assert "estimator regressors" in txt
    declared = set(re.findall(r"\b(edgedet_[a-z_0-9]+)\s*\(", txt))
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in ops.EXPORTS and hasattr(lib, name), name
    assert lib.edgedet_reg_workspace_size(3, 34, 0, 0) == 3 * 34 * 34 * 8
    assert lib.edgedet_reg_workspace_size(3, 35, 0, 0) == 3 * 36 * 36 * 8  # the Jacobi order is even
    assert lib.edgedet_reg_workspace_size(2, 34, 100, 150) == (100 * 150 + 2 * 100) * 8
    assert lib.edgedet_reg_workspace_size(1, 256, 0, 0) < 0 and lib.edgedet_reg_workspace_size(1, 0, 0, 0) < 0
