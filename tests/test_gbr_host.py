"""Host side of the gradient boosting regressor (edgeml_amd.gbr): the numpy restatement (tests/gbr_ref.py)
against G9 (tests/golden/g9_gbr.npz: the restatement at the reference's options, checked stage by stage against
regression.py's own GBR runs under sklearn 1.7.2 by tests/golden/make_golden_gbr.py), the option defaults, the
CLI's arguments, the refusals, the pickle loader and the C-ABI's new exports.  No device needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from tests import gbr_ref as B
from tests import regress_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW_EXPORTS = ("edgedet_gbr_workspace_size", "edgedet_gbr_prepare", "edgedet_gbr_fit", "edgedet_gbr_model_predict",
               "edgedet_gbr_best_split")
EARLY = 20


@pytest.fixture(scope="module")
def g9():
    g = {}
    for name in ("g7_regressors.npz", "g9_gbr.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g9") or k in ("features", "reward", "split")})
    return g


def test_fixture_conditions(g9):
    assert str(g9["sklearn_version"]) == "1.7.2"
    T = int(g9["T"])
    assert T >= 150 and int(g9["keep"]) == 120 and float(g9["learning_rate"]) == 0.1 and int(g9["max_depth"]) == 3
    for f, m in enumerate(g9["split"]):
        n, y = int((~m).sum()), g9["reward"][~m]
        assert int(g9[f"q{f}"]) == 55
        assert g9[f"nodes{f}"].shape == (T,) and 0 < int(g9[f"tied_nodes{f}"]) < int(g9[f"nodes{f}"].sum())
        assert g9[f"nodes{f}"].max() <= 7
        # the restatement's distance from sklearn's own training estimates, and the bound it was held to
        bound = T * (n * EPS * float(np.abs(y - y.mean()).max()) + 2.0 ** -55)
        dist = max(float(np.abs(g9[f"est{f}"][~m] - sk).max()) for sk in g9[f"sklearn_train_est{f}"])
        assert dist == float(g9[f"dist{f}"]) <= bound
        assert float(g9[f"val_spread{f}"]) > 1e-3  # sklearn's own val_est is a draw: the ties decide that much


def test_restatement_reproduces_the_first_stages(g9):
    for f, m in enumerate(g9["split"]):
        tr = ~m
        mean, scale, _ = R.scaler(g9["features"][tr])
        z32 = B.standardise32(g9["features"], mean, scale)
        init, q = B.init_and_q(g9["reward"][tr])
        assert (init, q) == (float(g9[f"init{f}"]), int(g9[f"q{f}"]))
        fit = B.fit(z32[tr], g9["reward"][tr], z32, 0.1, EARLY, 3)
        for key in ("feature", "threshold", "value"):
            np.testing.assert_array_equal(fit[key], g9[f"{key}{f}"][:EARLY])
        np.testing.assert_array_equal(fit["nodes"], g9[f"nodes{f}"][:EARLY])
        np.testing.assert_array_equal(fit["est"], g9[f"est{EARLY}_{f}"])
        np.testing.assert_array_equal(fit["est"][tr], fit["train_F"])  # the walk by threshold is the partition
        np.testing.assert_array_equal(B.predict(fit, z32, 0.1, 3), fit["est"])


def test_restatement_rules():
    """The threshold rule, the tie rule and the exact impurity rule on hand-made nodes."""
    a = np.float32(0.25)
    near, far = np.float32(0.25 + 6e-8), np.float32(0.25 + 2e-7)
    assert near > a and not near > a + B.FEATURE_THRESHOLD and far > a + B.FEATURE_THRESHOLD
    rq = np.array([5, -5], np.int64)
    node = np.zeros(2, np.int64)
    for b, feature in ((near, -1), (far, 0)):
        z = np.array([[a], [b]], np.float32)
        rec = B.best_split(z, B.orders(z), node, rq, 1, 26)[0]
        assert rec["feature"] == feature and rec["leaf"] == (feature < 0)
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, 40).astype(np.float32)
    rq = np.rint(x * 1000).astype(np.int64) << 30
    node = np.zeros(40, np.int64)
    for z in (np.stack([x[::-1], x, x], 1), np.stack([x[::-1], x, -x], 1)):  # a copy, a negated copy
        rec = B.best_split(np.ascontiguousarray(z), B.orders(z), node, rq, 1, 40)[0]
        assert rec["feature"] == 1 and rec["tied"]
    # n sum rq^2 - S^2 = d^2 k (n - k) for k rows d quanta above the rest; at q = 26 the bound is n^2
    for d, leaf in ((0, True), (2, True), (3, False)):
        assert B.impurity_leaf(np.array([1 << 50] * 32 + [(1 << 50) + d] * 32, np.int64), 26) == leaf


def test_option_defaults_are_the_references():
    from edgeml_amd import gbr, regress
    o = gbr.GBROpt()
    assert (o.learning_rate, o.n_estimators, o.subsample, o.max_depth) == (0.1, 1000, 1.0, 3)
    assert sorted(gbr.FITS) == ["GBR"] and gbr._Folds is regress._Folds
    assert gbr.NAMES["GBR"] == "Gradient Boosting Regressor"


def test_cli_arguments():
    from edgeml_amd import estimator, gbr
    a = gbr.getargs(["d", "r", "s", "o", "--model", "GBR", "--normalize", "--model-dir", "m"])
    assert (a.data_dir, a.reward_path, a.split_path, a.save_dir) == ("d", "r", "s", "o")
    assert a.model == "GBR" and a.normalize and a.model_dir == "m" and a.stage == 24
    assert (a.n_estimators, a.learning_rate, a.max_depth) == (1000, 0.1, 3)
    b = gbr.getargs(["d", "r", "s", "o", "--n-estimators", "50", "--learning-rate", "0.05", "--max-depth", "4"])
    assert b.model == "GBR" and (b.n_estimators, b.learning_rate, b.max_depth) == (50, 0.05, 4) and b.model_dir == ""
    with pytest.raises(SystemExit) as e:  # the estimator CLI still refuses it, and now says where it is
        estimator.check_model(estimator.getargs(["d", "r", "s", "o", "--model", "GBR"]))
    assert "--model GBR is not built" in str(e.value) and "python -m edgeml_amd.gbr fits GBR" in str(e.value)


def test_refusals(g9):
    import torch
    from edgeml_amd import gbr
    args = (g9["features"], g9["reward"], g9["split"])
    with pytest.raises(ValueError, match="subsample = 0.5"):
        gbr.fit_gbr(*args, gbr.GBROpt(subsample=0.5))
    for depth in (0, 5):
        with pytest.raises(ValueError, match=f"max_depth = {depth}"):
            gbr.fit_gbr(*args, gbr.GBROpt(max_depth=depth))
    with pytest.raises(ValueError, match="n_estimators = 0"):
        gbr.fit_gbr(*args, gbr.GBROpt(n_estimators=0))
    for name in ("RFR", "SGD", "LR"):
        with pytest.raises(SystemExit, match=f"--model {name}"):
            gbr.main(gbr.getargs(["d", "r", "s", "o", "--model", name]))
    with pytest.raises(SystemExit, match="max_depth = 5"):
        gbr.main(gbr.getargs(["d", "r", "s", "o", "--max-depth", "5"]))
    if not torch.cuda.is_available():  # the refusal only exists where no device does
        with pytest.raises(RuntimeError, match="no CPU path"):
            gbr.fit_gbr(*args)


def _model(D=9, T=4, depth=3, seed=1):
    rng = np.random.default_rng(seed)
    ni, nv = (1 << depth) - 1, (2 << depth) - 1
    return {"model": "GBR", "mean": rng.normal(0, 1, D), "scale": rng.uniform(0.5, 2, D), "init": 0.25,
            "learning_rate": 0.1, "max_depth": depth, "feature": rng.integers(-1, D, (T, ni)).astype(np.int16),
            "threshold": rng.normal(0, 1, (T, ni)), "value": rng.normal(0, 1, (T, nv)), "q": 55}


def test_load_estimator_takes_gbr_files_and_refuses_broken_ones(tmp_path):
    from edgeml_amd import gbr, offload
    D = 9
    good = _model(D)

    def load(m, width=D):
        with open(tmp_path / "wts.pickle", "wb") as f:
            pickle.dump(m, f)
        return offload.load_estimator(str(tmp_path / "wts.pickle"), width)

    est = load(good)
    assert est.kind == "gbr" and est.width == D and isinstance(est.model, gbr.GBRModel) and est.workspace_bytes(64) == 0
    assert (est.model.T, est.model.depth, est.model.init, est.model.learning_rate) == (4, 3, 0.25, 0.1)
    np.testing.assert_array_equal(est.model.feature, good["feature"])
    np.testing.assert_array_equal(est.model.value, good["value"])
    with pytest.raises(ValueError, match="features, the cascade makes 10"):
        load(good, D + 1)
    for key in ("feature", "value", "init", "max_depth"):
        with pytest.raises(ValueError, match=f"a GBR file without '{key}'"):
            load({k: v for k, v in good.items() if k != key})
    for key, bad in (("value", good["value"][:, :-1]), ("threshold", good["threshold"][:-1]),
                     ("feature", good["feature"][:, :3]), ("max_depth", 2), ("scale", good["scale"][:-1])):
        with pytest.raises(ValueError, match="tree arrays of shapes|'scale'"):
            load({**good, key: bad})
    with pytest.raises(ValueError, match="integers from -1 to 8"):
        load({**good, "feature": np.full_like(good["feature"], D)})
    with pytest.raises(ValueError, match="max_depth = 5"):
        load({**good, "max_depth": 5})
    with pytest.raises(ValueError, match="must be finite"):
        load({**good, "value": np.full_like(good["value"], np.nan)})
    info = {"mean": good["mean"][None], "scale": good["scale"][None], "init": np.array([0.25]), "q": np.array([55]),
            "learning_rate": 0.1, "max_depth": 3, "feature": good["feature"][None], "threshold": good["threshold"][None],
            "value": good["value"][None]}
    m = gbr.model_data(info, 0)
    assert sorted(m) == sorted(["model", "q", *gbr.KEYS]) and m["model"] == "GBR"
    assert all(isinstance(v, (np.ndarray, float, int, str)) for v in m.values())
    assert load(m).kind == "gbr"


def test_header_declares_and_library_exports_the_new_names():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        txt = f.read()
    assert "gradient boosting regressor" in txt
    declared = set(re.findall(r"\b(edgedet_[a-z_0-9]+)\s*\(", txt))
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in ops.EXPORTS and hasattr(lib, name), name
    off = (ctypes.c_int64 * 3)(0, 5, 12)
    cand = 2 * 8 * 34
    assert lib.edgedet_gbr_workspace_size(off, 2, 34) == 12 * 8 + 3 * cand * 8 + 2 * 8 * 8 + 2 * 8 * 4 * 8 + cand * 4 \
        + 2 * 8 * 4 + 16
    assert lib.edgedet_gbr_workspace_size(off, 2, 256) < 0 and lib.edgedet_gbr_workspace_size(off, 2, 0) < 0
    assert lib.edgedet_gbr_workspace_size((ctypes.c_int64 * 3)(0, 5, 5), 2, 34) < 0  # an empty fold
    assert lib.edgedet_gbr_workspace_size(None, 2, 34) < 0 and lib.edgedet_gbr_workspace_size(off, 0, 34) < 0
