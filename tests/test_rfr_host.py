"""Host side of the random forest regressor (edgeml_amd.rfr): the numpy restatement (tests/rfr_ref.py) against
G11 (tests/golden/g11_rfr.npz: the restatement at the reference's options and at min_samples_split = 20, checked
tree by tree against regression.py's own RFR runs under sklearn 1.7.2 by tests/golden/make_golden_rfr.py), the
bootstrap, the option checks, the CLI's arguments, the refusals, the pickle loader and the C-ABI's new exports.
No device needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from tests import regress_ref as R
from tests import rfr_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW_EXPORTS = ("edgedet_rfr_node_cap", "edgedet_rfr_workspace_size", "edgedet_rfr_best_split_workspace_size",
               "edgedet_rfr_fit", "edgedet_rfr_best_split", "edgedet_rfr_model_predict")


@pytest.fixture(scope="module")
def g11():
    g = {}
    for name in ("g7_regressors.npz", "g11_rfr.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g11") or k in ("features", "reward", "split")})
    g["n"] = [int((~m).sum()) for m in g["split"]]
    return g


def standardised(g, f):
    tr = ~g["split"][f]
    mean, scale, _ = R.scaler(g["features"][tr])
    return tr, F.standardise32(g["features"], mean, scale)


def test_fixture_conditions(g11):
    assert str(g11["sklearn_version"]) == "1.7.2"
    assert (int(g11["T"]), int(g11["max_depth"]), int(g11["keep"])) == (100, 20, 3)
    assert g11["seeds"].tolist() == [0, 1] and g11["min_samples_split"].tolist() == [100, 20]
    splits = tied = 0
    for mss in (100, 20):
        for seed in (0, 1):
            for f, m in enumerate(g11["split"]):
                key = f"o{mss}_s{seed}_{f}"
                n, y = g11["n"][f], g11["reward"][~m]
                assert int(g11[f"q_{key}"]) == 55 and g11[f"node_count_{key}"].shape == (100,)
                # every in-bag leaf value was within this bound of sklearn's own, tree by tree
                bound = n * EPS * float(np.abs(y - float(g11[f"init_{key}"])).max()) + 2.0 ** -55
                assert float(g11[f"value_dist_{key}"]) <= bound
                # a split node has two children and the root is nobody's child
                assert int(g11[f"split_nodes_{key}"]) == int((g11[f"node_count_{key}"] - 1).sum()) // 2
                if mss == 20:
                    splits += int(g11[f"split_nodes_{key}"])
                    tied += int(g11[f"tied_nodes_{key}"])
                    assert int(g11[f"tied_nodes_{key}"]) > 0 and int(g11[f"node_count_{key}"].max()) > 30
                    # the whole-forest estimates differ from sklearn's where the tie rule decided: documentation
                    assert 0.0 < float(g11[f"val_dist_{key}"]) < 1e-2
                else:
                    assert int(g11[f"node_count_{key}"].max()) <= 7
    assert splits > 8000 and 150 < tied < splits // 20  # the tie rule decides a few per cent of the real trees


def test_bootstrap_is_the_stored_one(g11):
    from edgeml_amd import rfr
    for seed in (0, 1):
        counts = rfr.bootstrap_counts(seed, 3, 100, g11["n"])
        assert [c.shape for c in counts] == [(100, n) for n in g11["n"]] and all(c.dtype == np.uint8 for c in counts)
        assert all(np.all(c.sum(axis=1) == n) for c, n in zip(counts, g11["n"]))
        assert F.counts_digest(counts) == str(g11[f"counts_sha256_s{seed}"])
        assert max(int(c.max()) for c in counts) == int(g11[f"counts_max_s{seed}"])
        for a, b in zip(counts, F.bootstrap_counts(seed, 3, 100, g11["n"])):
            np.testing.assert_array_equal(a, b)
    # the chain: one RandomState(seed), one randint per fold in fold order, nothing else drawn in between
    rs = np.random.RandomState(1)
    first = rs.randint(np.iinfo(np.int32).max, size=100)
    np.testing.assert_array_equal(F.tree_seeds(1, 3, 100)[0], first)
    np.testing.assert_array_equal(F.tree_seeds(1, 3, 100)[1], rs.randint(np.iinfo(np.int32).max, size=100))
    n = g11["n"][0]
    np.testing.assert_array_equal(rfr.bootstrap_counts(1, 3, 100, g11["n"])[0][7],
                                  np.bincount(np.random.RandomState(first[7]).randint(0, n, n), minlength=n))


def test_restatement_reproduces_g11(g11):
    """The whole forests at the reference's options (small trees), the stored first trees at min_samples_split 20."""
    keep = int(g11["keep"])
    for f in range(len(g11["split"])):
        tr, z32 = standardised(g11, f)
        y = g11["reward"][tr]
        for seed in (0, 1):
            counts = F.bootstrap_counts(seed, 3, 100, g11["n"])[f]
            key = f"o100_s{seed}_{f}"
            fit = F.fit(z32[tr], y, z32, counts, 20, 100)
            assert (fit["init"], fit["q"]) == (float(g11[f"init_{key}"]), int(g11[f"q_{key}"]))
            assert fit["feature"].shape == (100, F.node_cap(20, g11["n"][f])) and fit["feature"].dtype == np.int16
            assert F.digest(fit) == str(g11[f"sha256_{key}"])
            np.testing.assert_array_equal(fit["est"], g11[f"est_{key}"])
            np.testing.assert_array_equal(fit["node_count"], g11[f"node_count_{key}"])
            assert fit["tied_nodes"] == int(g11[f"tied_nodes_{key}"])
        counts = F.bootstrap_counts(0, 3, 100, g11["n"])[f][:keep]
        for mss in (100, 20):
            key = f"o{mss}_s0_{f}"
            fit = F.fit(z32[tr], y, z32, counts, 20, mss)
            np.testing.assert_array_equal(fit["node_count"], g11[f"node_count_{key}"][:keep])
            for name, _ in F.ARRAYS:
                stored = g11[f"{name}_{key}"]
                np.testing.assert_array_equal(fit[name][:, :stored.shape[1]], stored, err_msg=f"{key} {name}")
                assert np.all(fit[name][:, stored.shape[1]:] == (-1 if name in ("feature", "left") else 0))
            assert F.predict(fit, z32).shape == (len(z32),)


def test_restatement_rules():
    """The threshold rule, weights, a row of weight 0, the tie rule and the exact impurity rule on hand-made nodes."""
    a = np.float32(0.25)
    near, far = np.float32(0.25 + 6e-8), np.float32(0.25 + 2e-7)
    assert near > a and not near > a + F.FEATURE_THRESHOLD and far > a + F.FEATURE_THRESHOLD
    yq, slot, w = np.array([5, -5], np.int64), np.zeros(2, np.int64), np.ones(2, np.int64)
    for b, feature in ((near, -1), (far, 0)):
        z = np.array([[a], [b]], np.float32)
        rec = F.best_split(z, F.orders(z), slot, w, yq, 1, 26)[0]
        assert rec["feature"] == feature and rec["leaf"] == (feature < 0)
    # weights: the left side of the best split carries 1 + 3 = 4 of W = 7, two of the three in-bag rows left
    z = np.array([[0.1], [0.2], [0.3], [0.4]], np.float32)
    rec = F.best_split(z, F.orders(z), np.zeros(4, np.int64), np.array([1, 3, 0, 3]), np.array([8, 8, 99, -8]) << 30,
                       1, 40)[0]
    assert (rec["cnt"], rec["W"], rec["S"]) == (3, 7, 8 << 30)
    assert (rec["wl"], rec["cl"], rec["Sl"]) == (4, 2, 32 << 30)
    assert rec["threshold"] == float(np.float32(0.2)) / 2.0 + float(np.float32(0.4)) / 2.0  # the weightless row is skipped
    assert not rec["leaf"] and F.best_split(z, F.orders(z), np.zeros(4, np.int64), np.array([1, 3, 0, 3]),
                                            np.array([8, 8, 99, -8]) << 30, 1, 40, min_samples_split=4)[0]["leaf"]
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, 40).astype(np.float32)
    yq = np.rint(x * 1000).astype(np.int64) << 30
    w = rng.integers(0, 4, 40)
    for z in (np.stack([x[::-1], x, x], 1), np.stack([x[::-1], x, -x], 1)):  # a copy, a negated copy
        rec = F.best_split(np.ascontiguousarray(z), F.orders(z), np.zeros(40, np.int64), w, yq, 1, 40)[0]
        assert rec["feature"] == 1 and rec["tied"]
    # W sum w yq^2 - S^2 = d^2 A B for rows of weight A in all d quanta above rows of weight B; at q = 26 the bound is W^2
    for d, leaf in ((0, True), (2, True), (3, False)):
        assert F.impurity_leaf(*F.node_sums(np.arange(4), np.array([1, 3, 3, 1]),
                                            np.array([1 << 50, 1 << 50, (1 << 50) + d, (1 << 50) + d]))[1:], 26) == leaf


def test_option_defaults_and_checks(g11):
    from edgeml_amd import regress, rfr
    o = rfr.RFROpt()
    assert (o.n_estimators, o.max_depth, o.min_samples_split) == (100, 20, 100)
    assert sorted(rfr.FITS) == ["RFR"] and rfr._Folds is regress._Folds and rfr.NAMES["RFR"] == "Random Forest Regressor"
    assert rfr.node_cap(20, 237) == 473 == F.node_cap(20, 237) and rfr.node_cap(3, 237) == 15
    args = (g11["features"], g11["reward"], g11["split"])
    with pytest.raises(ValueError, match="max_depth = 0"):
        rfr.fit_rfr(*args, rfr.RFROpt(max_depth=0))
    for mss in (1, 0):
        with pytest.raises(ValueError, match=f"min_samples_split = {mss}"):
            rfr.fit_rfr(*args, rfr.RFROpt(min_samples_split=mss))
    with pytest.raises(ValueError, match="n_estimators = 0"):
        rfr.fit_rfr(*args, rfr.RFROpt(n_estimators=0))


def test_cli_arguments_and_refusals():
    import torch
    from edgeml_amd import estimator, gbr, rfr
    a = rfr.getargs(["d", "r", "s", "o", "--model", "RFR", "--normalize", "--model-dir", "m"])
    assert (a.data_dir, a.reward_path, a.split_path, a.save_dir) == ("d", "r", "s", "o")
    assert a.model == "RFR" and a.normalize and a.model_dir == "m" and a.stage == 24 and a.seed == 0
    assert (a.n_estimators, a.max_depth, a.min_samples_split) == (100, 20, 100)
    b = rfr.getargs(["d", "r", "s", "o", "--n-estimators", "7", "--max-depth", "4", "--min-samples-split", "20",
                     "--seed", "3"])
    assert b.model == "RFR" and (b.n_estimators, b.max_depth, b.min_samples_split, b.seed) == (7, 4, 20, 3)
    for name in ("GBR", "SGD", "LR", "SVR"):
        with pytest.raises(SystemExit, match=f"--model {name}"):
            rfr.main(rfr.getargs(["d", "r", "s", "o", "--model", name]))
    with pytest.raises(SystemExit, match="--stage 24"):
        rfr.main(rfr.getargs(["d", "r", "s", "o", "--stage", "17"]))
    with pytest.raises(SystemExit, match="max_depth = 0"):
        rfr.main(rfr.getargs(["d", "r", "s", "o", "--max-depth", "0"]))
    with pytest.raises(SystemExit, match="min_samples_split = 1"):
        rfr.main(rfr.getargs(["d", "r", "s", "o", "--min-samples-split", "1"]))
    with pytest.raises(SystemExit) as e:  # the estimator CLI still refuses it, and now says where it is
        estimator.check_model(estimator.getargs(["d", "r", "s", "o", "--model", "RFR"]))
    assert "--model RFR is not built" in str(e.value) and "python -m edgeml_amd.rfr fits RFR" in str(e.value)
    with pytest.raises(SystemExit, match="--model RFR"):
        gbr.main(gbr.getargs(["d", "r", "s", "o", "--model", "RFR"]))
    if not torch.cuda.is_available():  # the refusal only exists where no device does
        x = np.zeros((4, 2))
        with pytest.raises(RuntimeError, match="no CPU path"):
            rfr.fit_rfr(x, np.zeros(4), np.array([[True, False, False, False]]))


def _model(D=9, seed=1):
    """Two trees in arrays of cap 7: a root with two leaves, and a root whose right child splits again."""
    rng = np.random.default_rng(seed)
    feature = np.array([[2, -1, -1, -1, -1, -1, -1], [0, -1, 8, -1, -1, -1, -1]], np.int16)
    left = np.array([[1, -1, -1, -1, -1, -1, -1], [1, -1, 3, -1, -1, -1, -1]], np.int32)
    threshold = np.where(feature >= 0, rng.normal(0, 1, feature.shape), 0.0)
    count = np.array([3, 5], np.int32)
    value = np.where(np.arange(7)[None, :] < count[:, None], rng.normal(0, 1, feature.shape), 0.0)
    nsamp = np.where(np.arange(7)[None, :] < count[:, None], 5, 0).astype(np.int32)
    return {"model": "RFR", "mean": rng.normal(0, 1, D), "scale": rng.uniform(0.5, 2, D), "init": 0.25, "q": 55,
            "feature": feature, "threshold": threshold, "left": left, "value": value, "n_node_samples": nsamp,
            "node_count": count}


def test_load_estimator_takes_rfr_files_and_refuses_broken_ones(tmp_path):
    from edgeml_amd import offload, rfr
    D = 9
    good = _model(D)

    def load(m, width=D):
        with open(tmp_path / "wts.pickle", "wb") as f:
            pickle.dump(m, f)
        return offload.load_estimator(str(tmp_path / "wts.pickle"), width)

    est = load(good)
    assert est.kind == "rfr" and est.width == D and isinstance(est.model, rfr.RFRModel) and est.workspace_bytes(64) == 0
    assert (est.model.T, est.model.cap, est.model.init) == (2, 7, 0.25)
    np.testing.assert_array_equal(est.model.left, good["left"])
    np.testing.assert_array_equal(est.model.value, good["value"])
    with pytest.raises(ValueError, match="features, the cascade makes 10"):
        load(good, D + 1)
    with pytest.raises(ValueError, match="not a wts<fold>.pickle of edgeml_amd.rfr"):
        rfr.load({**good, "model": "GBR"})
    for key in ("feature", "left", "value", "init", "node_count"):
        with pytest.raises(ValueError, match=f"an RFR file without '{key}'"):
            load({k: v for k, v in good.items() if k != key})
    for key, bad in (("value", good["value"][:, :-1]), ("threshold", good["threshold"][:-1]),
                     ("left", good["left"][:, :3]), ("node_count", good["node_count"][:1]),
                     ("scale", good["scale"][:-1])):
        with pytest.raises(ValueError, match="tree arrays of shapes|'scale'"):
            load({**good, key: bad})
    with pytest.raises(ValueError, match="integers from -1 to 8"):
        load({**good, "feature": np.where(good["feature"] >= 0, D, -1).astype(np.int16)})
    for left in ([[1, -1, -1, -1, -1, -1, -1], [1, -1, 4, -1, -1, -1, -1]],    # the right child is past node_count
                 [[0, -1, -1, -1, -1, -1, -1], [1, -1, 3, -1, -1, -1, -1]],    # a node that is its own child
                 [[1, -1, -1, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1, -1]]):  # a split node without children
        with pytest.raises(ValueError, match="'left' out of range"):
            load({**good, "left": np.array(left, np.int32)})
    with pytest.raises(ValueError, match="'node_count' must hold integers from 1 to 7"):
        load({**good, "node_count": np.array([3, 8], np.int32)})
    for key in ("value", "threshold"):
        with pytest.raises(ValueError, match="must be finite"):
            load({**good, key: np.full_like(good[key], np.nan)})
    with pytest.raises(ValueError, match="must be finite"):
        load({**good, "init": float("inf")})
    info = {"mean": good["mean"][None], "scale": good["scale"][None], "init": np.array([0.25]), "q": np.array([55]),
            "node_count": good["node_count"][None], **{key: [good[key]] for key in rfr.ARRAYS}}
    m = rfr.model_data(info, 0)
    assert sorted(m) == sorted(["model", "q", *rfr.KEYS]) and m["model"] == "RFR"
    assert all(isinstance(v, (np.ndarray, float, int, str)) for v in m.values())
    assert load(m).kind == "rfr"


def test_header_declares_and_library_exports_the_new_names():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        txt = f.read()
    assert "random forest regressor" in txt
    declared = set(re.findall(r"\b(edgedet_[a-z_0-9]+)\s*\(", txt))
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in ops.EXPORTS and hasattr(lib, name), name
    assert lib.edgedet_rfr_node_cap(237, 20) == 473 and lib.edgedet_rfr_node_cap(237, 3) == 15
    assert lib.edgedet_rfr_node_cap(4000, 64) == 7999 and lib.edgedet_rfr_node_cap(1, 1) == 1
    assert lib.edgedet_rfr_node_cap(0, 20) < 0 and lib.edgedet_rfr_node_cap(237, 0) < 0
    off = (ctypes.c_int64 * 3)(0, 5, 12)
    size = lambda *a: lib.edgedet_rfr_workspace_size(*a)  # noqa: E731
    base = size(off, 2, 34, 10, 20, 2, 1)
    assert base > 0 and base % 8 == 0 and size(off, 2, 34, 10, 20, 2, 4) > base > size(off, 2, 34, 10, 2, 2, 1)
    for bad in ((off, 2, 256, 10, 20, 2, 1), (off, 2, 0, 10, 20, 2, 1), (off, 2, 34, 0, 20, 2, 1),
                (off, 2, 34, 10, 0, 2, 1), (off, 2, 34, 10, 65, 2, 1), (off, 2, 34, 10, 20, 1, 1),
                (off, 2, 34, 10, 20, 2, 0), (off, 2, 34, 10, 20, 2, 17), (None, 2, 34, 10, 20, 2, 1),
                (off, 0, 34, 10, 20, 2, 1), ((ctypes.c_int64 * 3)(0, 5, 5), 2, 34, 10, 20, 2, 1)):
        assert size(*bad) < 0, bad[1:]
    unit = lib.edgedet_rfr_best_split_workspace_size
    assert unit(100, 5, 8, 2) > 0 and unit(0, 5, 8, 2) < 0 and unit(100, 256, 8, 2) < 0 and unit(100, 5, 0, 2) < 0 \
        and unit(100, 5, 8, 17) < 0
