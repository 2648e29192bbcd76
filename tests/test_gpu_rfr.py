"""The random forest regressor of edgeml_amd.rfr (csrc/rfr.hip) against G11 (tests/golden/g11_rfr.npz) and the
numpy restatement (tests/rfr_ref.py).  Every comparison is exact: the bootstrap is numpy's frozen stream, the
weighted sums are integers, every gain is a fixed sequence of individually rounded float64 operations on them,
and one rule decides among bit-equal gains, so the device has no freedom a tolerance would have to cover.  G11
itself was held to regression.py's own RFR under sklearn 1.7.2, tree by tree, when it was made
(tests/golden/make_golden_rfr.py)."""
import os
import pickle

import numpy as np
import pytest

from tests import regress_ref as R
from tests import rfr_ref as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = tuple(name for name, _ in F.ARRAYS)


@pytest.fixture(scope="module")
def g11():
    g = {}
    for name in ("g7_regressors.npz", "g11_rfr.npz"):
        with np.load(os.path.join(HERE, "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g11") or k in ("features", "reward", "split")})
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    g["n"] = [int((~m).sum()) for m in g["split"]]
    ref = []
    for m in g["split"]:  # the standardised rows of the restatement, once
        tr = ~m
        mean, scale, _ = R.scaler(g["features"][tr])
        ref.append({"tr": tr, "z32": F.standardise32(g["features"], mean, scale), "y": g["reward"][tr]})
    g["ref"] = ref
    return g


@pytest.fixture(scope="module")
def fits(g11):
    """(min_samples_split, seed) -> the fit of all folds at the reference's other options; fitted once each,
    shared, never modified."""
    from edgeml_amd import rfr
    cache = {}

    def get(mss, seed):
        if (mss, seed) not in cache:
            cache[mss, seed] = rfr.fit_rfr(g11["features"], g11["reward"], g11["split"],
                                           rfr.RFROpt(min_samples_split=mss), seed=seed)
        return cache[mss, seed]
    return get


def all_rows(g, results, f):
    est = np.empty(len(g["reward"]))
    est[~g["split"][f]], est[g["split"][f]] = results[f]["train_est"], results[f]["val_est"]
    return est


def model_of(info, f):
    return {**{key: info[key][f] for key in ARRAYS}, "node_count": info["node_count"][f]}


def same_info(a, b):
    for key in ("init", "q", "mean", "scale", "node_count", "tied_nodes"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for key in ARRAYS:
        for x, y in zip(a[key], b[key]):
            np.testing.assert_array_equal(x, y, err_msg=key)


def check_against_restatement(g, results, info, counts, depth, mss, folds=None):
    for f in (range(g["folds"]) if folds is None else folds):
        r = g["ref"][f]
        want = F.fit(r["z32"][r["tr"]], r["y"], r["z32"], counts[f], depth, mss)
        for key in ARRAYS:
            np.testing.assert_array_equal(info[key][f], want[key], err_msg=f"fold {f} {key}")
        np.testing.assert_array_equal(info["node_count"][f], want["node_count"])
        assert info["tied_nodes"][f] == want["tied_nodes"]
        assert (info["init"][f], info["q"][f]) == (want["init"], want["q"])
        np.testing.assert_array_equal(all_rows(g, results, f), want["est"])
    return want


# ------------------------------------------------------------------------------------- the whole fit
@pytest.mark.parametrize("mss,seed", [(100, 0), (20, 0), (100, 1), (20, 1)])
def test_whole_fit_is_g11(g11, fits, mss, seed):
    results, info = fits(mss, seed)
    T = int(g11["T"])
    tied = 0
    for f in range(g11["folds"]):
        key = f"o{mss}_s{seed}_{f}"
        cap = F.node_cap(20, g11["n"][f])
        assert info["feature"][f].shape == (T, cap) and info["feature"][f].dtype == np.int16
        assert info["left"][f].dtype == np.int32 and info["n_node_samples"][f].dtype == np.int32
        if seed == 0:
            for name in ARRAYS:
                stored = g11[f"{name}_{key}"]
                np.testing.assert_array_equal(info[name][f][:len(stored), :stored.shape[1]], stored,
                                              err_msg=f"fold {f} {name}")
        assert F.digest(model_of(info, f)) == str(g11[f"sha256_{key}"])
        assert info["init"][f] == float(g11[f"init_{key}"]) and info["q"][f] == int(g11[f"q_{key}"])
        np.testing.assert_array_equal(info["node_count"][f], g11[f"node_count_{key}"])
        assert info["tied_nodes"][f] == int(g11[f"tied_nodes_{key}"])
        tied += int(info["tied_nodes"][f])
        np.testing.assert_array_equal(all_rows(g11, results, f), g11[f"est_{key}"])
    assert (tied > 0) == (mss == 20)  # the tie rule is exercised on the real trees


# ------------------------------------------------------------------------------------- scan units
def device_best_split(z32, slot, w, yq, nn, q, mss, groups):
    """edgedet_rfr_best_split on one tree: z32 [n, D] float32, slot [n] (a value outside 0..nn-1: in no node), w
    [n], yq [n]."""
    import torch
    from edgeml_amd import ops
    n, D = z32.shape
    order = F.orders(z32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g_ord, g_val = t(order.astype(np.int32)), t(np.take_along_axis(z32.T, order, axis=1))
    g_slot, g_w, g_yq = t(slot.astype(np.int32)), t(w.astype(np.uint8)), t(yq.astype(np.int64))
    L, p = ops.lib(), ops._ptr
    wb = int(L.edgedet_rfr_best_split_workspace_size(n, D, nn, groups))
    assert wb > 0
    ws = torch.zeros(wb // 8, dtype=torch.float64, device="cuda")
    kinds = {"cnt": torch.int32, "W": torch.int32, "S": torch.int64, "feature": torch.int32, "threshold": torch.float64,
             "gain": torch.float64, "wl": torch.int32, "cl": torch.int32, "Sl": torch.int64, "leaf": torch.int32,
             "tied": torch.int32}
    out = {k: torch.full((nn,), np.nan if d == torch.float64 else -7, dtype=d, device="cuda") for k, d in kinds.items()}
    ops.check(L.edgedet_rfr_best_split(p(g_ord), p(g_val), n, D, p(g_slot), p(g_w), p(g_yq), nn, q, mss, groups, p(ws),
                                       wb, *[p(out[k]) for k in kinds], ops.stream_handle()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, order


def check_split(z32, slot, w, yq, nn, q=40, mss=2, groups=(1, 3)):
    """Device against restatement, exact in every field, at more than one grid shape; returns the restatement's
    records."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32)
    slot, w, yq = np.asarray(slot, np.int64), np.asarray(w, np.int64), np.asarray(yq, np.int64)
    for G in groups:
        got, order = device_best_split(z32, slot, w, yq, nn, q, mss, G)
        want = F.best_split(z32, order, slot, w, yq, nn, q, mss)
        for m, r in enumerate(want):
            where = f"node {m}, {G} groups"
            for key in ("cnt", "W", "S", "feature", "threshold", "wl", "cl", "Sl"):
                assert got[key][m] == r[key], (where, key, got[key][m], r[key])
            assert np.float64(got["gain"][m]).view(np.int64) == np.float64(r["gain"]).view(np.int64), where  # the bits
            assert bool(got["leaf"][m]) == r["leaf"] and bool(got["tied"][m]) == r["tied"], where
    return want


def quanta(rng, signal, q=40):
    """Target quanta around a signal: |yq| < 2^(q - 1), far inside 2^(62 - ceil(log2 n)) at q = 40."""
    r = 0.2 * np.tanh(signal) + 0.02 * rng.normal(0, 1, len(signal))
    return np.rint(np.ldexp(r, q)).astype(np.int64)


def test_scan_a_node_of_two_rows():
    rng = np.random.default_rng(1)
    z = rng.normal(0, 1, (10, 3))
    slot = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1])
    w = np.array([2, 1, 3, 0, 1, 1, 4, 1, 1, 2])
    want = check_split(z, slot, w, quanta(rng, z[:, 1]), 2)
    assert want[0]["cnt"] == 2 and want[0]["cl"] == 1 and want[0]["W"] == 4 and want[0]["feature"] >= 0
    assert want[1]["cnt"] == 7 and want[1]["W"] == 12


@pytest.mark.parametrize("n,D,nn,top", [(237, 7, 4, 4), (1500, 5, 300, 3), (300, 205, 2, 7), (64, 1, 1, 2), (65, 2, 1, 2)])
def test_scan_shapes(n, D, nn, top):
    """n = 237 is no multiple of the 64-row chunk; 1,500 rows in 300 nodes are more live nodes than one LDS pass
    holds (128), so the level is scanned in three slices; 205 features are the widest the reference uses, with
    weights up to the largest count a bootstrap of the fixture draws."""
    rng = np.random.default_rng(n + D)
    z = np.round(rng.normal(0, 1, (n, D)), 2)  # two decimals: many equal values inside a list
    slot = rng.integers(-1, nn, n)             # -1: rows in a finished leaf
    w = rng.integers(0, top + 1, n)            # 0: out of bag
    want = check_split(z, slot, w, quanta(rng, z[:, D // 2] - z[:, 0]), nn)
    assert sum(r["feature"] >= 0 for r in want) > nn // 2 and max(r["W"] for r in want) > top


def test_scan_sixty_four_nodes_in_one_chunk():
    """The first 64 rows of feature 0's list sit in 64 different nodes, and so do the next 64: every lane of a chunk
    is a round of its own.  150 in-bag rows in 75 nodes, as a level looks at min_samples_split = 2."""
    rng = np.random.default_rng(5)
    n, nn = 150, 75
    slot = np.concatenate([np.arange(64), np.arange(64), 64 + np.arange(22) // 2])
    z = rng.normal(0, 1, (n, 3))
    z[:, 0] = np.arange(n) / 16.0
    w = rng.integers(1, 4, n)
    want = check_split(z, slot, w, quanta(rng, z[:, 1]), nn)
    assert len(set(slot[F.orders(z.astype(np.float32))[0][:64]])) == 64
    assert all(r["cnt"] == 2 and r["feature"] >= 0 for r in want)


def test_scan_a_row_of_weight_zero_between_two_candidates():
    z = np.array([[0.1], [0.2], [0.3], [0.4]])
    want = check_split(z, np.zeros(4, int), np.array([1, 3, 0, 3]), np.array([8, 8, 99, -8]) << 30, 1, groups=(1,))
    assert (want[0]["cnt"], want[0]["W"], want[0]["wl"], want[0]["cl"]) == (3, 7, 4, 2)
    assert want[0]["threshold"] == float(np.float32(0.2)) / 2.0 + float(np.float32(0.4)) / 2.0


def test_scan_a_column_constant_inside_one_node():
    rng = np.random.default_rng(2)
    n = 200
    z = rng.normal(0, 1, (n, 3))
    slot = (np.arange(n) % 2)
    z[slot == 0, 0] = 0.5                      # constant in node 0 only
    want = check_split(z, slot, rng.integers(0, 3, n), quanta(rng, 3 * z[:, 0]), 2)
    assert want[0]["feature"] in (1, 2) and want[1]["feature"] == 0


def test_scan_feature_threshold():
    """sklearn's FEATURE_THRESHOLD, in float32: 0.25 and 0.25 + 6e-8 are not split, 0.25 and 0.25 + 2e-7 are."""
    yq = np.array([1 << 30, -(1 << 30)])
    for delta, feature in ((6e-8, -1), (2e-7, 0)):
        z = np.array([[0.25], [0.25 + delta]], np.float32)
        assert z[1, 0] > z[0, 0]
        want = check_split(z, np.zeros(2, int), np.array([2, 1]), yq, 1, groups=(1,))
        assert want[0]["feature"] == feature and want[0]["leaf"] == (feature < 0)
    # inside a longer list: only the wide gap is a candidate
    z = np.array([[0.25], [0.25 + 6e-8], [0.25 + 2.6e-7], [0.25 + 3.2e-7]], np.float32)
    want = check_split(z, np.zeros(4, int), np.ones(4, int), np.array([4, 1, -2, -3]) << 30, 1, groups=(1,))
    assert want[0]["cl"] == 2


def test_scan_tie_rules():
    """A duplicated column, and a negated duplicate (the complementary partition: diff changes sign, diff * diff
    and wl * wr do not, so the gain is bit-equal): the lower index wins, and the node counts as tied, whichever wave
    or workgroup met which column."""
    rng = np.random.default_rng(3)
    x, other = rng.normal(0, 1, 150), rng.normal(0, 1, 150)
    yq, w = quanta(rng, 2 * x), rng.integers(0, 4, 150)
    for cols in ((other, x, x), (other, x, -x), (other, -x, x), (other, x, other, other, other, x),
                 (x, other, other, other, x, other, other)):
        want = check_split(np.stack(cols, 1), np.zeros(150, int), w, yq, 1, groups=(1, 2, 3))
        assert want[0]["feature"] == (0 if cols[0] is x else 1) and want[0]["tied"]
    want = check_split(np.stack((other, x, other + x), 1), np.zeros(150, int), w, yq, 1)
    assert want[0]["feature"] == 1 and not want[0]["tied"]


def test_scan_exact_impurity_rule_with_weights():
    """W sum w yq^2 - S^2 <= W^2 2^(2q - 52), exactly.  With rows of weight A in all d quanta above rows of weight B
    the left side is d^2 A B; here A = B = W / 2 (the weights alternate 1, 3 on one half and 3, 1 on the other), so
    at q = 26 (right side W^2) two quanta sit exactly on the bound and three are above it; at q = 27 (right side
    4 W^2) the same holds for four and five.  The offset 2^50 makes the squares need all 128 bits' worth of care."""
    n = 64
    z = np.arange(n, dtype=np.float32)[:, None] / 8
    w = np.array([1, 3] * (n // 4) + [3, 1] * (n // 4))
    base = 1 << 50
    for q, on, above in ((26, 2, 3), (27, 4, 5)):
        for d, leaf in ((0, True), (1, True), (on, True), (above, False)):
            yq = np.array([base] * (n // 2) + [base + d] * (n // 2))
            want = check_split(z, np.zeros(n, int), w, yq, 1, q=q, groups=(1,))
            assert want[0]["leaf"] == leaf and want[0]["feature"] == 0, (q, d)  # gain 0 is still a valid candidate
    # uneven weights: A = 5 against B = 123: 25 * 5 * 123 < 128^2 <= 36 * 5 * 123
    w = np.array([2] * 60 + [1] * 3 + [5])
    for d, leaf in ((5, True), (6, False)):
        yq = np.array([base] * (n - 1) + [base + d])
        assert check_split(z, np.zeros(n, int), w, yq, 1, q=26, groups=(1,))[0]["leaf"] is leaf
    # min_samples_split closes a node that has a candidate
    want = check_split(z, np.zeros(n, int), w, yq, 1, q=26, mss=65, groups=(1,))
    assert want[0]["leaf"] and want[0]["feature"] == 0


# ------------------------------------------------------------------------------------------ shapes
def test_wide_rows_against_the_restatement():
    """1,500 training rows at the reference's 205 features, four trees: many chunks per list, 52 features per
    workgroup and wave."""
    from edgeml_amd import rfr
    rng = np.random.default_rng(11)
    N, D, T = 1600, 205, 4
    x = np.round(rng.normal(0, 1, (N, D)), 1)
    y = np.tanh(x[:, 3] - x[:, 200]) + 0.1 * rng.normal(0, 1, N)
    split = np.zeros((1, N), bool)
    split[0, 1500:] = True
    results, info = rfr.fit_rfr(x, y, split, rfr.RFROpt(n_estimators=T), seed=4)
    mean, scale, _ = R.scaler(x[:1500])
    z32 = F.standardise32(x, mean, scale)
    want = F.fit(z32[:1500], y[:1500], z32, F.bootstrap_counts(4, 1, T, [1500])[0], 20, 100)
    for key in ARRAYS:
        np.testing.assert_array_equal(info[key][0], want[key], err_msg=key)
    np.testing.assert_array_equal(info["node_count"][0], want["node_count"])
    np.testing.assert_array_equal(np.concatenate([results[0]["train_est"], results[0]["val_est"]]), want["est"])
    assert want["node_count"].min() > 7


@pytest.mark.parametrize("depth,mss,T", [(1, 2, 5), (3, 20, 1), (20, 2, 6)])
def test_other_shapes_against_the_restatement(g11, depth, mss, T):
    from edgeml_amd import rfr
    results, info = rfr.fit_rfr(g11["features"], g11["reward"], g11["split"],
                                rfr.RFROpt(n_estimators=T, max_depth=depth, min_samples_split=mss), seed=2)
    want = check_against_restatement(g11, results, info, F.bootstrap_counts(2, 3, T, g11["n"]), depth, mss)
    if depth == 1:
        assert np.all(info["node_count"] == 3)
    if mss == 2:  # down to single rows: most of these splits are decided by the tie rule
        assert depth == 1 or (want["node_count"].min() > 250 and want["tied_nodes"] > 100)


def test_the_depth_limit_of_twenty_is_reached():
    """Indicator features, one per row: every candidate separates a single row from the rest of its node, so the
    tree is a chain of one row per level that only the depth limit ends."""
    from edgeml_amd import rfr
    n = 26
    x = np.eye(n)
    y = np.random.default_rng(7).normal(0, 1, n)
    split = np.zeros((1, n), bool)
    counts = [np.stack([np.ones(n, np.uint8), 1 + np.arange(n, dtype=np.uint8) % 3])]
    mean, scale, _ = R.scaler(x)
    z32 = F.standardise32(x, mean, scale)
    for depth, deepest in ((20, 20), (64, n - 1)):
        results, info = rfr.fit_rfr(x, y, split, rfr.RFROpt(n_estimators=2, max_depth=depth, min_samples_split=2),
                                    counts=counts)
        want = F.fit(z32, y, z32, counts[0], depth, 2)
        for key in ARRAYS:
            np.testing.assert_array_equal(info[key][0], want[key], err_msg=key)
        np.testing.assert_array_equal(results[0]["train_est"], want["est"])
        for t in range(2):
            assert F.tree_depth(want["feature"][t], want["left"][t], want["node_count"][t]) == deepest


def test_constant_targets(g11):
    """0.25 n is exact, so F0 = 0.25, every quantum is 0, every root is pure and every tree a single leaf."""
    from edgeml_amd import rfr
    y = np.full(len(g11["reward"]), 0.25)
    results, info = rfr.fit_rfr(g11["features"], y, g11["split"], rfr.RFROpt(n_estimators=3, min_samples_split=2))
    assert np.all(info["node_count"] == 1) and np.all(info["tied_nodes"] == 0) and np.all(info["init"] == 0.25)
    for f in range(g11["folds"]):
        assert np.all(info["feature"][f] == -1) and np.all(info["left"][f] == -1)
        assert np.all(info["value"][f][:, 0] == 0.25) and np.all(info["value"][f][:, 1:] == 0.0)
        assert np.all(all_rows(g11, results, f) == 0.25)


# ------------------------------------------------------------------------------------- determinism
def test_folds_together_equal_one_at_a_time(g11, fits):
    from edgeml_amd import rfr
    results3, info3 = fits(20, 0)
    counts = rfr.bootstrap_counts(0, 3, 100, g11["n"])
    for f in range(g11["folds"]):
        results, info = rfr.fit_rfr(g11["features"], g11["reward"], g11["split"][f:f + 1],
                                    rfr.RFROpt(min_samples_split=20), counts=counts[f:f + 1])
        for key in ARRAYS:
            np.testing.assert_array_equal(info[key][0], info3[key][f], err_msg=f"fold {f} {key}")
        for key in ("init", "q", "node_count", "tied_nodes"):
            np.testing.assert_array_equal(info[key][0], info3[key][f], err_msg=f"fold {f} {key}")
        np.testing.assert_array_equal(results[0]["val_est"], results3[f]["val_est"])
        np.testing.assert_array_equal(results[0]["train_est"], results3[f]["train_est"])


@pytest.mark.parametrize("groups", [None, 1, 5])
def test_two_runs_are_bit_identical_at_any_grid_shape(g11, fits, groups):
    from edgeml_amd import rfr
    results, info = rfr.fit_rfr(g11["features"], g11["reward"], g11["split"], rfr.RFROpt(min_samples_split=20),
                                groups=groups)
    same_info(info, fits(20, 0)[1])
    for f in range(g11["folds"]):
        np.testing.assert_array_equal(all_rows(g11, results, f), all_rows(g11, fits(20, 0)[0], f))


# ----------------------------------------------------------------------------------------- predict
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_model_predict_equals_the_fit(g11, fits, batch):
    import torch
    from edgeml_amd import rfr
    results, info = fits(20, 0)
    for f in range(g11["folds"]):
        model = rfr.load(rfr.model_data(info, f)).to("cuda")
        x = np.ascontiguousarray(g11["features"][g11["split"][f]][:batch])
        est = torch.full((batch,), np.nan, dtype=torch.float64, device="cuda")
        model.predict_into(torch.from_numpy(x).cuda(), est)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(est.cpu().numpy(), results[f]["val_est"][:batch])
        z32 = F.standardise32(x, info["mean"][f], info["scale"][f])
        np.testing.assert_array_equal(est.cpu().numpy(), F.predict(model_of(info, f), z32))
    np.testing.assert_array_equal(model.predict(g11["features"]), all_rows(g11, results, g11["folds"] - 1))


# ------------------------------------------------------------------------------------ CLI end to end
@pytest.fixture(scope="module")
def files(g11, tmp_path_factory):
    td = tmp_path_factory.mktemp("g11")
    fdir = td / "features"
    for i, x in enumerate(g11["features"]):
        (fdir / f"{i:06d}").mkdir(parents=True)
        np.save(fdir / f"{i:06d}" / "stage24_output_features.npy", x)
    np.savez(td / "reward.npz", reward=g11["reward"])
    np.save(td / "split.npy", g11["split"])
    return td


def test_cli_round_trip(g11, fits, files, capsys):
    import torch
    from edgeml_amd import offload, rfr
    results, info = fits(20, 1)
    save, mdir = files / "est", files / "model"
    rfr.main(rfr.getargs([str(files / "features"), str(files / "reward.npz"), str(files / "split.npy"), str(save),
                          "--model", "RFR", "--model-dir", str(mdir), "--min-samples-split", "20", "--seed", "1"]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("fold ")]
    assert len(lines) == g11["folds"]
    assert all("Trained Random Forest Regressor model with training MSE: " in ln and ", validation MSE: " in ln
               for ln in lines)
    D = g11["D"]
    for f in range(g11["folds"]):
        with np.load(save / f"estimate{f + 1}.npz", allow_pickle=False) as z:
            assert sorted(z.files) == ["train_est", "train_time", "val_est", "val_time"]
            np.testing.assert_array_equal(z["train_est"], results[f]["train_est"])
            np.testing.assert_array_equal(z["val_est"], results[f]["val_est"])
        with open(mdir / f"wts{f + 1}.pickle", "rb") as fh:
            m = pickle.load(fh)
        assert m["model"] == "RFR" and all(isinstance(m[k], (np.ndarray, float, int, str)) for k in m)
        assert sorted(m) == sorted(["model", "q", *rfr.KEYS])
        for key in ARRAYS:
            np.testing.assert_array_equal(m[key], info[key][f])
    # the cascade's side: the saved model of fold 1 decides on the device
    est = offload.load_estimator(str(mdir / "wts1.pickle"), D)
    assert est.kind == "rfr"
    with pytest.raises(ValueError, match=f"features, the cascade makes {D + 1}"):
        offload.load_estimator(str(mdir / "wts1.pickle"), D + 1)
    val = results[0]["val_est"]
    threshold = float(np.median(val))
    x = torch.from_numpy(np.ascontiguousarray(g11["features"][g11["split"][0]])).cuda()
    for a in range(0, len(val), 64):  # the cascade's batches hold up to 64 images
        b = min(a + 64, len(val))
        out = torch.full((b - a,), np.nan, dtype=torch.float64, device="cuda")
        flag = torch.full((b - a,), 7, dtype=torch.uint8, device="cuda")
        est.decide(x[a:b].contiguous(), threshold, out, flag, (None, None, None))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), val[a:b])
        np.testing.assert_array_equal(flag.cpu().numpy().astype(bool), val[a:b] > threshold)
    assert 0 < int((val > threshold).sum()) < len(val)


# ---------------------------------------------------------------------------------- argument checks
def test_launchers_refuse_bad_arguments():
    import ctypes

    import torch
    from edgeml_amd import ops
    L, p = ops.lib(), ops._ptr
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")  # stands for every device buffer: nothing is launched
    P, S = p(d), ops.stream_handle()
    off = (ctypes.c_int64 * 3)(0, 4, 9)
    q = (ctypes.c_int32 * 2)(55, 55)
    low = (ctypes.c_int32 * 2)(55, 25)

    def refused(rc, what):
        assert rc == -1, what
        assert what in L.edgedet_last_error().decode(), L.edgedet_last_error().decode()

    def fit(N=9, D=3, off=off, folds=2, q_host=q, T=5, depth=3, mss=2, groups=1, first=P, est=P, wb=1 << 20):
        return L.edgedet_rfr_fit(first, N, D, P, P, P, P, P, P, off, P, folds, P, q_host, P, P, P, T, depth, mss, groups,
                                 P, wb, P, P, P, P, P, P, P, P, est, S)

    for kw in ({"D": 0}, {"D": 256}, {"N": 0}):
        refused(fit(**kw), "rfr_fit: 1 <= features <= 255")
    for kw in ({"off": (ctypes.c_int64 * 3)(0, 4, 4)}, {"off": None}, {"folds": 0}):
        refused(fit(**kw), "rfr_fit: every fold needs")
    for kw in ({"depth": 0}, {"depth": 65}, {"T": 0}, {"mss": 1}, {"groups": 0}, {"groups": 17}):
        refused(fit(**kw), "rfr_fit: n_estimators >= 1")
    for kw in ({"first": None}, {"est": None}, {"q_host": None}):
        refused(fit(**kw), "rfr_fit: null pointer")
    refused(fit(q_host=low), "rfr_fit: 26 <= q")
    refused(fit(wb=64), "rfr_fit: workspace smaller")

    def split(n=9, D=3, nn=2, q=40, mss=2, groups=1, first=P, last=P, wb=1 << 20):
        return L.edgedet_rfr_best_split(first, P, n, D, P, P, P, nn, q, mss, groups, P, wb, P, P, P, P, P, P, P, P, P, P,
                                        last, S)

    for kw in ({"D": 0}, {"D": 256}, {"n": 0}):
        refused(split(**kw), "rfr_best_split: 1 <= features <= 255")
    for kw in ({"nn": 0}, {"mss": 1}, {"groups": 0}, {"groups": 17}):
        refused(split(**kw), "rfr_best_split: 1 <= nodes")
    refused(split(q=25), "rfr_best_split: 26 <= q")
    for kw in ({"first": None}, {"last": None}):
        refused(split(**kw), "rfr_best_split: null pointer")
    refused(split(wb=64), "rfr_best_split: workspace smaller")

    def predict(B=2, D=3, T=5, cap=7, first=P, est=P):
        return L.edgedet_rfr_model_predict(first, B, D, P, P, P, P, P, P, T, cap, est, S)

    for kw in ({"D": 0}, {"D": 256}, {"B": 0}):
        refused(predict(**kw), "rfr_model_predict: 1 <= features <= 255")
    for kw in ({"T": 0}, {"cap": 0}):
        refused(predict(**kw), "rfr_model_predict: n_estimators >= 1")
    for kw in ({"first": None}, {"est": None}):
        refused(predict(**kw), "rfr_model_predict: null pointer")
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0  # nothing ran
