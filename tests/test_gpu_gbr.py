"""The gradient boosting regressor of edgeml_amd.gbr (csrc/gbr.hip) against G9 (tests/golden/g9_gbr.npz) and the
numpy restatement (tests/gbr_ref.py).  Every comparison is exact: the residual sums are integers, every gain is
a fixed sequence of individually rounded float64 operations on them, and one rule decides among bit-equal gains,
so the device has no freedom a tolerance would have to cover.  G9 itself was held to regression.py's own GBR
under sklearn 1.7.2, leaf partition by leaf partition, when it was made (tests/golden/make_golden_gbr.py)."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import gbr_ref as B
from tests import regress_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("feature", "threshold", "value")


@pytest.fixture(scope="module")
def g9():
    g = {}
    for name in ("g7_regressors.npz", "g9_gbr.npz"):
        with np.load(os.path.join(HERE, "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g9") or k in ("features", "reward", "split")})
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    ref = []
    for m in g["split"]:  # the standardised rows of the restatement, once
        tr = ~m
        mean, scale, _ = R.scaler(g["features"][tr])
        ref.append({"tr": tr, "z32": B.standardise32(g["features"], mean, scale), "y": g["reward"][tr]})
    g["ref"] = ref
    return g


@pytest.fixture(scope="module")
def fits(g9):
    """The reference's options on all folds, fitted once; shared, never modified."""
    from edgeml_amd import gbr
    return gbr.fit_gbr(g9["features"], g9["reward"], g9["split"])


def all_rows(g, results, f):
    est = np.empty(len(g["reward"]))
    est[~g["split"][f]], est[g["split"][f]] = results[f]["train_est"], results[f]["val_est"]
    return est


def same_info(a, b):
    for key in (*ARRAYS, "init", "q", "mean", "scale", "nodes", "tied_nodes"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ------------------------------------------------------------------------------------- the whole fit
def test_whole_fit_is_g9(g9, fits):
    results, info = fits
    T, keep = int(g9["T"]), int(g9["keep"])
    assert info["feature"].shape == (g9["folds"], T, 7) and info["value"].shape == (g9["folds"], T, 15)
    assert info["feature"].dtype == np.int16
    for f in range(g9["folds"]):
        for key in ARRAYS:
            np.testing.assert_array_equal(info[key][f][:keep], g9[f"{key}{f}"], err_msg=f"fold {f} {key}")
        assert B.digest(info["feature"][f], info["threshold"][f], info["value"][f]) == str(g9[f"sha256_{f}"])
        assert info["init"][f] == float(g9[f"init{f}"]) and info["q"][f] == int(g9[f"q{f}"])
        np.testing.assert_array_equal(info["nodes"][f], g9[f"nodes{f}"])
        assert info["tied_nodes"][f] == int(g9[f"tied_nodes{f}"]) > 0  # the tie rule is exercised
        np.testing.assert_array_equal(all_rows(g9, results, f), g9[f"est{f}"])
        for sk in g9[f"sklearn_train_est{f}"]:  # regression.py's own fit under three seeds
            assert np.abs(results[f]["train_est"] - sk).max() <= float(g9[f"dist{f}"])


# ------------------------------------------------------------------------------------- scan units
def device_best_split(z32, node, rq, nn, q):
    """edgedet_gbr_best_split on one fold: z32 [n, D] float32, node [n] (a value >= nn: in no node), rq [n]."""
    import torch
    from edgeml_amd import ops
    n, D = z32.shape
    order = B.orders(z32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g_ord, g_val = t(order.astype(np.int32)), t(np.take_along_axis(z32.T, order, axis=1))
    g_node, g_rq = t(np.where((node >= 0) & (node < nn), node, 255).astype(np.uint8)), t(rq.astype(np.int64))
    L, p = ops.lib(), ops._ptr
    wb = int(L.edgedet_gbr_workspace_size((ctypes.c_int64 * 2)(0, n), 1, D))
    assert wb > 0
    ws = torch.zeros(wb // 8, dtype=torch.float64, device="cuda")
    out = {"feature": torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
           "threshold": torch.full((nn,), np.nan, dtype=torch.float64, device="cuda"),
           "gain": torch.full((nn,), np.nan, dtype=torch.float64, device="cuda"),
           "wl": torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
           "Sl": torch.full((nn,), -7, dtype=torch.int64, device="cuda"),
           "leaf": torch.full((nn,), -7, dtype=torch.int32, device="cuda"),
           "tied": torch.full((nn,), -7, dtype=torch.int32, device="cuda")}
    ops.check(L.edgedet_gbr_best_split(p(g_ord), p(g_val), n, D, p(g_node), p(g_rq), nn, q, p(ws), wb,
                                       *[p(out[k]) for k in ("feature", "threshold", "gain", "wl", "Sl", "leaf", "tied")],
                                       ops.stream_handle()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, order


def check_split(z32, node, rq, nn, q=40):
    """Device against restatement, exact in every field; returns the restatement's records."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32)
    node, rq = np.asarray(node, np.int64), np.asarray(rq, np.int64)
    got, order = device_best_split(z32, node, rq, nn, q)
    want = B.best_split(z32, order, node, rq, nn, q)
    for m, w in enumerate(want):
        where = f"node {m}"
        assert got["feature"][m] == w["feature"], where
        assert got["threshold"][m] == w["threshold"], where
        assert np.float64(got["gain"][m]).view(np.int64) == np.float64(w["gain"]).view(np.int64), where  # the bits
        assert got["wl"][m] == w["wl"] and got["Sl"][m] == w["Sl"], where
        assert bool(got["leaf"][m]) == w["leaf"] and bool(got["tied"][m]) == w["tied"], where
    return want


def quanta(rng, signal, q=40):
    """Residual quanta around a signal: |rq| < 2^(q - 1), far inside 2^(62 - ceil(log2 n)) at q = 40."""
    r = 0.2 * np.tanh(signal) + 0.02 * rng.normal(0, 1, len(signal))
    return np.rint(np.ldexp(r, q)).astype(np.int64)


def test_scan_a_node_of_two_rows():
    rng = np.random.default_rng(1)
    z = rng.normal(0, 1, (10, 3))
    node = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1])
    want = check_split(z, node, quanta(rng, z[:, 1]), 2)
    assert want[0]["cnt"] == 2 and want[0]["wl"] == 1 and want[0]["feature"] >= 0 and want[1]["cnt"] == 8


@pytest.mark.parametrize("n,D,nn", [(237, 7, 4), (1500, 5, 8), (300, 205, 2), (64, 1, 1), (65, 2, 1)])
def test_scan_shapes(n, D, nn):
    """n = 237 is no multiple of the 64-row chunk; 1,500 rows in eight nodes take many chunks per list with
    every node's running sums carried across them; 205 features are the widest the reference uses."""
    rng = np.random.default_rng(n + D)
    z = np.round(rng.normal(0, 1, (n, D)), 2)  # two decimals: many equal values inside a list
    node = rng.integers(0, nn + 1, n)          # the value nn: rows in a finished leaf
    want = check_split(z, node, quanta(rng, z[:, D // 2] - z[:, 0]), nn)
    assert all(w["feature"] >= 0 and w["cnt"] > n // (2 * (nn + 1)) for w in want)


def test_scan_a_column_constant_inside_one_node():
    rng = np.random.default_rng(2)
    n = 200
    z = rng.normal(0, 1, (n, 3))
    node = (np.arange(n) % 2)
    z[node == 0, 0] = 0.5                      # constant in node 0 only
    want = check_split(z, node, quanta(rng, 3 * z[:, 0]), 2)
    assert want[0]["feature"] in (1, 2) and want[1]["feature"] == 0


def test_scan_feature_threshold():
    """sklearn's FEATURE_THRESHOLD, in float32: 0.25 and 0.25 + 6e-8 are not split, 0.25 and 0.25 + 2e-7 are."""
    rq = np.array([1 << 30, -(1 << 30)])
    for delta, feature in ((6e-8, -1), (2e-7, 0)):
        z = np.array([[0.25], [0.25 + delta]], np.float32)
        assert z[1, 0] > z[0, 0]
        want = check_split(z, np.zeros(2, int), rq, 1)
        assert want[0]["feature"] == feature and want[0]["leaf"] == (feature < 0)
    # inside a longer list: only the wide gap is a candidate
    z = np.array([[0.25], [0.25 + 6e-8], [0.25 + 2.6e-7], [0.25 + 3.2e-7]], np.float32)
    want = check_split(z, np.zeros(4, int), np.array([4, 1, -2, -3]) << 30, 1)
    assert want[0]["wl"] == 2


def test_scan_tie_rules():
    """A duplicated column, and a negated duplicate (the complementary partition: diff changes sign, diff * diff
    and wl * wr do not, so the gain is bit-equal): the lower index wins, and the node counts as tied."""
    rng = np.random.default_rng(3)
    x, other = rng.normal(0, 1, 150), rng.normal(0, 1, 150)
    rq = quanta(rng, 2 * x)
    for cols in ((other, x, x), (other, x, -x), (other, -x, x)):
        want = check_split(np.stack(cols, 1), np.zeros(150, int), rq, 1)
        assert want[0]["feature"] == 1 and want[0]["tied"]
    want = check_split(np.stack((other, x, other + x), 1), np.zeros(150, int), rq, 1)
    assert want[0]["feature"] == 1 and not want[0]["tied"]


def test_scan_exact_impurity_rule():
    """n sum rq^2 - S^2 <= n^2 2^(2q - 52), exactly.  With k rows d quanta above the other n - k the left side is
    d^2 k (n - k) <= d^2 n^2 / 4, so at q = 26 (right side n^2) a difference of one or two quanta is always a
    leaf, two quanta on half the rows sit exactly on the bound, and three quanta on half the rows are above it;
    at q = 27 (right side 4 n^2) the same holds for four and five quanta.  The offset 2^50 makes the squares need
    all 128 bits' worth of care."""
    n = 64
    z = np.arange(n, dtype=np.float32)[:, None] / 8
    base = 1 << 50
    for q, on, above in ((26, 2, 3), (27, 4, 5)):
        for d, leaf in ((0, True), (1, True), (on, True), (above, False)):
            rq = np.array([base] * (n // 2) + [base + d] * (n // 2))
            want = check_split(z, np.zeros(n, int), rq, 1, q=q)
            assert want[0]["leaf"] == leaf and want[0]["feature"] == 0, (q, d)  # gain 0 is still a valid candidate
    rq = np.array([base] * (n - 1) + [base + 9])  # one row apart: 81 (n - 1) > n^2, no leaf; 64 (n - 1) < n^2, a leaf
    assert check_split(z, np.zeros(n, int), rq, 1, q=26)[0]["leaf"] is False
    rq[-1] = base + 8
    assert check_split(z, np.zeros(n, int), rq, 1, q=26)[0]["leaf"] is True


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("depth,T", [(1, 5), (4, 6), (3, 1)])
def test_other_shapes_against_the_restatement(g9, depth, T):
    from edgeml_amd import gbr
    results, info = gbr.fit_gbr(g9["features"], g9["reward"], g9["split"],
                                gbr.GBROpt(n_estimators=T, max_depth=depth))
    for f, r in enumerate(g9["ref"]):
        want = B.fit(r["z32"][r["tr"]], r["y"], r["z32"], 0.1, T, depth)
        for key in ARRAYS:
            np.testing.assert_array_equal(info[key][f], want[key], err_msg=f"fold {f} {key}")
        np.testing.assert_array_equal(info["nodes"][f], want["nodes"])
        assert info["tied_nodes"][f] == want["tied_nodes"]
        np.testing.assert_array_equal(all_rows(g9, results, f), want["est"])
    if depth == 4:
        assert info["nodes"].max() > 7  # the fourth level is used


def test_constant_targets(g9):
    """0.25 n is exact, so F0 = 0.25, every residual is 0 and every tree a single leaf of value 0."""
    from edgeml_amd import gbr
    y = np.full(len(g9["reward"]), 0.25)
    results, info = gbr.fit_gbr(g9["features"], y, g9["split"], gbr.GBROpt(n_estimators=3))
    assert np.all(info["feature"] == -1) and np.all(info["value"] == 0.0) and np.all(info["threshold"] == 0.0)
    assert np.all(info["nodes"] == 0) and np.all(info["tied_nodes"] == 0) and np.all(info["init"] == 0.25)
    for f in range(g9["folds"]):
        assert np.all(all_rows(g9, results, f) == 0.25)


def test_residual_overflow_is_reported(g9):
    """A learning rate of 3 doubles the residuals every stage; the restatement names the same stage."""
    from edgeml_amd import gbr
    r = g9["ref"][0]
    with pytest.raises(OverflowError) as want:
        B.fit(r["z32"][r["tr"]], r["y"], r["z32"], 3.0, 12, 3)
    with pytest.raises(RuntimeError, match=f"fold 1: {want.value}"):
        gbr.fit_gbr(g9["features"], g9["reward"], g9["split"], gbr.GBROpt(learning_rate=3.0, n_estimators=12))


# ------------------------------------------------------------------------------------- determinism
def test_folds_together_equal_one_at_a_time(g9, fits):
    from edgeml_amd import gbr
    for f in range(g9["folds"]):
        results, info = gbr.fit_gbr(g9["features"], g9["reward"], g9["split"][f:f + 1])
        for key in (*ARRAYS, "init", "q", "nodes", "tied_nodes"):
            np.testing.assert_array_equal(info[key][0], fits[1][key][f], err_msg=f"fold {f} {key}")
        np.testing.assert_array_equal(results[0]["val_est"], fits[0][f]["val_est"])
        np.testing.assert_array_equal(results[0]["train_est"], fits[0][f]["train_est"])


def test_two_runs_are_bit_identical(g9, fits):
    from edgeml_amd import gbr
    results, info = gbr.fit_gbr(g9["features"], g9["reward"], g9["split"])
    same_info(info, fits[1])
    for f in range(g9["folds"]):
        np.testing.assert_array_equal(all_rows(g9, results, f), all_rows(g9, fits[0], f))


# ----------------------------------------------------------------------------------------- predict
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_model_predict_equals_the_fit(g9, fits, batch):
    import torch
    from edgeml_amd import gbr
    results, info = fits
    for f in range(g9["folds"]):
        model = gbr.load(gbr.model_data(info, f)).to("cuda")
        x = np.ascontiguousarray(g9["features"][g9["split"][f]][:batch])
        est = torch.full((batch,), np.nan, dtype=torch.float64, device="cuda")
        model.predict_into(torch.from_numpy(x).cuda(), est)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(est.cpu().numpy(), results[f]["val_est"][:batch])
        z32 = B.standardise32(x, info["mean"][f], info["scale"][f])
        walk = B.predict({"init": info["init"][f], **{k: info[k][f] for k in ARRAYS}}, z32, 0.1, 3)
        np.testing.assert_array_equal(est.cpu().numpy(), walk)
    np.testing.assert_array_equal(model.predict(g9["features"]), all_rows(g9, results, g9["folds"] - 1))


# ------------------------------------------------------------------------------------ CLI end to end
@pytest.fixture(scope="module")
def files(g9, tmp_path_factory):
    td = tmp_path_factory.mktemp("g9")
    fdir = td / "features"
    for i, x in enumerate(g9["features"]):
        (fdir / f"{i:06d}").mkdir(parents=True)
        np.save(fdir / f"{i:06d}" / "stage24_output_features.npy", x)
    np.savez(td / "reward.npz", reward=g9["reward"])
    np.save(td / "split.npy", g9["split"])
    return td


def test_cli_round_trip(g9, fits, files, capsys):
    import torch
    from edgeml_amd import gbr, offload
    save, mdir = files / "est", files / "model"
    gbr.main(gbr.getargs([str(files / "features"), str(files / "reward.npz"), str(files / "split.npy"), str(save),
                          "--model", "GBR", "--model-dir", str(mdir)]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("fold ")]
    assert len(lines) == g9["folds"]
    assert all("Trained Gradient Boosting Regressor model with training MSE: " in ln and ", validation MSE: " in ln
               for ln in lines)
    D = g9["D"]
    for f in range(g9["folds"]):
        with np.load(save / f"estimate{f + 1}.npz", allow_pickle=False) as z:
            assert sorted(z.files) == ["train_est", "train_time", "val_est", "val_time"]
            np.testing.assert_array_equal(z["train_est"], fits[0][f]["train_est"])
            np.testing.assert_array_equal(z["val_est"], fits[0][f]["val_est"])
        with open(mdir / f"wts{f + 1}.pickle", "rb") as fh:
            m = pickle.load(fh)
        assert m["model"] == "GBR" and all(isinstance(m[k], (np.ndarray, float, int, str)) for k in m)
        assert sorted(m) == sorted(["model", "mean", "scale", "init", "learning_rate", "max_depth", "feature",
                                    "threshold", "value", "q"])
        for key in ARRAYS:
            np.testing.assert_array_equal(m[key], fits[1][key][f])
    # the cascade's side: the saved model of fold 1 decides on the device
    est = offload.load_estimator(str(mdir / "wts1.pickle"), D)
    assert est.kind == "gbr"
    with pytest.raises(ValueError, match=f"features, the cascade makes {D + 1}"):
        offload.load_estimator(str(mdir / "wts1.pickle"), D + 1)
    val = fits[0][0]["val_est"]
    threshold = float(np.median(val))
    x = torch.from_numpy(np.ascontiguousarray(g9["features"][g9["split"][0]])).cuda()
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
    import torch
    from edgeml_amd import ops
    L, p = ops.lib(), ops._ptr
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")  # stands for every device buffer: nothing is launched
    P, S = p(d), ops.stream_handle()
    off = (ctypes.c_int64 * 3)(0, 4, 9)
    empty = (ctypes.c_int64 * 3)(0, 4, 4)
    q = (ctypes.c_int32 * 2)(55, 55)
    low = (ctypes.c_int32 * 2)(55, 25)

    def refused(rc, what):
        assert rc == -1, what
        assert what in L.edgedet_last_error().decode(), L.edgedet_last_error().decode()

    def fit(N=9, D=3, off=off, folds=2, q_host=q, T=5, depth=3, first=P, status=P, wb=1 << 20):
        return L.edgedet_gbr_fit(first, N, D, P, P, P, P, P, off, P, folds, P, q_host, P, 0.1, T, depth, P, wb, P, P, P, P,
                                 P, P, status, S)

    for kw in ({"D": 0}, {"D": 256}, {"N": 0}):
        refused(fit(**kw), "gbr_fit: 1 <= features <= 255")
    for kw in ({"off": empty}, {"off": None}, {"folds": 0}):
        refused(fit(**kw), "gbr_fit: every fold needs")
    for kw in ({"depth": 0}, {"depth": 5}, {"T": 0}):
        refused(fit(**kw), "gbr_fit: 1 <= max_depth <= 4")
    for kw in ({"first": None}, {"status": None}, {"q_host": None}):
        refused(fit(**kw), "gbr_fit: null pointer")
    refused(fit(q_host=low), "gbr_fit: 26 <= q")
    refused(fit(wb=64), "gbr_fit: workspace smaller")

    def split(n=9, D=3, nn=2, q=40, first=P, last=P, wb=1 << 20):
        return L.edgedet_gbr_best_split(first, P, n, D, P, P, nn, q, P, wb, P, P, P, P, P, P, last, S)

    for kw in ({"D": 0}, {"D": 256}, {"n": 0}):
        refused(split(**kw), "gbr_best_split: 1 <= features <= 255")
    for nn in (0, 3, 16):
        refused(split(nn=nn), "gbr_best_split: 1, 2, 4 or 8 nodes")
    refused(split(q=25), "gbr_best_split: 26 <= q")
    for kw in ({"first": None}, {"last": None}):
        refused(split(**kw), "gbr_best_split: null pointer")
    refused(split(wb=64), "gbr_best_split: workspace smaller")

    def predict(B=2, D=3, T=5, depth=3, first=P, est=P):
        return L.edgedet_gbr_model_predict(first, B, D, P, P, P, P, P, 0.0, 0.1, T, depth, est, S)

    for kw in ({"D": 0}, {"D": 256}, {"B": 0}):
        refused(predict(**kw), "gbr_model_predict: 1 <= features <= 255")
    for kw in ({"depth": 0}, {"depth": 5}, {"T": 0}):
        refused(predict(**kw), "gbr_model_predict: 1 <= max_depth <= 4")
    for kw in ({"first": None}, {"est": None}):
        refused(predict(**kw), "gbr_model_predict: null pointer")
    for kw in ({"D": 0}, {"D": 256}, {"N": 0}, {"folds": 0}):
        a = {"N": 9, "D": 3, "folds": 2, **kw}
        refused(L.edgedet_gbr_prepare(P, a["N"], a["D"], P, P, a["folds"], P, S), "gbr_prepare: 1 <= features <= 255")
    refused(L.edgedet_gbr_prepare(None, 9, 3, P, P, 2, P, S), "gbr_prepare: null pointer")
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0  # nothing ran
