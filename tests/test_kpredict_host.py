"""Host side of prediction from saved SVR / KNR models (edgeml_amd.kpredict, csrc/kpredict.hip): the five new
exports, what a KNR wts<k>.pickle holds, the loaders and their refusals, and the launchers' own refusals (each
returns before anything is launched, so none needs a device).  No device needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("edgedet_kmodel_prepare", "edgedet_kmodel_workspace_size", "edgedet_svr_model_predict",
               "edgedet_knn_model_predict", "edgedet_offload_flag")


def test_header_declares_and_library_exports_the_new_names():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        txt = f.read()
    declared = set(re.findall(r"\b(edgedet_[a-z_0-9]+)\s*\(", txt))
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in ops.EXPORTS and hasattr(lib, name), name
    assert "int edgedet_offload_flag(" in txt and "int64_t edgedet_kmodel_workspace_size(" in txt


def test_workspace_sizes():
    from edgeml_amd import ops
    ws = ops.lib().edgedet_kmodel_workspace_size
    # SVR: one partial per (row, tile of sixteen support vectors); never empty
    assert ws(1350, 205, 32, 0) == 32 * 85 * 8 and ws(16, 34, 1, 0) == 8 and ws(17, 34, 3, 0) == 3 * 2 * 8
    assert ws(0, 34, 64, 0) == 8
    # KNR: the distances [B][n] and room for the selected positions, rounded up to 8 bytes
    assert ws(4000, 205, 3, 1) == 3 * 4000 * 8 + 3 * 4000 * 4
    assert ws(5, 34, 1, 1) == 40 + 24
    for bad in ((10, 0, 1, 0), (10, 256, 1, 0), (10, 34, 0, 0), (-1, 34, 1, 0), (0, 34, 1, 1), (10, 34, 1, 2),
                (10, 34, 65535 * 16 + 1, 0)):
        assert ws(*bad) < 0, bad


def _knr_info(rng, N=11, D=6, kn=3):
    split = np.zeros((2, N), bool)
    split[0, ::3], split[1, 1::3] = True, True
    info = {"mean": rng.normal(0, 1, (2, D)), "scale": rng.uniform(0.5, 2, (2, D)), "n_neighbors": kn,
            "train_rows": [np.nonzero(~m)[0].astype(np.int32) for m in split]}
    return split, info


def test_knr_model_data_holds_the_training_rows_and_targets():
    from edgeml_amd import regress
    rng = np.random.default_rng(5)
    split, info = _knr_info(rng)
    feats, y = rng.normal(0, 1, (11, 2, 3)), rng.normal(0, 1, (2, 11))  # features flatten; per-fold targets
    for f in range(2):
        m = regress.model_data("KNR", info, f, feats, y)
        assert sorted(m) == ["mean", "model", "n_neighbors", "scale", "target", "train"]
        assert m["train"].dtype == m["target"].dtype == np.float64
        np.testing.assert_array_equal(m["train"], feats.reshape(11, 6)[~split[f]])
        np.testing.assert_array_equal(m["target"], y[f][~split[f]])
        np.testing.assert_array_equal(m["mean"], info["mean"][f])
        assert m["n_neighbors"] == 3 and m["model"] == "KNR"
        pickle.loads(pickle.dumps(m))  # plain numpy data
    one = regress.model_data("KNR", info, 1, feats, y[0])  # one target vector for every fold
    np.testing.assert_array_equal(one["target"], y[0][~split[1]])
    # without the rows: the file of before
    assert sorted(regress.model_data("KNR", info, 0)) == ["mean", "model", "n_neighbors", "scale"]


def _svr_file(path, D, n=4, **over):
    rng = np.random.default_rng(D + n)
    m = {"model": "SVR", "mean": rng.normal(0, 1, D), "scale": rng.uniform(0.5, 2, D), "intercept": 0.25,
         "gamma": 0.125, "support": rng.normal(0, 1, (n, D)), "beta": rng.uniform(-0.05, 0.05, n),
         "violation": 1e-10, "iterations": 11}
    m.update(over)
    with open(path, "wb") as f:
        pickle.dump(m, f)
    return m


def _knr_file(path, D, n=9, kn=3, rows=True, **over):
    rng = np.random.default_rng(D * n)
    m = {"model": "KNR", "mean": rng.normal(0, 1, D), "scale": rng.uniform(0.5, 2, D), "n_neighbors": kn}
    if rows:
        m.update(train=rng.normal(0, 1, (n, D)), target=rng.normal(0, 1, n))
    m.update(over)
    with open(path, "wb") as f:
        pickle.dump(m, f)
    return m


def test_load_estimator_svr_needs_support_true(tmp_path):
    from edgeml_amd import offload
    D = 9
    m = _svr_file(tmp_path / "svr.pickle", D)
    with pytest.raises(ValueError, match="does not predict from them yet"):
        offload.load_estimator(str(tmp_path / "svr.pickle"), D)
    e = offload.load_estimator(str(tmp_path / "svr.pickle"), D, support=True)
    assert e.kind == "svr" and e.width == D
    k = e.model
    assert (k.kind, k.n, k.width, k.gamma, k.intercept) == ("svr", 4, D, 0.125, 0.25)
    for key, a in (("mean", k.mean), ("scale", k.scale), ("support", k.rows), ("beta", k.weight)):
        assert a.dtype == np.float64 and a.flags.c_contiguous and np.array_equal(a, m[key])
    with pytest.raises(ValueError, match="takes 9 features, the cascade makes 10"):
        offload.load_estimator(str(tmp_path / "svr.pickle"), D + 1, support=True)
    # no support vector at all is a model: every estimate is the intercept
    _svr_file(tmp_path / "empty.pickle", D, support=np.zeros((0, D)), beta=np.zeros(0))
    assert offload.load_estimator(str(tmp_path / "empty.pickle"), D, support=True).model.n == 0


def test_load_estimator_knr_with_and_without_rows(tmp_path):
    from edgeml_amd import offload
    D = 7
    m = _knr_file(tmp_path / "knr.pickle", D)
    for support in (False, True):
        e = offload.load_estimator(str(tmp_path / "knr.pickle"), D, support)
        assert e.kind == "knr" and e.width == D and e.model.n_neighbors == 3 and e.model.n == 9
        assert np.array_equal(e.model.rows, m["train"]) and np.array_equal(e.model.weight, m["target"])
    with pytest.raises(ValueError, match="takes 7 features, the cascade makes 205"):
        offload.load_estimator(str(tmp_path / "knr.pickle"), 205)
    _knr_file(tmp_path / "old.pickle", D, rows=False)
    for support in (False, True):
        with pytest.raises(ValueError, match="KNR file holds no training rows"):
            offload.load_estimator(str(tmp_path / "old.pickle"), D, support)
    with pytest.raises(SystemExit, match="KNR"):  # the CLI, before it looks at the image directory
        offload.main(offload.getargs([str(tmp_path / "none"), str(tmp_path / "out"), "--estimator",
                                      str(tmp_path / "old.pickle"), "--threshold", "0"]))
    assert not os.path.exists(tmp_path / "out")


def test_length_and_neighbour_refusals(tmp_path):
    from edgeml_amd import kpredict, offload
    D = 5
    _svr_file(tmp_path / "a.pickle", D, beta=np.zeros(3))  # four support rows
    with pytest.raises(ValueError, match="'beta' has 3 entries, expected 4"):
        offload.load_estimator(str(tmp_path / "a.pickle"), D, support=True)
    _svr_file(tmp_path / "b.pickle", D, support=np.zeros((4, D + 1)))
    with pytest.raises(ValueError, match="'support' has shape"):
        kpredict.load(str(tmp_path / "b.pickle"))
    _svr_file(tmp_path / "c.pickle", D, beta=np.array([0.01, np.nan, 0.0, 0.0]))
    with pytest.raises(ValueError, match="'beta' is not finite"):
        kpredict.load(str(tmp_path / "c.pickle"))
    _svr_file(tmp_path / "d.pickle", D, gamma=float("inf"))
    with pytest.raises(ValueError, match="'gamma' is not finite"):
        kpredict.load(str(tmp_path / "d.pickle"))
    _knr_file(tmp_path / "e.pickle", D, target=np.zeros(8))  # nine training rows
    with pytest.raises(ValueError, match="'target' has 8 entries, expected 9"):
        offload.load_estimator(str(tmp_path / "e.pickle"), D)
    _knr_file(tmp_path / "f.pickle", D, kn=10)
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 10, "
                                         "n_samples_fit = 9, n_samples = 9"):
        offload.load_estimator(str(tmp_path / "f.pickle"), D)
    _knr_file(tmp_path / "g.pickle", D, kn=0)
    with pytest.raises(ValueError, match="Expected n_neighbors > 0"):
        kpredict.load(str(tmp_path / "g.pickle"))
    _knr_file(tmp_path / "h.pickle", D, scale=np.zeros(D))
    with pytest.raises(ValueError, match="zero in 'scale'"):
        kpredict.load(str(tmp_path / "h.pickle"))
    with pytest.raises(ValueError, match="neither SVR nor KNR"):
        kpredict.load({"model": "LR", "mean": np.zeros(D), "scale": np.ones(D), "coef": np.zeros(D), "intercept": 0.0})
    with pytest.raises(ValueError, match="holds no training rows"):
        kpredict.load({"model": "KNR", "mean": np.zeros(D), "scale": np.ones(D), "n_neighbors": 2})
    with pytest.raises(ValueError, match="not a wts<fold>.pickle"):
        kpredict.load({"something": 1})
    k = kpredict.load(_knr_file(tmp_path / "i.pickle", D))  # the dict itself
    assert k.kind == "knr" and k.n == 9


def test_launchers_refuse_on_the_host():
    """Null pointers, a short workspace, k > n, bad sizes: an error code and a message, nothing launched
    (the pointers below are never dereferenced: 8 stands for 'not null')."""
    from edgeml_amd import ops
    L = ops.lib()
    p, nul = ctypes.c_void_p(8), ctypes.c_void_p(0)

    def refused(rc, text):
        return rc < 0 and text in L.edgedet_last_error().decode()

    svr = lambda **o: L.edgedet_svr_model_predict(*[{**dict(  # noqa: E731
        feat=p, B=4, D=34, mean=p, scale=p, z=p, norm=p, beta=p, n=20, gamma=0.1, icpt=0.0, ws=p, wb=4 * 2 * 8, est=p,
        st=nul), **o}[k] for k in ("feat", "B", "D", "mean", "scale", "z", "norm", "beta", "n", "gamma", "icpt", "ws",
                                   "wb", "est", "st")])
    knn = lambda **o: L.edgedet_knn_model_predict(*[{**dict(  # noqa: E731
        feat=p, B=4, D=34, mean=p, scale=p, z=p, norm=p, y=p, n=20, k=3, ws=p, wb=4 * 20 * 12, est=p, nbr=nul,
        st=nul), **o}[k] for k in ("feat", "B", "D", "mean", "scale", "z", "norm", "y", "n", "k", "ws", "wb", "est",
                                   "nbr", "st")])
    for key in ("feat", "mean", "scale", "z", "norm", "beta", "ws", "est"):
        assert refused(svr(**{key: nul}), "null pointer"), key
    for key in ("feat", "mean", "scale", "z", "norm", "y", "ws", "est"):
        assert refused(knn(**{key: nul}), "null pointer"), key
    assert refused(svr(wb=4 * 2 * 8 - 1), "workspace smaller") and refused(knn(wb=4 * 20 * 12 - 1), "workspace smaller")
    assert refused(knn(k=21), "n_neighbors") and refused(knn(k=0), "n_neighbors")
    assert refused(knn(n=0, k=1), "training rows")
    for bad in (dict(D=0), dict(D=256), dict(B=0), dict(n=-1)):
        assert refused(svr(**bad), "features") and refused(knn(**bad), "features"), bad
    assert refused(L.edgedet_kmodel_prepare(nul, 5, 34, p, p, p, p, nul), "null pointer")
    assert refused(L.edgedet_kmodel_prepare(p, 5, 34, p, p, p, nul, nul), "null pointer")
    assert refused(L.edgedet_kmodel_prepare(p, 5, 256, p, p, p, p, nul), "features")
    assert L.edgedet_kmodel_prepare(nul, 0, 34, p, p, nul, nul, nul) == 0  # no rows: nothing to do, nothing launched
    assert refused(L.edgedet_offload_flag(nul, 4, 0.5, p, nul), "null pointer")
    assert refused(L.edgedet_offload_flag(p, 4, 0.5, nul, nul), "null pointer")
    assert refused(L.edgedet_offload_flag(p, 0, 0.5, p, nul), "bad sizes")
