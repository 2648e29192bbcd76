"""Host side of the baseline policies in the cascade (edgeml_amd.offload --baseline af|dcsb): the parser's
accepted and refused combinations, the loader's acceptances and refusals each way round, the unchanged refusal
without `baseline`, the two exports, the CLI refusing before it touches the image directory, and the numpy
restatement of the DCSB rule (tests/cascade_rules_ref.py) against the reference's recorded estimates and the
hand-derived decisions of the crafted batches.  No device needed."""
import os
import pickle

import numpy as np
import pytest

from tests import cascade_rules_ref as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
D = 205


@pytest.fixture(scope="module")
def g6():
    with np.load(os.path.join(HERE, "golden", "g6_baselines.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _dump(path, obj):
    with open(path, "wb") as f:
        pickle.dump(obj, f)
    return str(path)


def _af(width=D, seed=0):
    rng = np.random.default_rng(seed)
    return {"coef": rng.normal(0, 1, width), "intercept": 0.375, "classes": [0, 1], "positive_weight": 3.0}


def _lr(width=D):
    rng = np.random.default_rng(1)
    return {"model": "LR", "mean": rng.normal(0, 1, width), "scale": rng.uniform(0.5, 2, width),
            "coef": rng.normal(0, 1, width), "intercept": 0.5}


DCSB = (0.35546875, 5, np.float64(0.4))  # the tuple baseline.fit_dcsb_folds returns and baseline.main pickles


# ------------------------------------------------------------------------------------------ parser
def test_parser_accepts_baseline_without_a_threshold():
    from edgeml_amd import offload
    for b in ("af", "dcsb"):
        o = offload.getargs(["imgs", "out", "--estimator", "M/3.0/wts1.pickle", "--baseline", b])
        assert (o.baseline, o.estimator, o.threshold, o.ratio, o.estimates) == (b, "M/3.0/wts1.pickle", None, None, None)
        o = offload.getargs(["imgs", "out", "--estimator", "w", "--baseline", b, "--weak-batch", "4", "--strong-batch",
                             "2", "--weak-dir", "wk", "--k", "3", "--dataset", "voc", "--decode", "host", "--fold", "2"])
        assert (o.weak_batch, o.strong_batch, o.weak_dir, o.k, o.dataset, o.decode) == (4, 2, "wk", 3, "voc", "host")
    assert offload.getargs(["imgs", "out", "--estimator", "w", "--threshold", "1"]).baseline is None


@pytest.mark.parametrize("baseline", ["af", "dcsb"])
@pytest.mark.parametrize("extra", [["--ratio", "0.3"], ["--estimates", "e"], ["--ratio", "0.3", "--estimates", "e"],
                                   ["--threshold", "0"], ["--threshold", "0.5"], ["--stage", "3"], ["--resize", "8"],
                                   ["--stage", "3", "--resize", "8"], ["--pools", "1", "1"], ["--pools"], ["--fused"]])
def test_parser_refuses_what_a_classifier_does_not_have(baseline, extra):
    from edgeml_amd import offload
    with pytest.raises(SystemExit, match="a classifier has no ratio"):
        offload.getargs(["imgs", "out", "--estimator", "w", "--baseline", baseline] + extra)


def test_parser_rules_without_baseline_stay():
    from edgeml_amd import offload
    for bad in (["imgs", "out", "--estimator", "w"],
                ["imgs", "out", "--estimator", "w", "--ratio", "0.3"],
                ["imgs", "out", "--estimator", "w", "--threshold", "1", "--estimates", "e"],
                ["imgs", "out", "--estimator", "w", "--baseline", "svm"],
                ["imgs", "out", "--baseline", "af"]):
        with pytest.raises(SystemExit):
            offload.getargs(bad)


# ------------------------------------------------------------------------------------------ loader
def test_loader_accepts_the_af_file(tmp_path):
    from edgeml_amd import baseline, offload
    m = _af()
    e = offload.load_estimator(_dump(tmp_path / "wts1.pickle", m), D, baseline="af")
    assert e.kind == "af" and e.width == D and e.kind in offload.CLASSIFIER_KINDS
    Dp = baseline.pad_features(np.zeros((1, D)))[0].shape[1]
    assert e.v.dtype == np.float64 and e.v.shape == (Dp,) == (208,)
    assert np.array_equal(e.v[:D], m["coef"]) and e.v[D] == 0.375 and not e.v[D + 1:].any()
    # what fit_af_folds returns also carries n_iter and grad_norm, and classes may be an array
    m2 = dict(_af(145), n_iter=7, grad_norm=1e-9, classes=np.array([0, 1]))
    e = offload.load_estimator(_dump(tmp_path / "wts2.pickle", m2), 145, baseline="af")
    assert e.width == 145 and e.v.shape == (160,) and e.v[145] == 0.375


def test_loader_accepts_the_dcsb_tuple(tmp_path):
    from edgeml_amd import offload
    e = offload.load_estimator(_dump(tmp_path / "wts1.pickle", DCSB), D, baseline="dcsb")
    assert e.kind == "dcsb" and e.width == 0
    assert (e.conf_thresh, e.num_thresh, e.area_thresh) == (0.35546875, 5, 0.4)
    assert type(e.conf_thresh) is float and type(e.num_thresh) is int and type(e.area_thresh) is float
    e = offload.load_estimator(_dump(tmp_path / "wts2.pickle", (0.5, np.int64(3), 0.25)), 95, baseline="dcsb")
    assert (e.conf_thresh, e.num_thresh, e.area_thresh) == (0.5, 3, 0.25)


def test_loader_refuses_the_wrong_kind_each_way_round(tmp_path):
    from edgeml_amd import offload
    af, dcsb, lr = (_dump(tmp_path / n, m) for n, m in (("af.pickle", _af()), ("dcsb.pickle", DCSB), ("lr.pickle", _lr())))
    with pytest.raises(ValueError, match="--baseline dcsb expects the DCSB file"):
        offload.load_estimator(af, D, baseline="dcsb")
    with pytest.raises(ValueError, match="--baseline af expects the Adaptive Feeding file"):
        offload.load_estimator(dcsb, D, baseline="af")
    with pytest.raises(ValueError, match="--baseline af expects the Adaptive Feeding file"):
        offload.load_estimator(lr, D, baseline="af")  # it has a mean: a regressor on standardised features
    with pytest.raises(ValueError, match="--baseline dcsb expects the DCSB file"):
        offload.load_estimator(lr, D, baseline="dcsb")
    with pytest.raises(ValueError, match="takes 205 features, the cascade makes 95"):
        offload.load_estimator(af, 95, baseline="af")
    for bad in ((0.3, 5), (0.3, 5.0, 0.4), (0.3, True, 0.4), ("0.3", 5, 0.4), (1, 5, 0.4), [0.3, 5, 0.4]):
        with pytest.raises(ValueError, match="--baseline dcsb expects"):
            offload.load_estimator(_dump(tmp_path / "bad.pickle", bad), D, baseline="dcsb")
    for bad in (dict(_af(), classes=[1, 0]), dict(_af(), classes=[0, 1, 2]), {"coef": np.zeros(D), "classes": [0, 1]}):
        with pytest.raises(ValueError, match="--baseline af expects"):
            offload.load_estimator(_dump(tmp_path / "bad.pickle", bad), D, baseline="af")
    with pytest.raises(ValueError, match="exceed the decision kernel's 256 columns"):
        offload.load_estimator(_dump(tmp_path / "wide.pickle", _af(256)), 256, baseline="af")
    with pytest.raises(ValueError, match="one of af, dcsb"):
        offload.load_estimator(af, D, baseline="svm")


def test_both_files_are_still_refused_without_baseline(tmp_path):
    from edgeml_amd import offload
    for name, m, hint in (("af.pickle", _af(), "--baseline af"), ("dcsb.pickle", DCSB, "--baseline dcsb")):
        with pytest.raises(ValueError, match="not a wts<fold>.pickle of edgeml_amd.estimator") as e:
            offload.load_estimator(_dump(tmp_path / name, m), D, support=True)
        assert hint in str(e.value)
    with pytest.raises(ValueError, match=r"not a wts<fold>.pickle of edgeml_amd.estimator --model-dir$"):
        offload.load_estimator(_dump(tmp_path / "other.pickle", {"something": 1}), D)
    e = offload.load_estimator(_dump(tmp_path / "lr.pickle", _lr()), D)  # and a regressor loads as before
    assert e.kind == "linear" and e.width == D


def test_classifier_takes_threshold_zero_only(tmp_path):
    from edgeml_amd import offload
    for e in (offload.load_estimator(_dump(tmp_path / "a.pickle", _af()), D, baseline="af"),
              offload.load_estimator(_dump(tmp_path / "d.pickle", DCSB), D, baseline="dcsb")):
        with pytest.raises(ValueError, match="classifier.*threshold is 0.0"):
            offload.run(str(tmp_path / "none"), e, 0.5)
        with pytest.raises(ValueError, match="classifier.*threshold is 0.0"):
            e.decide(None, 0.5, None, None)


# ------------------------------------------------------------------------------------------ ABI and CLI
def test_abi_declares_the_two_exports():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        header = f.read()
    lib = ops.lib()
    for name, nargs in (("edgedet_offload_dcsb", 13), ("edgedet_offload_svm", 8)):
        assert name in ops.EXPORTS and f"int {name}(" in header and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert header.index("offloading cascade (csrc/offload.hip)") < header.index("int edgedet_offload_dcsb(") < \
        header.index("int edgedet_offload_svm(") < header.index("int edgedet_offload_pack(")


def test_cli_refuses_before_it_touches_the_image_directory(tmp_path):
    from edgeml_amd import offload
    af, dcsb, lr = (_dump(tmp_path / n, m) for n, m in (("af.pickle", _af()), ("dcsb.pickle", DCSB), ("lr.pickle", _lr())))
    none, out = str(tmp_path / "none"), str(tmp_path / "out")
    for wts, b, msg in ((af, "dcsb", "expects the DCSB file"), (dcsb, "af", "expects the Adaptive Feeding file"),
                        (lr, "af", "expects the Adaptive Feeding file")):
        with pytest.raises(SystemExit, match=msg):
            offload.main(offload.getargs([none, out, "--estimator", wts, "--baseline", b]))
    with pytest.raises(SystemExit, match="the cascade makes 95"):
        offload.main(offload.getargs([none, out, "--estimator", af, "--baseline", "af", "--k", "3"]))
    with pytest.raises(SystemExit, match="not a wts<fold>.pickle.*--baseline af"):
        offload.main(offload.getargs([none, out, "--estimator", af, "--threshold", "0"]))
    assert not os.path.exists(out)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("K", [29, 40])
def test_restatement_reproduces_the_reference_estimates(g6, K):
    rows, nrow = C.pack_rows(g6["det_rows"], g6["det_off"], K)
    assert nrow.max() == 29 and nrow.min() == 0
    split = g6["split"]
    for f in range(3):
        model = (float(g6["dcsb/conf_thresh"][f]), int(g6["dcsb/num_thresh"][f]), g6["dcsb/area_thresh"][f])
        est = C.dcsb_decide(rows, nrow, model)[3]
        assert np.array_equal(est[~split[f]], g6[f"dcsb/train_est{f}"])
        assert np.array_equal(est[split[f]], g6[f"dcsb/val_est{f}"])
        assert 0 < est.sum() < len(est)


@pytest.mark.parametrize("K", C.KS)
def test_restatement_gives_the_hand_derived_decisions(K):
    from edgeml_amd import baseline
    seen = set()
    for name, rows, nrow, model, want in C.crafted(K):
        en, dn, ea, est = C.dcsb_decide(rows, nrow, model)
        for b, w in enumerate(want):
            assert w is None or est[b] == w, (name, b)
        en2, dn2, ea2, est2 = C.dcsb_decide(C.with_garbage(rows, nrow), nrow, model)
        assert np.array_equal(en, en2) and np.array_equal(dn, dn2) and ea.tobytes() == ea2.tobytes()
        if name == "thresholds":
            assert model[2] == baseline.area_grid()[20] and ea[4] == model[2] and ea[5] < model[2]
            assert (en[0], dn[0], en[2], en[3]) == (2, 0, model[1], model[1] + 1) and en[1] == dn[1] == 2
        if name == "high_conf":
            assert (en[0], dn[0], ea[0]) == (0, 2, 0.0) and (en[4], dn[4]) == (0, 4)
        if name == "lengths":
            assert list(nrow[:6]) == [0, K, 63, 64, 65, K + 9] and (en[6], dn[6]) == (1, 0) and abs(ea[6] - 0.01) < 1e-12
        seen.add(name)
    assert seen == {"lengths", "thresholds", "high_conf"}
