"""edgeml_amd.baseline (csrc/baseline.hip) on the device against the reference's baseline.py.

The fixture tests/golden/g6_baselines.npz holds the reference's own results (fit_dcsb, fit_af with
sklearn's LinearSVC; tests/golden/make_golden_baselines.py); nothing here reads the reference or sklearn.

* DCSB is bit-exact: thresholds compared with ==, estimates with array_equal, every fold in one launch,
  plus edge cases against a numpy restatement of fit_dcsb below.
* Adaptive Feeding is the optimum of a 1-strongly convex objective f, so |v - v*| <= |grad f(v)| and
  two approximate solutions' decision values differ by at most (g_a + g_b) |x~|.  Every bound below is
  that inequality with gradient norms recomputed here in float64; no tolerance is fitted to the results.
"""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g6():
    with np.load(os.path.join(HERE, "golden", "g6_baselines.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------ DCSB
def _fixture_dets(g):
    """Per image (conf, area) as baseline.main builds them: xywh -> xyxy (reward.xywh2xyxy), get_area."""
    from edgeml_amd import baseline, reward
    off, rows = g["det_off"], g["det_rows"]
    weak = []
    for i in range(len(off) - 1):
        r = rows[off[i]:off[i + 1]]
        weak.append((r[:, 0].astype(int), reward.xywh2xyxy(r[:, 1:5]), r[:, 5]) if len(r) else ())
    label_num = np.diff(g["label_off"]).astype(int)
    return baseline.dcsb_inputs(weak), label_num


def _filter_box(feature, conf):
    num, area = [], []
    for box in feature:
        m = box[0] > conf
        num.append(int(np.sum(m)))
        a = box[1][m]
        area.append(0 if len(a) == 0 else np.amin(a))
    return np.array(num, dtype=int), np.array(area, dtype=float)


def _estimate(feature, model):
    conf_thresh, num_thresh, area_thresh = model
    en, ea = _filter_box(feature, conf_thresh)
    dn, _ = _filter_box(feature, 0.5)
    cls = en != dn
    cls[cls] = np.logical_or(en[cls] > num_thresh, ea[cls] < area_thresh)
    return cls.astype(int)


def _ref_dcsb(dets, label_num, reward01, val_mask):
    """baseline.py:67-152 restated (the bisection bounded at 64 halvings: None when it does not end)."""
    train = [d for d, v in zip(dets, val_mask) if not v]
    tr_label, tr_reward = label_num[~val_mask], reward01[~val_mask]
    low, high, mid, done, steps = 0, 1, 0, False, 0
    while not done:
        if steps == 64:
            return None
        mid = (low + high) / 2
        num, _ = _filter_box(train, mid)
        diff = np.sum(num) - np.sum(tr_label)
        if diff >= 0:
            low = mid
        else:
            high = mid
        with np.errstate(divide="ignore", invalid="ignore"):
            done = bool(np.float64(abs(diff)) / np.float64(np.sum(tr_label)) < 1e-4)
        steps += 1
    en, ea = _filter_box(train, mid)
    dn, _ = _filter_box(train, 0.5)
    tc = en != dn
    grid = np.arange(0.2, 0.9, 0.01)
    counts = np.zeros((10, len(grid)), int)
    best, model = 0, None
    for n in range(1, 11):
        for ai, a in enumerate(grid):
            c = np.copy(tc)
            c[tc] = np.logical_or(en[tc] > n, ea[tc] < a)
            counts[n - 1, ai] = np.sum(c.astype(int) == tr_reward)
        ab = int(np.argmax(counts[n - 1]))
        if counts[n - 1, ab] > best:
            best, model = counts[n - 1, ab], (mid, n, grid[ab])
    est = _estimate(dets, model)
    return model, est[~val_mask], est[val_mask], counts


def _rand_case(seed, n_img, max_mid=6, n_folds=2):
    """Images with confident (> 0.5), middle (0.3 .. 0.5) and weak (< 0.3) boxes; the label count is the
    number of boxes above 0.3, so the bisection ends where the confidences leave a gap around 0.3."""
    rng = np.random.default_rng(seed)
    dets, lab = [], []
    for i in range(n_img):
        nh, nm, nl = rng.integers(0, 4), rng.integers(0, max_mid + 1), rng.integers(0, 8)
        conf = np.concatenate([rng.uniform(0.5, 0.95, nh), rng.uniform(0.31, 0.5, nm), rng.uniform(0.05, 0.29, nl)])
        if i % 11 == 3:
            conf = np.zeros(0)
        w, h = rng.uniform(0.4, 1.0, len(conf)), rng.uniform(0.4, 1.0, len(conf))
        dets.append((conf, w * h))
        lab.append(int(np.sum(conf > 0.3)))
    lab = np.array(lab, dtype=int)
    en, ea = _filter_box(dets, 0.3)
    dn, _ = _filter_box(dets, 0.5)
    r = np.logical_and(en != dn, np.logical_or(en > 4, ea < 0.3))
    r = np.where(rng.uniform(size=n_img) < 0.1, ~r, r).astype(int)
    if n_folds == 1:
        return dets, lab, r, (rng.uniform(size=n_img) < 0.3)[None]
    fold = rng.permutation(np.arange(n_img) % n_folds)
    return dets, lab, r, np.stack([fold == f for f in range(n_folds)])


def _check_against_restatement(dets, lab, r, split):
    from edgeml_amd import baseline
    res, models = baseline.fit_dcsb_folds(dets, lab, r, split)
    assert len(res) == len(models) == len(split)
    all_counts = []
    for f, m in enumerate(split):
        ref = _ref_dcsb(dets, lab, r, m)
        assert ref is not None
        model, tr, va, counts = ref
        assert models[f][0] == model[0] and models[f][1] == model[1] and models[f][2] == model[2], (f, models[f], model)
        assert res[f]["train_est"].dtype == np.int64 and res[f]["val_est"].dtype == np.int64
        np.testing.assert_array_equal(res[f]["train_est"], tr)
        np.testing.assert_array_equal(res[f]["val_est"], va)
        all_counts.append(counts)
    return models, all_counts


def test_dcsb_equals_the_reference_on_every_fold(g6):
    from edgeml_amd import baseline
    dets, label_num = _fixture_dets(g6)
    y = np.where(g6["reward"] > 0, 1, 0)
    res, models = baseline.fit_dcsb_folds(dets, label_num, y, g6["split"])
    for f in range(len(g6["split"])):
        print("fold", f, models[f], "reference", g6["dcsb/conf_thresh"][f], g6["dcsb/num_thresh"][f],
              g6["dcsb/area_thresh"][f])
        assert models[f][0] == g6["dcsb/conf_thresh"][f]
        assert models[f][1] == g6["dcsb/num_thresh"][f]
        assert models[f][2] == g6["dcsb/area_thresh"][f]
        assert type(models[f][0]) is float and type(models[f][1]) is int and type(models[f][2]) is np.float64
        np.testing.assert_array_equal(res[f]["train_est"], g6[f"dcsb/train_est{f}"])
        np.testing.assert_array_equal(res[f]["val_est"], g6[f"dcsb/val_est{f}"])
        assert res[f]["train_est"].dtype == np.int64


def test_dcsb_single_fold():
    dets, lab, r, split = _rand_case(1, 64, n_folds=1)
    assert split.shape == (1, 64) and 0 < split.sum() < 64
    _check_against_restatement(dets, lab, r, split)


def test_dcsb_validation_fold_without_detections():
    dets, lab, r, split = _rand_case(2, 90)
    empty = np.array([len(d[0]) == 0 for d in dets])
    split = np.stack([empty, ~empty & (np.arange(90) % 2 == 0)])  # fold 0 validates on the empty images only
    assert split[0].sum() > 0 and all(len(dets[i][0]) == 0 for i in np.nonzero(split[0])[0])
    _check_against_restatement(dets, lab, r, split)


def test_dcsb_first_of_tied_cells_wins():
    """At most one box above the threshold per image: est_num > n is false for every n, so the ten
    n_thresh rows of the accuracy table are equal and n_thresh = 1 at the first best area must win."""
    dets, lab, r, split = _rand_case(3, 70, max_mid=1)
    dets = [(c[c < 0.5], a[c < 0.5]) for c, a in dets]  # no confident boxes: the count above 0.3 is 0 or 1
    lab = np.array([int(np.sum(c > 0.3)) for c, _ in dets])
    models, counts = _check_against_restatement(dets, lab, r, split)
    for f in range(len(split)):
        c = counts[f]
        assert np.array_equal(c[0], c[1]) and np.array_equal(c[0], c[9])          # rows tie
        assert np.sum(c == c.max()) >= 10                                          # ten cells share the maximum
        assert models[f][1] == 1 and models[f][2] == np.arange(0.2, 0.9, 0.01)[int(np.argmax(c[0]))]


def test_dcsb_130_images_three_folds():
    dets, lab, r, split = _rand_case(4, 130, n_folds=3)
    _check_against_restatement(dets, lab, r, split)


def test_dcsb_unreachable_label_count_raises_and_the_device_survives(g6):
    from edgeml_amd import baseline
    dets, lab, r, split = _rand_case(5, 40)
    lab = lab + 50  # more labels than detections: the reference's bisection never ends
    assert _ref_dcsb(dets, lab, r, split[0]) is None
    with pytest.raises(RuntimeError, match="DCSB confidence search did not converge"):
        baseline.fit_dcsb_folds(dets, lab, r, split)
    with pytest.raises(RuntimeError, match="DCSB confidence search did not converge"):
        baseline.fit_dcsb_folds(dets, np.zeros_like(lab), r, split)  # sum(label) == 0: 0 / 0 never passes
    test_dcsb_equals_the_reference_on_every_fold(g6)


# ------------------------------------------------------------------------------ Adaptive Feeding
def _objective(v, xt, y, pw):
    """f(v) and grad f(v) of the LinearSVC(dual=False) objective, float64."""
    s, c = np.where(y == 1, 1.0, -1.0), np.where(y == 1, pw, 1.0)
    h = np.maximum(0.0, 1.0 - s * (xt @ v))
    return 0.5 * v @ v + np.sum(c * h * h), v - xt.T @ (2.0 * c * s * h)


def _newton(xt, y, pw):
    """The same optimum by a float64 numpy Newton method (the oracle of the shape cases)."""
    s, c = np.where(y == 1, 1.0, -1.0), np.where(y == 1, pw, 1.0)
    v = np.zeros(xt.shape[1])
    for _ in range(100):
        f0, g = _objective(v, xt, y, pw)
        if np.linalg.norm(g) <= 1e-11:
            break
        act = 1.0 - s * (xt @ v) > 0
        H = np.eye(len(v)) + 2.0 * (xt[act].T * c[act]) @ xt[act]
        p = np.linalg.solve(H, -g)
        t = 1.0
        while _objective(v + t * p, xt, y, pw)[0] > f0 + 1e-4 * t * (g @ p) + 1e-14 * abs(f0) and t > 1e-9:
            t *= 0.5
        v = v + t * p
    return v


def _vec(model):
    return np.concatenate([model["coef"], [model["intercept"]]])


def test_af_reaches_the_reference_optimum(g6):
    from edgeml_amd import baseline
    x, split = g6["features"], g6["split"]
    y = np.where(g6["reward"] > 0, 1, 0)
    pw = float(g6["positive_weight"])
    res, models = baseline.fit_af_folds(x, y, split, pw)
    xt = np.concatenate([x, np.ones((len(x), 1))], 1)
    norms = np.linalg.norm(xt, axis=1)
    for f, m in enumerate(split):
        v = _vec(models[f])
        assert v.shape == (146,) and models[f]["classes"] == [0, 1] and models[f]["positive_weight"] == pw
        f_eng, g = _objective(v, xt[~m], y[~m], pw)
        g_eng = float(np.linalg.norm(g))
        v_def = np.concatenate([g6["af/coef_default"][f], [g6["af/intercept_default"][f]]])
        f_def = _objective(v_def, xt[~m], y[~m], pw)[0]
        g_ref = float(g6["af/gnorm_ref"][f])
        d_eng, d_ref = xt @ v, g6["af/decision_ref"][f]
        bound = (g_eng + g_ref) * norms
        err = np.abs(d_eng - d_ref)
        print(f"fold {f}: {models[f]['n_iter']} Newton steps, device |grad| {models[f]['grad_norm']:.3e}, host "
              f"|grad| {g_eng:.3e}, |grad f(v_ref)| {g_ref:.3e}, f {f_eng:.12g} (default tol {f_def:.12g}), max |d - "
              f"d_ref| {err.max():.3e}, min bound {bound.min():.3e}, min |d_ref| {np.abs(d_ref).min():.3e}")
        assert g_eng <= 1e-6
        assert models[f]["grad_norm"] <= 1e-8 and models[f]["n_iter"] <= 100
        assert f_eng <= f_def * (1 + 1e-9)
        assert np.all(err <= bound)
        outside = np.abs(d_ref) > bound
        assert np.all(outside)  # the fixture has no sample inside the band
        pred = np.concatenate([res[f]["train_est"], res[f]["val_est"]])
        order = np.concatenate([np.nonzero(~m)[0], np.nonzero(m)[0]])
        np.testing.assert_array_equal(pred[outside[order]], (d_ref[order] > 0).astype(np.int64)[outside[order]])
        np.testing.assert_array_equal(res[f]["train_est"], g6[f"af/train_est{f}"])
        np.testing.assert_array_equal(res[f]["val_est"], g6[f"af/val_est{f}"])
        assert res[f]["train_est"].dtype == np.int64 and res[f]["val_est"].dtype == np.int64


def _af_shape_case():
    """100 rows x 145 features (D + 1 = 146, padded to 160): fold 0 trains on 77 rows, fold 1 on the 60
    rows in which feature 30 is zero."""
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 1, (100, 145))
    x[:, :20] = rng.poisson(0.7, (100, 20))
    x[40:, 30] = 0.0
    wtrue = rng.normal(0, 1, 145)
    y = ((x - x.mean(0)) @ wtrue + 0.5 * rng.normal(0, 1, 100) > 0).astype(int)
    split = np.zeros((2, 100), bool)
    split[0, 77:] = True
    split[1, :40] = True
    return x, y, split


@pytest.mark.parametrize("pw", [1.0, 3.0])
def test_af_shapes_against_a_numpy_newton_solver(pw):
    from edgeml_amd import baseline
    x, y, split = _af_shape_case()
    assert (~split[0]).sum() == 77 and np.all(x[~split[1], 30] == 0) and np.any(x[~split[0], 30] != 0)
    res, models = baseline.fit_af_folds(x, y, split, pw)
    xt = np.concatenate([x, np.ones((100, 1))], 1)
    norms = np.linalg.norm(xt, axis=1)
    for f, m in enumerate(split):
        v, v_np = _vec(models[f]), _newton(xt[~m], y[~m], pw)
        g_eng = float(np.linalg.norm(_objective(v, xt[~m], y[~m], pw)[1]))
        g_np = float(np.linalg.norm(_objective(v_np, xt[~m], y[~m], pw)[1]))
        err = np.abs(xt @ v - xt @ v_np)
        print(f"pw {pw} fold {f}: {models[f]['n_iter']} steps, |grad| device {g_eng:.3e} numpy {g_np:.3e}, max |d - "
              f"d_np| {err.max():.3e}, bound {((g_eng + g_np) * norms).min():.3e}")
        assert g_eng <= 1e-6 and g_np <= 1e-6
        assert np.all(err <= (g_eng + g_np) * norms)
        e = np.concatenate([res[f]["train_est"], res[f]["val_est"]])
        order = np.concatenate([np.nonzero(~m)[0], np.nonzero(m)[0]])
        np.testing.assert_array_equal(e, (xt[order] @ v > 0).astype(np.int64))
    assert models[1]["coef"][30] == 0.0 and models[0]["coef"][30] != 0.0


def test_af_single_class_fold_raises_value_error():
    from edgeml_amd import baseline
    x, y, split = _af_shape_case()
    y = y.copy()
    y[40:] = 1  # fold 1's training rows hold one class only
    with pytest.raises(ValueError, match="2 classes"):
        baseline.fit_af_folds(x, y, split)


def test_hessian_matrix_instruction_is_exact_on_integers():
    """The fp64 matrix-instruction Hessian H = I + X^T diag(w) X on small integers, where every product and
    sum is exact in float64: any wrong lane or register map shows as a wrong element."""
    import torch
    from edgeml_amd import ops
    rng = np.random.default_rng(5)
    for n, dp, use_idx in ((77, 160, True), (5, 16, False), (130, 48, True)):
        x = rng.integers(-4, 5, (n + 9, dp)).astype(np.float64)
        idx = rng.permutation(n + 9)[:n].astype(np.int32) if use_idx else None
        w = rng.integers(0, 4, n).astype(np.float64)
        rows = x[idx] if use_idx else x[:n]
        want = np.eye(dp) + (rows.T * w) @ rows
        g_x, g_w = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
        g_idx = torch.from_numpy(idx).cuda() if use_idx else None
        H = torch.full((dp, dp), np.nan, dtype=torch.float64, device="cuda")
        ops.check(ops.lib().edgedet_svm_hessian(ops._ptr(g_x), dp, ops._ptr(g_idx), n, ops._ptr(g_w), ops._ptr(H),
                                                ops.stream_handle()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(H.cpu().numpy(), want)


# ------------------------------------------------------------------------------------ end to end
def test_cli_end_to_end_feeds_evaluate(g6, tmp_path):
    from edgeml_amd import baseline, evaluate, features
    from edgeml_amd.reward import set_data
    g = g6
    n = len(g["reward"])
    weak, strong, labels, feat = (str(tmp_path / d) for d in ("weak", "strong", "labels", "features"))
    for d in (weak, strong, labels):
        os.makedirs(d)
    for i in range(n):
        name = f"{i:06d}"
        if g["det_file"][i]:
            np.save(os.path.join(weak, name + ".npy"), g["det_rows"][g["det_off"][i]:g["det_off"][i + 1]])
        lab = g["label_rows"][g["label_off"][i]:g["label_off"][i + 1]]
        np.save(os.path.join(labels, name + ".npy"), lab)
        if len(lab):  # the strong detector: the labels themselves, confidence 0.9
            np.save(os.path.join(strong, name + ".npy"), np.concatenate([lab, np.full((len(lab), 1), 0.9)], 1))
    np.savez(str(tmp_path / "reward.npz"), reward=g["reward"])
    np.save(str(tmp_path / "split.npy"), g["split"])
    features.main(features.getargs([weak, feat, labels, "--k", str(int(g["k"])), "--dataset", "voc"]))
    common = [str(tmp_path / "reward.npz"), str(tmp_path / "split.npy")]
    est_af, est_dcsb = str(tmp_path / "est_af"), str(tmp_path / "est_dcsb")
    baseline.main(baseline.getargs([feat] + common + [est_af, "--model_dir", str(tmp_path / "m_af")]))
    baseline.main(baseline.getargs([weak] + common + [est_dcsb, "--baseline", "dcsb", "--label_dir", labels,
                                                      "--model_dir", str(tmp_path / "m_dcsb")]))
    k = len(g["split"])
    assert sorted(os.listdir(est_af)) == ["3.0"] and sorted(os.listdir(str(tmp_path / "m_af"))) == ["3.0"]
    assert sorted(os.listdir(os.path.join(est_af, "3.0"))) == [f"estimate{f + 1}.npz" for f in range(k)]
    assert sorted(os.listdir(est_dcsb)) == [f"estimate{f + 1}.npz" for f in range(k)]
    assert sorted(os.listdir(str(tmp_path / "m_dcsb"))) == [f"wts{f + 1}.pickle" for f in range(k)]
    for f in range(k):
        for d, tag in ((os.path.join(est_af, "3.0"), "af"), (est_dcsb, "dcsb")):
            with np.load(os.path.join(d, f"estimate{f + 1}.npz")) as z:
                assert set(z.files) == {"train_est", "val_est", "train_time", "val_time"}
                assert z["train_est"].dtype == np.int64 and z["val_est"].dtype == np.int64
                np.testing.assert_array_equal(z["train_est"], g[f"{tag}/train_est{f}"])
                np.testing.assert_array_equal(z["val_est"], g[f"{tag}/val_est{f}"])
        with open(str(tmp_path / "m_dcsb" / f"wts{f + 1}.pickle"), "rb") as fh:
            m = pickle.load(fh)
        assert m == (g["dcsb/conf_thresh"][f], g["dcsb/num_thresh"][f], g["dcsb/area_thresh"][f])
        assert type(m[0]) is float and type(m[1]) is int and type(m[2]) is np.float64
        with open(str(tmp_path / "m_af" / "3.0" / f"wts{f + 1}.pickle"), "rb") as fh:
            m = pickle.load(fh)
        assert set(m) == {"coef", "intercept", "classes", "positive_weight"} and m["coef"].shape == (145,)
    weak_data, strong_data, labs = set_data(weak, strong, labels)
    res = evaluate.test_map(weak_data, strong_data, labs, [os.path.join(est_af, "3.0"), est_dcsb], g["split"])
    print("realized mAP", res)
    assert res.shape == (2, 11) and np.all(np.isfinite(res))
