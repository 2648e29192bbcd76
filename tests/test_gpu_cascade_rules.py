"""The cascade run by the two comparison baselines (edgeml_amd.offload --baseline af|dcsb), end to end on
tests/test_gpu_offload.py's set-up: 12 synthetic JPEGs (8 of 480 x 640, 4 of 427 x 640), weak batch 4, strong
batch 2, seeded synthetic weights.  The file route is computed once: the weak rows of run_batches(raw=True) +
fmt.format_batch, then the numpy restatement of the DCSB rule (tests/cascade_rules_ref.py), and
features.output_features + edgedet_svm_decision for Adaptive Feeding.  Nobody has measured the confidences of the
synthetic SSDLite weights, so the two models are chosen from the data: the first candidate that offloads at least
one and keeps at least one image of each size (no candidate: the test fails).  Per rule:

1. `offloaded` and `estimate` equal the file route bit for bit, `threshold` is 0.0;
2. the non-offloaded files are `edgeml_amd.detect --model ssd`'s bytes, the offloaded ones
   `edgeml_amd.detect --model faster_rcnn --batch 2`'s on the offloaded subset;
3. the strong batches are size_batches of the selected images, and a second run is identical.
"""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from tests import cascade_rules_ref as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(480, 640)] * 8 + [(427, 640)] * 4
NC, K = 80, 25
D = NC + 5 * K


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _splits(sel):
    """Offloads at least one and keeps at least one image of each size (sel [..., 12] bool)."""
    a, b = sel[..., :8], sel[..., 8:]
    return a.any(-1) & ~a.all(-1) & b.any(-1) & ~b.all(-1)


def _svm_decision(feat, v):
    from edgeml_amd import baseline, ops
    xt, _ = baseline.pad_features(feat)
    g_x, g_v = _t(xt), _t(v.reshape(1, -1))
    out = torch.zeros((1, len(xt)), dtype=torch.float64, device=DEV)
    ops.check(ops.lib().edgedet_svm_decision(ops._ptr(g_x), len(xt), xt.shape[1], ops._ptr(g_v), 1, ops._ptr(out),
                                             ops.stream_handle()))
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


def _choose_dcsb(rows, nrow):
    """The first (conf_thresh, num_thresh, area_thresh) that splits both sizes: conf_thresh from the midpoints
    between the observed confidences (ascending), num_thresh 1..10, area_thresh from baseline.area_grid()."""
    from edgeml_amd import baseline
    feature = C.image_features(rows, nrow)
    conf = np.unique(np.concatenate([f[0] for f in feature]))
    nums, grid = np.arange(1, 11), baseline.area_grid()
    dn, _ = C.filter_box(feature, 0.5)
    for mid in 0.5 * (conf[:-1] + conf[1:]):
        en, ea = C.filter_box(feature, mid)
        sel = (en != dn) & ((en > nums[:, None, None]) | (ea < grid[None, :, None]))  # [num][area][image]
        ok = np.argwhere(_splits(sel))
        if len(ok):
            return float(mid), int(nums[ok[0][0]]), np.float64(grid[ok[0][1]])
    return None


def _choose_af(feat):
    """The first seeded hand-written SVM that splits both sizes with every decision value away from zero:
    weights on the class counts and on the top box's confidence, the bias halfway between two decision values."""
    for seed in range(64):
        rng = np.random.default_rng(seed)
        coef = np.zeros(D)
        coef[:NC] = rng.uniform(-1, 1, NC)
        coef[NC + 4] = 2.0  # row 0's confidence: the columns after the class counts are xc, yc, w, h, conf
        s = np.sort(feat @ coef)
        b = -0.5 * (s[5] + s[6])
        v = np.concatenate([coef, [b], np.zeros((D + 1 + 15) // 16 * 16 - D - 1)])
        dec = _svm_decision(feat, v)
        if _splits(dec > 0) and np.abs(dec).min() > 1e-6:
            return {"coef": coef, "intercept": float(b), "classes": [0, 1], "positive_weight": 3.0}, dec
    return None, None


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    """The images, the file route, the two chosen models and the weak detect CLI's files."""
    from PIL import Image
    from edgeml_amd import detect, distributed, features, fmt, synthetic
    root = tmp_path_factory.mktemp("cascade_rules")
    img_dir = root / "imgs"
    img_dir.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(synthetic.make_scene(7000 + i, h, w).transpose(1, 2, 0)).save(img_dir / f"{i:012d}.jpg")
    names = sorted(os.listdir(img_dir))
    weak = detect.load_weak_models("ssd", "", 91).to(DEV)
    data = detect.ObjectDetectionDataset(str(img_dir))
    sizes = detect.image_sizes(data)
    assert sizes == SIZES
    chunks = distributed.size_batches(sizes, 4)
    tagged = (((nm, hw), buf) for nm, hw, buf in detect._decoded_batches(data, chunks, sizes))
    rows = {}
    for (nm, (h, w)), counts, boxes, scores, labels in weak.run_batches(tagged, raw=True):
        rows.update(zip(nm, fmt.format_batch(boxes, scores, labels, counts, h, w, "coco")))
    per_image = [rows[n] for n in names]
    feat = features.output_features(per_image, NC, K, DEV)
    assert feat.shape == (12, D)
    Kmax = max(len(r) for r in per_image) + 3
    padded, nrow = np.zeros((12, Kmax, 6)), np.array([len(r) for r in per_image], np.int32)
    for b, r in enumerate(per_image):
        padded[b, :len(r)] = r
    dcsb = _choose_dcsb(padded, nrow)
    assert dcsb is not None, "no DCSB candidate offloads and keeps an image of each size"
    dcsb_est = C.dcsb_decide(padded, nrow, dcsb)[3].astype(np.float64)
    af, af_est = _choose_af(feat)
    assert af is not None, "no hand-written SVM offloads and keeps an image of each size with min |dec| > 1e-6"
    assert _splits(dcsb_est > 0) and _splits(af_est > 0)
    paths = {"dcsb": str(root / "dcsb1.pickle"), "af": str(root / "af1.pickle")}
    for b, m in (("dcsb", dcsb), ("af", af)):
        with open(paths[b], "wb") as f:
            pickle.dump(m, f)
    weak_ref = str(root / "weak_ref")
    detect.main(detect.getargs([str(img_dir), weak_ref, "--model", "ssd", "--batch", "4"]))
    return {"root": root, "img_dir": str(img_dir), "names": names, "rows": rows, "sizes": sizes, "wts": paths,
            "est": {"dcsb": dcsb_est, "af": af_est}, "weak_ref": weak_ref, "weak": weak, "feat": feat, "af": af}


@pytest.fixture(scope="module", params=["dcsb", "af"])
def cascade(request, route):
    """One CLI run of the cascade under the rule, a second one, and the strong detect CLI run on its subset."""
    from edgeml_amd import detect, offload
    rule, root = request.param, route["root"]
    args = ["--estimator", route["wts"][rule], "--baseline", rule, "--weak-batch", "4", "--strong-batch", "2"]
    out, again = str(root / f"{rule}_out"), str(root / f"{rule}_again")
    res = offload.main(offload.getargs([route["img_dir"], out] + args))
    res2 = offload.main(offload.getargs([route["img_dir"], again] + args))
    sel = route["est"][rule] > 0.0
    sub, strong_ref = root / f"{rule}_offloaded", str(root / f"{rule}_strong_ref")
    sub.mkdir()
    for n, s in zip(route["names"], sel):
        if s:
            shutil.copy(os.path.join(route["img_dir"], n), sub / n)
    detect.main(detect.getargs([str(sub), strong_ref, "--model", "faster_rcnn", "--batch", "2"]))
    return {"rule": rule, "res": res, "res2": res2, "out": out, "again": again, "strong_ref": strong_ref, "sel": sel,
            "est": route["est"][rule]}


def test_decisions_equal_the_file_route(route, cascade):
    res = cascade["res"]
    assert res["names"] == route["names"]
    assert res["estimate"].dtype == np.float64 and res["estimate"].tobytes() == cascade["est"].tobytes()
    assert res["offloaded"].dtype == bool and np.array_equal(res["offloaded"], cascade["sel"])
    assert res["threshold"] == 0.0 and res["ratio_realized"] == cascade["sel"].mean()
    if cascade["rule"] == "dcsb":
        assert set(np.unique(res["estimate"])) == {0.0, 1.0}
    for n in route["names"]:
        assert res["weak_rows"][n].tobytes() == route["rows"][n].tobytes()


def test_files_are_the_detect_cli_s(route, cascade):
    files = [n[:-4] + ".npy" for n in route["names"]]
    assert sorted(os.listdir(cascade["out"])) == files + ["offload.npz"]
    assert sorted(os.listdir(cascade["strong_ref"])) == [f for f, s in zip(files, cascade["sel"]) if s]
    for f, s in zip(files, cascade["sel"]):
        ref = os.path.join(cascade["strong_ref"] if s else route["weak_ref"], f)
        assert _read(os.path.join(cascade["out"], f)) == _read(ref), (f, s)


def test_strong_batches_are_size_batches_of_the_selected(route, cascade):
    from edgeml_amd.distributed import size_batches
    sel = [i for i in range(12) if cascade["sel"][i]]
    want = [[route["names"][sel[j]] for j in b] for b in size_batches([route["sizes"][i] for i in sel], 2)]
    assert cascade["res"]["strong_batches"] == want


def test_one_weak_model_serves_the_rules_in_turn(route):
    """The slot buffers of a weak model's plans outlive a run: dcsb (which makes no features), then af, then dcsb
    again on the same model object.  Both models here offload nothing, so no strong model is loaded."""
    from edgeml_amd import offload
    coef, b = route["af"]["coef"], route["af"]["intercept"] - 1e3
    v = np.concatenate([coef, [b], np.zeros((D + 1 + 15) // 16 * 16 - D - 1)])
    want = _svm_decision(route["feat"], v)
    assert np.all(want < 0)
    af = offload.Estimator("af", D, v=v)
    dcsb = offload.Estimator("dcsb", 0, conf_thresh=0.5, num_thresh=1, area_thresh=0.9)  # est_num == det_num always
    for e in (dcsb, af, dcsb, af):
        res = offload.run(route["img_dir"], e, 0.0, K, weak=route["weak"], weak_batch=4, strong_batch=2)
        assert not res["offloaded"].any() and res["strong_batches"] == []
        assert res["estimate"].tobytes() == (want if e is af else np.zeros(12)).tobytes()


def test_offload_npz_and_a_second_run(route, cascade):
    with np.load(os.path.join(cascade["out"], "offload.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["estimate", "names", "offloaded", "ratio_realized", "threshold"]
        assert [str(n) for n in z["names"]] == route["names"]
        assert z["estimate"].dtype == np.float64 and z["estimate"].tobytes() == cascade["est"].tobytes()
        assert z["offloaded"].dtype == bool and np.array_equal(z["offloaded"], cascade["sel"])
        assert float(z["threshold"]) == 0.0 and float(z["ratio_realized"]) == cascade["sel"].sum() / 12
    res, res2 = cascade["res"], cascade["res2"]
    assert res2["estimate"].tobytes() == res["estimate"].tobytes() and np.array_equal(res2["offloaded"], res["offloaded"])
    assert res2["strong_batches"] == res["strong_batches"]
    files = sorted(os.listdir(cascade["out"]))
    assert sorted(os.listdir(cascade["again"])) == files
    for f in files:
        if f.endswith(".npy"):
            assert _read(os.path.join(cascade["again"], f)) == _read(os.path.join(cascade["out"], f)), f
