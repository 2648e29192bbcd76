"""The offloading cascade driven by a saved SVR and by a saved KNR model (edgeml_amd.offload kinds "svr" and
"knr", csrc/kpredict.hip): the 12 synthetic JPEGs and the batch sizes of tests/test_gpu_offload.py, one
hand-written model of each kind, one CLI run per kind.  Exact contracts:

1. `estimate` equals, bit for bit, kpredict.KernelModel.predict on features.output_features of the file
   route's weak rows (all 12 rows in one call, where the cascade decides in weak batches of 4);
2. `offloaded` is estimate > threshold;
3. the strong batches are distributed.size_batches of the selected images;
4. every kept image's file is its weak file, byte for byte.
"""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(480, 640)] * 8 + [(427, 640)] * 4
NC, TOPK = 80, 25
D = NC + 5 * TOPK


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    """The images and the file route: weak rows from run_batches(raw=True) + fmt.format_batch, then the
    stage-24 features."""
    from PIL import Image
    from edgeml_amd import detect, distributed, features, fmt, synthetic
    root = tmp_path_factory.mktemp("offload_kernel_models")
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
    feat = np.asarray(features.output_features([rows[n] for n in names], NC, TOPK, DEV), np.float64)
    assert feat.shape == (12, D)
    return {"root": root, "img_dir": str(img_dir), "names": names, "feat": feat, "sizes": sizes}


def _model(kind, feat):
    """Stored rows around the images' own feature rows: 20 support vectors, or 40 training rows with k = 3."""
    rng = np.random.default_rng(31 if kind == "svr" else 32)
    n = 20 if kind == "svr" else 40
    rows = feat[np.arange(n) % 12] + rng.normal(0, 0.05, (n, D))
    base = {"mean": np.full(D, 0.25), "scale": np.full(D, 2.0)}
    if kind == "svr":
        return {"model": "SVR", **base, "gamma": 1.0 / D, "support": rows, "beta": rng.uniform(-0.05, 0.05, n),
                "intercept": 0.5}
    return {"model": "KNR", **base, "n_neighbors": 3, "train": rows, "target": rng.uniform(0, 1, n)}


def _threshold(est):
    """Halfway between two neighbouring estimates, at least 1e-6 from both, offloading about three images."""
    s = np.sort(np.unique(est))[::-1]
    for above in (3, 2, 4, 1, 5, 6, 7, 8, 9, 10):
        if above < len(s) and s[above - 1] - s[above] > 4e-6:
            return float(0.5 * (s[above - 1] + s[above]))
    raise AssertionError(f"no two estimates are 4e-6 apart: {s}")


@pytest.mark.parametrize("kind", ["svr", "knr"])
def test_cascade_decides_by_the_saved_model(route, kind):
    from edgeml_amd import kpredict, offload
    from edgeml_amd.distributed import size_batches
    m = _model(kind, route["feat"])
    root = route["root"]
    wts = root / f"wts_{kind}.pickle"
    with open(wts, "wb") as f:
        pickle.dump(m, f)
    est = kpredict.load(str(wts)).to(DEV).predict(route["feat"])  # the file route
    assert est.dtype == np.float64 and est.shape == (12,)
    thr = _threshold(est)
    sel = est > thr
    assert np.abs(est - thr).min() >= 1e-6 and 1 <= sel.sum() < 12
    out, wk = str(root / f"cascade_{kind}"), str(root / f"weak_{kind}")
    res = offload.main(offload.getargs([route["img_dir"], out, "--estimator", str(wts), "--threshold", repr(thr),
                                        "--weak-batch", "4", "--strong-batch", "2", "--weak-dir", wk]))
    assert res["names"] == route["names"]
    assert res["estimate"].dtype == np.float64 and res["estimate"].tobytes() == est.tobytes()
    assert res["offloaded"].dtype == bool and np.array_equal(res["offloaded"], sel)
    idx = [i for i in range(12) if sel[i]]
    want = [[route["names"][idx[j]] for j in b] for b in size_batches([route["sizes"][i] for i in idx], 2)]
    assert res["strong_batches"] == want
    with np.load(os.path.join(out, "offload.npz"), allow_pickle=False) as z:
        assert z["estimate"].tobytes() == est.tobytes() and np.array_equal(z["offloaded"], sel)
    files = [n[:-4] + ".npy" for n in route["names"]]
    assert sorted(os.listdir(wk)) == files and sorted(os.listdir(out)) == files + ["offload.npz"]
    for f, s in zip(files, sel):
        if not s:
            assert _read(os.path.join(out, f)) == _read(os.path.join(wk, f)), f
