"""The offloading cascade end to end (edgeml_amd.offload) on 12 synthetic JPEGs: 8 of one COCO-like size
and 4 of another, weak batch 4, strong batch 2, seeded synthetic weights, a hand-written estimator.
Three exact contracts:

1. decisions: `estimate` and `offloaded` equal, bit for bit, the file route (weak rows from
   run_batches(raw=True) + fmt.format_batch, features.output_features, edgedet_reg_predict /
   edgedet_mlp_predict called directly, the strict `>`);
2. weak files: the non-offloaded images' files and everything in --weak-dir are `edgeml_amd.detect
   --model ssd`'s bytes;
3. strong files: the offloaded images' files are `edgeml_amd.detect --model faster_rcnn --batch 2`'s
   bytes on a directory holding only the offloaded images.
"""
import ctypes
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(480, 640)] * 8 + [(427, 640)] * 4
NC, K = 80, 25
D = NC + 5 * K
WANT = (5, 2)  # offloaded images of the first and of the second size


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reg_predict(x, m):
    from edgeml_amd import ops
    g = [_t(np.asarray(a, np.float64)) for a in (x, m["mean"], m["scale"], m["coef"], [m["intercept"]])]
    out = torch.zeros(len(x), dtype=torch.float64, device=DEV)
    ops.check(ops.lib().edgedet_reg_predict(ops._ptr(g[0]), len(x), x.shape[1], ops._ptr(g[1]), ops._ptr(g[2]),
                                            ops._ptr(g[3]), ops._ptr(g[4]), 1, ops._ptr(out), ops.stream_handle()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _mlp_predict(x, dims, state):
    from edgeml_amd import ops
    g_x, g_s = _t(np.asarray(x, np.float32)), _t(state)
    out = torch.zeros(len(x), dtype=torch.float32, device=DEV)
    dims_host = (ctypes.c_int32 * len(dims))(*dims)
    ops.check(ops.lib().edgedet_mlp_predict(ops._ptr(g_x), dims[0], None, len(x), len(dims) - 1, dims_host,
                                            ops._ptr(g_s), ops._ptr(out), ops.stream_handle()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _linear(seed):
    """A hand-written linear estimator: weights on the class counts and on the top box's confidence."""
    rng = np.random.default_rng(seed)
    coef = np.zeros(D)
    coef[:NC] = rng.uniform(-1, 1, NC)
    coef[NC + 4] = 2.0  # row 0's confidence: the columns after the class are xc, yc, w, h, conf
    return {"model": "LR", "mean": np.full(D, 0.25), "scale": np.full(D, 2.0), "coef": coef, "intercept": 0.5}


def _split_threshold(est, want):
    """A threshold halfway between two estimates that offloads want[0] of the first 8 images and want[1]
    of the last 4, or None."""
    s = np.sort(est)[::-1]
    n = sum(want)
    t = 0.5 * (s[n - 1] + s[n])
    sel = est > t
    ok = (int(sel[:8].sum()), int(sel[8:].sum())) == want and np.abs(est - t).min() > 1e-4
    return float(t) if ok else None


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    """The images, the shared models and the file route run with the code the cascade joins."""
    from PIL import Image
    from edgeml_amd import detect, distributed, features, fmt, synthetic
    root = tmp_path_factory.mktemp("offload")
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
    assert [len(c) for c in chunks] == [4, 4, 4]
    tagged = (((nm, hw), buf) for nm, hw, buf in detect._decoded_batches(data, chunks, sizes))
    rows = {}
    for (nm, (h, w)), counts, boxes, scores, labels in weak.run_batches(tagged, raw=True):
        rows.update(zip(nm, fmt.format_batch(boxes, scores, labels, counts, h, w, "coco")))
    feat = features.output_features([rows[n] for n in names], NC, K, DEV)
    assert feat.shape == (12, D) and all(len(rows[n]) > 0 for n in names)
    # the first hand-written estimator under which one threshold splits the images 5 + 2
    model = thr = None
    for seed in range(64):
        m = _linear(seed)
        t = _split_threshold(((feat - m["mean"]) / m["scale"]) @ m["coef"] + m["intercept"], WANT)
        if t is not None:
            model, thr = m, t
            break
    assert model is not None, "no candidate estimator splits the images 5 + 2"
    est = _reg_predict(feat, model)
    sel = est > thr
    # the conditions the tests below rely on
    assert (int(sel[:8].sum()), int(sel[8:].sum())) == WANT
    assert np.abs(est - thr).min() > 1e-6
    wts = root / "wts1.pickle"
    with open(wts, "wb") as f:
        pickle.dump(model, f)
    return {"root": root, "img_dir": str(img_dir), "names": names, "weak": weak, "rows": rows, "feat": feat,
            "est": est, "thr": thr, "sel": sel, "wts": str(wts), "sizes": sizes}


@pytest.fixture(scope="module")
def cascade(route):
    """One CLI run of the cascade and the two detect CLI runs it must reproduce."""
    from edgeml_amd import detect, offload
    root = route["root"]
    out, wk = str(root / "cascade"), str(root / "cascade_weak")
    res = offload.main(offload.getargs([route["img_dir"], out, "--estimator", route["wts"], "--threshold",
                                        repr(route["thr"]), "--weak-batch", "4", "--strong-batch", "2",
                                        "--weak-dir", wk]))
    weak_ref, strong_ref, sub = str(root / "weak_ref"), str(root / "strong_ref"), root / "offloaded"
    detect.main(detect.getargs([route["img_dir"], weak_ref, "--model", "ssd", "--batch", "4"]))
    sub.mkdir()
    for n, s in zip(route["names"], route["sel"]):
        if s:
            shutil.copy(os.path.join(route["img_dir"], n), sub / n)
    detect.main(detect.getargs([str(sub), strong_ref, "--model", "faster_rcnn", "--batch", "2"]))
    return {"res": res, "out": out, "weak_dir": wk, "weak_ref": weak_ref, "strong_ref": strong_ref}


def test_decisions_equal_the_file_route(route, cascade):
    res = cascade["res"]
    assert res["names"] == route["names"]
    assert res["estimate"].dtype == np.float64 and res["estimate"].tobytes() == route["est"].tobytes()
    assert res["offloaded"].dtype == bool and np.array_equal(res["offloaded"], route["sel"])
    # the cascade's weak rows are the file route's
    for n in route["names"]:
        assert res["weak_rows"][n].tobytes() == route["rows"][n].tobytes()


def test_strong_batches_are_size_batches_of_the_selected(route, cascade):
    from edgeml_amd.distributed import size_batches
    sel = [i for i in range(12) if route["sel"][i]]
    want = [[route["names"][sel[j]] for j in b] for b in size_batches([route["sizes"][i] for i in sel], 2)]
    assert [len(b) for b in want] == [2, 2, 1, 2]
    assert cascade["res"]["strong_batches"] == want


def test_weak_files_are_the_detect_cli_s(route, cascade):
    files = [n[:-4] + ".npy" for n in route["names"]]
    assert sorted(os.listdir(cascade["weak_dir"])) == files == sorted(os.listdir(cascade["weak_ref"]))
    assert sorted(os.listdir(cascade["out"])) == files + ["offload.npz"]
    for f, s in zip(files, route["sel"]):
        ref = _read(os.path.join(cascade["weak_ref"], f))
        assert _read(os.path.join(cascade["weak_dir"], f)) == ref, f
        assert (_read(os.path.join(cascade["out"], f)) == ref) == (not s), f


def test_strong_files_are_the_detect_cli_s_on_the_offloaded(route, cascade):
    files = [n[:-4] + ".npy" for n, s in zip(route["names"], route["sel"]) if s]
    assert sorted(os.listdir(cascade["strong_ref"])) == files and len(files) == sum(WANT)
    for f in files:
        got = np.load(os.path.join(cascade["out"], f))
        assert got.dtype == np.float64 and got.shape[1:] == (6,)
        assert _read(os.path.join(cascade["out"], f)) == _read(os.path.join(cascade["strong_ref"], f)), f


def test_offload_npz_fields(route, cascade):
    with np.load(os.path.join(cascade["out"], "offload.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["estimate", "names", "offloaded", "ratio_realized", "threshold"]
        assert [str(n) for n in z["names"]] == route["names"]
        assert z["estimate"].dtype == np.float64 and z["estimate"].tobytes() == route["est"].tobytes()
        assert z["offloaded"].dtype == bool and np.array_equal(z["offloaded"], route["sel"])
        assert float(z["threshold"]) == route["thr"]
        assert float(z["ratio_realized"]) == sum(WANT) / 12


def test_ratio_gives_test_py_35_threshold_and_a_second_run_is_identical(route, cascade):
    """--ratio on an estimate1.npz whose test.py:35 element is an estimate that splits the images the
    same way: the second run's files are the first run's, byte for byte."""
    from edgeml_amd import offload
    root = route["root"]
    est = route["est"]
    # 21 training estimates; at ratio 0.3 test.py:35 takes the 7th largest (index int(20 * 0.3) = 6): put the
    # largest not-offloaded estimate there, so `>` offloads the same 7 images
    t = float(np.sort(est[~route["sel"]])[-1])
    train = np.concatenate([t + 1.0 + np.arange(6), [t], t - 1.0 - np.arange(14)])
    assert train[np.argsort(-train)[int((len(train) - 1) * 0.3)]] == t
    assert np.array_equal(est > t, route["sel"])
    est_dir = root / "estimates"
    est_dir.mkdir()
    np.savez(est_dir / "estimate1.npz", train_est=train, val_est=est, train_time=0.0, val_time=0.0)
    out = str(root / "cascade2")
    res = offload.main(offload.getargs([route["img_dir"], out, "--estimator", route["wts"], "--ratio", "0.3",
                                        "--estimates", str(est_dir), "--weak-batch", "4", "--strong-batch", "2"]))
    assert res["threshold"] == t
    assert res["estimate"].tobytes() == est.tobytes() and np.array_equal(res["offloaded"], route["sel"])
    files = sorted(f for f in os.listdir(cascade["out"]) if f.endswith(".npy"))
    assert sorted(f for f in os.listdir(out) if f.endswith(".npy")) == files
    for f in files:
        assert _read(os.path.join(out, f)) == _read(os.path.join(cascade["out"], f)), f


def test_threshold_above_every_estimate_builds_no_strong_plan(route, monkeypatch):
    from edgeml_amd import detect, models, offload

    def refuse(*a, **k):
        raise AssertionError("a strong plan was built")
    monkeypatch.setattr(models.FasterRCNNFPNv2, "build_plan", refuse)
    loaded = []
    real = detect.load_weak_models
    monkeypatch.setattr(detect, "load_weak_models", lambda name, *a: loaded.append(name) or real(name, *a))
    out = str(route["root"] / "none")
    thr = float(route["est"].max())  # equal is not above: strict
    res = offload.main(offload.getargs([route["img_dir"], out, "--estimator", route["wts"], "--threshold", repr(thr),
                                        "--weak-batch", "4", "--strong-batch", "2"]))
    assert loaded == ["ssd"] and res["strong_batches"] == []
    assert not res["offloaded"].any() and res["ratio_realized"] == 0.0
    assert res["estimate"].tobytes() == route["est"].tobytes()
    for n in route["names"]:
        got = np.load(os.path.join(out, n[:-4] + ".npy"))
        assert got.tobytes() == route["rows"][n].tobytes() and got.shape == route["rows"][n].shape


def test_mlp_estimator_decisions(route):
    """A hand-packed [205, 16, 16, 16, 16, 1] MLP state through the wts<fold>.pth contract."""
    from edgeml_amd import estimator, offload
    from edgeml_amd.distributed import size_batches
    dims = [D, 16, 16, 16, 16, 1]
    spec = estimator.MlpSpec(dims)
    state = spec.init_state(np.random.default_rng(11))
    for l in range(spec.L - 1):  # BatchNorm: shift 0.5, running mean 0, variance 4 (the ReLUs stay alive)
        e, d = spec.off[l], dims[l + 1]
        state[e["be"]:e["be"] + d], state[e["rm"]:e["rm"] + d], state[e["rv"]:e["rv"] + d] = 0.5, 0.0, 4.0
    estimator.save_state(str(route["root"] / "mlp"), spec, state, 0)
    ref = _mlp_predict(route["feat"], dims, state).astype(np.float64)
    s = np.sort(ref)
    assert s[-3] > s[-4]
    thr = float(s[-4])  # an estimate itself: that image stays, the three above it go
    res = offload.run(route["img_dir"], str(route["root"] / "mlp" / "wts1.pth"), thr, K, weak=route["weak"],
                      weak_batch=4, strong_batch=2)
    assert res["estimate"].tobytes() == ref.tobytes()
    assert np.array_equal(res["offloaded"], ref > thr) and res["offloaded"].sum() == 3
    sel = [i for i in range(12) if ref[i] > thr]
    want = [[route["names"][sel[j]] for j in b] for b in size_batches([route["sizes"][i] for i in sel], 2)]
    assert sorted(map(tuple, res["strong_batches"])) == sorted(map(tuple, want))
    for n, off in zip(route["names"], res["offloaded"]):
        assert (res["rows"][n].tobytes() == route["rows"][n].tobytes()) == (not off), n
