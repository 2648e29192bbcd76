"""The hidden-layer loop end to end on 12 synthetic JPEGs (8 of one size, 4 of another), seeded synthetic weights:

    python -m edgeml_amd.maps     imgs features --stages 7
    python -m edgeml_amd.convnet  features reward split est --weak ssd --stage 7 --resize 8 --channels 8 4 --epochs 2
    python -m edgeml_amd.offload  imgs out --estimator wts1.pth --stage 7 --resize 8 --threshold T --fused

T is the midpoint of two of the file route's estimates (the dumped maps -> convnet.pool_maps -> the same inference
entry, tapnet.TapNet.infer), which are pairwise distinct.  The cascade's `estimate` equals the file route's bit
for bit and `offloaded` its strict `>`; the files are the detect CLI's bytes, as in tests/test_gpu_offload.py.
"""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(480, 640)] * 8 + [(427, 640)] * 4
STAGE, S = 7, 8
OFFLOAD = 3  # images sent to the strong detector


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    from PIL import Image
    from edgeml_amd import convnet, detect, maps, offload, synthetic, tapnet
    root = tmp_path_factory.mktemp("loop")
    img_dir = root / "imgs"
    img_dir.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(synthetic.make_scene(7000 + i, h, w).transpose(1, 2, 0)).save(img_dir / f"{i:012d}.jpg")
    names = sorted(os.listdir(img_dir))
    feat = str(root / "features")
    maps.main(maps.getargs([str(img_dir), feat, "--stages", str(STAGE), "--batch", "4"]))
    rng = np.random.default_rng(0)
    np.savez(root / "reward.npz", reward=rng.uniform(0, 1, len(names)))
    split = np.zeros((1, len(names)), bool)
    split[0, ::4] = True
    np.save(root / "split.npy", split)
    cwd = os.getcwd()
    os.chdir(root)  # the save and model directories are relative: lib/utils.py parse_path drops a leading separator
    try:
        convnet.main(convnet.getargs([feat, "reward.npz", "split.npy", "est", "--weak", "ssd", "--stage", str(STAGE),
                                      "--resize", str(S), "--channels", "8", "4", "--epochs", "2", "--model-dir", "model",
                                      "--seed", "0"]))
    finally:
        os.chdir(cwd)
    wts = str(root / "model_last" / "wts1.pth")
    # the file route: dumped maps -> pool_maps -> the same inference entry
    est = offload.load_estimator(wts, 205, stage=STAGE, resize=S)
    assert est.net.fits
    pooled = convnet.pool_maps(convnet.load_maps(feat, STAGE, tapnet.ssd_names()), S)
    ref, _ = tapnet.predict(est.net, pooled, 0.0, fused=True)
    # the layered forward in the weak batches of 4 (the conv engine chooses its tile by the batch's pixel count)
    ref_layered = np.concatenate([tapnet.predict(est.net, pooled[b:b + 4].contiguous(), 0.0, fused=False)[0]
                                  for b in range(0, len(names), 4)])
    s = np.sort(ref)[::-1]
    # the precondition: pairwise distinct estimates, the threshold strictly between two of them
    assert np.all(np.diff(s) < 0), s
    thr = float(0.5 * (s[OFFLOAD - 1] + s[OFFLOAD]))
    assert s[OFFLOAD] < thr < s[OFFLOAD - 1]
    sel = ref > thr
    out, wk = str(root / "cascade"), str(root / "cascade_weak")
    res = offload.main(offload.getargs([str(img_dir), out, "--estimator", wts, "--threshold", repr(thr), "--stage",
                                        str(STAGE), "--resize", str(S), "--weak-batch", "4", "--strong-batch", "2",
                                        "--weak-dir", wk, "--fused"]))
    weak_ref, strong_ref, sub = str(root / "weak_ref"), str(root / "strong_ref"), root / "offloaded"
    detect.main(detect.getargs([str(img_dir), weak_ref, "--model", "ssd", "--batch", "4"]))
    sub.mkdir()
    for n, f in zip(names, sel):
        if f:
            shutil.copy(os.path.join(img_dir, n), sub / n)
    detect.main(detect.getargs([str(sub), strong_ref, "--model", "faster_rcnn", "--batch", "2"]))
    return {"root": root, "img_dir": str(img_dir), "names": names, "wts": wts, "ref": ref, "ref_layered": ref_layered,
            "thr": thr, "sel": sel, "res": res, "out": out, "weak_dir": wk, "weak_ref": weak_ref,
            "strong_ref": strong_ref}


def test_decisions_equal_the_file_route(loop):
    res = loop["res"]
    assert res["names"] == loop["names"]
    assert res["estimate"].dtype == np.float64 and res["estimate"].tobytes() == loop["ref"].tobytes()
    assert res["offloaded"].dtype == bool and np.array_equal(res["offloaded"], loop["sel"])
    assert int(res["offloaded"].sum()) == OFFLOAD
    with np.load(os.path.join(loop["out"], "offload.npz"), allow_pickle=False) as z:
        assert z["estimate"].tobytes() == loop["ref"].tobytes() and np.array_equal(z["offloaded"], loop["sel"])
        assert float(z["threshold"]) == loop["thr"]


def test_files_are_the_detect_cli_s(loop):
    files = [n[:-4] + ".npy" for n in loop["names"]]
    assert sorted(os.listdir(loop["weak_dir"])) == files == sorted(os.listdir(loop["weak_ref"]))
    assert sorted(os.listdir(loop["out"])) == files + ["offload.npz"]
    strong = [f for f, s in zip(files, loop["sel"]) if s]
    assert sorted(os.listdir(loop["strong_ref"])) == strong and len(strong) == OFFLOAD
    for f, s in zip(files, loop["sel"]):
        ref = _read(os.path.join(loop["weak_ref"], f))
        assert _read(os.path.join(loop["weak_dir"], f)) == ref, f
        assert _read(os.path.join(loop["out"], f)) == (_read(os.path.join(loop["strong_ref"], f)) if s else ref), f


def test_layered_path_in_the_cascade_equals_its_file_route(loop):
    """The default path, and a threshold no estimate exceeds: the layered eval forward's bits, no strong model."""
    from edgeml_amd import offload
    thr = float(loop["ref_layered"].max())  # equal is not above: strict
    res = offload.main(offload.getargs([loop["img_dir"], str(loop["root"] / "layered"), "--estimator", loop["wts"],
                                        "--threshold", repr(thr), "--stage", str(STAGE), "--resize", str(S),
                                        "--weak-batch", "4"]))
    assert res["estimate"].tobytes() == loop["ref_layered"].tobytes()
    assert not res["offloaded"].any() and res["strong_batches"] == []
