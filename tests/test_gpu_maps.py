"""The producer of SSDLite's hidden-layer maps (python -m edgeml_amd.maps) and the cascade hook's pooling, on 6
synthetic JPEGs of two sizes, weak batch 4, seeded synthetic weights:

1. the dumped [C, H, W] files are the plan's buffers (read through plan.buffer after a plain run of the same
   batch), transposed, bit for bit;
2. they are byte-identical between --decode gpu and --decode host, and --save-dir writes the detect CLI's files;
3. convnet.pool_maps(convnet.load_maps(..., names=ssd), S), the training route, equals the pooled tensor the
   cascade's hook makes from the tapped buffers, bit for bit.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(480, 640)] * 4 + [(427, 640)] * 2
STAGES = (7, 18)
S = 8


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    from PIL import Image
    from edgeml_amd import detect, maps, synthetic
    root = tmp_path_factory.mktemp("maps")
    img_dir = root / "imgs"
    img_dir.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(synthetic.make_scene(7100 + i, h, w).transpose(1, 2, 0)).save(img_dir / f"{i:012d}.jpg")
    names = sorted(os.listdir(img_dir))
    out = {}
    for decode in ("gpu", "host"):
        fd = str(root / f"features_{decode}")
        maps.main(maps.getargs([str(img_dir), fd, "--stages", *map(str, STAGES), "--batch", "4", "--decode", decode,
                                "--save-dir", str(root / f"weak_{decode}")]))
        out[decode] = fd
    detect.main(detect.getargs([str(img_dir), str(root / "weak_ref"), "--model", "ssd", "--batch", "4"]))
    return {"root": root, "img_dir": str(img_dir), "names": names, "features": out}


def test_files_are_the_plan_buffers_transposed(dumped):
    from edgeml_amd import detect, distributed, tapnet
    weak = detect.load_weak_models("ssd", "", 91).to(DEV)
    data = detect.ObjectDetectionDataset(dumped["img_dir"])
    sizes = detect.image_sizes(data)
    chunks = distributed.size_batches(sizes, 4)
    assert [len(c) for c in chunks] == [4, 2]
    tokens = tapnet.ssd_names()
    assert [tokens[s] for s in STAGES] == ["IR", "Extra"]
    seen = 0
    for nm, (h, w), buf in detect._decoded_batches(data, chunks, sizes, device_decode=False):
        plan = weak.build_plan(len(nm), h, w, True).finalize()
        plan.input.tensor().copy_(buf.to(DEV))
        plan.run()
        torch.cuda.synchronize()
        for s in STAGES:
            for t in tapnet.stage_table(91, weak.reduced_tail, len(nm), h, w, True, s):
                x = plan.buffer(t.buffer).tensor().cpu().numpy()
                assert x.shape == (t.images, t.H, t.W, t.C)
                for j in range(t.images):
                    name = nm[t.image0 + j]
                    f = np.load(os.path.join(dumped["features"]["gpu"], name[:-4], f"stage{s}_{tokens[s]}_features.npy"))
                    assert f.dtype == np.float32 and f.shape == (t.C, t.H, t.W)
                    assert f.tobytes() == np.ascontiguousarray(x[j].transpose(2, 0, 1)).tobytes(), (name, s)
                    assert np.abs(f).max() > 0
                    seen += 1
    assert seen == len(SIZES) * len(STAGES)


def test_decode_routes_agree_and_the_weak_files_are_the_detect_cli_s(dumped):
    root = dumped["root"]
    dirs = [n[:-4] for n in dumped["names"]]
    for decode in ("gpu", "host"):
        assert sorted(os.listdir(dumped["features"][decode])) == dirs
    for d in dirs:
        files = sorted(os.listdir(os.path.join(dumped["features"]["gpu"], d)))
        assert files == ["stage18_Extra_features.npy", "stage7_IR_features.npy"]
        for f in files:
            assert _read(os.path.join(dumped["features"]["gpu"], d, f)) == \
                _read(os.path.join(dumped["features"]["host"], d, f)), (d, f)
        for decode in ("gpu", "host"):
            assert _read(str(root / f"weak_{decode}" / (d + ".npy"))) == _read(str(root / "weak_ref" / (d + ".npy"))), d


def test_training_route_pooling_equals_the_cascade_hook_s(dumped):
    from edgeml_amd import convnet, detect, distributed, offload, tapnet
    pooled = convnet.pool_maps(convnet.load_maps(dumped["features"]["gpu"], 7, tapnet.ssd_names()), S).cpu().numpy()
    assert pooled.shape == (len(SIZES), S, S, 80)
    spec = convnet.ConvSpec(80, [8, 4], [3, 3], [True, True], [16], (S, S), True)
    net = tapnet.TapNet(spec, spec.init_state(np.random.default_rng(0)), fused=True)  # batch-independent bits
    est = offload.Estimator("convnet", 205, net=net, stage=7, resize=S, map_shape=(80, 20, 20))
    chain = offload.Chain(est, 0.0, 80, 25, "coco")

    def hook(plan, sl, stream, tag):
        chain(plan, sl, stream, tag)
        sl["post"]["pooled"] = sl["offload"]["pooled"].clone()

    weak = detect.load_weak_models("ssd", "", 91).to(DEV)
    data = detect.ObjectDetectionDataset(dumped["img_dir"])
    sizes = detect.image_sizes(data)
    tagged = (((nm, hw), buf) for nm, hw, buf in
              detect._decoded_batches(data, distributed.size_batches(sizes, 4), sizes))
    got, ests = {}, {}
    for (nm, hw), counts, boxes, scores, labels, ex in weak.run_batches(tagged, raw=True, post=hook):
        p = ex["pooled"].cpu().numpy()
        for j, n in enumerate(nm):
            got[n], ests[n] = p[j], ex["estimate"][j]
    for i, n in enumerate(dumped["names"]):
        assert got[n].tobytes() == pooled[i].tobytes(), n
    # and the hook's estimates are the file route's through the same inference entry
    ref, _ = tapnet.predict(net, torch.from_numpy(pooled).to(DEV), 0.0)
    assert np.array([ests[n] for n in dumped["names"]]).tobytes() == ref.tobytes()


def test_two_chains_pool_and_decide_as_one_batch():
    """A batch of 16 runs as two chains of 8: the hook pools each chain's buffer into its rows of the batch, and the
    estimates are those of the whole batch's maps through the training route's pooling."""
    from edgeml_amd import convnet, detect, offload, tapnet
    weak = detect.load_weak_models("ssd", "", 91).to(DEV)
    taps = tapnet.stage_table(91, weak.reduced_tail, 16, 64, 96, True, 7)
    assert [(t.image0, t.images) for t in taps] == [(0, 8), (8, 8)]
    spec = convnet.ConvSpec(80, [8, 4], [3, 3], [True, True], [16], (S, S), True)
    net = tapnet.TapNet(spec, spec.init_state(np.random.default_rng(0)), fused=True)  # batch-independent bits
    chain = offload.Chain(offload.Estimator("convnet", 205, net=net, stage=7, resize=S, map_shape=(80, 20, 20)), 0.0, 80,
                          25, "coco")

    def hook(plan, sl, stream, tag):
        chain(plan, sl, stream, tag)
        sl["post"]["pooled"] = sl["offload"]["pooled"].clone()
        sl["post"]["maps"] = torch.cat([plan.buffer(t.buffer).tensor() for t in taps])

    imgs = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (16, 3, 64, 96), dtype=np.uint8))
    (out,) = list(weak.run_batches([("b", imgs)], raw=True, post=hook))
    ex = out[-1]
    maps = ex["maps"].cpu().numpy()
    assert maps.shape == (16, 20, 20, 80)
    pooled = convnet.pool_maps([m.transpose(2, 0, 1) for m in maps], S)
    assert ex["pooled"].cpu().numpy().tobytes() == pooled.cpu().numpy().tobytes()
    assert len({p.tobytes() for p in pooled.cpu().numpy()}) == 16
    ref, _ = tapnet.predict(net, pooled, 0.0)
    assert ex["estimate"].tobytes() == ref.tobytes()
    # a --resize 0 net (no BatchNorm, a global mean) reads the tapped maps themselves through the layered forward,
    # chain by chain: held to the float64 budget of tests/convnet_ref.py against the torch reference on the same maps
    from tests import convnet_ref as R
    from tests import tapnet_cases as T
    spec0 = convnet.ConvSpec(80, [8, 4], [3, 3], [True, False], [16], None, False)
    state0 = spec0.init_state(np.random.default_rng(1))
    net0 = tapnet.TapNet(spec0, state0)
    assert not net0.fits
    chain0 = offload.Chain(offload.Estimator("convnet", 205, net=net0, stage=7, resize=0, map_shape=(80, 20, 20)), 0.0,
                           80, 25, "coco")
    (out,) = list(weak.run_batches([("b", imgs)], raw=True, post=chain0))
    got = out[-1]["estimate"]
    ref64, ref32 = T.ref(spec0, state0, maps, torch.float64), T.ref(spec0, state0, maps, torch.float32)
    ratio, E = R.yardstick(got, ref64, ref32)
    assert 0 < E <= 1e-3 * ref64.std() and ratio <= 1.0, (ratio, E, ref64.std())
    assert np.array_equal(out[-1]["flag"].astype(bool), got > 0.0)
