"""Host-side checks of the conv-stack estimator (edgeml_amd.convnet): state layout, the (h, w, c) <-> (c, h, w)
permutation, the mask hash, the reference restatement against the golden run of the reference, and the refusals.
No device needed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import convnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spec(resize=True):
    from edgeml_amd import convnet
    return convnet.ConvSpec(12, [20, 8], [3, 5], [True, False], [16, 16], (6, 6) if resize else None, resize)


@pytest.mark.parametrize("resize", [True, False])
def test_convspec_pack_unpack_round_trip(resize):
    spec = _spec(resize)
    state = np.random.default_rng(0).normal(size=spec.ns).astype(np.float32)
    named = spec.unpack(state)
    assert named["conv_stacks.1.0.weight"].shape == (8, 20, 5, 5)
    assert named["linear_stacks.0.0.weight"].shape == (16, 8 * 3 * 3 if resize else 8)
    assert ("conv_stacks.0.1.running_var" in named) == resize and "linear_stacks.2.1.weight" not in named
    assert sum(v.size for v in named.values()) == spec.ns
    assert np.array_equal(spec.pack(named), state)
    init = spec.init_state(np.random.default_rng(1))
    n0 = spec.unpack(init)
    assert np.abs(n0["conv_stacks.1.0.weight"]).max() <= np.sqrt(6 / (20 * 25)) and np.abs(n0["conv_stacks.1.0.bias"]).max() <= 1 / np.sqrt(500)
    if resize:
        assert (n0["conv_stacks.0.1.weight"] == 1).all() and (n0["conv_stacks.0.1.running_var"] == 1).all()
        assert (n0["linear_stacks.1.1.bias"] == 0).all() and (n0["linear_stacks.1.1.running_mean"] == 0).all()


def _numpy_nhwc_eval(spec, state, x_nhwc):
    """Eval-mode forward straight from the DEVICE layout of the state: NHWC maps, weights [Cout][k][k][Cin], the
    first linear layer's columns in (h, w, c) order."""
    a = x_nhwc.astype(np.float64)
    for lay in spec.layers:
        co, ci, k = lay["cout"], lay["cin"], lay["k"]
        w = state[lay["w"]:lay["w"] + co * k * k * ci].astype(np.float64)
        b = state[lay["b"]:lay["b"] + co].astype(np.float64)
        if lay["kind"] == "conv":
            B, H, W, _ = a.shape
            p = k // 2
            ap = np.pad(a, ((0, 0), (p, p), (p, p), (0, 0)))
            w = w.reshape(co, k, k, ci)
            z = np.zeros((B, H, W, co))
            for kh in range(k):
                for kw in range(k):
                    z += ap[:, kh:kh + H, kw:kw + W, :] @ w[:, kh, kw, :].T
            z += b
        else:
            z = a.reshape(a.shape[0], -1) @ w.reshape(co, ci).T + b
        if lay["last"]:
            return z.ravel()
        if lay["bn"]:
            g, be, rm, rv = (state[lay[q]:lay[q] + co].astype(np.float64) for q in ("g", "be", "rm", "rv"))
            z = (z - rm) / np.sqrt(rv + 1e-5) * g + be
        a = np.maximum(z, 0)
        if lay["pool"]:
            B, H, W, C = a.shape
            a = a[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max((2, 4))


def test_pth_permutation_matches_nhwc_evaluation(tmp_path):
    """A .pth written from a random state, loaded into the ref net, equals a numpy NHWC evaluation of that state."""
    from edgeml_amd import convnet
    spec = _spec()
    rng = np.random.default_rng(5)
    state = spec.init_state(rng)
    for lay in spec.layers:
        if lay["bn"]:
            for q, lo, hi in (("g", 0.5, 1.5), ("be", -0.5, 0.5), ("rm", -0.5, 0.5), ("rv", 0.5, 2.0)):
                state[lay[q]:lay[q] + lay["cout"]] = rng.uniform(lo, hi, lay["cout"])
    convnet.save_state(str(tmp_path), spec, state, 0)
    named = {k: v.numpy() for k, v in torch.load(tmp_path / "wts1.pth", weights_only=True).items()}
    x = rng.normal(size=(4, 12, 6, 6)).astype(np.float32)
    net = R.build(spec, named, torch.float64).eval()
    with torch.no_grad():
        ref = net(torch.from_numpy(x).double()).numpy().ravel()
    got = _numpy_nhwc_eval(spec, state, x.transpose(0, 2, 3, 1))
    assert np.abs(ref).max() > 1e-3 and np.allclose(got, ref, rtol=0, atol=1e-12)
    assert np.array_equal(spec.pack(named), state)


def test_mask_hash_literals():
    """The numpy hash against the same hash on Python integers, and against literal words."""
    assert (R.hash_int(0, 0), R.hash_int(1, 2), R.hash_int(2 ** 63 + 5, 2 ** 40 + 9)) == (0x6db6ca64, 0x30883360, 0x9a6b8c2e)
    seed, fold, step, layer = 1234567, 3, 41, 5
    a = (seed ^ (fold << 48) ^ (layer << 40)) & (2 ** 64 - 1)
    idx = np.array([0, 1, 7, 4095, 2 ** 20 + 3, 2 ** 32 - 1])
    words = [R.hash_int(a, (step << 32) | int(i)) for i in idx]
    for p in (0.1, 0.5, 0.9):
        exp = [np.float32(w >> 8) * np.float32(1 / 16777216) >= np.float32(p) for w in words]
        assert list(R.mask_keep(seed, fold, step, layer, idx, p)) == exp
    big = R.mask_keep(seed, fold, step, layer, np.arange(200000), 0.1)
    assert abs(big.mean() - 0.9) < 0.005
    assert not np.array_equal(big, R.mask_keep(seed, fold, step + 1, layer, np.arange(200000), 0.1))
    assert not np.array_equal(big, R.mask_keep(seed, fold + 1, step, layer, np.arange(200000), 0.1))
    from edgeml_amd import convnet
    assert convnet.layer_key(seed, fold, layer) == a


def test_ref32_reproduces_the_golden_estimates():
    """tests/convnet_ref.py in float32 against the reference's own run (tests/golden/g_convnet.npz, dropout off): the
    pooling, then best and last estimates of every fold within the yardstick."""
    g, opts, spec, pooled = R.golden_setup(0.0)
    for f, mask in enumerate(g["split"]):
        r64 = R.fit(spec, opts, pooled, g["reward"], mask, g["init"][f], torch.float64, fold=f)
        r32 = R.fit(spec, opts, pooled, g["reward"], mask, g["init"][f], torch.float32, fold=f)
        for tag in ("best", "last"):
            for e in ("train_est", "val_est"):
                ratio, E = R.yardstick(g[tag][f][e], r64[tag][e], r32[tag][e])
                assert E > 0 and ratio <= 1.0, (f, tag, e, ratio, E)
                assert g[tag][f][e].shape == r32[tag][e].shape
            for k, v in g[tag + "_state"][f].items():
                if not k.endswith(".0.bias"):
                    ratio, E = R.yardstick(v, r64[tag + "_state"][k], r32[tag + "_state"][k])
                    assert ratio <= 1.0, (f, tag, k, ratio, E)


def _args(*extra):
    from edgeml_amd import convnet
    return convnet.getargs(["d", "r", "s", "o", *extra])


def test_cli_refusals():
    from edgeml_amd import convnet
    with pytest.raises(SystemExit, match="edgeml_amd.estimator"):
        convnet.main(_args("--channels", "8"))  # --stage 24 is the default
    with pytest.raises(SystemExit, match="--channels"):
        convnet.main(_args("--stage", "17"))
    with pytest.raises(SystemExit, match="odd kernel sizes"):
        convnet.main(_args("--stage", "17", "--channels", "8", "8", "--kernels", "3", "4"))
    with pytest.raises(SystemExit, match="Only fully convolutional NN can take feature maps"):
        convnet.main(_args("--stage", "17", "--channels", "8", "--model", "LR"))
    kernels, pools = convnet.check_args(_args("--stage", "3", "--channels", "8", "8", "8"))
    assert kernels == [3, 3, 3] and pools == [True, True, False]
    with pytest.raises(ValueError, match="odd kernel sizes"):
        convnet.ConvSpec(12, [8], [2], [False], [16], (6, 6), True)
    with pytest.raises(ValueError, match="multiples of 4"):
        convnet.ConvSpec(10, [8], [3], [False], [16], (6, 6), True)


def test_last_batch_of_one_row_is_refused(monkeypatch):
    """A last training batch of one row under BatchNorm (torch raises there): refused before any launch."""
    from edgeml_amd import convnet, ops
    monkeypatch.setattr(ops, "need_device", lambda module: None)
    monkeypatch.setattr(convnet, "to_device_maps", lambda f, device="cuda": f)
    opts = convnet.ConvOpt(channels=[8], kernels=[3], pools=[False], hidden=[16], batch_size=4)
    split = np.zeros((1, 7), bool)
    split[0, :2] = True  # 5 training rows in batches of 4
    with pytest.raises(ValueError, match="last training batch has one row"):
        convnet.fit_folds(np.zeros((7, 4, 3, 3), np.float32), np.zeros(7), split, opts)


def test_stage_refusals_name_the_convnet_cli():
    from edgeml_amd import estimator, gbr, rfr, svr
    with pytest.raises(SystemExit, match=r"stages 0-23.*python -m edgeml_amd\.convnet"):
        estimator.check_model(estimator.getargs(["d", "r", "s", "o", "--stage", "17"]))
    for mod in (svr, gbr, rfr):
        with pytest.raises(SystemExit, match=r"--stage 24.*python -m edgeml_amd\.convnet"):
            mod.main(mod.getargs(["d", "r", "s", "o", "--stage", "17"]))


def test_offload_refuses_a_conv_stack_file(tmp_path):
    from edgeml_amd import convnet, offload
    spec = _spec()
    convnet.save_state(str(tmp_path), spec, spec.init_state(np.random.default_rng(0)), 0)
    with pytest.raises(ValueError, match="conv_stacks"):
        offload.load_estimator(str(tmp_path / "wts1.pth"), 72)


def test_exports_declared_and_bound():
    from edgeml_amd import ops
    names = [n for n in ops.EXPORTS if n.startswith("edgedet_cnn_")]
    assert len(names) == 14
    header = open(os.path.join(ROOT, "include", "edgedet.h")).read()
    src = open(os.path.join(ROOT, "edgeml-object-detection_amd", "csrc", "convnet.hip")).read()
    opsrc = open(os.path.join(ROOT, "edgeml-object-detection_amd", "ops.py")).read()
    for n in names:
        assert re.search(rf"\bint {n}\(", header), n
        assert re.search(rf'extern "C" int {n}\(', src), n
        assert f"L.{n}.argtypes" in opsrc, n
