"""The conv-stack ORIE estimator on the device (edgeml_amd.convnet, csrc/convnet.hip) against tests/convnet_ref.py.

The yardstick of every float quantity (tests/convnet_ref.py): the reference in float64 and in float32 from the same
inputs gives E = max |ref32 - ref64|; the device result passes when max |got - ref64| <= 4 E, on condition that
0 < E <= 1e-3 std(ref64) and 4 E >= 2^-24 max |ref64|, half a float32 ulp, below which no float32 result can be held
(both checked from the references alone).  Trained parameters for which that condition cannot
hold (after a handful of Adam steps an entry whose gradient changes sign within rounding moves by 2 lr, which is not
small against the spread of a barely-moved tensor) are compared through the estimates only, and so are the biases in
front of a BatchNorm and the running means that track them (exactly-zero gradients: Adam turns rounding noise into
steps), as tests/test_gpu_estimator.py does.  Set EDGEDET_CONVNET_REPORT to a file to collect the measured ratios
(profiles/convnet_budget.txt).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import convnet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def report(line):
    print(line)
    path = os.environ.get("EDGEDET_CONVNET_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def hold(name, got, r64, r32, outputs_only_ok=False):
    """The yardstick.  Returns False when the condition on E fails for a quantity that may be compared through the
    estimates only."""
    r64 = np.asarray(r64, np.float64)
    ratio, E = R.yardstick(got, r64, r32)
    sd = float(np.std(r64)) if r64.size > 1 else float(np.abs(r64).max())
    # the device result is a float32: no float32 lies closer than half an ulp (<= 2^-24 max |ref64|) to an arbitrary
    # ref64, so a yardstick below that (ref32 landing next to ref64 by luck, as happens with one-element quantities)
    # is none either
    cond = 0 < E <= 1e-3 * sd and 4 * E >= 2.0 ** -24 * float(np.abs(r64).max())
    report(f"{name}: err / 4E = {ratio:.3f}  E = {E:.3e}  E / std = {E / sd if sd else float('inf'):.2e}"
           + ("" if cond else "  (condition on E not met: compared through the estimates only)"))
    if not cond:
        assert outputs_only_ok, f"{name}: E = {E:.3e} against std {sd:.3e} is no usable yardstick"
        return False
    assert ratio <= 1.0, f"{name}: max error is {ratio:.2f} x the budget 4 E (E = {E:.3e})"
    return True


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def nchw(a):
    return np.asarray(a).transpose(0, 3, 1, 2)


def dev_wgrad(x, dy, k):
    """x [B, Cin, H, W], dy [B, Cout, H, W] numpy -> (dW [Cout, Cin, k, k], db [Cout]) from the device."""
    from edgeml_amd import ops
    L = ops.lib()
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    gx, gdy = t(nhwc(x).astype(np.float32)), t(nhwc(dy).astype(np.float32))
    dw = torch.full((Cout, k, k, Cin), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    ops.check(L.edgedet_cnn_wgrad(_p(gx), _p(gdy), B, H, W, Cin, Cout, k, _p(dw), ops.stream_handle()))
    ops.check(L.edgedet_cnn_col_reduce(_p(gdy), None, None, B * H * W, Cout, 1.0, _p(db), None, ops.stream_handle()))
    torch.cuda.synchronize()
    return dw.cpu().numpy().transpose(0, 3, 1, 2), db.cpu().numpy()


GRAD_SHAPES = [(5, 6, 6, 12, 20, 3), (16, 8, 8, 20, 8, 5), (1, 7, 5, 4, 4, 1)]  # B, H, W, Cin, Cout, k


def _grad_case(shape):
    B, H, W, Cin, Cout, k = shape
    rs = np.random.RandomState(B * 100 + k)
    x = rs.randn(B, Cin, H, W).astype(np.float32)
    dy = rs.randn(B, Cout, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, k, k) / np.sqrt(Cin * k * k)).astype(np.float32)
    return x, dy, w


@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_weight_and_bias_gradient(shape):
    """(a) dW on the f32 MFMA and db against torch float64, E from torch float32."""
    B, H, W, Cin, Cout, k = shape
    x, dy, _ = _grad_case(shape)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = (torch.nn.grad.conv2d_weight(torch.from_numpy(x).to(dt), (Cout, Cin, k, k), torch.from_numpy(dy).to(dt),
                                               padding=k // 2).numpy(), torch.from_numpy(dy).to(dt).sum((0, 2, 3)).numpy())
    dw, db = dev_wgrad(x, dy, k)
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    hold(f"wgrad {shape} dW", dw, ref[torch.float64][0], ref[torch.float32][0])
    hold(f"wgrad {shape} db", db, ref[torch.float64][1], ref[torch.float32][1])


def test_weight_gradient_selection_is_exact():
    """(a) One nonzero per channel of x and of dy: every dW entry is a single product (or zero), bit for bit."""
    B, H, W, Cin, Cout, k = 2, 6, 6, 12, 20, 3
    rs = np.random.RandomState(3)
    x = np.zeros((B, Cin, H, W), np.float32)
    dy = np.zeros((B, Cout, H, W), np.float32)
    for c in range(Cin):
        x[1, c, 2 + rs.randint(3), 2 + rs.randint(3)] = np.float32(rs.uniform(0.5, 2.0) * rs.choice([-1, 1]))
    for c in range(Cout):
        dy[c % 2, c, 2 + rs.randint(3), 2 + rs.randint(3)] = np.float32(rs.uniform(0.5, 2.0) * rs.choice([-1, 1]))
    exp = torch.nn.grad.conv2d_weight(torch.from_numpy(x).double(), (Cout, Cin, k, k), torch.from_numpy(dy).double(),
                                      padding=1).numpy().astype(np.float32)  # one product each: one rounding
    dw, db = dev_wgrad(x, dy, k)
    assert (exp != 0).sum() >= 20, "the case must hit the kernel window"
    assert np.array_equal(dw, exp)
    assert np.array_equal(db, dy.sum((0, 2, 3)))


@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_forward_and_data_gradient_through_repack(shape):
    """(b) The repacked weights: the forward conv and the data gradient on the conv engine."""
    from edgeml_amd import ops
    L = ops.lib()
    B, H, W, Cin, Cout, k = shape
    x, dy, w = _grad_case(shape)
    bias = np.random.RandomState(9).randn(Cout).astype(np.float32)
    gw = t(np.ascontiguousarray(w.transpose(0, 2, 3, 1)))  # [Cout][k][k][Cin]
    wf = torch.zeros(Cout * int(L.edgedet_conv_weight_k(k, k, Cin)), device=DEV)
    wb = torch.zeros(Cin * int(L.edgedet_conv_weight_k(k, k, Cout)), device=DEV)
    s = ops.stream_handle()
    ops.check(L.edgedet_cnn_repack(_p(gw), Cout, Cin, k, _p(wf), _p(wb), s))
    gx, gdy, gb, zero = t(nhwc(x)), t(nhwc(dy)), t(bias), torch.zeros(Cin, device=DEV)
    y = torch.empty((B, H, W, Cout), device=DEV)
    dx = torch.empty((B, H, W, Cin), device=DEV)
    ops.check(L.edgedet_conv2d_ex(_p(gx), B, H, W, Cin, _p(wf), None, _p(gb), Cout, k, k, 1, k // 2, 0, None, _p(y), 0, s))
    ops.check(L.edgedet_conv2d_ex(_p(gdy), B, H, W, Cout, _p(wb), None, _p(zero), Cin, k, k, 1, k // 2, 0, None, _p(dx), 0, s))
    torch.cuda.synchronize()
    ref = {}
    for dt in (torch.float64, torch.float32):
        tw = torch.from_numpy(w).to(dt)
        ref[dt] = (torch.nn.functional.conv2d(torch.from_numpy(x).to(dt), tw, torch.from_numpy(bias).to(dt), padding="same").numpy(),
                   torch.nn.grad.conv2d_input((B, Cin, H, W), tw, torch.from_numpy(dy).to(dt), padding=k // 2).numpy())
    hold(f"conv {shape} forward", nchw(y.cpu().numpy()), ref[torch.float64][0], ref[torch.float32][0])
    hold(f"conv {shape} dX", nchw(dx.cpu().numpy()), ref[torch.float64][1], ref[torch.float32][1])


def test_batchnorm_relu_dropout_forward_backward():
    """(c) BatchNorm2d train forward and backward, ReLU, Dropout; the mask equals the numpy hash bit for bit."""
    from edgeml_amd import convnet, ops
    L = ops.lib()
    B, C, H, W, p, seed, fold, layer, step = 5, 20, 6, 6, 0.1, 77, 2, 1, 9
    rs = np.random.RandomState(4)
    z = (rs.randn(B, C, H, W) * rs.uniform(0.5, 2, (1, C, 1, 1)) + rs.randn(1, C, 1, 1)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), (0.3 * rs.randn(C)).astype(np.float32)
    da = rs.randn(B, C, H, W).astype(np.float32)
    rm0, rv0 = rs.randn(C).astype(np.float32), rs.uniform(0.5, 2, C).astype(np.float32)
    keep = R.mask_keep(seed, fold, step, layer, np.arange(z.size).reshape(z.shape), p)
    M = B * H * W
    gz, gg, gbe, gda = t(nhwc(z)), t(gamma), t(beta), t(nhwc(da))
    rm, rv = t(rm0), t(rv0)
    mean, inv = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    xhat, a, dz = torch.empty_like(gz), torch.empty_like(gz), torch.empty_like(gz)
    sdy, sdyx = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    s = ops.stream_handle()
    key = convnet.layer_key(seed, fold, layer)
    ops.check(L.edgedet_cnn_bn_stats(_p(gz), M, C, _p(rm), _p(rv), _p(mean), _p(inv), s))
    ops.check(L.edgedet_cnn_act_fwd(_p(gz), M, C, H * W, _p(gg), _p(gbe), _p(mean), _p(inv), 1, p, key, step, _p(xhat), _p(a), s))
    scale = 1.0 / (1.0 - p)
    ops.check(L.edgedet_cnn_col_reduce(_p(gda), _p(a), _p(xhat), M, C, scale, _p(sdy), _p(sdyx), s))
    ops.check(L.edgedet_cnn_act_bwd(_p(gda), _p(a), _p(xhat), M, C, scale, _p(gg), _p(inv), _p(sdy), _p(sdyx), 1, _p(dz), s))
    # a mask check that does not depend on ReLU: beta = 10 keeps every pre-dropout value positive
    a10 = torch.empty_like(gz)
    ops.check(L.edgedet_cnn_act_fwd(_p(gz), M, C, H * W, _p(gg), _p(t(np.full(C, 10, np.float32))), _p(mean), _p(inv), 1, p,
                                    key, step, None, _p(a10), s))
    torch.cuda.synchronize()
    assert np.array_equal(nchw(a10.cpu().numpy()) != 0, keep)
    assert 0.05 < 1 - keep.mean() < 0.15
    ref = {}
    for dt in (torch.float64, torch.float32):
        bn = torch.nn.BatchNorm2d(C).to(dt)
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(gamma))
            bn.bias.copy_(torch.from_numpy(beta))
            bn.running_mean.copy_(torch.from_numpy(rm0))
            bn.running_var.copy_(torch.from_numpy(rv0))
        bn.train()
        zt = torch.from_numpy(z).to(dt).requires_grad_(True)
        out = torch.relu(bn(zt)) * torch.from_numpy(keep).to(dt) * scale
        out.backward(torch.from_numpy(da).to(dt))
        ref[dt] = [v.detach().numpy() for v in (out, zt.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]
    got = [nchw(a.cpu().numpy()), nchw(dz.cpu().numpy()), sdyx.cpu().numpy(), sdy.cpu().numpy(), rm.cpu().numpy(),
           rv.cpu().numpy()]
    for name, g, r64, r32 in zip(("a", "dz", "dgamma", "dbeta", "running_mean", "running_var"), got, ref[torch.float64],
                                 ref[torch.float32]):
        hold(f"bn2d {name}", g, r64, r32)


def test_maxpool_6_3_1_ties_and_routing():
    """(c) MaxPool2d(2, 2) 6 -> 3 -> 1 with ties in the windows: values, torch's argmax, and the routed gradient."""
    from edgeml_amd import ops
    L = ops.lib()
    B, C = 3, 8
    rs = np.random.RandomState(8)
    x = rs.randint(0, 3, (B, C, 6, 6)).astype(np.float32)  # three values: most windows hold a tie
    s = ops.stream_handle()
    cur, H = t(nhwc(x)), 6
    tx = torch.from_numpy(x).double().requires_grad_(True)
    tcur = tx
    idxs = []
    for _ in range(2):
        y = torch.empty((B, H // 2, H // 2, C), device=DEV)
        idx = torch.empty((B, H // 2, H // 2, C), dtype=torch.int32, device=DEV)
        ops.check(L.edgedet_cnn_maxpool_fwd(_p(cur), B, H, H, C, _p(y), _p(idx), s))
        tcur, tidx = torch.nn.functional.max_pool2d(tcur, 2, 2, return_indices=True)
        torch.cuda.synchronize()
        assert np.array_equal(nchw(y.cpu().numpy()), tcur.detach().numpy())
        assert np.array_equal(nchw(idx.cpu().numpy()), tidx.numpy())
        idxs.append((idx, H))
        cur, H = y, H // 2
    assert H == 1
    g = rs.randn(B, C, 1, 1).astype(np.float32)
    tcur.backward(torch.from_numpy(g).double())
    d = t(nhwc(g))
    for idx, Hin in reversed(idxs):
        dx = torch.empty((B, Hin, Hin, C), device=DEV)
        ops.check(L.edgedet_cnn_maxpool_bwd(_p(d), _p(idx), B, Hin, Hin, C, _p(dx), s))
        d = dx
    torch.cuda.synchronize()
    assert np.array_equal(nchw(d.cpu().numpy()), tx.grad.numpy().astype(np.float32))


POOL_SHAPES = [(5, 7), (7, 5), (6, 6)]


def _ragged_maps(n, seed, C=12):
    rs = np.random.RandomState(seed)
    return [rs.randn(C, *POOL_SHAPES[i % 3]).astype(np.float32) for i in range(n)]


@pytest.mark.parametrize("size", [6, 3])
def test_pooling_load(tmp_path, size):
    """(d) Maps of three shapes in one directory: load_maps + pool_maps against numpy padding + the oracle's roi_align,
    exactly (the tolerance of the roi_align unit test, tests/test_gpu_kernels.py)."""
    from edgeml_amd import convnet
    maps = _ragged_maps(7, 21)
    for i, m in enumerate(maps):
        os.makedirs(tmp_path / f"im{i:02d}")
        np.save(tmp_path / f"im{i:02d}" / "stage17_C3_features.npy", m)
    loaded = convnet.load_maps(str(tmp_path), 17)
    assert all(np.array_equal(a, b) for a, b in zip(loaded, maps))
    got = convnet.pool_maps(loaded, size).cpu().numpy()
    assert np.array_equal(nchw(got), R.pool_ref(maps, size))


def _skip_names(spec):
    """Biases in front of a BatchNorm and the running means that track them: through outputs only."""
    return {lay["name"] + ".0.bias" for lay in spec.layers if lay["bn"]} | {lay["name"] + ".1.running_mean"
                                                                          for lay in spec.layers if lay["bn"]}


def _hold_state(tag, spec, got_vec, r64, r32, grads=False):
    got = spec.unpack(got_vec)
    skip = _skip_names(spec)
    n = 0
    for k, v in r64.items():
        if k in skip or (grads and k not in got):
            continue
        n += bool(hold(f"{tag} {k}", got[k], v, r32[k], outputs_only_ok=not grads))
    return n


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_one_training_step(dropout):
    """(e) forward, backward, Adam of channels 12 -> 20 -> 8, kernels [3, 5], pools [1, 1], hidden [16, 16] on 6 x 6 maps,
    batch 16: every gradient and the updated state."""
    from edgeml_amd import convnet
    g, opts, spec, pooled = R.golden_setup(dropout)
    X, y = pooled[:16], g["reward"][:16].astype(np.float32)
    named = g["init"][0]
    r64 = R.step(spec, opts, named, X, y, torch.float64, seed=5, fold=1)
    r32 = R.step(spec, opts, named, X, y, torch.float32, seed=5, fold=1)
    net = convnet.Trainer(spec, opts, spec.pack(named), 16, 36, seed=5, fold=1)
    net.train_step(t(nhwc(X)), t(y), 16, 6, 6, opts.learning_rate)
    torch.cuda.synchronize()
    hold(f"step p={dropout} loss", net.loss.cpu().numpy(), r64[0], r32[0])
    G = np.zeros(spec.ns, np.float32)
    G[:spec.np] = net.G.cpu().numpy()
    assert _hold_state(f"step p={dropout} grad", spec, G, r64[1], r32[1], grads=True) >= 10
    assert _hold_state(f"step p={dropout} state", spec, net.P.cpu().numpy(), r64[2], r32[2]) >= 10


def _hold_fit(tag, spec, f, best, last, info, r64, r32):
    assert info["best_epoch"][f] == r64["best_epoch"] == r32["best_epoch"]
    for k in ("train_loss", "test_loss"):
        hold(f"{tag} fold {f} {k}", info[k][f], r64[k], r32[k])
    for name, res in (("best", best[f]), ("last", last[f])):
        for e in ("train_est", "val_est"):
            hold(f"{tag} fold {f} {name} {e}", res[e], r64[name][e], r32[name][e])
    _hold_state(f"{tag} fold {f} last", spec, info["last_state"][f], r64["last_state"], r32["last_state"])


@pytest.mark.parametrize("weight", [False, True])
def test_short_fit_golden(weight):
    """(f) The golden data, 3 folds (training sets of 26 / 27 / 27 rows in batches of 16), 4 epochs, milestones [2, 3],
    dropout on with shared masks, MSE and the weighted loss; lr 5e-5, the largest of those tried on the CPU at which
    E <= 1e-3 std holds for every loss and estimate of every fold.  A second fit is bit-identical."""
    from edgeml_amd import convnet
    g, opts, spec, pooled = R.golden_setup(0.1, weight)
    opts.learning_rate = 5e-5
    init = np.stack([spec.pack(n) for n in g["init"]])
    best, last, info = convnet.fit_folds(pooled, g["reward"], g["split"], opts, seed=3, init=init)
    for f in range(len(g["split"])):
        ref = [R.fit(spec, opts, pooled, g["reward"], g["split"][f], g["init"][f], dt, seed=3, fold=f)
               for dt in (torch.float64, torch.float32)]
        _hold_fit(f"fit weight={int(weight)}", spec, f, best, last, info, *ref)
    best2, last2, info2 = convnet.fit_folds(pooled, g["reward"], g["split"], opts, seed=3, init=init)
    assert np.array_equal(info["last_state"], info2["last_state"]) and np.array_equal(info["best_state"], info2["best_state"])
    assert np.array_equal(info["train_loss"], info2["train_loss"]) and np.array_equal(info["test_loss"], info2["test_loss"])
    assert all(np.array_equal(a[e], b[e]) for a, b in zip(best + last, best2 + last2) for e in ("train_est", "val_est"))


def test_short_fit_ragged_resize_0():
    """(g) --resize 0: ragged maps of three shapes, batch 1, no BatchNorm, global mean; 2 epochs."""
    from edgeml_amd import convnet
    maps = _ragged_maps(12, 33)
    rs = np.random.RandomState(2)
    y = np.array([0.4 + 0.2 * np.tanh(m[:4].mean()) for m in maps]) + 0.01 * rs.randn(12)
    split = np.zeros((2, 12), bool)
    split[0, ::3], split[1, 1::4] = True, True
    opts = convnet.ConvOpt(channels=[8, 8], kernels=[3, 3], pools=[True, False], hidden=[16], resize=False, max_epoch=2,
                           milestones=[1], batch_size=1, learning_rate=1e-3, dropout=0.1)
    spec = convnet.make_spec(maps, opts)
    rng = np.random.default_rng(1)
    init = np.stack([spec.init_state(rng) for _ in range(2)])
    best, last, info = convnet.fit_folds(maps, y, split, opts, seed=4, init=init)
    for f in range(2):
        ref = [R.fit(spec, opts, maps, y, split[f], spec.unpack(init[f]), dt, seed=4, fold=f)
               for dt in (torch.float64, torch.float32)]
        _hold_fit("ragged", spec, f, best, last, info, *ref)


def test_cli_end_to_end(tmp_path):
    """(h) python -m edgeml_amd.convnet in a temporary directory: regression.py's files, keys and shapes; wts<k>.pth
    loaded into the ref net reproduces val_est."""
    g = R.load_golden()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for i, m in enumerate(g["maps"]):
        os.makedirs(tmp_path / "features" / f"img{i:03d}")
        np.save(tmp_path / "features" / f"img{i:03d}" / "stage17_C3_features.npy", m)
    np.savez(tmp_path / "reward.npz", reward=g["reward"])
    np.save(tmp_path / "split.npy", g["split"])
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, "-m", "edgeml_amd.convnet", "features", "reward.npz", "split.npy", "est", "--stage", "17",
           "--resize", "6", "--channels", "20", "8", "--kernels", "3", "5", "--hidden", "16", "16", "--model-dir", "model",
           "--normalize", "--weight"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    from edgeml_amd import convnet
    spec = convnet.ConvSpec(12, [20, 8], [3, 5], [True, True], [16, 16], (6, 6), True)
    pooled = R.pool_ref(g["maps"], 6)
    for tag in ("best", "last"):
        for f, mask in enumerate(g["split"]):
            with np.load(tmp_path / f"est_{tag}" / f"estimate{f + 1}.npz") as z:
                assert sorted(z.files) == ["train_est", "train_time", "val_est", "val_time"]
                assert z["train_est"].shape == ((~mask).sum(),) and z["val_est"].shape == (mask.sum(),)
                assert z["train_time"].shape == () and z["val_time"].shape == ()
                val = z["val_est"]
            named = {k: v.numpy() for k, v in torch.load(tmp_path / f"model_{tag}" / f"wts{f + 1}.pth", weights_only=True).items()}
            assert named["conv_stacks.1.0.weight"].shape == (8, 20, 5, 5)
            out = {}
            for dt in (torch.float64, torch.float32):
                net = R.build(spec, named, dt, 0.0).eval()
                with torch.no_grad():
                    out[dt] = net(torch.from_numpy(pooled[mask]).to(dt)).numpy().ravel()
            hold(f"cli {tag} fold {f} val_est", val, out[torch.float64], out[torch.float32])
