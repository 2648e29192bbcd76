"""Drop-in for regression.py's CNN estimator on the weak detector's hidden-layer feature maps (stages 0-23,
the method the paper is named for): lib/nn_model.py's EdgeDetectionNet with conv stacks (Conv2d 'same',
BatchNorm2d, ReLU, Dropout, optional MaxPool 2x2) in front of the linear stacks, trained on the device by the
loop of regression.py:242-355 (fit_CNN).

    python -m edgeml_amd.convnet data_dir reward_path split_path save_dir --stage N [--resize S]
        --channels 64 32 [--kernels 3 3] [--pools 1 1] [--hidden 16 16 16 16]
        [--normalize] [--weight] [--model-dir D] [--seed 0] [--weak yolov5|ssd] [--epochs 100]

Reads <data_dir>/<image>/stage{N}_{name}_features.npy ([C, h, w] maps written by the reference's YOLOv5
scripts) in sorted directory order, the reward npz and the k-fold split, and writes estimate<k>.npz into
<save_dir>_best and <save_dir>_last (and, with --model-dir, wts<k>.pth under EdgeDetectionNet's state-dict
names), as edgeml_amd.estimator does for stage 24.

--weak ssd reads the maps python -m edgeml_amd.maps wrote from SSDLite's backbone instead: the stage numbers and
file-name tokens are those of the library's stage table (edgeml_amd.tapnet.stage_table, stages 1-20), and the
trained file drives the cascade (python -m edgeml_amd.offload --stage N --resize S).

--resize S > 0 pads every map square (zeros at the bottom or the right, lib/metrics.py roi_padding) and
RoI-aligns it to S x S (lib/data.py load_feature: box [0, 0, w, h], scale 1, aligned=False, adaptive sampling)
on the device (edgedet_roi_align, maps of equal shape in one call).  --resize 0 keeps the maps' own shapes:
batch 1, no BatchNorm anywhere and a global mean after the conv stacks (regression.py:420-426).

The reference makes its users edit CNNOpt in the source; here the architecture is given by arguments:
--channels are the OUTPUT channels of the conv layers (the input channels come from the data), --kernels
defaults to 3 and --pools to the reference's [1, 1, 0, ...], both cut to the number of layers; the first
linear width is derived from the data and the final Linear -> 1 is always present.

The step is a sequence of plain kernel launches on one stream (csrc/convnet.hip): the conv
forward and data gradient run on the conv engine (edgedet_conv2d_ex, fp32 MFMA), the weight gradient on
edgedet_cnn_wgrad; folds run one after another.  No kernel uses atomics: two fits of the same inputs are
bit-identical.  State vectors hold conv weights as [Cout][k][k][Cin] and the first linear layer's columns in
the device's (h, w, c) flatten order; ConvSpec.unpack permutes both to torch's layout.

Dropout masks come from the counter hash of csrc/dropout_hash.hpp keyed by (seed, fold, step, layer, NCHW flat
index of the element); tests/convnet_ref.py mask_keep is its numpy restatement.
"""
import ctypes
import os
import time
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from . import estimator, ops

# lib/data.py:99-100: the stage names of the YOLOv5 detectors (file names, copied as data)
V5_NAMES = ['Conv', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C3', 'SPPF', 'Conv', 'Upsample', 'Concat',
            'C3', 'Conv', 'Upsample', 'Concat', 'C3', 'Conv', 'Concat', 'C3', 'Conv', 'Concat', 'C3', 'output']

_M64 = (1 << 64) - 1


@dataclass
class ConvOpt:
    """regression.py:220-236 CNNOpt for the hidden-layer maps; channels are the conv layers' output channels."""
    channels: List = field(default_factory=list)
    kernels: List = field(default_factory=lambda: [3, 3, 3, 3, 3])
    pools: List = field(default_factory=lambda: [True, True, False, False, False])
    hidden: List = field(default_factory=lambda: [16, 16, 16, 16])
    resize: bool = True
    learning_rate: float = 5e-3
    gamma: float = 0.5
    weight_decay: float = 5e-5
    milestones: List = field(default_factory=lambda: [60, 75, 90])
    max_epoch: int = 100
    batch_size: int = 64
    weight: bool = False
    dropout: float = 0.1


def layer_key(seed, fold, layer):
    """The first word of the dropout hash: seed ^ fold << 48 ^ layer << 40 (the second is step << 32 | index)."""
    return ((int(seed) & _M64) ^ ((int(fold) << 48) & _M64) ^ ((int(layer) << 40) & _M64)) & _M64


class ConvSpec:
    """The net's shape and its state layout: for every conv layer w [Cout][k][k][Cin], b and (resize) gamma,
    beta; for every linear layer W [d_out][d_in], b and (hidden, resize) gamma, beta; then the running mean /
    var of every BatchNorm in the same order.  hw = (H, W) of the (resized) input maps, None when resize is off
    (global mean: the first linear width is the last conv layer's channels)."""

    def __init__(self, cin, channels, kernels, pools, hidden, hw=None, resize=True):
        channels = [int(c) for c in channels]
        n = len(channels)
        if n < 1:
            raise ValueError("--channels: at least one conv layer (its output channels) is needed")
        kernels = [int(k) for k in list(kernels)[:n]]
        pools = [bool(p) for p in list(pools)[:n]]
        if len(kernels) < n or len(pools) < n:
            raise ValueError(f"--kernels / --pools: fewer entries than the {n} conv layers of --channels")
        for k in kernels:
            if k < 1 or k % 2 == 0:
                raise ValueError(f"kernel size {k}: only odd kernel sizes are built (padding='same' pads an even "
                                 "kernel asymmetrically)")
        for c in [int(cin)] + channels:
            if c % 4 != 0:
                raise ValueError(f"{c} channels: the conv engine and RoIAlign take channel counts that are multiples "
                                 "of 4 (input maps and every --channels entry)")
        self.resize = bool(resize)
        if self.resize == (hw is None):
            raise ValueError("ConvSpec: hw goes with resize=True and only with it")
        self.cin, self.channels, self.kernels, self.pools = int(cin), channels, kernels, pools
        self.hw = None if hw is None else (int(hw[0]), int(hw[1]))
        self.layers = []
        c, o = self.cin, 0
        h, w = self.hw if self.hw else (None, None)
        for i in range(n):
            lay = {"kind": "conv", "name": f"conv_stacks.{i}", "cin": c, "cout": channels[i], "k": kernels[i],
                   "pool": pools[i], "bn": self.resize, "last": False}
            if self.hw and pools[i]:
                if h < 2 or w < 2:
                    raise ValueError(f"conv layer {i}: MaxPool2d(2, 2) on a {h} x {w} map")
                h, w = h // 2, w // 2
            c = channels[i]
            self.layers.append(lay)
        self.out_hw = (h, w) if self.hw else None
        d0 = c * h * w if self.hw else c
        self.dims = [d0] + [int(v) for v in hidden] + [1]
        for l in range(len(self.dims) - 1):
            last = l == len(self.dims) - 2
            self.layers.append({"kind": "lin", "name": f"linear_stacks.{l}", "cin": self.dims[l],
                                "cout": self.dims[l + 1], "k": 1, "pool": False, "bn": self.resize and not last,
                                "last": last})
        for lay in self.layers:
            nw = lay["cout"] * lay["k"] * lay["k"] * lay["cin"]
            lay["w"], lay["b"] = o, o + nw
            o += nw + lay["cout"]
            if lay["bn"]:
                lay["g"], lay["be"] = o, o + lay["cout"]
                o += 2 * lay["cout"]
        self.np = o
        for lay in self.layers:
            if lay["bn"]:
                lay["rm"], lay["rv"] = o, o + lay["cout"]
                o += 2 * lay["cout"]
        self.ns = o
        self.nconv = n

    def init_state(self, rng):
        """kaiming_uniform_ weights (bound sqrt(6 / fan_in), fan_in = Cin k k), PyTorch's default bias init
        (bound 1 / sqrt(fan_in)), BatchNorm weight 1, bias 0, running mean 0 and var 1."""
        s = np.zeros(self.ns, np.float32)
        for lay in self.layers:
            fan = lay["cin"] * lay["k"] * lay["k"]
            nw = lay["cout"] * fan
            s[lay["w"]:lay["w"] + nw] = rng.uniform(-1, 1, nw) * np.sqrt(6.0 / fan)
            s[lay["b"]:lay["b"] + lay["cout"]] = rng.uniform(-1, 1, lay["cout"]) / np.sqrt(fan)
            if lay["bn"]:
                s[lay["g"]:lay["g"] + lay["cout"]] = 1.0
                s[lay["rv"]:lay["rv"] + lay["cout"]] = 1.0
        return s

    def _weight_to_torch(self, lay, flat):
        co, ci, k = lay["cout"], lay["cin"], lay["k"]
        if lay["kind"] == "conv":
            return flat.reshape(co, k, k, ci).transpose(0, 3, 1, 2)           # [Cout, Cin, k, k]
        if lay is self.layers[self.nconv] and self.hw:                         # (h, w, c) -> (c, h, w) columns
            h, w = self.out_hw
            return flat.reshape(co, h, w, ci // (h * w)).transpose(0, 3, 1, 2).reshape(co, ci)
        return flat.reshape(co, ci)

    def _weight_from_torch(self, lay, arr):
        co, ci, k = lay["cout"], lay["cin"], lay["k"]
        arr = np.asarray(arr)
        if lay["kind"] == "conv":
            return arr.reshape(co, ci, k, k).transpose(0, 2, 3, 1).reshape(-1)
        if lay is self.layers[self.nconv] and self.hw:
            h, w = self.out_hw
            return arr.reshape(co, ci // (h * w), h, w).transpose(0, 2, 3, 1).reshape(-1)
        return arr.reshape(-1)

    def unpack(self, state):
        """{name: array} in torch's EdgeDetectionNet naming and layouts (copies): conv weights [Cout, Cin, k, k],
        the first linear layer's columns in torch's (c, h, w) flatten order."""
        state = np.asarray(state)
        out = {}
        for lay in self.layers:
            p, co = lay["name"], lay["cout"]
            nw = co * lay["k"] * lay["k"] * lay["cin"]
            out[p + ".0.weight"] = np.ascontiguousarray(self._weight_to_torch(lay, state[lay["w"]:lay["w"] + nw]))
            out[p + ".0.bias"] = state[lay["b"]:lay["b"] + co].copy()
            if lay["bn"]:
                for key, nm in (("g", "weight"), ("be", "bias"), ("rm", "running_mean"), ("rv", "running_var")):
                    out[f"{p}.1.{nm}"] = state[lay[key]:lay[key] + co].copy()
        return out

    def pack(self, named, dtype=np.float32):
        """The inverse of unpack: a state vector from EdgeDetectionNet-named arrays (num_batches_tracked ignored)."""
        s = np.zeros(self.ns, dtype)
        for lay in self.layers:
            p, co = lay["name"], lay["cout"]
            nw = co * lay["k"] * lay["k"] * lay["cin"]
            s[lay["w"]:lay["w"] + nw] = self._weight_from_torch(lay, np.asarray(named[p + ".0.weight"], dtype))
            s[lay["b"]:lay["b"] + co] = np.asarray(named[p + ".0.bias"], dtype).reshape(-1)
            if lay["bn"]:
                for key, nm in (("g", "weight"), ("be", "bias"), ("rm", "running_mean"), ("rv", "running_var")):
                    s[lay[key]:lay[key] + co] = np.asarray(named[f"{p}.1.{nm}"], dtype).reshape(-1)
        return s


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(off))


class Trainer:
    """One net on the device: its state P [ns], gradient G [np], Adam moments, the conv engine's weight packs and
    every activation buffer, for batches of up to `batch` maps of up to max_hw pixels.  train_step / loss_eval /
    predict are the three passes of fit_CNN; the launches all go to the current stream."""

    def __init__(self, spec, opts, state, batch, max_hw, seed=0, fold=0, device="cuda"):
        self.spec, self.opts, self.seed, self.fold, self.dev = spec, opts, seed, fold, device
        self.L = ops.lib()
        self.batch = int(batch)
        f32 = dict(dtype=torch.float32, device=device)
        self.P = torch.from_numpy(np.ascontiguousarray(state, np.float32).reshape(spec.ns)).to(device)
        self.G = torch.zeros(spec.np, **f32)
        self.am, self.av = torch.zeros(spec.np, **f32), torch.zeros(spec.np, **f32)
        self.step = 0
        big = 1
        self.buf = []
        hw = int(max_hw)  # pixels of a layer's input map (ragged maps: the largest, pooled ones only shrink)
        if spec.hw is not None:
            h, w = spec.hw
            hw = h * w
        kL = self.L.edgedet_conv_weight_k
        for lay in spec.layers:
            conv = lay["kind"] == "conv"
            n = self.batch * (hw if conv else 1) * lay["cout"]
            big = max(big, n, self.batch * (hw if conv else 1) * lay["cin"])
            b = {"z": torch.empty(n, **f32), "a": torch.empty(n, **f32)}
            if lay["bn"]:
                b["xhat"] = torch.empty(n, **f32)
                b["mean"], b["invstd"] = torch.empty(lay["cout"], **f32), torch.empty(lay["cout"], **f32)
            if conv:
                b["wf"] = torch.zeros(lay["cout"] * int(kL(lay["k"], lay["k"], lay["cin"])), **f32)
                b["wb"] = torch.zeros(lay["cin"] * int(kL(lay["k"], lay["k"], lay["cout"])), **f32)
                b["zero"] = torch.zeros(lay["cin"], **f32)
                if lay["pool"]:
                    b["y"] = torch.empty(n, **f32)
                    b["idx"] = torch.empty(n, dtype=torch.int32, device=device)
                    if spec.hw is not None:
                        h, w = h // 2, w // 2
                        hw = h * w
            self.buf.append(b)
        self.gm = torch.empty(self.batch * spec.channels[-1], **f32)
        self.d = [torch.empty(big, **f32) for _ in range(3)]
        self.loss = torch.zeros(1, **f32)
        self.repack()

    def _s(self):
        return ops.stream_handle()

    def repack(self):
        for lay, b in zip(self.spec.layers, self.buf):
            if lay["kind"] == "conv":
                ops.check(self.L.edgedet_cnn_repack(_p(self.P, lay["w"]), lay["cout"], lay["cin"], lay["k"], _p(b["wf"]),
                                                    _p(b["wb"]) if lay is not self.spec.layers[0] else None, self._s()))

    def set_state(self, state):
        self.P.copy_(state if torch.is_tensor(state) else torch.from_numpy(np.asarray(state, np.float32)))
        self.repack()

    def forward(self, x, B, H, W, train):
        """x: device tensor holding [B][H][W][Cin].  Leaves the prediction [B] in the last layer's z."""
        L, sp, s = self.L, self.spec, self._s()
        drop = float(self.opts.dropout) if train else 0.0
        cur = x
        self.shapes = []
        for li, (lay, b) in enumerate(zip(sp.layers, self.buf)):
            conv = lay["kind"] == "conv"
            if conv:
                ops.check(L.edgedet_conv2d_ex(_p(cur), B, H, W, lay["cin"], _p(b["wf"]), None, _p(self.P, lay["b"]),
                                              lay["cout"], lay["k"], lay["k"], 1, lay["k"] // 2, 0, None, _p(b["z"]), 0, s))
                M, HW = B * H * W, H * W
            else:
                if li == sp.nconv and not sp.resize:
                    ops.check(L.edgedet_cnn_gmean_fwd(_p(cur), B, H * W, lay["cin"], _p(self.gm), s))
                    cur = self.gm
                ops.check(L.edgedet_cnn_linear_fwd(_p(cur), B, lay["cin"], lay["cout"], _p(self.P, lay["w"]),
                                                   _p(self.P, lay["b"]), _p(b["z"]), s))
                M, HW = B, 1
            self.shapes.append((cur, B, H, W))
            if lay["last"]:
                break
            C = lay["cout"]
            if lay["bn"] and train:
                ops.check(L.edgedet_cnn_bn_stats(_p(b["z"]), M, C, _p(self.P, lay["rm"]), _p(self.P, lay["rv"]),
                                                 _p(b["mean"]), _p(b["invstd"]), s))
                mode, mean, inv = 1, _p(b["mean"]), _p(b["invstd"])
            elif lay["bn"]:
                mode, mean, inv = 2, _p(self.P, lay["rm"]), _p(self.P, lay["rv"])
            else:
                mode, mean, inv = 0, None, None
            ops.check(L.edgedet_cnn_act_fwd(_p(b["z"]), M, C, HW, _p(self.P, lay["g"]) if lay["bn"] else None,
                                            _p(self.P, lay["be"]) if lay["bn"] else None, mean, inv, mode, drop,
                                            layer_key(self.seed, self.fold, li), self.step,
                                            _p(b["xhat"]) if lay["bn"] and train else None, _p(b["a"]), s))
            cur = b["a"]
            if lay["pool"]:
                ops.check(L.edgedet_cnn_maxpool_fwd(_p(cur), B, H, W, C, _p(b["y"]), _p(b["idx"]), s))
                cur, H, W = b["y"], H // 2, W // 2
        return self.buf[-1]["z"]

    def backward(self, y, B):
        """Gradients of the loss over the batch of the last train-mode forward into G; y [B] device targets.
        The loss itself goes to self.loss."""
        L, sp, s = self.L, self.spec, self._s()
        drop = float(self.opts.dropout)
        scale = 1.0 / (1.0 - drop) if drop > 0 else 1.0
        da, dz, dn = self.d
        ops.check(L.edgedet_cnn_loss(_p(self.buf[-1]["z"]), _p(y), B, int(bool(self.opts.weight)), _p(self.loss),
                                     _p(dz), s))
        for li in range(len(sp.layers) - 1, -1, -1):
            lay, b = sp.layers[li], self.buf[li]
            x_in, _, H, W = self.shapes[li]
            conv = lay["kind"] == "conv"
            C = lay["cout"]
            M = B * H * W if conv else B
            if not lay["last"]:  # da holds the gradient behind (pool,) dropout and ReLU
                if lay["pool"]:
                    ops.check(L.edgedet_cnn_maxpool_bwd(_p(da), _p(b["idx"]), B, H, W, C, _p(dn), s))
                    da, dn = dn, da
                if lay["bn"]:
                    ops.check(L.edgedet_cnn_col_reduce(_p(da), _p(b["a"]), _p(b["xhat"]), M, C, scale,
                                                       _p(self.G, lay["be"]), _p(self.G, lay["g"]), s))
                ops.check(L.edgedet_cnn_act_bwd(_p(da), _p(b["a"]), _p(b["xhat"]) if lay["bn"] else None, M, C, scale,
                                                _p(self.P, lay["g"]) if lay["bn"] else None,
                                                _p(b["invstd"]) if lay["bn"] else None,
                                                _p(self.G, lay["be"]) if lay["bn"] else None,
                                                _p(self.G, lay["g"]) if lay["bn"] else None, int(lay["bn"]), _p(dz), s))
            if conv:
                ops.check(L.edgedet_cnn_wgrad(_p(x_in), _p(dz), B, H, W, lay["cin"], C, lay["k"], _p(self.G, lay["w"]), s))
            else:
                ops.check(L.edgedet_cnn_wgrad(_p(x_in), _p(dz), B, 1, 1, lay["cin"], C, 1, _p(self.G, lay["w"]), s))
            ops.check(L.edgedet_cnn_col_reduce(_p(dz), None, None, M, C, 1.0, _p(self.G, lay["b"]), None, s))
            if li == 0:
                break
            if conv:  # the data gradient: the same conv over dz with the flipped, transposed pack
                ops.check(L.edgedet_conv2d_ex(_p(dz), B, H, W, C, _p(b["wb"]), None, _p(b["zero"]), lay["cin"], lay["k"],
                                              lay["k"], 1, lay["k"] // 2, 0, None, _p(da), 0, s))
            else:
                ops.check(L.edgedet_cnn_linear_dx(_p(dz), B, lay["cin"], C, _p(self.P, lay["w"]), _p(da), s))
                if li == sp.nconv and not sp.resize:
                    ops.check(L.edgedet_cnn_gmean_bwd(_p(da), B, H * W, lay["cin"], _p(dn), s))
                    da, dn = dn, da
        self.d = [da, dz, dn]

    def adam(self, lr):
        self.step += 1
        bc1, bc2 = 1.0 - 0.9 ** self.step, 1.0 - 0.999 ** self.step
        ops.check(self.L.edgedet_cnn_adam(_p(self.P), _p(self.G), _p(self.am), _p(self.av), self.spec.np, lr / bc1,
                                          bc2 ** 0.5, float(self.opts.weight_decay), self._s()))
        self.repack()

    def train_step(self, x, y, B, H, W, lr):
        """forward (train mode), loss, backward, Adam: one iteration of fit_CNN's train()."""
        self.forward(x, B, H, W, True)
        self.backward(y, B)
        self.adam(lr)

    def eval_loss(self, x, y, B, H, W, out):
        """Eval-mode forward and the batch loss into out[0] (a device view)."""
        pred = self.forward(x, B, H, W, False)
        ops.check(self.L.edgedet_cnn_loss(_p(pred), _p(y), B, int(bool(self.opts.weight)), _p(out), None, self._s()))


class _Rows:
    """The maps of one row set in dataset order on the device: one tensor [n, H, W, C] (resized) or a list of
    [1, h, w, C] tensors (ragged, batch 1)."""

    def __init__(self, maps, idx, y, batch, device):
        self.n, self.ragged = len(idx), isinstance(maps, list)
        self.y = torch.from_numpy(np.ascontiguousarray(y[idx], np.float32)).to(device) if len(idx) else None
        if self.ragged:
            self.x = [maps[i] for i in idx]
            self.batch = 1
        else:
            self.x = maps[torch.from_numpy(np.asarray(idx, np.int64)).to(device)].contiguous() if len(idx) else None
            self.batch = batch

    def batches(self):
        for b0 in range(0, self.n, self.batch):
            n = min(self.batch, self.n - b0)
            x = self.x[b0] if self.ragged else self.x[b0:b0 + n]
            yield b0, n, x, int(x.shape[1]), int(x.shape[2])


def to_device_maps(features, device="cuda"):
    """[N, C, H, W] (or a list of [C, h, w]) numpy maps as NHWC device tensors."""
    if isinstance(features, (list, tuple)):
        return [torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.float32).transpose(1, 2, 0)[None])).to(device)
                for f in features]
    if torch.is_tensor(features):
        return features
    return torch.from_numpy(np.ascontiguousarray(np.asarray(features, np.float32).transpose(0, 2, 3, 1))).to(device)


def make_spec(features, opts):
    ragged = isinstance(features, (list, tuple))
    if ragged:
        cin = int(np.asarray(features[0]).shape[0]) if not torch.is_tensor(features[0]) else int(features[0].shape[-1])
        return ConvSpec(cin, opts.channels, opts.kernels, opts.pools, opts.hidden, None, False)
    if torch.is_tensor(features):  # NHWC on the device (pool_maps)
        return ConvSpec(int(features.shape[3]), opts.channels, opts.kernels, opts.pools, opts.hidden,
                        (int(features.shape[1]), int(features.shape[2])), True)
    f = np.asarray(features)
    return ConvSpec(f.shape[1], opts.channels, opts.kernels, opts.pools, opts.hidden, f.shape[2:], True)


def lr_at(opts, epoch):
    """MultiStepLR: lr * gamma per milestone reached, chained in double as the scheduler does."""
    lr = float(opts.learning_rate)
    for m in opts.milestones:
        if m <= epoch:
            lr *= float(opts.gamma)
    return lr


def fit_folds(features, rewards, split, opts, seed=0, device="cuda", init=None):
    """Train one conv net per fold of `split` ((k, N) bool, True = validation), one fold after another.

    features: [N, C, S, S] maps (numpy, or the NHWC device tensor of pool_maps) with opts.resize, else a list of
    N [C, h, w] maps (batch 1, no BatchNorm, global mean).  rewards [N] or [k, N].  Returns (best, last, info)
    like estimator.fit_folds: per fold {train_est, val_est, train_time, val_time}; info = {train_loss, test_loss
    [k, epochs], best_epoch [k], best_state, last_state [k, ns], spec}."""
    ops.need_device("edgeml_amd.convnet")
    split = np.asarray(split, dtype=bool)
    k, N = split.shape
    y = np.asarray(rewards, dtype=np.float32)
    y = np.broadcast_to(y, (k, N)) if y.ndim == 1 else y.reshape(k, N)
    ragged = isinstance(features, (list, tuple))
    if ragged == bool(opts.resize):
        raise ValueError("fit_folds: a list of maps goes with resize=False, an array [N, C, S, S] with resize=True")
    spec = make_spec(features, opts)
    maps = features if ragged and torch.is_tensor(features[0]) else to_device_maps(features, device)
    batch = 1 if ragged else int(opts.batch_size)
    max_hw = max(int(m.shape[1]) * int(m.shape[2]) for m in maps) if ragged else spec.hw[0] * spec.hw[1]
    if init is None:
        rng = np.random.default_rng(seed)
        init = np.stack([spec.init_state(rng) for _ in range(k)])
    init = np.asarray(init, np.float32).reshape(k, spec.ns)
    E = int(opts.max_epoch)
    best, last = [], []
    info = {"train_loss": np.zeros((k, E)), "test_loss": np.zeros((k, E)), "best_epoch": np.zeros(k, np.int64),
            "best_state": np.zeros((k, spec.ns), np.float32), "last_state": np.zeros((k, spec.ns), np.float32),
            "spec": spec}
    for f in range(k):
        tr_idx, va_idx = np.nonzero(~split[f])[0], np.nonzero(split[f])[0]
        if spec.resize and len(tr_idx) % batch == 1:
            raise ValueError(f"fold {f + 1}: the last training batch has one row and BatchNorm cannot normalise one "
                             f"value per channel (torch raises there too): {len(tr_idx)} rows in batches of {batch}")
        tr, va = _Rows(maps, tr_idx, y[f], batch, device), _Rows(maps, va_idx, y[f], batch, device)
        net = Trainer(spec, opts, init[f], batch, max_hw, seed=seed, fold=f, device=device)
        ntb, nvb = -(-tr.n // tr.batch), -(-va.n // va.batch)
        g_trl = torch.zeros(max(ntb, 1), dtype=torch.float32, device=device)
        g_tel = torch.zeros(max(nvb, 1), dtype=torch.float32, device=device)
        best_loss, best_state = np.inf, net.P.clone()
        for ep in range(E):
            lr = lr_at(opts, ep)
            for bi, (b0, n, x, H, W) in enumerate(tr.batches()):
                net.forward(x, n, H, W, True)
                net.backward(tr.y[b0:b0 + n], n)
                g_trl[bi:bi + 1].copy_(net.loss)
                net.adam(lr)
            for bi, (b0, n, x, H, W) in enumerate(va.batches()):
                net.eval_loss(x, va.y[b0:b0 + n], n, H, W, g_tel[bi:bi + 1])
            # regression.py:291,306: the batch losses are summed as Python floats
            trl = sum(float(v) for v in g_trl[:ntb].cpu().numpy()) / max(ntb, 1)
            tel = sum(float(v) for v in g_tel[:nvb].cpu().numpy()) / nvb if nvb else 0.0
            info["train_loss"][f, ep], info["test_loss"][f, ep] = trl, tel
            if tel < best_loss:
                best_loss, info["best_epoch"][f] = tel, ep
                best_state = net.P.clone()
        last_state = net.P.clone()
        res = []
        for st in (best_state, last_state):
            net.set_state(st)
            ests, times = [], []
            for rows in (tr, va):
                out = torch.zeros(max(rows.n, 1), dtype=torch.float32, device=device)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b0, n, x, H, W in rows.batches():
                    out[b0:b0 + n].copy_(net.forward(x, n, H, W, False)[:n])
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / max(rows.n, 1))
                ests.append(out[:rows.n].cpu().numpy())
            res.append({"train_est": ests[0], "val_est": ests[1], "train_time": times[0], "val_time": times[1]})
        best.append(res[0])
        last.append(res[1])
        info["best_state"][f], info["last_state"][f] = best_state.cpu().numpy(), last_state.cpu().numpy()
    return best, last, info


def load_maps(data_dir, stage, names=V5_NAMES):
    """lib/data.py:87-124: every image directory's stage{N}_{name}_features.npy, in sorted order.  names: the
    stage -> name table (a list or a dict): YOLOv5's, or SSDLite's (edgeml_amd.tapnet.ssd_names())."""
    images = sorted(f for f in os.listdir(data_dir) if not os.path.isfile(os.path.join(data_dir, f)))
    return [np.load(os.path.join(data_dir, im, f"stage{stage}_{names[stage]}_features.npy"), allow_pickle=False)
            for im in images]


def pool_maps(maps, size, device="cuda"):
    """load_feature's pooling (func="avg") on the device: roi_padding (zeros at the bottom or the right up to a
    square) and roi_align with box [0, 0, w, h], scale 1, aligned=False, the adaptive sampling grid, to
    [size, size]; maps of equal shape go through one edgedet_roi_align call.  Returns NHWC [N, size, size, C]."""
    ops.need_device("edgeml_amd.convnet")
    if not maps:
        raise ValueError("no feature maps found")
    C = int(maps[0].shape[0])
    if C % 4 != 0:
        raise ValueError(f"{C} channels: edgedet_roi_align takes channel counts that are multiples of 4")
    out = torch.empty((len(maps), size, size, C), dtype=torch.float32, device=device)
    groups = {}
    for i, m in enumerate(maps):
        if m.ndim != 3 or m.shape[0] != C:
            raise ValueError(f"map {i}: shape {m.shape}, expected [{C}, h, w]")
        groups.setdefault(tuple(m.shape[1:]), []).append(i)
    for (h, w), ids in groups.items():
        s = max(h, w)
        feat = np.zeros((len(ids), s, s, C), np.float32)
        feat[:, :h, :w] = np.stack([np.asarray(maps[i], np.float32).transpose(1, 2, 0) for i in ids])
        rois = np.zeros((len(ids), 5), np.float32)
        rois[:, 0] = np.arange(len(ids))
        rois[:, 3], rois[:, 4] = w, h
        got = ops.roi_align_nhwc(torch.from_numpy(feat).to(device), torch.from_numpy(rois).to(device), 1.0,
                                 output_size=size, sampling_ratio=0)
        out[torch.tensor(ids, device=device)] = got
    return out


def save_state(path, spec, state, index):
    """wts<k>.pth under EdgeDetectionNet's state-dict names and torch's layouts (ConvSpec.unpack)."""
    os.makedirs(path, exist_ok=True)
    named = {k: torch.from_numpy(np.array(v, dtype=np.float32)) for k, v in spec.unpack(np.asarray(state)).items()}
    torch.save(named, os.path.join(path, f"wts{index + 1}.pth"))


def check_args(opts):
    """Refuse what this CLI does not build, naming what does."""
    if getattr(opts, "weak", "yolov5") == "ssd":
        from . import tapnet
        try:
            tapnet.stage_info(opts.stage)
        except ValueError as e:
            raise SystemExit(f"--weak ssd --stage {opts.stage}: not in SSDLite's stage table (edgeml_amd.tapnet."
                             f"stage_table: 1-16 mobilenet_v3_large.features, 17-20 backbone.extra): {e}") from None
    elif opts.stage == 24:
        raise SystemExit("edgeml_amd.convnet trains on the hidden-layer feature maps of stages 0-23; --stage 24 (the "
                         "output features) is python -m edgeml_amd.estimator")
    elif not 0 <= opts.stage < 24:
        raise SystemExit(f"--stage {opts.stage}: the YOLOv5 stages are 0-23 (and 24, the output features)")
    if opts.model != "CNN":
        raise SystemExit("Only fully convolutional NN can take feature maps from hidden layers as inputs: "
                         f"--model {opts.model} with --stage {opts.stage} (regression.py:422); use --model CNN")
    if not opts.channels:
        raise SystemExit("--channels: give the output channels of every conv layer (e.g. --channels 64 32); a net "
                         "without conv layers on the stage-24 features is python -m edgeml_amd.estimator")
    if opts.epochs < 1:
        raise SystemExit("--epochs: at least one epoch")
    if opts.resize < 0:
        raise SystemExit("--resize: 0 (keep the maps' shapes) or the side S of the pooled maps")
    n = len(opts.channels)
    kernels = (list(opts.kernels) + [3] * n)[:n] if opts.kernels else [3] * n
    bad = [k for k in kernels if k < 1 or k % 2 == 0]
    if bad:
        raise SystemExit(f"--kernels {bad[0]}: only odd kernel sizes are built (padding='same' pads an even kernel "
                         "asymmetrically)")
    pools = (list(opts.pools) + [0] * n)[:n] if opts.pools is not None else ([1, 1] + [0] * n)[:n]
    return kernels, [bool(p) for p in pools]


def main(opts):
    kernels, pools = check_args(opts)
    if opts.weak == "ssd":
        from . import tapnet
        maps = load_maps(opts.data_dir, opts.stage, tapnet.ssd_names())
    else:
        maps = load_maps(opts.data_dir, opts.stage)
    reward, split = estimator.load_reward_split(opts, len(maps))
    cnn = ConvOpt(channels=list(opts.channels), kernels=kernels, pools=pools, hidden=list(opts.hidden),
                  resize=opts.resize > 0, weight=opts.weight and opts.normalize, max_epoch=opts.epochs)
    try:
        feats = pool_maps(maps, opts.resize) if cnn.resize else maps
        if not cnn.resize:
            cnn.batch_size = 1  # regression.py:423-426
        y = estimator.fold_targets(reward, split, opts.normalize, np.float32)
        t0 = time.perf_counter()
        best, last, info = fit_folds(feats, y, split, cnn, seed=opts.seed)
    except ValueError as e:
        raise SystemExit(f"edgeml_amd.convnet: {e}")
    print(f"trained {len(split)} folds x {cnn.max_epoch} epochs in {time.perf_counter() - t0:.2f} s")
    save_best, save_last = estimator.parse_path(opts.save_dir)
    for cv_idx in range(len(split)):
        print(f"fold {cv_idx + 1}: best test loss {info['test_loss'][cv_idx].min():.6f}")
        estimator.save_result(save_best, best[cv_idx], cv_idx)
        estimator.save_result(save_last, last[cv_idx], cv_idx)
    if opts.model_dir != "":
        for path, states in zip(estimator.parse_path(opts.model_dir), (info["best_state"], info["last_state"])):
            for cv_idx in range(len(split)):
                save_state(path, info["spec"], states[cv_idx], cv_idx)
    return best, last


def getargs(argv=None):
    a = estimator.base_parser("CNN", prog="python -m edgeml_amd.convnet")
    a.add_argument("--channels", type=int, nargs="*", default=[], help="output channels of every conv layer")
    a.add_argument("--kernels", type=int, nargs="*", default=None, help="kernel sizes (odd), default 3")
    a.add_argument("--pools", type=int, nargs="*", default=None, help="1: MaxPool2d(2, 2) after the layer; default 1 1 0 ...")
    a.add_argument("--hidden", type=int, nargs="*", default=[16, 16, 16, 16], help="hidden linear widths")
    a.add_argument("--seed", type=int, default=0)
    a.add_argument("--epochs", type=int, default=100, help="training epochs (the reference's max_epoch, 100)")
    a.add_argument("--weak", choices=("yolov5", "ssd"), default="yolov5",
                   help="whose hidden-layer maps data_dir holds: YOLOv5's, or SSDLite's (python -m edgeml_amd.maps)")
    return a.parse_args(argv)


if __name__ == "__main__":
    main(getargs())
