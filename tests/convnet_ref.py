"""A torch-CPU restatement of lib/nn_model.py EdgeDetectionNet with conv stacks and of regression.py fit_CNN's
loop (regression.py:242-355), the reference of tests/test_gpu_convnet.py and tests/test_convnet_host.py.

It takes a dtype (float32 or float64), an explicit initial state (EdgeDetectionNet's state-dict names) and explicit
dropout masks: mask_keep is the numpy restatement of the device's counter hash (csrc/dropout_hash.hpp), keyed by
(seed, fold, step, layer, NCHW flat index), so a fit with dropout on is comparable step for step.  pool_ref is
load_feature's pooling: numpy roi_padding + the oracle's roi_align.

The yardstick of every trained quantity: run the ref in float64 and float32 from the same start;
E = max |ref32 - ref64| is the float32 rounding scale and a result passes when max |got - ref64| <= 4 E
(the factor of tests/test_gpu_conv_budget.py), provided 0 < E <= 1e-3 std(ref64).
"""
import numpy as np
import torch

_M64 = (1 << 64) - 1


def mask_keep(seed, fold, step, layer, index, p):
    """True where the element with NCHW flat index `index` is kept: u >= p for u = the top 24 bits of
    splitmix64(seed ^ fold << 48 ^ layer << 40, step << 32 | index)."""
    with np.errstate(over="ignore"):
        a = np.uint64(((int(seed) & _M64) ^ ((int(fold) << 48) & _M64) ^ ((int(layer) << 40) & _M64)) & _M64)
        b = np.uint64(int(step) << 32) | np.asarray(index).astype(np.uint64)
        z = a * np.uint64(0x9E3779B97F4A7C15) + b + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def hash_int(a, b):
    """The same hash on Python integers (an independent check of the numpy form)."""
    z = (a * 0x9E3779B97F4A7C15 + b + 0x632BE59BD9B4E019) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return ((z ^ (z >> 31)) >> 32) & 0xFFFFFFFF


class MaskDropout(torch.nn.Module):
    """nn.Dropout with the mask given from outside: y = x * mask / (1 - p) in train mode."""

    def __init__(self, p, layer):
        super().__init__()
        self.p, self.layer, self.ctx = p, layer, None  # ctx = (seed, fold, step), set before each train forward

    def forward(self, x):
        if not self.training or self.p <= 0 or self.ctx is None:
            return x
        seed, fold, step = self.ctx
        keep = mask_keep(seed, fold, step, self.layer, np.arange(x.numel()).reshape(tuple(x.shape)), self.p)
        return x * torch.from_numpy(keep).to(x.dtype) * (1.0 / (1.0 - self.p))


class RefNet(torch.nn.Module):
    """EdgeDetectionNet (lib/nn_model.py:28-112): channels = [Cin, C1, ...], linear = [d0, ..., 1]; the dropout
    layers take explicit masks, numbered conv layers first, then the linear ones."""

    def __init__(self, channels, kernels, pools, linear, resize=True, p=0.1):
        super().__init__()
        nn = torch.nn
        self.resize = resize
        self.conv_stacks, self.linear_stacks = nn.ModuleList(), nn.ModuleList()
        self.drops = []
        li = 0
        for cin, cout, k, pool in zip(channels[:-1], channels[1:], kernels, pools):
            mods = [nn.Conv2d(cin, cout, k, padding="same")]
            if resize:
                mods.append(nn.BatchNorm2d(cout))
            mods += [nn.ReLU(), MaskDropout(p, li)]
            self.drops.append(mods[-1])
            if pool:
                mods.append(nn.MaxPool2d(2, 2))
            self.conv_stacks.append(nn.Sequential(*mods))
            li += 1
        for l, (din, dout) in enumerate(zip(linear[:-1], linear[1:])):
            mods = [nn.Linear(din, dout)]
            if l < len(linear) - 2:
                if resize:
                    mods.append(nn.BatchNorm1d(dout))
                mods += [nn.ReLU(), MaskDropout(p, li)]
                self.drops.append(mods[-1])
            self.linear_stacks.append(nn.Sequential(*mods))
            li += 1

    def forward(self, x):
        for conv in self.conv_stacks:
            x = conv(x)
        if not self.resize:
            x = torch.mean(x, dim=(2, 3), keepdim=True)
        x = torch.flatten(x, 1)
        for lin in self.linear_stacks:
            x = lin(x)
        return x

    def set_ctx(self, ctx):
        for d in self.drops:
            d.ctx = ctx


def build(spec, named, dtype, p=0.1):
    """RefNet of a ConvSpec (edgeml_amd.convnet) loaded with the named state."""
    net = RefNet([spec.cin] + spec.channels, spec.kernels, spec.pools, spec.dims, spec.resize, p).to(dtype)
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in named.items()}
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k for k in missing.missing_keys), missing
    return net


def named_state(net):
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items() if "num_batches_tracked" not in k}


def _loss(pred, y, weighted):
    return torch.mean((pred - y) ** 2 * y) if weighted else torch.mean((pred - y) ** 2)


def _batches(maps, y, idx, batch, dtype):
    """(X [n, C, H, W], y [n, 1]) in dataset order; `maps` an array [N, C, H, W] or a list of [C, h, w]."""
    for b0 in range(0, len(idx), batch):
        ids = idx[b0:b0 + batch]
        X = torch.from_numpy(np.stack([np.asarray(maps[i], np.float32) for i in ids])).to(dtype)
        yield X, torch.from_numpy(np.asarray(y[ids], np.float32)).to(dtype).reshape(-1, 1)


def step(spec, opts, named, X, y, dtype, seed=0, fold=0):
    """One training step (forward, backward, Adam at the initial learning rate) from the named state.  X [B, C, H, W]
    and y [B] numpy.  Returns (loss, grads {name: array}, state {name: array}) in float64 numpy."""
    torch.manual_seed(0)
    net = build(spec, named, dtype, opts.dropout)
    opt = torch.optim.Adam(net.parameters(), lr=opts.learning_rate, weight_decay=opts.weight_decay)
    net.train()
    net.set_ctx((seed, fold, 0))
    pred = net(torch.from_numpy(np.asarray(X, np.float32)).to(dtype))
    loss = _loss(pred, torch.from_numpy(np.asarray(y, np.float32)).to(dtype).reshape(-1, 1), opts.weight)
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().numpy().astype(np.float64) for k, p in net.named_parameters()}
    opt.step()
    return loss.item(), grads, {k: v.astype(np.float64) for k, v in named_state(net).items()}


def fit(spec, opts, maps, y, val_mask, named, dtype, seed=0, fold=0):
    """fit_CNN for one fold.  Returns {train_loss, test_loss [epochs], best_epoch, best, last: {train_est, val_est},
    best_state, last_state: named}."""
    import copy
    net = build(spec, named, dtype, opts.dropout)
    best_net = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=opts.learning_rate, weight_decay=opts.weight_decay)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(opts.milestones), gamma=opts.gamma)
    val_mask = np.asarray(val_mask, bool)
    tr, va = np.nonzero(~val_mask)[0], np.nonzero(val_mask)[0]
    batch = opts.batch_size if spec.resize else 1
    out = {"train_loss": [], "test_loss": [], "best_epoch": 0}
    best_err, nstep = np.inf, 0
    for ep in range(opts.max_epoch):
        net.train()
        tl, nb = 0.0, 0
        for X, t in _batches(maps, y, tr, batch, dtype):
            net.set_ctx((seed, fold, nstep))
            loss = _loss(net(X), t, opts.weight)
            opt.zero_grad()
            loss.backward()
            opt.step()
            tl += loss.item()
            nb += 1
            nstep += 1
        out["train_loss"].append(tl / nb)
        net.eval()
        te, nv = 0.0, 0
        with torch.no_grad():
            for X, t in _batches(maps, y, va, batch, dtype):
                te += _loss(net(X), t, opts.weight).item()
                nv += 1
        te /= nv
        if te < best_err:
            best_err, best_net, out["best_epoch"] = te, copy.deepcopy(net), ep
        out["test_loss"].append(te)
        sched.step()
    for key, m in (("best", best_net), ("last", net)):
        m.eval()
        with torch.no_grad():
            est = [np.concatenate([m(X).numpy().astype(np.float64) for X, _ in _batches(maps, y, ids, batch, dtype)]).ravel()
                   for ids in (tr, va)]
        out[key] = {"train_est": est[0], "val_est": est[1]}
        out[key + "_state"] = named_state(m)
    out["train_loss"], out["test_loss"] = np.array(out["train_loss"]), np.array(out["test_loss"])
    return out


def pool_ref(maps, size):
    """lib/data.py load_feature(pool=True, func="avg"): roi_padding (lib/metrics.py:21-35) and roi_align with the
    box [0, 0, w, h], scale 1, aligned=False, adaptive sampling.  Returns [N, C, size, size] float32."""
    from oracle import tv_ops
    out = []
    for m in maps:
        c, h, w = m.shape
        pad = ((0, 0), (0, w - h), (0, 0)) if h < w else ((0, 0), (0, 0), (0, h - w))
        fm = np.pad(np.asarray(m, np.float32), pad)
        got = tv_ops.roi_align(torch.from_numpy(fm[None]), np.array([[0, 0, 0, w, h]], np.float32), 1.0, out=size,
                               sampling_ratio=0)
        out.append(np.asarray(got)[0])
    return np.stack(out).astype(np.float32)


def yardstick(got, ref64, ref32, what=""):
    """(ratio, E): max |got - ref64| / (4 E) with E = max |ref32 - ref64|."""
    r64 = np.asarray(ref64, np.float64)
    E = float(np.max(np.abs(np.asarray(ref32, np.float64) - r64)))
    err = float(np.max(np.abs(np.asarray(got, np.float64) - r64)))
    return err / (4 * E) if E > 0 else (0.0 if err == 0 else np.inf), E


def load_golden():
    """tests/golden/g_convnet.npz (make_golden_convnet.py): the reference's own run of regression.main() with
    --stage 17 --resize 6 --model CNN, dropout off."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_convnet.npz"))
    n = int(z["n"])
    g = {"maps": [z[f"map/{i:03d}"] for i in range(n)], "reward": z["reward"], "split": z["split"],
         "resize": int(z["cfg"][1]), "epochs": int(z["cfg"][2]), "batch": int(z["cfg"][3]),
         "channels": [int(v) for v in z["channels"]], "kernels": [int(v) for v in z["kernels"]],
         "pools": [bool(v) for v in z["pools"]], "linear": [int(v) for v in z["linear"]],
         "milestones": [int(v) for v in z["milestones"]]}
    k = g["split"].shape[0]
    for tag in ("init", "best_state", "last_state"):
        g[tag] = [{key.split("/", 2)[2]: z[key] for key in z.files if key.startswith(f"{tag}/{f}/")} for f in range(k)]
    for tag in ("best", "last"):
        g[tag] = [{e: z[f"{tag}/{f}/{e}"] for e in ("train_est", "val_est")} for f in range(k)]
    return g


def golden_setup(dropout, weight=False):
    """(golden, ConvOpt, ConvSpec, pooled maps [N, C, S, S]) of the golden run's configuration."""
    from edgeml_amd import convnet
    g = load_golden()
    opts = convnet.ConvOpt(channels=g["channels"][1:], kernels=g["kernels"], pools=g["pools"], hidden=g["linear"][1:-1],
                           resize=True, max_epoch=g["epochs"], milestones=g["milestones"], batch_size=g["batch"],
                           weight=weight, dropout=dropout)
    spec = convnet.ConvSpec(g["channels"][0], opts.channels, opts.kernels, opts.pools, opts.hidden,
                            (g["resize"], g["resize"]), True)
    return g, opts, spec, pool_ref(g["maps"], g["resize"])
