"""The weak detector's hidden-layer maps in the cascade: SSDLite's stage table (csrc/lower.hip, read through
edgedet_ssdlite_taps: Python holds no copy of it) and the eval-mode inference of a trained conv-stack estimator
(edgeml_amd.convnet) from a batch of pooled maps: convnet.Trainer's layered eval forward (the default) or, on
request and for a net inside the kernel's fit rule, one fused launch (csrc/tapnet.hip).
"""
import ctypes

import numpy as np
import torch

from . import convnet, ops

TAP_DTYPE = np.dtype([("stage", "<i4"), ("chain", "<i4"), ("token", "S8"), ("buffer", "S96"), ("image0", "<i8"),
                      ("images", "<i8"), ("C", "<i8"), ("H", "<i8"), ("W", "<i8")])
SSD_SIZE = 320  # the side SSDLite resizes every image to: the table's geometry does not depend on the image size


class Tap:
    """One row of the stage table: stage, chain, the file-name token, the plan buffer's name, the chain's images
    [image0, image0 + images) of the batch and the map's C, H, W."""

    def __init__(self, row):
        self.stage, self.chain = int(row["stage"]), int(row["chain"])
        self.token = bytes(row["token"]).split(b"\0", 1)[0].decode()
        self.buffer = bytes(row["buffer"]).split(b"\0", 1)[0].decode()
        self.image0, self.images = int(row["image0"]), int(row["images"])
        self.C, self.H, self.W = int(row["C"]), int(row["H"]), int(row["W"])

    def __repr__(self):
        return (f"Tap(stage {self.stage} {self.token}, chain {self.chain}, {self.buffer!r}, images {self.image0}+"
                f"{self.images}, C {self.C}, {self.H} x {self.W})")


def stage_table(num_classes=91, reduced_tail=True, B=1, H=SSD_SIZE, W=SSD_SIZE, u8=False, stage=-1):
    """edgedet_ssdlite_taps: the taps of `stage` (one per chain), or of every stage (stage=-1), of the SSDLite
    plan of (B, H, W).  Raises ValueError for a stage outside the table and for stage 0 under the fused stem."""
    L = ops.lib()
    args = (int(num_classes), int(bool(reduced_tail)), int(B), int(H), int(W), int(bool(u8)), int(stage))
    n = L.edgedet_ssdlite_taps(*args, None, 0)
    if n < 0:
        raise ValueError(L.edgedet_last_error().decode())
    out = np.zeros(int(n), dtype=TAP_DTYPE)
    if L.edgedet_ssdlite_taps(*args, out.ctypes.data, int(n)) != n:
        raise ValueError(L.edgedet_last_error().decode())
    return [Tap(r) for r in out]


def ssd_names(num_classes=91, reduced_tail=True):
    """{stage: token} of every stage the default lowering gives a buffer: the `names` of convnet.load_maps."""
    return {t.stage: t.token for t in stage_table(num_classes, reduced_tail)}


def stage_info(stage, num_classes=91, reduced_tail=True):
    """The (token, C, H, W) of a stage; ValueError (naming the table) when it has none."""
    t = stage_table(num_classes, reduced_tail, stage=stage)[0]
    return t.token, t.C, t.H, t.W


def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*[int(v) for v in values])


class TapNet:
    """A trained conv-stack net (a ConvSpec and its state vector) that predicts on the device.  infer() runs the
    layered eval forward by default (in the weak stage the fused kernel measured no faster);
    fused=True takes the fused kernel, which is an error for a net outside its fit rule (edgedet_tapnet_fits)."""

    def __init__(self, spec, state, fused=None):
        self.spec = spec
        self.state = np.ascontiguousarray(np.asarray(state, np.float32).reshape(spec.ns))
        self.fused = fused
        self._dev = None
        self._trainer = None
        if spec.resize:
            self._net = (spec.hw[0], spec.cin, spec.nconv, _i32(spec.channels), _i32(spec.kernels), _i32(spec.pools),
                         len(spec.dims) - 1, _i32(spec.dims))
            square = spec.hw[0] == spec.hw[1]
            self.fits = square and bool(ops.lib().edgedet_tapnet_fits(*self._net))
        else:
            self._net, self.fits = None, False  # no BatchNorm, a global mean: the layered forward only

    def lds_bytes(self):
        """The LDS the fused kernel would take (edgedet_tapnet_lds), or -1."""
        return int(ops.lib().edgedet_tapnet_lds(*self._net)) if self._net else -1

    def device_state(self, device):
        if self._dev is None or self._dev.device != torch.device(device):
            self._dev = torch.from_numpy(self.state).to(device)
        return self._dev

    def trainer(self, device, batch, max_hw=None):
        """A new convnet.Trainer holding this net's state: the layered path's buffers, for batches up to `batch`
        on one stream (the caller keeps one per stream)."""
        hw = max_hw if max_hw is not None else (self.spec.hw[0] * self.spec.hw[1] if self.spec.hw else 1)
        return convnet.Trainer(self.spec, convnet.ConvOpt(), self.state, batch, hw, device=device)

    def use_fused(self, fused=None):
        fused = self.fused if fused is None else fused
        if fused and not self.fits:
            raise ValueError("the fused kernel does not take this net (edgedet_tapnet_fits): use the layered forward")
        return bool(fused)

    def infer(self, x, threshold, est, flag, stream=None, trainer=None, fused=None):
        """x [B, H, W, C] float32 on the device (the pooled maps; H = W = S for a resize net) -> est [B] float64
        and flag [B] uint8 = est > threshold, enqueued on `stream` (the current one when None; the layered path
        always issues on the current stream)."""
        ops._need_cuda(x, est, flag)
        B, H, W, C = (int(v) for v in x.shape)
        if C != self.spec.cin or (self.spec.hw and (H, W) != self.spec.hw) or not x.is_contiguous():
            raise ValueError(f"maps {tuple(x.shape)}: the net takes contiguous [B, {self.spec.hw}, {self.spec.cin}]")
        L = ops.lib()
        if self.use_fused(fused):
            st = self.device_state(x.device)
            ops.check(L.edgedet_tapnet_infer(ops._ptr(x), B, *self._net, ops._ptr(st), st.numel(), float(threshold),
                                             ops._ptr(est), ops._ptr(flag), ops.stream_handle(stream)))
            return
        if trainer is None:
            if self._trainer is None or self._trainer.batch < B or self._trainer.hw < H * W:
                self._trainer = self.trainer(x.device, max(B, 64), H * W)
                self._trainer.hw = H * W
            trainer = self._trainer
        with torch.cuda.stream(stream) if stream is not None else _Null():
            z = trainer.forward(x, B, H, W, False)
            ops.check(L.edgedet_tapnet_finish(ops._ptr(z), B, float(threshold), ops._ptr(est), ops._ptr(flag),
                                              ops.stream_handle()))


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def predict(net, x, threshold=0.0, fused=None):
    """(est [B] float64, flag [B] bool) as numpy arrays: TapNet.infer on fresh buffers, synchronised."""
    est = torch.empty(int(x.shape[0]), dtype=torch.float64, device=x.device)
    flag = torch.empty(int(x.shape[0]), dtype=torch.uint8, device=x.device)
    net.infer(x, threshold, est, flag, fused=fused)
    torch.cuda.synchronize()
    return est.cpu().numpy(), flag.cpu().numpy().astype(bool)


def default_pools(n):
    """The convnet CLI's default: a pool after each of the first two conv layers."""
    return ([True, True] + [False] * n)[:n]


def spec_from_named(path, named, stage_c, resize, pools=None):
    """The ConvSpec of a conv-stack state dict (EdgeDetectionNet's names), rebuilt from the tensor shapes.
    A file with BatchNorm tensors is a --resize S net (S = `resize`, pools as given or the CLI's default); one
    without is a --resize 0 net.  ValueError when Cin is not the stage's channel count `stage_c`, or when the
    first linear width is not the pooled geometry's; the message names both numbers."""
    n = 0
    while f"conv_stacks.{n}.0.weight" in named:
        n += 1
    L = 0
    while f"linear_stacks.{L}.0.weight" in named:
        L += 1
    if n == 0 or L == 0:
        raise ValueError(f"{path}: conv_stacks.<i>.0.weight and linear_stacks.<l>.0.weight tensors expected")
    cw = [tuple(named[f"conv_stacks.{i}.0.weight"].shape) for i in range(n)]
    lw = [tuple(named[f"linear_stacks.{l}.0.weight"].shape) for l in range(L)]
    if any(len(s) != 4 or s[2] != s[3] for s in cw) or any(cw[i][1] != cw[i - 1][0] for i in range(1, n)):
        raise ValueError(f"{path}: the conv layers {cw} do not chain")
    if any(len(s) != 2 for s in lw) or any(lw[l][1] != lw[l - 1][0] for l in range(1, L)) or lw[-1][0] != 1:
        raise ValueError(f"{path}: the linear layers {lw} do not chain to one output")
    cin, channels, kernels = int(cw[0][1]), [int(s[0]) for s in cw], [int(s[2]) for s in cw]
    if cin != int(stage_c):
        raise ValueError(f"{path}: the first conv layer takes {cin} channels, the stage's map has {int(stage_c)}")
    hidden = [int(s[0]) for s in lw[:-1]]
    bn = "conv_stacks.0.1.weight" in named
    pools = default_pools(n) if pools is None else [bool(p) for p in pools]
    if not bn:
        spec = convnet.ConvSpec(cin, channels, kernels, pools, hidden, None, False)
    else:
        if not resize or resize < 1:
            raise ValueError(f"{path}: a --resize S net (it has BatchNorm tensors): give --stage N and --resize S")
        spec = convnet.ConvSpec(cin, channels, kernels, pools, hidden, (int(resize), int(resize)), True)
    if spec.dims[0] != int(lw[0][1]):
        raise ValueError(f"{path}: the first linear layer takes {int(lw[0][1])} inputs, the pooled geometry "
                         f"(resize {resize or 0}, pools {[int(p) for p in spec.pools]}) gives {spec.dims[0]}")
    missing = [k for k in spec.unpack(np.zeros(spec.ns, np.float32)) if k not in named]
    if missing:
        raise ValueError(f"{path}: missing tensors {missing[:4]}")
    return spec
