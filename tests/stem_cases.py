"""Seeded inputs and the record-level driver of the SSD stem exactness tests (tests/test_gpu_stem_exact.py)
and of their fixture (tests/golden/make_golden_stem.py, g10_stem_exact.npz): both must see the same bytes.

A case is (name, B, H, W, H0, W0): a [B][3][H0][W0] source image resized to H x W by the transform, stem
output [B][Ho][Wo][16].  run() drives edgedet_plan_run with a PREPROCESS record followed by the non-fused
SSD_STEM record on its NHWC4 output, and the fused SSD_STEM record on the source image, as
tests/test_gpu_kernels.py test_ssd_stem_folded_transform_bit_identical does."""
import ctypes
import hashlib

import numpy as np
import torch

DEV = "cuda"

CASES = [
    ("37x50_from_61x45", 3, 37, 50, 61, 45),      # down in one axis, up in the other, partial tiles on both edges
    ("33x31_from_480x640", 2, 33, 31, 480, 640),  # strong downscale, two tile rows
    ("2x3_from_5x4", 3, 2, 3, 5, 4),              # one tile, nearly all halo
    ("16x16_from_16x16", 2, 16, 16, 16, 16),      # scale 1
    ("320x320_from_640x640", 1, 320, 320, 640, 640),  # the workload's exact ratio 2
]
DIGEST_ONLY = {"320x320_from_640x640"}  # stored as a SHA-256 of the output bytes, not as an array
NORMS = {"ssd": [0.5] * 6, "imagenet": [0.485, 0.456, 0.406, 0.229, 0.224, 0.225]}


def inputs(case):
    """The uint8 source image and the six stem weight arrays (packed, on the host) of a case."""
    from edgeml_amd.plan import pack_conv_weight, pack_dw_weight
    name, B, H, W, H0, W0 = case
    g = torch.Generator().manual_seed(1000 * H + 10 * W + H0 + W0)
    img8 = torch.randint(0, 256, (B, 3, H0, W0), generator=g, dtype=torch.uint8)
    w0p, _, ld0, _ = pack_conv_weight((torch.randn(16, 3, 3, 3, generator=g) / 5).numpy(), 4)
    b0 = torch.randn(16, generator=g) * 0.1
    wd = pack_dw_weight((torch.randn(16, 1, 3, 3, generator=g) / 3).numpy())
    bd = torch.randn(16, generator=g) * 0.1
    w1p, _, ld1, _ = pack_conv_weight((torch.randn(16, 16, 1, 1, generator=g) / 4).numpy())
    b1 = torch.randn(16, generator=g) * 0.1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return img8, [t(w0p), b0, t(wd), bd, t(w1p), b1], ld0, ld1


def run(case, u8, norm):
    """(non-fused, fused) stem outputs of a case on the device, both NaN-filled beforehand."""
    from edgeml_amd import ops
    name, B, H, W, H0, W0 = case
    img8, wts, ld0, ld1 = inputs(case)
    src = (img8 if u8 else img8.float() / 255).to(DEV)
    wts = [w.to(DEV) for w in wts]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x4 = torch.full((B, H, W, 4), float("nan"), device=DEV)
    outs = [torch.full((B, Ho, Wo, 16), float("nan"), device=DEV) for _ in range(2)]
    rec = np.zeros(3, dtype=ops.OP_DTYPE)
    rec[0]["kind"] = ops.PREPROCESS
    rec[0]["i"][:7] = [B, H0, W0, H, W, H, W]
    rec[0]["p"][2 if u8 else 0] = src.data_ptr()
    rec[0]["p"][1] = x4.data_ptr()
    rec[0]["f"][:6] = NORMS[norm]
    for k, fused in ((1, False), (2, True)):
        rec[k]["kind"] = ops.SSD_STEM
        rec[k]["i"][:9] = [B, H, W, Ho, Wo, ld0, ld1, H0 if fused else 0, W0 if fused else 0]
        if fused:
            rec[k]["p"][9 if u8 else 8] = src.data_ptr()
            rec[k]["f"][:6] = NORMS[norm]
        else:
            rec[k]["p"][0] = x4.data_ptr()
        for j, t in enumerate(wts):
            rec[k]["p"][1 + j] = t.data_ptr()
        rec[k]["p"][7] = outs[k - 1].data_ptr()
    ops.check(ops.lib().edgedet_plan_run(rec.ctypes.data_as(ctypes.c_void_p), 3, ops.stream_handle()))
    torch.cuda.synchronize()
    return outs[0], outs[1]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
