"""The offloading cascade's device kernels (csrc/offload.hip) one by one, each against the code that
defines it at the parent commit, bit for bit:

* edgedet_offload_rows against fmt.format_batch (the G1 golden arrays, every COCO id, empty and
  all-dropped images, W != H, voc mode);
* edgedet_offload_features against features.output_features (k = 25 and k = 3);
* edgedet_offload_decide against edgedet_reg_predict / edgedet_mlp_predict and the strict comparison;
* edgedet_offload_pack / edgedet_offload_gather against tensor indexing, with nothing written past the
  packed images.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------- formatter
def _check_rows(boxes, scores, labels, counts, h, w, ds):
    from edgeml_amd import fmt, offload
    B, K = scores.shape
    want = fmt.format_batch(boxes, scores, labels, counts, h, w, ds)
    rows, nrow = offload.format_rows(_t(np.asarray(counts, np.int32)), _t(boxes), _t(scores), _t(labels), h, w, ds)
    torch.cuda.synchronize()
    rows, nrow = rows.cpu().numpy(), nrow.cpu().numpy()
    assert rows.dtype == np.float64 and rows.shape == (B, K, 6)
    for b in range(B):
        assert nrow[b] == len(want[b]), (b, nrow[b], len(want[b]))
        assert rows[b, :nrow[b]].tobytes() == want[b].tobytes(), (ds, b)
    return want


def test_rows_match_format_batch_on_g1():
    from edgeml_amd.labelmap import DROPPED
    with np.load(os.path.join(HERE, "golden", "g1_format.npz"), allow_pickle=False) as z:
        g1 = {k: z[k] for k in z.files}
    keys = sorted({k.rsplit("/", 1)[0] for k in g1 if "/" in k and k != "coco_to_yolov5"})
    assert len(keys) == 6
    rng = np.random.default_rng(0)
    seen = set()
    for key in keys:
        ds = key.split("/")[0]
        h, w = (int(v) for v in g1[key + "/hw"])
        n = len(g1[key + "/scores"])
        ids = np.arange(91) if ds == "coco" else np.arange(21)
        drop = np.array(DROPPED) if ds == "coco" else np.zeros(4, np.int64)
        K = max(n, len(ids)) + 7
        boxes = (rng.random((4, K, 4)) * 600).astype(np.float32)  # garbage past each count
        scores = rng.random((4, K)).astype(np.float32)
        labels = np.ones((4, K), np.int64)
        boxes[0, :n], scores[0, :n], labels[0, :n] = g1[key + "/boxes"].reshape(n, 4), g1[key + "/scores"], g1[key + "/labels"]
        labels[2, :len(ids)] = ids              # every id, the dropped ones among them
        labels[3, :len(drop)] = drop            # nothing survives
        counts = [n, 0, len(ids), len(drop)]
        want = _check_rows(boxes, scores, labels, counts, h, w, ds)
        assert len(want[1]) == 0 and len(want[3]) == 0
        assert len(want[2]) == (80 if ds == "coco" else 20)
        assert np.array_equal(want[2][:, 0], np.arange(len(want[2])))
        # image 0 is the reference's own file content (past the .npy header)
        assert g1[key + "/npy_bytes"].tobytes().endswith(want[0].tobytes())
        seen.add((ds, h != w))
    assert {d for d, _ in seen} == {"coco", "voc"}


@pytest.mark.parametrize("ds", ["coco", "voc"])
def test_rows_ragged_batch_wider_than_high(ds):
    """More rows than one 64-lane pass, counts 0 and K, W != H."""
    rng = np.random.default_rng(1)
    B, K = 9, 300
    boxes = (rng.random((B, K, 4)) * 600).astype(np.float32)
    scores = rng.random((B, K)).astype(np.float32)
    counts = rng.integers(0, K + 1, B)
    counts[:3] = (0, K, 65)
    labels = rng.integers(0, 91, (B, K)) if ds == "coco" else rng.integers(0, 21, (B, K))
    _check_rows(boxes, scores, labels.astype(np.int64), counts, 427, 640, ds)


# ---------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("k", [25, 3])
def test_features_match_output_features(k):
    from edgeml_amd import features, offload
    rng = np.random.default_rng(2)
    nc, K = 80, 48
    lens = [0, 2, 3, 10, 25, 26, 40, K]
    per_image = []
    for n in lens:
        r = np.column_stack([rng.integers(0, nc, n).astype(np.float64), rng.random((n, 5))]).reshape(n, 6)
        per_image.append(r)
    per_image[3][0, 0] = 85.0    # out of range: counted nowhere
    per_image[3][1, 0] = -3.0
    per_image[3][2, 0] = 7.9     # int() truncates to class 7
    per_image[6][30, 0] = 200.0  # beyond the top k rows
    want = features.output_features(per_image, nc, k, DEV)
    rows = rng.random((len(lens), K, 6)) + 100.0  # garbage past nrow must not show
    for b, r in enumerate(per_image):
        rows[b, :len(r)] = r
    got = offload.row_features(_t(rows), _t(np.array(lens, np.int32)), nc, k)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (len(lens), nc + 5 * k) == want.shape
    assert got.tobytes() == want.tobytes()
    assert not got[0].any() and got[3, 7] >= 1.0 and got[:, :nc].sum(1).max() <= k


# ---------------------------------------------------------------------------------------- decide
def _feat(B, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((B, D))
    x[:, :D // 3] = rng.poisson(1.0, (B, D // 3))
    x[1] = 0.0  # an image without detections
    return x


def _flags_at(est_fn, ref):
    """est_fn(threshold) -> (est, flag): the estimates never depend on the threshold and equal ref
    bit for bit; an estimate equal to the threshold is not offloaded, the next double above it is."""
    j = int(np.argsort(ref)[len(ref) // 2])
    t = float(ref[j])
    est, flag = est_fn(t)
    assert est.dtype == np.float64 and flag.dtype == np.uint8
    assert est.tobytes() == ref.tobytes()
    assert np.array_equal(flag, (ref > t).astype(np.uint8)) and flag[j] == 0 and 0 < flag.sum() < len(ref)
    below = float(np.nextafter(t, -np.inf))
    assert np.nextafter(below, np.inf) == ref[j]
    est, flag = est_fn(below)
    assert est.tobytes() == ref.tobytes()
    assert np.array_equal(flag, (ref > below).astype(np.uint8)) and flag[j] == 1
    est, flag = est_fn(float("inf"))
    assert not flag.any()
    est, flag = est_fn(float("-inf"))
    assert flag.all()


def _decide(e, x):
    B, D = x.shape
    g_x = _t(x)
    est = torch.zeros(B, dtype=torch.float64, device=DEV)
    flag = torch.full((B,), 7, dtype=torch.uint8, device=DEV)
    scratch = (torch.zeros((B, D), dtype=torch.float32, device=DEV), torch.zeros(B, dtype=torch.float32, device=DEV))

    def run(threshold):
        e.decide(g_x, threshold, est, flag, scratch)
        torch.cuda.synchronize()
        return est.cpu().numpy(), flag.cpu().numpy()
    return run


@pytest.mark.parametrize("D", [205, 34])
def test_decide_linear_equals_reg_predict(D):
    from edgeml_amd import offload, ops
    B = 37
    rng = np.random.default_rng(D)
    x = _feat(B, D, D)
    mean, scale, coef = rng.normal(0, 1, D), rng.uniform(0.5, 2.0, D), rng.normal(0, 1, D)
    icpt = 0.3125
    g = [_t(a) for a in (x, mean, scale, coef, np.array([icpt]))]
    out = torch.zeros(B, dtype=torch.float64, device=DEV)
    ops.check(ops.lib().edgedet_reg_predict(ops._ptr(g[0]), B, D, ops._ptr(g[1]), ops._ptr(g[2]), ops._ptr(g[3]),
                                            ops._ptr(g[4]), 1, ops._ptr(out), ops.stream_handle()))
    torch.cuda.synchronize()
    ref = out.cpu().numpy()
    np.testing.assert_allclose(ref, ((x - mean) / scale) @ coef + icpt, rtol=1e-10, atol=1e-10)
    e = offload.Estimator("linear", D, mean=mean, scale=scale, coef=coef, intercept=icpt)
    _flags_at(_decide(e, x), ref)


def test_decide_mlp_equals_mlp_predict():
    from edgeml_amd import estimator, offload, ops
    dims = [34, 16, 16, 1]
    B, D = 37, dims[0]
    spec = estimator.MlpSpec(dims)
    state = spec.init_state(np.random.default_rng(5))
    state[spec.np:] = np.random.default_rng(6).uniform(0.5, 1.5, spec.ns - spec.np)
    x = _feat(B, D, 9)
    g_x, g_s = _t(x.astype(np.float32)), _t(state)  # the cast estimator.fit_folds makes
    out = torch.zeros(B, dtype=torch.float32, device=DEV)
    dims_host = (ctypes.c_int32 * len(dims))(*dims)
    ops.check(ops.lib().edgedet_mlp_predict(ops._ptr(g_x), D, None, B, spec.L, dims_host, ops._ptr(g_s), ops._ptr(out),
                                            ops.stream_handle()))
    torch.cuda.synchronize()
    ref32 = out.cpu().numpy()
    assert len(np.unique(ref32)) > B // 2
    e = offload.Estimator("mlp", D, dims=dims, state=state)
    _flags_at(_decide(e, x), ref32.astype(np.float64))


# ---------------------------------------------------------------------------------------- pack / gather
PATTERNS = {"none": lambda B: np.zeros(B, bool), "all": lambda B: np.ones(B, bool),
            "alternating": lambda B: np.arange(B) % 2 == 0, "last": lambda B: np.arange(B) == B - 1}


@pytest.mark.parametrize("B,shape", [(5, (3, 7, 9)), (3, (3, 16, 16)), (2, (3, 160, 200))])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_pack_moves_flagged_images_to_the_front(B, shape, pattern):
    """3x7x9 = 189 bytes: image starts off the 16-byte grid and a byte tail; 3x16x16: all 16-byte
    copies; 3x160x200: several workgroups per image."""
    from edgeml_amd import offload
    rng = np.random.default_rng(B)
    src = rng.integers(0, 256, (B,) + shape, dtype=np.uint8)
    flags = PATTERNS[pattern](B)
    # 2 is as good as 1: any non-zero flag counts
    g_flag, g_src = _t(flags.astype(np.uint8) * 2), _t(src)
    dst = torch.full((B,) + shape, 0xAB, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    index = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    offload.pack(g_flag, g_src, dst, count, index)
    torch.cuda.synchronize()
    sel = np.nonzero(flags)[0]
    n = len(sel)
    assert int(count.item()) == n
    got, idx = dst.cpu().numpy(), index.cpu().numpy()
    assert np.array_equal(idx[:n], sel) and np.all(idx[n:] == -1)
    assert np.array_equal(got[:n], src[sel])
    assert np.all(got[n:] == 0xAB)  # nothing written past the last packed image
    assert np.array_equal(g_src.cpu().numpy(), src)


@pytest.mark.parametrize("shape", [(3, 7, 9), (3, 16, 16)])
def test_gather_two_sources_with_a_short_last_batch(shape):
    from edgeml_amd import offload
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (5,) + shape, dtype=np.uint8)
    b = rng.integers(0, 256, (3,) + shape, dtype=np.uint8)
    g = {"a": _t(a), "b": _t(b)}
    host = {"a": a, "b": b}
    pairs = [("a", 3), ("b", 0), ("b", 2), ("a", 0), ("a", 4)]
    Bs = 2
    batches = [pairs[s:s + Bs] for s in range(0, len(pairs), Bs)]
    assert [len(p) for p in batches] == [2, 2, 1]
    for p in batches:
        out = offload.gather([(g[s], j) for s, j in p])
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and tuple(out.shape) == (len(p),) + shape
        assert np.array_equal(out.cpu().numpy(), np.stack([host[s][j] for s, j in p]))
    # into a caller's larger buffer: the images past the batch stay as they were
    out = torch.full((4,) + shape, 0xAB, dtype=torch.uint8, device=DEV)
    offload.gather([(g["b"], 1)], out=out[:1])
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), b[1]) and bool((out[1:] == 0xAB).all())
    with pytest.raises(ValueError):
        offload.gather([(g["a"], 5)])
