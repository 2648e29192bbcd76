"""mlp_fit_kernel and mlp_predict_kernel (csrc/estimator.hip) against tests/mlp_ref.py Fit32, bit for bit.

Fit32 restates the kernel operation for operation in numpy float32 and tests/test_mlp_ref_host.py anchors it to torch
float64 autograd, so every comparison here is np.array_equal on the uint32 views: the whole best and last states (the
biases in front of a BatchNorm and the running means included), the per-epoch train and test losses and Adam's two
moments.  The kernels are called through the C ABI, so the Adam buffer is visible.

* one step (epochs 1, rows <= batch): m == 0.1f * g pins every gradient entry, `last` the update; five layouts (an
  ordinary one with fewer rows than its batch, row stride H = 64 against dout = 3 with n * dout > 256, no hidden layer,
  8 layers, 4096 units per layer) x dropout 0 / 0.1 / 0.5 x MSE / weighted (targets with 0 and negative values);
* short fits: three folds of 19 / 16 / 10 rows at batch 8 in one launch, 3 epochs, milestones [1, 2], weight decay,
  seed 0xFEDCBA9876543210; the fold key; a tie of test losses; p = 0.9 at width 3; a last batch of one row;
* predict: n = 0, 1, 256, 257, idx null or a permutation with repeats, and the fit's own test loss recomputed from it;
* the 160 KiB LDS boundary and a rerun into the same buffers.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mlp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _same(got, ref, what):
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero(_bits(got).ravel() != _bits(ref).ravel())[0]
    assert len(bad) == 0, (what, len(bad), "first at", int(bad[0]), float(got.ravel()[bad[0]]), float(ref.ravel()[bad[0]]))


class Launch:
    """The device buffers of one edgedet_mlp_fit call; run() launches and reads everything back."""

    def __init__(self, c):
        from edgeml_amd import ops
        self.c, spec, F = c, c.spec, c.folds
        self.spec = spec
        off = lambda parts: np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int64)  # noqa: E731
        self.g = {"x": _t(c.x), "y": _t(c.y), "tr": _t(np.concatenate(c.tr + [np.zeros(1, np.int32)])),
                  "tro": _t(off(c.tr)), "va": _t(np.concatenate(c.va + [np.zeros(1, np.int32)])), "vao": _t(off(c.va)),
                  "init": _t(c.init)}
        # garbage in every output: the kernel writes all of it (and zeroes the Adam scratch itself)
        self.out = {k: torch.full(shape, 7.25, dtype=torch.float32, device=DEV)
                    for k, shape in (("best", (F, spec.ns)), ("last", (F, spec.ns)), ("adam", (F, 2 * spec.np)),
                                     ("trl", (F, c.epochs)), ("tel", (F, c.epochs)))}
        self.dims = (ctypes.c_int32 * len(c.dims))(*c.dims)
        self.ms = (ctypes.c_int32 * max(1, len(c.milestones)))(*(list(c.milestones) or [0]))
        self.ops = ops

    def run(self):
        c, g, o, ops = self.c, self.g, self.out, self.ops
        p = ops._ptr
        rc = ops.lib().edgedet_mlp_fit(p(g["x"]), c.x.shape[0], c.dims[0], p(g["y"]), p(g["tr"]), p(g["tro"]), p(g["va"]),
                                       p(g["vao"]), c.folds, self.spec.L, self.dims, p(g["init"]), p(o["best"]),
                                       p(o["last"]), p(o["adam"]), p(o["trl"]), p(o["tel"]), c.epochs, c.batch, c.lr,
                                       c.gamma, self.ms, len(c.milestones), c.weight_decay, int(c.weighted), c.dropout,
                                       c.seed, ops.stream_handle())
        ops.check(rc)
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in o.items()}
        n = self.spec.np
        return {"best": r["best"], "last": r["last"], "m": r["adam"][:, :n], "v": r["adam"][:, n:],
                "train_loss": r["trl"], "test_loss": r["tel"]}


def device_fit(c):
    return Launch(c).run()


def check_fit(c, got=None, refs=None):
    """Every output of every fold against Fit32."""
    got = device_fit(c) if got is None else got
    refs = [R.Fit32(c).fit(f) for f in range(c.folds)] if refs is None else refs
    for f, ref in enumerate(refs):
        for k in ("train_loss", "test_loss", "m", "v", "last", "best"):
            _same(got[k][f], ref[k], (c.name, "fold", f, k))
    return got, refs


@functools.lru_cache(maxsize=None)
def _short(weighted):
    c = R.short_fit_case(weighted)
    return c, tuple(R.Fit32(c).fit(f) for f in range(c.folds))


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("case", R.one_step_cases(), ids=lambda c: c.name)
def test_one_step(case):
    """m = 0.1f * g after one step, so every gradient entry is compared, and `last` holds the update."""
    assert case.epochs == 1 and len(case.tr[0]) <= case.batch
    ref = R.Fit32(case).fit(0, trace=True)
    got, _ = check_fit(case, refs=[ref])
    assert len(ref["trace"]) == 1
    g = ref["trace"][0]["G"] + F32(case.weight_decay) * case.init[0, :case.spec.np]
    _same(got["m"][0], F32(0.1) * g, (case.name, "m == 0.1f * g"))


# ------------------------------------------------------------------------------------------------ short fits
@pytest.mark.parametrize("weighted", [False, True], ids=["mse", "w"])
def test_three_folds_three_epochs(weighted):
    """Full batches, partial ones of 3 and 2, the step counter carried across epochs, fold-keyed masks, the learning
    rate halved at epochs 1 and 2, weight decay, best selection."""
    c, refs = _short(weighted)
    check_fit(c, refs=list(refs))


def test_fold_key():
    """Fold 1's data as a launch of its own is fold 0 there: another mask stream, another fit."""
    c, refs = _short(False)
    alone = R.single_fold(c, 1)
    got, _ = check_fit(alone)
    assert not np.array_equal(_bits(got["last"][0]), _bits(refs[1]["last"]))


def test_equal_test_losses_keep_the_earlier_state():
    c = R.tie_case()
    got, refs = check_fit(c)
    assert refs[0]["best_epoch"] == 0 and got["test_loss"][0, 0] == got["test_loss"][0, 2]
    assert not np.array_equal(_bits(got["best"][0]), _bits(got["last"][0]))


def test_rows_that_lose_every_unit():
    check_fit(R.sparse_case())


def test_last_batch_of_one_row():
    """torch refuses BatchNorm1d on one row in train mode, so there is no float64 anchor for this step: the kernel's
    written rule (the biased variance, 0, for the running estimate) is pinned against Fit32 only."""
    c = R.one_row_case()
    assert len(c.tr[0]) % c.batch == 1
    check_fit(c)


def test_rerun_into_the_same_buffers():
    """The kernel zeroes the Adam scratch itself: the same call twice gives the same bits."""
    c, refs = _short(False)
    launch = Launch(c)
    a = launch.run()
    b = launch.run()
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    check_fit(c, got=b, refs=list(refs))


# ------------------------------------------------------------------------------------------------ predict
def device_predict(dims, x, state, idx, n, sentinel=-3.5):
    from edgeml_amd import ops
    g_x, g_s = _t(x), _t(state)
    g_idx = None if idx is None else _t(np.asarray(idx, np.int32))
    out = torch.full((max(n, 1) + 3,), sentinel, dtype=torch.float32, device=DEV)
    dims_host = (ctypes.c_int32 * len(dims))(*dims)
    ops.check(ops.lib().edgedet_mlp_predict(ops._ptr(g_x), dims[0], None if g_idx is None else ops._ptr(g_idx), n,
                                            len(dims) - 1, dims_host, ops._ptr(g_s), ops._ptr(out), ops.stream_handle()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[n:] == sentinel)  # nothing written past row n
    return out[:n]


@pytest.fixture(scope="module")
def predict_ref():
    dims, x, state = R.predict_case()
    c = R.Case("predict", dims, x, np.zeros((1, len(x)), F32), [np.zeros(0, np.int32)], [np.zeros(0, np.int32)],
               state[None], 8)
    ref = R.Fit32(c).predict(state, x)
    ref.setflags(write=False)
    return dims, x, state, ref


@pytest.mark.parametrize("n", [0, 1, 256, 257])
@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "idx"])
def test_predict_equals_the_eval_forward(predict_ref, n, indexed):
    dims, x, state, ref = predict_ref
    idx = None
    if indexed:  # a permutation with repeats
        idx = np.random.default_rng(n).permutation(len(x))[:max(n, 1)].astype(np.int32)
        idx[n // 2:n // 2 + 2] = idx[0]
    got = device_predict(dims, x, state, idx, n)
    _same(got, ref[:n] if idx is None else ref[idx[:n]], ("predict", n, indexed))
    assert n < 2 or len(np.unique(got)) > n // 2


@pytest.mark.parametrize("weighted", [False, True], ids=["mse", "w"])
def test_test_loss_is_the_loss_of_predict_on_the_best_state(weighted):
    """Ties the eval forward inside the fit (in LDS) to mlp_predict_kernel: the best epoch's test loss is the mean of
    the batch losses recomputed from the predict kernel's outputs on the best state."""
    c, refs = _short(weighted)
    got = device_fit(c)
    f32 = R.Fit32(c)
    for f in range(c.folds):
        ep = refs[f]["best_epoch"]
        assert ep == int(np.argmin(got["test_loss"][f]))
        pred = device_predict(c.dims, c.x, got["best"][f], c.va[f], len(c.va[f]))
        yv = c.y[f, c.va[f]]
        losses = [f32.loss(pred[b0:b0 + c.batch], yv[b0:b0 + c.batch]) for b0 in range(0, len(yv), c.batch)]
        s = F32(0)
        for v in losses:
            s = s + v
        _same(s / F32(len(losses)), got["test_loss"][f, ep], (c.name, f, "test loss from predict"))


# ------------------------------------------------------------------------------------------------ LDS boundary
def test_largest_layout_that_fits_the_lds():
    from edgeml_amd import ops
    d0 = R.lds_limit_d0()
    assert R.lds_floats([d0, 64, 1], 64) * 4 <= 160 * 1024 < R.lds_floats([d0 + 1, 64, 1], 64) * 4
    c = R.lds_case(d0)
    assert len(range(0, len(c.tr[0]), c.batch)) == 2
    check_fit(c)
    with pytest.raises(ops.EdgeDetError, match="LDS"):
        device_fit(R.lds_case(d0 + 1))
