"""Host side of the offloading cascade (edgeml_amd.offload): the argument parser, the threshold rule of
test.py:35, the estimator-file loader and its refusals, the strong stage's batch queue as pure logic
against distributed.size_batches, and run_batches' unchanged default.  No device needed."""
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("edgedet_offload_rows", "edgedet_offload_features", "edgedet_offload_decide", "edgedet_offload_pack",
               "edgedet_offload_gather")


def test_parser_defaults_and_threshold_forms():
    from edgeml_amd import offload
    o = offload.getargs(["imgs", "out", "--estimator", "w/wts1.pickle", "--threshold", "0.25"])
    assert (o.img_dir, o.save_dir, o.estimator, o.threshold) == ("imgs", "out", "w/wts1.pickle", 0.25)
    assert (o.fold, o.k, o.dataset, o.weak, o.strong) == (1, 25, "coco", "ssd", "faster_rcnn")
    assert (o.weak_path, o.strong_path, o.weak_dir, o.weak_batch, o.strong_batch, o.decode) == ("", "", "", 0, 0, "gpu")
    assert o.ratio is None and o.estimates is None
    o = offload.getargs(["imgs", "out", "--estimator", "w.pth", "--ratio", "0.3", "--estimates", "est", "--fold", "2",
                         "--k", "3", "--dataset", "voc", "--strong-batch", "2", "--weak-dir", "wk", "--decode", "host"])
    assert (o.ratio, o.estimates, o.fold, o.k, o.dataset, o.strong_batch, o.weak_dir, o.decode) == \
        (0.3, "est", 2, 3, "voc", 2, "wk", "host")
    assert o.threshold is None
    for bad in (["imgs", "out", "--estimator", "w"],                                        # no threshold at all
                ["imgs", "out", "--estimator", "w", "--ratio", "0.3"],                      # ratio without estimates
                ["imgs", "out", "--estimator", "w", "--ratio", "0.3", "--estimates", "e", "--threshold", "1"],
                ["imgs", "out", "--estimator", "w", "--threshold", "1", "--estimates", "e"],
                ["imgs", "out", "--estimator", "w", "--ratio", "1.5", "--estimates", "e"],
                ["imgs", "out", "--threshold", "1"]):                                       # no estimator
        with pytest.raises(SystemExit):
            offload.getargs(bad)


def test_torchrun_world_is_refused(monkeypatch):
    from edgeml_amd import offload
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="sharding the cascade"):
        offload.main(offload.getargs(["imgs", "out", "--estimator", "w", "--threshold", "1"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_threshold_rule_is_test_py_35(tmp_path, dtype):
    from edgeml_amd import offload
    rng = np.random.default_rng(3)
    train = rng.normal(0, 1, 57).astype(dtype)
    train[5] = train[9]  # a tie
    np.savez(tmp_path / "estimate2.npz", train_est=train, val_est=train[:3], train_time=0.0, val_time=0.0)
    for ratio in (0.0, 0.1, 0.3, 0.5, 0.99, 1.0):
        # test.py:35 restated
        want = train[np.argsort(-train)[int((len(train) - 1) * ratio)]]
        got = offload.ratio_threshold(train, ratio)
        assert got == want and got.dtype == dtype
        o = offload.getargs(["i", "o", "--estimator", "w", "--ratio", str(ratio), "--estimates", str(tmp_path),
                             "--fold", "2"])
        t = offload.resolve_threshold(o)
        assert isinstance(t, float) and t == float(want)
        # the strict comparison in float64 equals the file route's comparison in the estimates' own type
        assert np.array_equal(train.astype(np.float64) > t, train > want)
    assert offload.ratio_threshold(train, 0.0) == train.max() and offload.ratio_threshold(train, 1.0) == train.min()
    o = offload.getargs(["i", "o", "--estimator", "w", "--threshold", "0.125"])
    assert offload.resolve_threshold(o) == 0.125


def _linear_file(path, D, model="LR"):
    rng = np.random.default_rng(D)
    m = {"model": model, "mean": rng.normal(0, 1, D), "scale": rng.uniform(0.5, 2, D), "coef": rng.normal(0, 1, D),
         "intercept": 0.375}
    if model == "KNR":
        del m["coef"], m["intercept"]
        m["n_neighbors"] = 5
    with open(path, "wb") as f:
        pickle.dump(m, f)
    return m


def test_loader_linear_and_refusals(tmp_path):
    from edgeml_amd import offload
    m = _linear_file(tmp_path / "wts1.pickle", 205)
    e = offload.load_estimator(str(tmp_path / "wts1.pickle"), 205)
    assert e.kind == "linear" and e.width == 205 and e.intercept == 0.375
    for k in ("mean", "scale", "coef"):
        assert getattr(e, k).dtype == np.float64 and np.array_equal(getattr(e, k), m[k])
    with pytest.raises(ValueError, match="takes 205 features, the cascade makes 95"):
        offload.load_estimator(str(tmp_path / "wts1.pickle"), 95)
    _linear_file(tmp_path / "wts2.pickle", 205, "KNR")
    with pytest.raises(ValueError, match="KNR file holds no training rows"):
        offload.load_estimator(str(tmp_path / "wts2.pickle"), 205)
    with open(tmp_path / "wts3.pickle", "wb") as f:
        pickle.dump({"something": 1}, f)
    with pytest.raises(ValueError, match="not a wts<fold>.pickle"):
        offload.load_estimator(str(tmp_path / "wts3.pickle"), 205)
    # the CLI refuses before it looks at the image directory (which does not exist)
    with pytest.raises(SystemExit, match="KNR"):
        offload.main(offload.getargs([str(tmp_path / "none"), str(tmp_path / "out"), "--estimator",
                                      str(tmp_path / "wts2.pickle"), "--threshold", "0"]))
    with pytest.raises(SystemExit, match="the cascade makes 95"):
        offload.main(offload.getargs([str(tmp_path / "none"), str(tmp_path / "out"), "--estimator",
                                      str(tmp_path / "wts1.pickle"), "--threshold", "0", "--k", "3"]))
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("dims", [[205, 16, 16, 16, 16, 1], [34, 16, 16, 1], [34, 1]])
def test_loader_reads_dims_from_pth(tmp_path, dims):
    from edgeml_amd import estimator, offload
    spec = estimator.MlpSpec(dims)
    state = spec.init_state(np.random.default_rng(1))
    state[spec.np:] = np.random.default_rng(2).uniform(0.5, 1.5, spec.ns - spec.np)  # running statistics
    estimator.save_state(str(tmp_path), spec, state, 0)
    named = torch.load(tmp_path / "wts1.pth", weights_only=True)
    assert set(named) == set(spec.unpack(state)) and all(v.dtype == torch.float32 for v in named.values())
    e = offload.load_estimator(str(tmp_path / "wts1.pth"), dims[0])
    assert e.kind == "mlp" and e.dims == dims and e.state.dtype == np.float32
    assert np.array_equal(e.state, state)
    with pytest.raises(ValueError, match=f"takes {dims[0]} features, the cascade makes 7"):
        offload.load_estimator(str(tmp_path / "wts1.pth"), 7)
    del named["linear_stacks.0.0.bias"]
    torch.save(named, tmp_path / "wts2.pth")
    with pytest.raises(ValueError, match="missing tensors"):
        offload.load_estimator(str(tmp_path / "wts2.pth"), dims[0])


def _queue_batches(sizes, flags, weak_batch, strong_batch):
    """The weak batches of size_batches(sizes, weak_batch) pushed through the queue, survivors by flag."""
    from edgeml_amd import offload
    from edgeml_amd.distributed import size_batches
    q = offload.BatchQueue(strong_batch)
    out = []
    for chunk in size_batches(sizes, weak_batch):
        ready = q.push(sizes[chunk[0]], [i for i in chunk if flags[i]])
        out += ready
    out += q.finish()
    assert q.finish() == []
    for size, b in out:
        assert 1 <= len(b) <= strong_batch and all(sizes[i] == size for i in b)
    return [b for _, b in out]


@pytest.mark.parametrize("weak_batch,strong_batch", [(4, 2), (4, 3), (3, 8), (64, 1), (5, 5)])
def test_queue_equals_size_batches_of_the_selected(weak_batch, strong_batch):
    from edgeml_amd.distributed import size_batches
    rng = np.random.default_rng(weak_batch * 10 + strong_batch)
    all_sizes = [(480, 640), (640, 480), (427, 640)]
    for trial in range(20):
        n = int(rng.integers(0, 40))
        sizes = [all_sizes[int(j)] for j in rng.integers(0, 3, n)]
        p = (0.0, 1.0, 0.3, 0.7)[trial % 4]
        flags = rng.random(n) < p
        got = _queue_batches(sizes, flags, weak_batch, strong_batch)
        sel = [i for i in range(n) if flags[i]]
        want = [[sel[j] for j in b] for b in size_batches([sizes[i] for i in sel], strong_batch)]
        # the same batches; their order is the weak size groups', not the selected images' first appearances
        assert sorted(map(tuple, got)) == sorted(map(tuple, want))


def test_queue_issue_example():
    """8 images of one size and 4 of another, weak batch 4, strong batch 2: 5 + 2 survivors."""
    sizes = [(480, 640)] * 8 + [(427, 640)] * 4
    flags = np.zeros(12, bool)
    flags[[0, 2, 3, 5, 7, 9, 10]] = True
    assert _queue_batches(sizes, flags, 4, 2) == [[0, 2], [3, 5], [7], [9, 10]]
    with pytest.raises(ValueError):
        from edgeml_amd import offload
        offload.BatchQueue(0)


def test_run_batches_keeps_post_none_as_default():
    from edgeml_amd import models
    sig = inspect.signature(models._Detector.run_batches)
    assert list(sig.parameters) == ["self", "batches", "inflight", "raw", "post"]
    assert sig.parameters["post"].default is None
    assert sig.parameters["raw"].default is False and sig.parameters["inflight"].default is None


def test_abi_declares_the_offload_exports():
    from edgeml_amd import ops
    with open(os.path.join(ROOT, "include", "edgedet.h")) as f:
        header = f.read()
    lib = ops.lib()
    for name in NEW_EXPORTS:
        assert name in ops.EXPORTS and f"int {name}(" in header and hasattr(lib, name)
