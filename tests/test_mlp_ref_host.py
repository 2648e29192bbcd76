"""Anchors tests/mlp_ref.py Fit32 (the float32 restatement that tests/test_gpu_mlp_exact.py holds the device to, bit for
bit) to torch's semantics, on the CPU: "equal to Fit32" then means "equal to Linear / BatchNorm1d / ReLU / masked
dropout / the oracle's losses under autograd, within float32 rounding".

One training step of every one-step case of the device file (mlp_ref.one_step_cases) plus the shipped default layout:
per quantity (pred, loss, every gradient tensor, every running mean and variance)

    max |Fit32 - Fit64| <= 4 E,   E = max |torch32 - Fit64|.

Two classes of quantity may instead stand within a floor in float32 ulps of max |Fit64|, because their E is a maximum
over few draws and can be small by luck (mlp_ref.floor_class):
* one element (the loss, the last layer's bias gradient): FLOOR_ULPS["one"];
* at most 8 elements in a step of at most 8 rows (the width 3 to 5 tensors of the small layouts): FLOOR_ULPS["few"].
Each floor is the smallest power of two that covers twice the worst error of its class among the quantities above 4 E
(profiles/mlp_budget.txt: 31.5 and 10.9 ulps).  Every other quantity, every multi-element one of the 64-row layouts
among them, is held to plain 4 E.
"""
import os

import numpy as np
import pytest

from tests import mlp_ref as R
from tests.convnet_ref import hash_int

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR_ULPS = {"one": 64, "few": 32}


@pytest.mark.parametrize("case", R.anchor_cases(), ids=lambda c: c.name)
def test_fit32_step_within_the_float64_budget(case):
    rows, zero = R.measure(case)
    assert len(rows) == 2 + 2 * case.spec.L + 3 * (case.spec.L - 1)  # the hidden biases go to `zero`
    for name, size, ratio, E, ulps in rows:
        floor = FLOOR_ULPS.get(R.floor_class(case, size), 0)
        assert ratio <= 1.0 or ulps <= floor, (case.name, name, size, ratio, E, ulps, floor)
    for name, g32, bound in zero:
        assert np.all(g32 <= bound), (case.name, name, g32, bound)


def test_keep_numpy_equals_the_integer_form():
    """10^4 keys: folds and layers above 0, steps from 2^12 up, a seed of at least 2^63; and the key spelled out."""
    rng = np.random.default_rng(0)
    n = 0
    for seed in (0, 5, R.SEED, 2 ** 63, 2 ** 64 - 1):
        for fold in (0, 1, 4):
            for layer in (0, 3, 6):
                for step in (0, 1, 2 ** 12, 2 ** 12 + 77, 2 ** 20 + 3):
                    units = np.concatenate([[0, 1, 4095], rng.integers(0, 4096, 42)])
                    for p in (0.1, 0.5, 0.9)[n % 3:n % 3 + 1]:
                        got = R.keep(seed, fold, step, layer, units, p)
                        assert list(got) == [R.keep_int(seed, fold, step, layer, int(u), p) for u in units]
                        n += len(units)
    assert n >= 10 ** 4
    # the key itself, spelled out: a = seed ^ fold << 48, b = step << 20 ^ layer << 16 ^ unit
    a, b = R.mlp_key(R.SEED, 2, 4097, 5, 300)
    assert a == 0xFEDCBA9876543210 ^ (2 << 48) and b == (4097 << 20) ^ (5 << 16) ^ 300
    h = hash_int(a, b)
    assert R.keep_int(R.SEED, 2, 4097, 5, 300, 0.5) == ((h >> 8) >= 2 ** 23)
    assert bool(np.all(R.keep(1, 0, 0, 0, np.arange(1000), 0.0)))  # u >= 0 always: p = 0 keeps everything
    # every field of the key matters
    base = R.keep(R.SEED, 1, 3, 2, np.arange(4096), 0.5)
    for other in ((R.SEED ^ 1, 1, 3, 2), (R.SEED, 0, 3, 2), (R.SEED, 1, 4, 2), (R.SEED, 1, 3, 1)):
        assert not np.array_equal(base, R.keep(*other, np.arange(4096), 0.5)), other


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_fraction(p):
    n = 2 ** 16
    frac = R.keep(R.SEED, 1, 7, 2, np.arange(n), p).mean()
    assert abs(frac - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), (p, frac)


def test_every_dropout_case_drops_and_keeps_in_every_hidden_layer():
    """Otherwise a device case would not pin the mask's indexing."""
    cases = R.dropout_cases()
    assert len(cases) == 2 * 2 * len(R.LAYOUTS) + 7
    for c in cases:
        census = R.mask_census(c)
        if len(c.dims) > 2:
            assert len(census) == c.folds * (len(c.dims) - 2)
        for key, (kept, dropped) in census.items():
            assert kept > 0 and dropped > 0, (c.name, key, kept, dropped)
    # the sparse case: some row loses every unit of a layer, some row keeps one
    c = R.sparse_case()
    m = R.layer_mask(c.seed, 0, 0, 0, c.batch, c.dims[1], c.dropout)
    assert (~m).all(1).any() and m.any()


def test_fold_key_changes_the_fit():
    """Fold 1 of the three-fold launch against the same data run as fold 0 of its own launch."""
    c = R.short_fit_case(False)
    a, b = R.Fit32(c).fit(1), R.Fit32(R.single_fold(c, 1)).fit(0)
    assert not np.array_equal(a["last"], b["last"]) and not np.array_equal(a["train_loss"], b["train_loss"])


def test_short_fit_covers_what_it_claims():
    c = R.short_fit_case(True)
    assert [len(t) % c.batch for t in c.tr] == [3, 0, 2] and c.seed >= 2 ** 63
    assert all((c.y[f, c.tr[f]] == 0).any() and (c.y[f, c.tr[f]] < 0).any() for f in range(c.folds))
    for w in (False, True):
        fits = [R.Fit32(R.short_fit_case(w)).fit(f) for f in range(3)]
        assert len({f["best_epoch"] for f in fits}) > 1 or any(f["best_epoch"] < 2 for f in fits)
    t = R.tie_case()
    r = R.Fit32(t).fit(0, trace=True)
    assert r["test_loss"][0] == r["test_loss"][1] == r["test_loss"][2] and r["best_epoch"] == 0
    assert not np.array_equal(r["best"], r["last"])  # the running statistics moved on
    assert np.array_equal(r["best"][:t.spec.np], t.init[0, :t.spec.np])
    d0 = R.lds_limit_d0()
    assert R.lds_floats([d0, 64, 1], 64) * 4 <= 160 * 1024 < R.lds_floats([d0 + 1, 64, 1], 64) * 4 and d0 == 119


def test_bias_correction_precondition_has_teeth():
    """bias_corrections refuses a step whose float32 result hangs on the last bit of the power."""
    for step in (1, 2, 3):
        R.bias_corrections(float(np.float32(R.LR)), step)
    with pytest.raises(AssertionError, match="one ulp"):  # CNNOpt's default sits on a tie at its first step
        R.bias_corrections(float(np.float32(5e-3)), 1)
    R.bias_corrections(float(np.float32(5e-3)), 1, strict=False)
    import math
    # a learning rate built so that lr / bc1 at step 2 sits on a float32 rounding boundary
    bc1 = 1.0 - math.pow(0.9, 2.0)
    mid = (float(np.float32(1.0)) + float(np.nextafter(np.float32(1.0), np.float32(2.0)))) / 2
    with pytest.raises(AssertionError, match="one ulp"):
        R.bias_corrections(mid * bc1, 2)


@pytest.mark.parametrize("case", ["mse", "weighted"])
def test_fit32_reproduces_the_reference_fit(case):
    """Fit32, dropout off, from the reference's own initial weights (tests/golden/g4_estimator.npz) ends at the
    reference's recorded estimates within the tolerance of test_gpu_estimator.py's test on the same file: the new
    reference joins the old one."""
    from edgeml_amd import estimator
    with np.load(os.path.join(HERE, "golden", "g4_estimator.npz"), allow_pickle=False) as z:
        g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "/")}
    ntr, nva, weight, epochs, batch = (int(v) for v in g["cfg"])
    dims = [int(v) for v in g["linear"]]
    spec = estimator.MlpSpec(dims)
    init = spec.pack({k[5:]: v for k, v in g.items() if k.startswith("init/")})
    idx = np.arange(ntr + nva, dtype=np.int32)
    c = R.Case("g4-" + case, dims, g["x"].astype(np.float32), g["y"].astype(np.float32)[None], [idx[:ntr]], [idx[ntr:]],
               init[None], batch, epochs=epochs, lr=5e-3, milestones=[int(m) for m in g["milestones"]],
               weighted=bool(weight),
               dropout=0.0)
    f = R.Fit32(c, strict_pow=False)  # the reference ran at lr 5e-3; a tolerance does not hang on pow's last bit
    r = f.fit(0)
    tol = 0.02 * float(np.std(g["y"]))
    for tag in ("best", "last"):
        for k, rows in (("train_est", idx[:ntr]), ("val_est", idx[ntr:])):
            d = float(np.abs(f.predict(r[tag], c.x[rows]).astype(np.float64) - g[f"{tag}/{k}"]).max())
            assert d <= tol, (case, tag, k, d, tol)
