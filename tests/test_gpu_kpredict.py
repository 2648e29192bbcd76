"""Prediction from saved SVR / KNR models (edgeml_amd.kpredict, csrc/kpredict.hip) on G7 / G8 (34 features;
folds of 237 / 242 / 241 training rows, none a multiple of the 16-wide tile) and on small synthetic models.

SVR is held to a derived gate (tests/kpredict_ref.svr_gate: the rounding bound on a kernel entry once for each
side, the reordering bound of the sum, the intercept add); nothing in it is fitted to what the device returns.
KNR is held to the fit bit for bit: the distances are the fit's chain per pair and the selection is its rule.
Every call here runs with canary elements behind est, nbr and the workspace, checked after the call.
"""
import os

import numpy as np
import pytest
import torch

from tests import kpredict_ref as K
from tests import regress_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
DEV = "cuda:0"
CANARY = -1234.5


def guarded(model, x, neighbors=False, chunk=None):
    """model.predict through predict_into, in calls of `chunk` rows, with canaries behind every output."""
    model.to(DEV)
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(len(x), -1))
    N, k = len(x), model.n_neighbors
    chunk = chunk or N
    est = np.empty(N)
    nbr = np.empty((N, k), np.int32) if neighbors else None
    for a in range(0, N, chunk):
        B = min(chunk, N - a)
        wb = model.workspace_bytes(B)
        ws = torch.full((wb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        g_est = torch.full((B + 8,), CANARY, dtype=torch.float64, device=DEV)
        g_nbr = torch.full((B + 2, k), -77, dtype=torch.int32, device=DEV) if neighbors else None
        model.predict_into(torch.from_numpy(x[a:a + B]).to(DEV), g_est[:B], ws[:wb],
                           g_nbr[:B] if neighbors else None)
        torch.cuda.synchronize()
        assert torch.all(g_est[B:] == CANARY) and torch.all(ws[wb:] == 0xA5), "a write past est or the workspace"
        est[a:a + B] = g_est[:B].cpu().numpy()
        if neighbors:
            assert torch.all(g_nbr[B:] == -77), "a write past nbr"
            nbr[a:a + B] = g_nbr[:B].cpu().numpy()
    return (est, nbr) if neighbors else est


@pytest.fixture(scope="module")
def g8():
    g = {}
    for name in ("g7_regressors.npz", "g8_svr.npz"):
        with np.load(os.path.join(HERE, "golden", name), allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files if name.startswith("g8") or k in ("features", "reward", "split")})
    g["folds"], g["D"] = len(g["split"]), g["features"].shape[1]
    assert g["D"] == 34 and [int((~m).sum()) for m in g["split"]] == [237, 242, 241]
    return g


def all_rows(g, results, f):
    est = np.empty(len(g["reward"]))
    est[~g["split"][f]], est[g["split"][f]] = results[f]["train_est"], results[f]["val_est"]
    return est


# -------------------------------------------------------------------------------------------- SVR
def test_svr_from_the_fixture_alone(g8):
    from edgeml_amd import kpredict
    x = g8["features"]
    for f, mask in enumerate(g8["split"]):
        tr = x[~mask]
        beta = g8[f"SVR/beta_cert{f}"]
        sv = np.nonzero(beta)[0]
        mean, scale = K.numpy_scaler(tr)
        m = {"model": "SVR", "mean": mean, "scale": scale, "gamma": float(g8[f"SVR/gamma{f}"]),
             "support": tr[sv].copy(), "beta": beta[sv].copy(), "intercept": float(g8[f"SVR/b_cert{f}"])}
        est = guarded(kpredict.load(m), x)
        want = g8[f"SVR/est_cert{f}"]
        gate, err = K.svr_gate(x, m, want), np.abs(est - want)
        print(f"fold {f}: {len(sv)} support vectors, max |est - est_cert| {err.max():.3e}, gate {gate.min():.3e} .. "
              f"{gate.max():.3e}, max err / gate {(err / gate).max():.4f}, spread of est {np.ptp(want):.3f}")
        assert len(est) == 360 and np.all(err <= gate)


@pytest.fixture(scope="module")
def svr_fit(g8):
    from edgeml_amd import svr
    return svr.fit_svr(g8["features"], g8["reward"], g8["split"])


def test_svr_against_the_fit(g8, svr_fit):
    from edgeml_amd import kpredict, svr
    results, info = svr_fit
    for f in range(g8["folds"]):
        m = svr.model_data("SVR", info, f, g8["features"])
        est = guarded(kpredict.load(m), g8["features"])
        want = all_rows(g8, results, f)
        gate, err = K.svr_gate(g8["features"], m, want), np.abs(est - want)
        print(f"fold {f}: {len(m['beta'])} support vectors, max |est - fit| {err.max():.3e}, max err / gate "
              f"{(err / gate).max():.4f}")
        assert np.all(err <= gate)
        # and against the restatement on the same file
        assert np.all(np.abs(est - K.svr_predict(g8["features"], m)) <= gate)


# -------------------------------------------------------------------------------------------- KNR
@pytest.mark.parametrize("k", [7, 1])
def test_knr_equals_the_fit_bit_for_bit(g8, k):
    """G7 holds identical rows (zero distances) and ties at the k-th place: equality covers them."""
    from edgeml_amd import kpredict, regress
    results, info = regress.fit_knr(g8["features"], g8["reward"], g8["split"], regress.KNROpt(n_neighbors=k))
    for f in range(g8["folds"]):
        m = regress.model_data("KNR", info, f, g8["features"], g8["reward"])
        assert m["train"].shape == (int((~g8["split"][f]).sum()), 34)
        est, nbr = guarded(kpredict.load(m), g8["features"], neighbors=True)
        assert np.array_equal(est, all_rows(g8, results, f)), f
        assert np.array_equal(nbr, info["neighbors"][f]), f
        # the call without nbr (the cascade's) selects into the workspace: the same estimates
        assert np.array_equal(guarded(kpredict.load(m), g8["features"]), est)


def test_knr_every_training_row_a_neighbour(g8):
    from edgeml_amd import kpredict, regress
    one = g8["split"][:1]
    n = int((~one[0]).sum())
    results, info = regress.fit_knr(g8["features"], g8["reward"], one, regress.KNROpt(n_neighbors=n))
    m = regress.model_data("KNR", info, 0, g8["features"], g8["reward"])
    est, nbr = guarded(kpredict.load(m), g8["features"], neighbors=True)
    assert np.array_equal(est, all_rows(g8, results, 0)) and np.array_equal(nbr, info["neighbors"][0])
    assert np.array_equal(nbr, np.broadcast_to(np.arange(n), (360, n)))
    assert np.all(est == R.sum_in_order(m["target"]) / n)


# ----------------------------------------------------------------------------------- independence
def synthetic(kind, n, D, seed, k=3):
    rng = np.random.default_rng(seed)
    mean, scale = rng.normal(0, 1, D), rng.uniform(0.5, 2, D)
    rows = mean + scale * rng.normal(0, 1, (n, D))
    if kind == "svr":
        return {"model": "SVR", "mean": mean, "scale": scale, "gamma": 1.0 / D, "support": rows,
                "beta": rng.uniform(-0.05, 0.05, n), "intercept": 0.375}
    return {"model": "KNR", "mean": mean, "scale": scale, "n_neighbors": min(k, n), "train": rows,
            "target": rng.normal(0, 1, n)}


def queries(m, B, seed):
    rng = np.random.default_rng(seed)
    return m["mean"] + m["scale"] * rng.normal(0, 1, (B, len(m["mean"])))


@pytest.mark.parametrize("kind", ["svr", "knr"])
def test_an_estimate_does_not_depend_on_its_batch(g8, kind):
    """37 rows at once, and in calls of 1, 5, 16, 17 and 32 rows in a permuted order."""
    from edgeml_amd import kpredict
    x = g8["features"][np.random.default_rng(3).permutation(360)[:37]]
    m = synthetic(kind, 83, 34, 21, k=7)
    m["support" if kind == "svr" else "train"][:] = g8["features"][100:183]  # real rows: duplicates and ties
    model = kpredict.load(m)
    once = torch.from_numpy(guarded(model, x))
    for chunk in (1, 5, 16, 17, 32):
        perm = np.random.default_rng(chunk).permutation(37)
        got = torch.from_numpy(guarded(model, x[perm], chunk=chunk))
        for j, i in enumerate(perm):
            assert torch.equal(got[j], once[i]), (chunk, j, i)
    assert np.array_equal(model.predict(x, chunk=9), once.numpy())  # the public route, its own chunks


# ------------------------------------------------------------------------------------------ edges
CASES = [(D, n, B) for D in (1, 34, 205) for n, B in ((1, 64), (15, 1), (16, 17), (17, 64))]


@pytest.mark.parametrize("D,n,B", CASES)
def test_svr_edges(D, n, B):
    from edgeml_amd import kpredict
    m = synthetic("svr", n, D, 1000 * D + n)
    x = queries(m, B, 7 * D + n)
    est = guarded(kpredict.load(m), x)
    want = K.svr_predict(x, m)
    gate = K.svr_gate(x, m, want)
    print(f"D {D} n {n} B {B}: max err / gate {(np.abs(est - want) / gate).max():.4f}, spread {np.ptp(want):.3e}")
    assert np.all(np.abs(est - want) <= gate)


@pytest.mark.parametrize("D,n,B", CASES)
def test_knr_edges(D, n, B):
    from edgeml_amd import kpredict
    m = synthetic("knr", n, D, 2000 * D + n)
    x = queries(m, B, 11 * D + n)
    x[0] = m["train"][n // 2]  # a query that is a training row: a zero distance
    est, nbr = guarded(kpredict.load(m), x, neighbors=True)
    K.check_knr(x, m, est, nbr)
    assert n // 2 in nbr[0]


@pytest.mark.parametrize("B", [1, 64])
def test_no_support_vector_gives_the_intercept(B):
    from edgeml_amd import kpredict
    m = synthetic("svr", 0, 34, 5)
    assert m["support"].shape == (0, 34)
    est = guarded(kpredict.load(m), queries(m, B, 9))
    assert est.shape == (B,) and np.all(est == 0.375)


def test_knr_4000_rows_500_neighbours():
    """More training rows than the selection's 256 threads, more neighbours than one pass of the target sum."""
    from edgeml_amd import kpredict
    m = synthetic("knr", 4000, 205, 77, k=500)
    x = queries(m, 3, 78)
    est, nbr = guarded(kpredict.load(m), x, neighbors=True)
    clear = K.check_knr(x, m, est, nbr)
    assert clear == 1.0  # random rows: no second distance within the band of the 500th


@pytest.mark.parametrize("n", [4096, 4097])
def test_knr_on_both_sides_of_the_register_held_keys(n):
    """Up to 4,096 training rows the selection keeps its keys in registers; past that it reads them again."""
    from edgeml_amd import kpredict
    m = synthetic("knr", n, 34, n, k=5)
    m["train"][n - 1] = m["train"][0]  # the last position ties with the first: the first is taken
    x = queries(m, 2, n + 1)
    x[1] = m["train"][0]
    est, nbr = guarded(kpredict.load(m), x, neighbors=True)
    K.check_knr(x, m, est, nbr)
    assert nbr[1, 0] == 0


# ------------------------------------------------------------------------------- flag and refusals
def test_offload_flag_is_strict():
    from edgeml_amd import ops
    thr = 0.3
    vals = np.array([thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf), -1.0, 2.0])
    est = torch.from_numpy(vals).to(DEV)
    flag = torch.full((len(vals) + 8,), 9, dtype=torch.uint8, device=DEV)
    ops.check(ops.lib().edgedet_offload_flag(ops._ptr(est), len(vals), thr, ops._ptr(flag), ops.stream_handle()))
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [0, 1, 0, 0, 1] + [9] * 8
    assert np.array_equal(est.cpu().numpy(), vals)  # only read


def test_refusals_launch_nothing():
    from edgeml_amd import kpredict, ops
    m = synthetic("knr", 20, 34, 1)
    model = kpredict.load(m).to(DEV)
    d, p, L = model._dev, ops._ptr, ops.lib()
    feat = torch.from_numpy(queries(m, 4, 2)).to(DEV)
    est = torch.full((4,), CANARY, dtype=torch.float64, device=DEV)
    wb = model.workspace_bytes(4)
    ws = torch.full((wb,), 0xA5, dtype=torch.uint8, device=DEV)
    st = ops.stream_handle()

    def knn(feat=feat, k=3, ws=ws, wb=wb, est=est):
        return L.edgedet_knn_model_predict(p(feat), 4, 34, p(d["mean"]), p(d["scale"]), p(d["z"]), p(d["norm"]),
                                           p(d["weight"]), 20, k, p(ws), wb, p(est), None, st)

    def svr(feat=feat, ws=ws, wb=wb, est=est):
        return L.edgedet_svr_model_predict(p(feat), 4, 34, p(d["mean"]), p(d["scale"]), p(d["z"]), p(d["norm"]),
                                           p(d["weight"]), 20, 0.1, 0.0, p(ws), wb, p(est), st)

    for rc in (knn(k=21), knn(k=0), knn(feat=None), knn(est=None), knn(ws=None), knn(wb=wb - 1), svr(feat=None),
               svr(ws=None), svr(wb=4 * 2 * 8 - 1), svr(est=None)):
        assert rc < 0 and L.edgedet_last_error()
    with pytest.raises(ops.EdgeDetError, match="workspace smaller"):
        model.predict_into(feat, est, ws[:wb - 8])
    torch.cuda.synchronize()
    assert torch.all(est == CANARY) and torch.all(ws == 0xA5)
    assert knn() == 0  # the same call, allowed
    torch.cuda.synchronize()
    assert not torch.any(est == CANARY)
