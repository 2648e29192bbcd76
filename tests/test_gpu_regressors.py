"""The four estimator regressors of edgeml_amd.regress (csrc/regress.hip) against G7 (tests/golden/
g7_regressors.npz: regression.py's own LR / EN / BR / KNR runs under sklearn 1.7.2, and the quantities the
bounds below are derived from; tests/golden/make_golden_regressors.py).  No bound here is fitted to what the
device returns: each comes from the reference's own error, from a rounding bound, or from the objective's
strong convexity.  Where the fixture stores one spread per fold, the gate uses the largest of the three: the
spread is a property of the two methods, the folds are three samples of it.
"""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import regress_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
SLACK = 64.0  # x the reference's own figure: room for another rotation / summation order


@pytest.fixture(scope="module")
def g7():
    with np.load(os.path.join(HERE, "golden", "g7_regressors.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["folds"] = len(g["split"])
    g["D"] = g["features"].shape[1]
    ref = []
    for f, m in enumerate(g["split"]):  # the restatement, once
        tr = ~m
        mean, scale, const = R.scaler(g["features"][tr])
        zr = R.standardise(g["features"], mean, scale)
        y = g["reward"][tr]
        # sklearn's own standardised, centred training matrix (its transform divides by the scale)
        zs = (g["features"] - g[f"scaler/mean{f}"]) / g[f"scaler/scale{f}"]
        zc = zs[tr] - zs[tr].mean(0)
        ref.append({"tr": tr, "n": int(tr.sum()), "mean": mean, "scale": scale, "const": const, "z": zr, "y": y,
                    "yc": y - y.mean(), "zs": zs, "zc": zc})
    g["ref"] = ref
    return g


def spread(g, key):
    return max(float(g[f"{key}{f}"]) for f in range(g["folds"]))


@pytest.fixture(scope="module")
def fits(g7):
    """Every model fitted once on all folds; shared, never modified."""
    from edgeml_amd import regress
    out = {}
    for name, opts in (("LR", None), ("EN", None), ("BR", None), ("KNR", regress.KNROpt(n_neighbors=int(g7["n_neighbors"])))):
        out[name] = regress.FITS[name](g7["features"], g7["reward"], g7["split"], opts)
    return out


def all_rows(g, results, f):
    est = np.empty(len(g["reward"]))
    est[~g["split"][f]], est[g["split"][f]] = results[f]["train_est"], results[f]["val_est"]
    return est


@pytest.fixture(scope="module")
def dev(g7):
    """The scaler, Gram and eigensolver outputs of all folds through the library's own calls."""
    import torch
    from edgeml_amd import regress
    fo = regress._Folds(g7["features"], g7["reward"], g7["split"], "cuda").upload()
    G = fo.gram()
    lam, vt, einfo = fo.eigh(G)
    torch.cuda.synchronize()
    return {"fo": fo, "mean": fo.mean.cpu().numpy(), "scale": fo.scale.cpu().numpy(), "ymean": fo.ymean.cpu().numpy(),
            "G": G.cpu().numpy(), "lam": lam.cpu().numpy(), "vt": vt.cpu().numpy(), "einfo": einfo}


# ------------------------------------------------------------------------------------ scaler and Gram
def test_scaler_equals_the_restatement(g7, dev):
    for f, r in enumerate(g7["ref"]):
        np.testing.assert_array_equal(dev["mean"][f], r["mean"])
        np.testing.assert_array_equal(dev["scale"][f], r["scale"])
        assert abs(dev["ymean"][f] - r["y"].mean()) <= r["n"] * EPS * np.abs(r["y"]).max()  # two summation orders
        # the all-zero column (class 3) and the column constant at 0.1 (the first box's width)
        nc = int(g7["num_class"])
        assert dev["scale"][f][nc - 1] == 1.0 and dev["scale"][f][nc + 2] == 1.0
        assert np.all(g7["features"][:, nc - 1] == 0) and np.all(g7["features"][:, nc + 2] == 0.1)
        assert int(np.sum(dev["scale"][f] == 1.0)) == 2


def gram_bound(za):
    """|fl(a.b) - a.b| <= n eps |a| |b| for the columns a, b of the augmented matrix."""
    c = np.linalg.norm(za, axis=0)
    return len(za) * EPS * np.outer(c, c)


def test_unit_gram_against_numpy(g7, dev):
    """edgedet_reg_gram as a unit operator (one matrix, rows 0..n, no index list)."""
    import torch
    from edgeml_amd import ops
    r, D = g7["ref"][1], g7["D"]
    x = np.ascontiguousarray(g7["features"][r["tr"]])
    n, Dp = len(x), (D + 1 + 15) // 16 * 16
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g_x, g_y, g_off = t(x), t(r["y"]), t(np.array([0, n], np.int64))
    g_mean, g_scale, g_ym = t(r["mean"]), t(r["scale"]), t(np.array([r["y"].mean()]))
    G = torch.full((Dp, Dp), np.nan, dtype=torch.float64, device="cuda")
    off_host = (ctypes.c_int64 * 2)(0, n)
    ops.check(ops.lib().edgedet_reg_gram(ops._ptr(g_x), n, D, ops._ptr(g_y), None, off_host, ops._ptr(g_off), 1,
                                         ops._ptr(g_mean), ops._ptr(g_scale), ops._ptr(g_ym), ops._ptr(G),
                                         ops.stream_handle()))
    G = G.cpu().numpy()
    za = np.concatenate([R.standardise(x, r["mean"], r["scale"]), (r["y"] - r["y"].mean())[:, None]], 1)
    want = za.T @ za
    err = np.abs(G[:D + 1, :D + 1] - want)
    bound = gram_bound(za)
    print("unit gram: max err", err.max(), "max err / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    assert np.array_equal(G, G.T)
    assert np.all(G[D + 1:] == 0) and np.all(G[:, D + 1:] == 0)  # the padding columns


def test_fold_gram_against_numpy(g7, dev):
    D = g7["D"]
    for f, r in enumerate(g7["ref"]):
        za = np.concatenate([r["z"][r["tr"]], (r["y"] - dev["ymean"][f])[:, None]], 1)
        G = dev["G"][f]
        assert np.all(np.abs(G[:D + 1, :D + 1] - za.T @ za) <= gram_bound(za))
        assert np.array_equal(G, G.T)


# ------------------------------------------------------------------------------------ eigensolver
def test_eigh_residuals_within_64x_numpys(g7, dev):
    D = g7["D"]
    recon_ref, orth_ref = spread(g7, "eigh/recon"), spread(g7, "eigh/orth")
    for f in range(g7["folds"]):
        G, lam, V = dev["G"][f][:D, :D], dev["lam"][f], dev["vt"][f].T
        recon = np.linalg.norm((V * lam) @ V.T - G)
        orth = np.linalg.norm(V.T @ V - np.eye(D))
        print(f"fold {f}: |V diag(lam) V^T - G| {recon:.3e} (numpy eigh {recon_ref:.3e}), |V^T V - I| {orth:.3e} "
              f"(numpy eigh {orth_ref:.3e}), sweeps {dev['einfo']['eigh_sweeps'][f]}, off-diagonal norm "
              f"{dev['einfo']['eigh_offnorm'][f]}")
        assert recon <= SLACK * recon_ref and orth <= SLACK * orth_ref
        assert np.all(lam >= 0)
        off, thresh = dev["einfo"]["eigh_offnorm"][f]
        assert off <= thresh and thresh == pytest.approx(D * EPS * np.linalg.norm(G), rel=1e-12)


# --------------------------------------------------------------------------------------------- LR
def test_lr(g7, fits):
    results, info = fits["LR"]
    for f, r in enumerate(g7["ref"]):
        coef = info["coef"][f]
        assert int(info["rank"][f]) == int(g7[f"LR/rank{f}"])
        assert info["min_ratio"][f] > 1e-6 > info["tau"]  # the kept spectrum is well clear of the cut
        null_dev = np.abs(g7[f"LR/null{f}"].T @ coef).max()
        g_dev = np.linalg.norm(r["zc"].T @ (r["zc"] @ coef - r["yc"]))
        g_ref, g_gram = float(g7[f"LR/g_ref{f}"]), float(g7[f"LR/g_gram{f}"])
        diff = np.abs(all_rows(g7, results, f) - g7[f"LR/est_ref{f}"]).max()
        bound = (g_dev + g_ref) / float(g7[f"LR/sigma_min{f}"])
        print(f"fold {f}: |n^T coef| {null_dev:.3e} (ref {spread(g7, 'LR/null_ref'):.3e}), |g_dev| {g_dev:.3e} "
              f"(ref {g_ref:.3e}, gram {g_gram:.3e}), max |est - ref| {diff:.3e} (bound {bound:.3e})")
        assert null_dev <= SLACK * spread(g7, "LR/null_ref")
        assert g_dev <= SLACK * max(g_ref, g_gram)
        assert diff <= bound
        assert abs(info["intercept"][f] - r["y"].mean()) <= r["n"] * EPS * np.abs(r["y"]).max()


# --------------------------------------------------------------------------------------------- BR
def test_br(g7, fits):
    results, info = fits["BR"]
    for f in range(g7["folds"]):
        assert int(info["n_iter"][f]) == int(g7[f"BR/n_iter{f}"])
        da = abs(info["alpha"][f] - float(g7[f"BR/alpha{f}"])) / float(g7[f"BR/alpha{f}"])
        dl = abs(info["lambda"][f] - float(g7[f"BR/lambda{f}"])) / float(g7[f"BR/lambda{f}"])
        de = np.abs(all_rows(g7, results, f) - g7[f"BR/est_ref{f}"]).max()
        print(f"fold {f}: alpha rel {da:.3e} (spread {spread(g7, 'BR/alpha_spread'):.3e}), lambda rel {dl:.3e} "
              f"(spread {spread(g7, 'BR/lambda_spread'):.3e}), est {de:.3e} (spread {spread(g7, 'BR/est_spread'):.3e})")
        assert da <= SLACK * spread(g7, "BR/alpha_spread")
        assert dl <= SLACK * spread(g7, "BR/lambda_spread")
        assert de <= SLACK * spread(g7, "BR/est_spread")


# --------------------------------------------------------------------------------------------- EN
def test_en(g7, fits):
    results, info = fits["EN"]
    mu = 0.01 * (1 - 0.5)  # the objective's strong convexity
    assert np.all(info["status"] == 0)
    for f, r in enumerate(g7["ref"]):
        n, D, w = r["n"], g7["D"], info["coef"][f]
        z_tr = r["z"][r["tr"]]
        Q, q = z_tr.T @ z_tr / n, z_tr.T @ r["yc"] / n
        tol = 1e-10 * np.abs(q).max()
        assert info["tol"][f] == pytest.approx(tol, rel=1e-9)
        assert info["znorm"][f] <= info["tol"][f]
        # the host's recomputation: two float64 evaluations of g = Q w - q differ by at most twice the
        # dot-product bound n eps (|w|_1 + |yc| / sqrt(n)) per component (standardised columns have norm sqrt(n))
        z_host = R.en_residual(Q, q, w)
        agree = 2 * np.sqrt(D) * n * EPS * (np.abs(w).sum() + np.linalg.norm(r["yc"]) / np.sqrt(n))
        print(f"fold {f}: |z| device {info['znorm'][f]:.3e}, host {z_host:.3e}, tol {tol:.3e}, sweeps "
              f"{info['sweeps'][f]}, agreement bound {agree:.3e}")
        assert abs(z_host - info["znorm"][f]) <= agree
        assert np.any(w == 0) and np.any(w != 0)
        est = all_rows(g7, results, f)
        rows = np.linalg.norm(r["z"], axis=1)
        for ref_est, z_ref in ((g7[f"EN/est_hi{f}"], float(g7[f"EN/z_hi{f}"])),
                               (g7[f"EN/est_ref{f}"], float(g7[f"EN/z_default{f}"]))):
            bound = rows * (info["znorm"][f] + z_ref) / mu
            print(f"   max |est - ref| {np.abs(est - ref_est).max():.3e}, min bound {bound.min():.3e}")
            assert np.all(np.abs(est - ref_est) <= bound)


# -------------------------------------------------------------------------------------------- KNR
def knr_exact(g7, f, k):
    r = g7["ref"][f]
    d2 = R.sqdist_direct(r["z"], r["z"][r["tr"]])
    nbr, est, dk = R.knr_exact(d2, r["y"], k)
    return d2, nbr, est, dk, R.knr_band(r["z"], r["z"][r["tr"]], g7["D"])


def test_knr(g7, fits):
    results, info = fits["KNR"]
    k = int(g7["n_neighbors"])
    straddles = 0
    for f, r in enumerate(g7["ref"]):
        d2, nbr_x, est_x, dk, beta = knr_exact(g7, f, k)
        nbr, est = info["neighbors"][f], all_rows(g7, results, f)
        inband = (np.abs(d2 - dk[:, None]) <= beta[:, None]).sum(1) > 1
        assert np.array_equal(inband, g7[f"KNR/inband{f}"]) and inband.mean() <= 0.10
        assert np.all(np.diff(nbr, axis=1) > 0) and nbr.min() >= 0 and nbr.max() < r["n"]
        ymax = np.abs(r["y"]).max()
        for i in range(len(est)):
            assert est[i] == R.sum_in_order(r["y"][nbr[i]]) / k  # the mean over the returned set, in order
            if not inband[i]:
                assert np.array_equal(nbr[i], nbr_x[i]), (f, i)
                assert abs(est[i] - g7[f"KNR/est_ref{f}"][i]) <= 2 * k * EPS * ymax
            else:
                closer = np.nonzero(d2[i] < dk[i] - beta[i])[0]
                assert np.all(np.isin(closer, nbr[i])) and np.all(d2[i][nbr[i]] <= dk[i] + beta[i]), (f, i)
        # an identical pair of training rows straddling the k-th place: the lower position is returned
        srt = np.argsort(d2, axis=1, kind="stable")
        for i in np.nonzero(np.take_along_axis(d2, srt[:, k - 1:k], 1) == np.take_along_axis(d2, srt[:, k:k + 1], 1))[0]:
            lo, hi = sorted((int(srt[i, k - 1]), int(srt[i, k])))
            if np.array_equal(r["z"][r["tr"]][lo], r["z"][r["tr"]][hi]) and np.sum(d2[i] == dk[i]) == 2:
                assert lo in nbr[i] and hi not in nbr[i], (f, i)
                straddles += 1
    assert straddles >= 1


def test_knr_k_limits(g7):
    from edgeml_amd import regress
    one = g7["split"][:1]
    r = g7["ref"][0]
    results, info = regress.fit_knr(g7["features"], g7["reward"], one, regress.KNROpt(n_neighbors=r["n"]))
    assert np.array_equal(info["neighbors"][0], np.broadcast_to(np.arange(r["n"]), (len(g7["reward"]), r["n"])))
    want = R.sum_in_order(r["y"]) / r["n"]
    assert np.all(results[0]["train_est"] == want) and np.all(results[0]["val_est"] == want)
    results, info = regress.fit_knr(g7["features"], g7["reward"], one, regress.KNROpt(n_neighbors=1))
    d2, nbr_x, est_x, dk, beta = knr_exact(g7, 0, 1)
    nb = info["neighbors"][0][:, 0]
    assert np.all(d2[np.arange(len(nb)), nb] <= dk + beta)
    np.testing.assert_array_equal(all_rows(g7, results, 0), r["y"][nb])
    # a training row's nearest neighbour is itself or an identical row at a lower position
    pos = np.cumsum(r["tr"]) - 1
    for i in np.nonzero(r["tr"])[0]:
        assert nb[i] <= pos[i] and np.array_equal(r["z"][r["tr"]][nb[i]], r["z"][i])
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit"):
        regress.fit_knr(g7["features"], g7["reward"], g7["split"], regress.KNROpt(n_neighbors=r["n"] + 1))


def test_knr_more_training_rows_than_selection_threads(g7):
    """340 training rows: every thread of the 256-wide selection scans more than one position."""
    from edgeml_amd import regress
    k = int(g7["n_neighbors"])
    one = np.zeros((1, len(g7["reward"])), bool)
    one[0, ::18] = True
    tr = ~one[0]
    assert tr.sum() > 256
    mean, scale, _ = R.scaler(g7["features"][tr])
    z, y = R.standardise(g7["features"], mean, scale), g7["reward"][tr]
    results, info = regress.fit_knr(g7["features"], g7["reward"], one, regress.KNROpt(n_neighbors=k))
    d2 = R.sqdist_direct(z, z[tr])
    nbr_x, est_x, dk = R.knr_exact(d2, y, k)
    beta = R.knr_band(z, z[tr], g7["D"])
    clear = (np.abs(d2 - dk[:, None]) <= beta[:, None]).sum(1) == 1
    assert clear.mean() >= 0.9
    nbr = info["neighbors"][0]
    np.testing.assert_array_equal(nbr[clear], nbr_x[clear])
    est = np.empty(len(tr))
    est[tr], est[~tr] = results[0]["train_est"], results[0]["val_est"]
    np.testing.assert_array_equal(est, [R.sum_in_order(y[nb]) / k for nb in nbr])


def test_lr_odd_width_pads_the_jacobi_order(g7):
    """D = 33: the eigensolver runs at order 34 with a zero row and column.  Against the numpy restatement on
    the same Gram route: the same rank, and a normal-equation residual within 64x the restatement's."""
    from edgeml_amd import regress
    x = g7["features"][:, :33]
    results, info = regress.fit_lr(x, g7["reward"], g7["split"])
    for f, m in enumerate(g7["split"]):
        tr = ~m
        mean, scale, _ = R.scaler(x[tr])
        z, y = R.standardise(x, mean, scale), g7["reward"][tr]
        G = R.gram(z[tr], y - y.mean())
        coef, rank, ratio = R.lr_from_gram(G)
        assert int(info["rank"][f]) == rank == 30
        g_np = np.linalg.norm(G[:33, :33] @ coef - G[:33, 33])
        g_dev = np.linalg.norm(G[:33, :33] @ info["coef"][f] - G[:33, 33])
        sigma_min = np.sqrt(ratio * np.linalg.eigvalsh(G[:33, :33]).max())
        diff = np.abs(all_rows(g7, results, f) - (z @ coef + y.mean())).max()
        print(f"fold {f}: |g_dev| {g_dev:.3e}, |g_numpy| {g_np:.3e}, max |est - restatement| {diff:.3e}")
        assert g_dev <= SLACK * g_np
        assert diff <= (g_dev + g_np) / sigma_min


# ------------------------------------------------------------------------ determinism and batching
def _flat(results, info):
    keys = sorted(k for k in info if k not in ("fit_time",) and isinstance(info[k], np.ndarray))
    return [r[p] for r in results for p in ("train_est", "val_est")], keys, [info[k] for k in keys]


@pytest.mark.parametrize("name", ["LR", "EN", "BR", "KNR"])
def test_folds_together_equal_one_at_a_time_and_reruns(g7, fits, name):
    from edgeml_amd import regress
    opts = regress.KNROpt(n_neighbors=int(g7["n_neighbors"])) if name == "KNR" else None
    est, keys, arrs = _flat(*fits[name])
    est2, keys2, arrs2 = _flat(*regress.FITS[name](g7["features"], g7["reward"], g7["split"], opts))
    assert keys == keys2
    for a, b in zip(est + arrs, est2 + arrs2):
        np.testing.assert_array_equal(a, b)
    for f in range(g7["folds"]):
        res1, info1 = regress.FITS[name](g7["features"], g7["reward"], g7["split"][f:f + 1], opts)
        np.testing.assert_array_equal(res1[0]["train_est"], fits[name][0][f]["train_est"])
        np.testing.assert_array_equal(res1[0]["val_est"], fits[name][0][f]["val_est"])
        for k_ in keys:
            np.testing.assert_array_equal(info1[k_][0], fits[name][1][k_][f])


# ------------------------------------------------------------------------------------ CLI end to end
@pytest.fixture(scope="module")
def files(g7, tmp_path_factory):
    td = tmp_path_factory.mktemp("g7")
    fdir = td / "features"
    for i, x in enumerate(g7["features"]):
        (fdir / f"{i:06d}").mkdir(parents=True)
        np.save(fdir / f"{i:06d}" / "stage24_output_features.npy", x)
    np.savez(td / "reward.npz", reward=g7["reward"])
    np.save(td / "split.npy", g7["split"])
    return td


@pytest.mark.parametrize("name", ["LR", "EN", "BR", "KNR"])
def test_cli_end_to_end(g7, fits, files, name, monkeypatch):
    from edgeml_amd import estimator, evaluate, regress
    if name == "KNR":  # the reference's default of 500 neighbours exceeds this dataset's training sets
        monkeypatch.setattr(regress._KNROPT, "n_neighbors", int(g7["n_neighbors"]))
    save, mdir = files / f"est_{name}", files / f"model_{name}"
    estimator.main(estimator.getargs([str(files / "features"), str(files / "reward.npz"), str(files / "split.npy"),
                                      str(save), "--model", name, "--model-dir", str(mdir)]))
    assert not os.path.exists(str(save) + "_best") and not os.path.exists(str(save) + "_last")
    for f in range(g7["folds"]):
        with np.load(save / f"estimate{f + 1}.npz", allow_pickle=False) as z:
            assert sorted(z.files) == ["train_est", "train_time", "val_est", "val_time"]
            assert z["train_est"].dtype == z["val_est"].dtype == np.float64
            assert z["train_time"].shape == z["val_time"].shape == ()
            np.testing.assert_array_equal(z["train_est"], fits[name][0][f]["train_est"])
            np.testing.assert_array_equal(z["val_est"], fits[name][0][f]["val_est"])
        with open(mdir / f"wts{f + 1}.pickle", "rb") as fh:
            m = pickle.load(fh)
        assert m["model"] == name and isinstance(m["mean"], np.ndarray) and isinstance(m["scale"], np.ndarray)
        if name != "KNR":
            np.testing.assert_array_equal(m["coef"], fits[name][1]["coef"][f])
    masks = evaluate.offload_masks([str(save)], g7["split"], len(g7["reward"]))
    assert masks.dtype == bool and masks.shape[0] == 1 and masks.shape[2] == len(g7["reward"]) and masks.any()
