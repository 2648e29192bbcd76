"""Estimates from a saved SVR or KNR model on the GPU (csrc/kpredict.hip): the "file route" the offloading
cascade is held to for these two kinds.

    model = kpredict.load("wts1.pickle")        # or the dict edgeml_amd.svr / regress.model_data returns
    est = model.to("cuda").predict(features)    # float64 [N], in chunks of any size

An SVR file holds {model, mean, scale, gamma, support (raw feature rows), beta, intercept}; a KNR file {model,
mean, scale, n_neighbors, train (raw training rows, training-list order), target}.  to() uploads the arrays and
standardises the stored rows once (edgedet_kmodel_prepare, in the fits' own order); predict() standardises the
queries in the load.  Float64 throughout; an estimate depends on the feature row and the model only, not on
the chunk it was computed in, and a KNR model reproduces edgeml_amd.regress.fit_knr's estimates and neighbours
bit for bit.  File validation and the per-device upload are edgeml_amd._saved's, shared with gbr.GBRModel.  There
is no CPU path.
"""
import numpy as np
import torch

from . import ops
from ._saved import DeviceModel, open_model, rows as _rows, scalar as _scalar, scaler, vec as _vec

KINDS = {"SVR": 0, "KNR": 1}
CHUNK = 4096  # rows per predict call: bounds the KNR distance workspace (8 n bytes a row)


class KernelModel(DeviceModel):
    """kind "svr": rows = the support vectors, weight = beta, gamma, intercept; kind "knr": rows = the training
    rows, weight = their targets, n_neighbors.  mean, scale [width] are the fold's StandardScaler."""
    module = "edgeml_amd.kpredict"

    def __init__(self, kind, mean, scale, rows, weight, gamma=0.0, intercept=0.0, n_neighbors=0):
        self.kind, self.width, self.n = kind, len(mean), len(rows)
        self.mean, self.scale, self.rows, self.weight = mean, scale, rows, weight
        self.gamma, self.intercept, self.n_neighbors = float(gamma), float(intercept), int(n_neighbors)

    # ------------------------------------------------------------------------------------ device side
    def _upload(self, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        d = {"mean": t(self.mean), "scale": t(self.scale), "weight": t(self.weight),
             "z": torch.empty((self.n, self.width), dtype=torch.float64, device=device),
             "norm": torch.empty((self.n,), dtype=torch.float64, device=device)}
        rows = t(self.rows)
        p = ops._ptr
        with torch.cuda.device(device):
            ops.check(ops.lib().edgedet_kmodel_prepare(p(rows), self.n, self.width, p(d["mean"]), p(d["scale"]),
                                                       p(d["z"]), p(d["norm"]), ops.stream_handle()))
            torch.cuda.current_stream().synchronize()  # rows may be freed; other streams may read z
        return d

    def workspace_bytes(self, B):
        wb = int(ops.lib().edgedet_kmodel_workspace_size(self.n, self.width, int(B), KINDS[self.kind.upper()]))
        if wb < 0:
            raise ValueError(f"edgeml_amd.kpredict: no workspace for {B} rows of {self.width} features against "
                             f"{self.n} stored rows")
        return wb

    def predict_into(self, feat, est, ws, nbr=None, stream=None):
        """One library call: feat [B, width] float64 and est [B] float64 on the prepared device, ws a uint8
        tensor of workspace_bytes(B); nbr [B, n_neighbors] int32 receives a KNR model's neighbours."""
        d = self._device_rows(feat, est, ws, nbr)
        B, p, L = int(feat.shape[0]), ops._ptr, ops.lib()
        if self.kind == "svr":
            ops.check(L.edgedet_svr_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]), p(d["z"]),
                                                  p(d["norm"]), p(d["weight"]), self.n, self.gamma, self.intercept,
                                                  p(ws), ws.numel(), p(est), ops.stream_handle(stream)))
        else:
            if nbr is not None and (nbr.dtype != torch.int32 or nbr.numel() < B * self.n_neighbors):
                raise ValueError("edgeml_amd.kpredict: neighbours [B][n_neighbors] in int32")
            ops.check(L.edgedet_knn_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]), p(d["z"]),
                                                  p(d["norm"]), p(d["weight"]), self.n, self.n_neighbors, p(ws),
                                                  ws.numel(), p(est), p(nbr), ops.stream_handle(stream)))

    def predict(self, features, chunk=CHUNK, neighbors=False):
        """Estimates float64 [N] of features [N, ...] (flattened to [N, width]); with neighbors=True a KNR
        model also returns the neighbours' positions int32 [N, n_neighbors], ascending."""
        dev, x = self._host_rows(features)
        if neighbors and self.kind != "knr":
            raise ValueError("edgeml_amd.kpredict: only a KNR model has neighbours")
        chunk = max(1, int(chunk))
        N, k = len(x), self.n_neighbors
        est = np.empty(N, np.float64)
        nbr = np.empty((N, k), np.int32) if neighbors else None
        if N == 0:
            return (est, nbr) if neighbors else est
        with torch.cuda.device(dev):
            ws = torch.empty(self.workspace_bytes(min(chunk, N)), dtype=torch.uint8, device=dev)
            g_est = torch.empty(min(chunk, N), dtype=torch.float64, device=dev)
            g_nbr = torch.empty((min(chunk, N), k), dtype=torch.int32, device=dev) if neighbors else None
            for a in range(0, N, chunk):
                b = min(a + chunk, N)
                self.predict_into(torch.from_numpy(x[a:b]).to(dev), g_est, ws, g_nbr)
                est[a:b] = g_est[:b - a].cpu().numpy()
                if neighbors:
                    nbr[a:b] = g_nbr[:b - a].cpu().numpy()
        return (est, nbr) if neighbors else est


def load(path_or_dict):
    """The KernelModel of an SVR or KNR wts<fold>.pickle (a path, or the dict itself); ValueError on anything
    else, on inconsistent shapes and on values that are not finite."""
    m, what = open_model(path_or_dict)
    if not isinstance(m, dict) or "mean" not in m or "scale" not in m:
        raise ValueError(f"{what}: not a wts<fold>.pickle of edgeml_amd.estimator / edgeml_amd.svr --model-dir")
    mean, scale = scaler(what, m)
    D = len(mean)
    kind = m.get("model")
    if kind == "SVR":
        if "support" not in m or "beta" not in m:
            raise ValueError(f"{what}: an SVR file without 'support' and 'beta'")
        support = _rows(what, m, "support", D)
        beta = _vec(what, m, "beta", len(support))
        gamma = _scalar(what, m, "gamma")
        if gamma <= 0.0:
            raise ValueError(f"{what}: gamma = {gamma!r} is not positive")
        return KernelModel("svr", mean, scale, support, beta, gamma=gamma, intercept=_scalar(what, m, "intercept"))
    if kind == "KNR":
        if "train" not in m or "target" not in m:
            raise ValueError(f"{what}: a KNR file holds no training rows (written before --model-dir stored them): "
                             f"train it again")
        train = _rows(what, m, "train", D)
        target = _vec(what, m, "target", len(train))
        kn, n = int(_scalar(what, m, "n_neighbors")), len(train)
        if kn > n:  # sklearn's wording (neighbors/_base.py kneighbors), as regress.fit_knr uses it
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {kn}, n_samples_fit = {n}, "
                             f"n_samples = {n}")
        if kn < 1:
            raise ValueError(f"Expected n_neighbors > 0. Got {kn}")
        return KernelModel("knr", mean, scale, train, target, n_neighbors=kn)
    raise ValueError(f"{what}: model {kind!r} is neither SVR nor KNR (a linear or CNN file predicts through "
                     f"edgeml_amd.offload.load_estimator)")
