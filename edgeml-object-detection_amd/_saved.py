"""What the saved-model predictors (kpredict.KernelModel, gbr.GBRModel) share: reading and validating a
wts<fold>.pickle's arrays, and the host side of a model that lives on one device."""
import pickle

import numpy as np
import torch

from . import ops


def open_model(path_or_dict):
    """(the pickled object, what to call it in a message) of a path, or of the dict itself."""
    if isinstance(path_or_dict, dict):
        return path_or_dict, "model"
    with open(path_or_dict, "rb") as f:
        return pickle.load(f), str(path_or_dict)


def vec(what, m, key, n=None):
    if key not in m:
        raise ValueError(f"{what}: no '{key}'")
    a = np.ascontiguousarray(np.asarray(m[key], np.float64).reshape(-1))
    if n is not None and len(a) != n:
        raise ValueError(f"{what}: '{key}' has {len(a)} entries, expected {n}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: '{key}' is not finite")
    return a


def rows(what, m, key, D):
    a = np.asarray(m[key], np.float64)
    if a.ndim != 2 or a.shape[1] != D:
        raise ValueError(f"{what}: '{key}' has shape {a.shape}, expected [rows][{D}] as mean and scale are {D} wide")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: '{key}' is not finite")
    return np.ascontiguousarray(a)


def scalar(what, m, key):
    if key not in m:
        raise ValueError(f"{what}: no '{key}'")
    v = float(m[key])
    if not np.isfinite(v):
        raise ValueError(f"{what}: '{key}' is not finite")
    return v


def scaler(what, m):
    """The fold's StandardScaler: mean and scale, float64 [D], finite, 1 <= D <= 255, no zero in scale."""
    mean = vec(what, m, "mean")
    D = len(mean)
    scale = vec(what, m, "scale", D)
    if not 1 <= D <= 255:
        raise ValueError(f"{what}: {D} features; the kernels take 1 to 255")
    if np.any(scale == 0.0):
        raise ValueError(f"{what}: a zero in 'scale'")
    return mean, scale


class DeviceModel:
    """A model of `width` features whose arrays are uploaded once per device.  A subclass sets `module` (the name
    its messages carry) and `width`, and has _upload(device) return the dict of its device arrays."""
    _dev = None

    def to(self, device):
        """Upload (and prepare) once per device; returns self."""
        ops.need_device(self.module)
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if self._dev is None or self._dev["device"] != device:
            self._dev = {"device": device, **self._upload(device)}
        return self

    def _host_rows(self, features):
        """predict's prologue: (the model's device, features flattened to contiguous float64 [N, width])."""
        ops.need_device(self.module)
        if self._dev is None:
            self.to("cuda")
        x = np.asarray(features, dtype=np.float64)
        x = np.ascontiguousarray(x.reshape(len(x), -1))
        if x.shape[1] != self.width:
            raise ValueError(f"{self.module}: the model takes {self.width} features, the rows have {x.shape[1]}")
        return self._dev["device"], x

    def _device_rows(self, feat, est, *more):
        """predict_into's prologue: the device arrays, after checking feat [B, width] and est [B] float64 on them."""
        d = self._dev
        if d is None or d["device"] != feat.device:
            raise ValueError(f"{self.module}: call to(device) with the features' device first")
        ops._need_cuda(feat, est, *more)
        if feat.dtype != torch.float64 or feat.dim() != 2 or feat.shape[1] != self.width or est.dtype != torch.float64 \
                or est.numel() < feat.shape[0]:
            raise ValueError(f"{self.module}: features [B][{self.width}] and estimates [B] in float64")
        return d
