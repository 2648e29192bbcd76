"""The fused conv-stack inference and the layered eval forward against a float64 error budget, on trained-like
states (the initialiser's weights, BatchNorm parameters and running statistics off their start values) and random
maps, over the geometries of tests/tapnet_cases.py.

The rule of tests/convnet_ref.py and the conv budget test: E = max |ref32 - ref64| is float32's own rounding scale
on this net (the torch CPU reference in both precisions) and a path passes when max |got - ref64| <= 4 E, provided
0 < E <= 1e-3 std(ref64) (checked on the CPU for these seeds).  Measured ratios max |got - ref64| / (4 E):
profiles/tapnet_budget.txt.
"""
import numpy as np
import pytest
import torch

from tests import convnet_ref as R
from tests import tapnet_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(T.CASES))
def test_both_paths_within_four_times_float32_s_own_error(name):
    from edgeml_amd import tapnet
    spec = T.spec_of(name)
    state, maps = T.trained_state(spec, 3), T.trained_maps(spec, 4)
    ref64, ref32 = T.ref(spec, state, maps, torch.float64), T.ref(spec, state, maps, torch.float32)
    net = tapnet.TapNet(spec, state)
    assert net.fits
    x = torch.from_numpy(maps).to(DEV)
    out = {}
    for fused in (True, False):
        est, _ = tapnet.predict(net, x, 0.0, fused=fused)
        ratio, E = R.yardstick(est, ref64, ref32)
        out["fused" if fused else "layered"] = ratio
        print(f"tapnet budget {name} {'fused' if fused else 'layered'}: ratio {ratio:.4f} E {E:.3e} "
              f"std {ref64.std():.3e}")
    assert 0 < E <= 1e-3 * ref64.std()
    assert out["fused"] <= 1.0 and out["layered"] <= 1.0, out
