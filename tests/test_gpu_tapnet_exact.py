"""The fused conv-stack inference (csrc/tapnet.hip, edgeml_amd.tapnet.TapNet) bit for bit.

Integer maps in [-3, 3], integer weights in [-2, 2] and integer biases, BatchNorm with gamma 1, beta 0, running mean
0 and running variance float32(1 - 1e-5), whose float32 eval scale 1 / sqrtf(rv + 1e-5f) is exactly 1.  Every
partial sum of the net, in any order, stays below 2^24 (tapnet_cases.abs_bound, asserted), so every float32 sum is
exact and the estimate must equal the float64 reference (tests/convnet_ref.build(...).eval()) bit for bit, on the
fused path and on the layered one, and must not depend on the batch an image runs in.

The reference's BatchNorm eps: in float64, float32(1 - 1e-5) + 1e-5 is 1 + 1.4e-8, not 1 (the scale would be
1.0000000068 and no reference value an integer), so the float64 reference takes eps = 1 - float64(rv), for which
rv + eps is exactly 1: the scale the construction means (tapnet_cases.exact_ref).
"""
import numpy as np
import pytest
import torch

from tests import tapnet_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_REF = {}


def _setup(name):
    """(spec, state, maps, ref64) of a case: computed once, shared and left unchanged."""
    if name not in _REF:
        spec = T.spec_of(name)
        state, maps = T.exact_state(spec, 1), T.exact_maps(spec, 2)
        assert T.abs_bound(spec, state, maps) < 2 ** 24
        ref = T.exact_ref(spec, state, maps)
        assert np.all(ref == np.round(ref)) and len(set(ref.tolist())) >= 4
        for a in (state, maps, ref):
            a.setflags(write=False)
        _REF[name] = (spec, state, maps, ref)
    return _REF[name]


@pytest.mark.parametrize("name", list(T.CASES))
def test_fused_and_layered_equal_the_float64_reference(name):
    from edgeml_amd import tapnet
    spec, state, maps, ref = _setup(name)
    net = tapnet.TapNet(spec, state)
    assert net.fits and net.use_fused(True) is True and net.use_fused() is False
    x = torch.from_numpy(maps.copy()).to(DEV)
    thr = float(np.median(ref))  # an estimate itself: the strict > keeps that image
    for B in T.BATCHES:
        for fused in (True, False):
            est, flag = tapnet.predict(net, x[:B].contiguous(), thr, fused=fused)
            what = f"{name} B={B} {'fused' if fused else 'layered'}"
            assert est.dtype == np.float64 and est.tobytes() == ref[:B].tobytes(), \
                f"{what}: {np.abs(est - ref[:B]).max()} at {int(np.abs(est - ref[:B]).argmax())}"
            assert np.array_equal(flag, ref[:B] > thr), what
    # an image's estimate does not depend on its place in the batch
    perm = np.random.default_rng(5).permutation(T.N)
    est, _ = tapnet.predict(net, x[torch.from_numpy(perm).to(DEV)].contiguous(), thr, fused=True)
    assert est.tobytes() == ref[perm].tobytes()


def test_infer_refuses_other_maps_and_a_forced_fused_path_outside_the_rule():
    from edgeml_amd import convnet, tapnet
    spec, state, maps, ref = _setup("tails")
    net = tapnet.TapNet(spec, state)
    est = torch.empty(2, dtype=torch.float64, device=DEV)
    flag = torch.empty(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="the net takes"):
        net.infer(torch.zeros((2, 5, 5, 8), device=DEV), 0.0, est, flag)
    big = convnet.ConvSpec(320, [320], [3], [False], [16], (8, 8), True)  # two planes of 164,352 bytes together
    far = tapnet.TapNet(big, big.init_state(np.random.default_rng(0)))
    assert not far.fits and far.use_fused() is False
    with pytest.raises(ValueError, match="fused kernel does not take"):
        far.infer(torch.zeros((2, 8, 8, 320), device=DEV), 0.0, est, flag, fused=True)
