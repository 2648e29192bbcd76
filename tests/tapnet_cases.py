"""The nets, states and inputs of tests/test_gpu_tapnet_exact.py and tests/test_gpu_tapnet_budget.py, and their CPU
references (tests/convnet_ref.py).  Everything here runs without a device.

Geometries: the smallest at which the fused kernel's indexing can go wrong.  (Cin, S, channels, kernels, pools):
the default net; a 5 x 5 map with 12 channels (an M tile and an N tile both partly empty, a 5 x 5 kernel whose taps
leave the map on every side, floor pooling that drops a row and a column); a 1 x 1 first layer and a pool in the
middle of three layers; a 1 x 1 map.  Hidden widths: four layers of 16, none, and a first linear width of 2048.
"""
import numpy as np
import torch

from tests import convnet_ref as R

BATCHES = (1, 3, 37)
N = max(BATCHES)
H4 = [16, 16, 16, 16]
#        Cin  S  channels     kernels    pools      hidden
CASES = {"default": (40, 8, [64, 32], [3, 3], [1, 1], H4),
         "default_nohidden": (40, 8, [64, 32], [3, 3], [1, 1], []),
         "tails": (4, 5, [12], [5], [1], H4),
         "tails_nohidden": (4, 5, [12], [5], [1], []),
         "three": (80, 4, [20, 8, 8], [1, 3, 3], [0, 1, 0], H4),
         "pixel": (16, 1, [4], [3], [0], H4),
         "pixel_nohidden": (16, 1, [4], [3], [0], []),
         "wide2048": (40, 8, [32], [3], [0], [16])}


def spec_of(name):
    from edgeml_amd import convnet
    cin, S, channels, kernels, pools, hidden = CASES[name]
    spec = convnet.ConvSpec(cin, channels, kernels, pools, hidden, (S, S), True)
    if name == "wide2048":
        assert spec.dims[0] == 2048
    return spec


def _bn_identity(spec, state):
    """gamma 1, beta 0, running mean 0, running var float32(1 - 1e-5): the eval scale is exactly 1 in float32
    (rv + 1e-5f rounds to 1) and in the float64 reference (checked by exact_state)."""
    for lay in spec.layers:
        if lay["bn"]:
            co = lay["cout"]
            state[lay["g"]:lay["g"] + co] = 1.0
            state[lay["be"]:lay["be"] + co] = 0.0
            state[lay["rm"]:lay["rm"] + co] = 0.0
            state[lay["rv"]:lay["rv"] + co] = np.float32(1.0 - 1e-5)


def exact_state(spec, seed):
    """Integer weights in [-2, 2] (about six nonzero per output, so the sums stay small), integer biases in
    [-2, 2], identity BatchNorm."""
    rng = np.random.default_rng(seed)
    state = np.zeros(spec.ns, np.float32)
    for lay in spec.layers:
        fan = lay["cin"] * lay["k"] * lay["k"]
        nw = lay["cout"] * fan
        w = rng.integers(-2, 3, nw) * (rng.random(nw) < min(1.0, 6.0 / fan))
        state[lay["w"]:lay["w"] + nw] = w
        state[lay["b"]:lay["b"] + lay["cout"]] = rng.integers(-2, 3, lay["cout"])
    _bn_identity(spec, state)
    rv = np.float32(1.0 - 1e-5)
    assert np.float32(1.0) / np.sqrt(rv + np.float32(1e-5), dtype=np.float32) == np.float32(1.0)
    assert 1.0 / np.sqrt(np.float64(rv) + 1e-5) != 1.0  # torch's float64 eval scale is not 1: see exact_ref
    return state


def exact_maps(spec, seed, n=N):
    """[n, S, S, Cin] integer maps in [-3, 3] (NHWC, float32)."""
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (n,) + spec.hw + (spec.cin,)).astype(np.float32)


def trained_state(spec, seed):
    """A trained-like state: the initialiser's weights, BatchNorm scales, shifts and running statistics moved off
    their start values."""
    rng = np.random.default_rng(seed)
    state = spec.init_state(rng)
    for lay in spec.layers:
        if lay["bn"]:
            co = lay["cout"]
            state[lay["g"]:lay["g"] + co] = rng.uniform(0.5, 1.5, co)
            state[lay["be"]:lay["be"] + co] = rng.uniform(0.1, 0.5, co)
            state[lay["rm"]:lay["rm"] + co] = rng.normal(0, 0.2, co)
            state[lay["rv"]:lay["rv"] + co] = rng.uniform(0.5, 1.5, co)
    return state


def trained_maps(spec, seed, n=N):
    rng = np.random.default_rng(seed)
    return np.abs(rng.normal(0, 1, (n,) + spec.hw + (spec.cin,))).astype(np.float32)


def ref(spec, state, maps, dtype, eps=None):
    """tests/convnet_ref.build(...).eval() on NHWC maps -> [n] float64."""
    net = R.build(spec, spec.unpack(np.asarray(state)), dtype).eval()
    if eps is not None:
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.eps = eps
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(maps).transpose(0, 3, 1, 2))).to(dtype)
    with torch.no_grad():
        return net(x).numpy().astype(np.float64).ravel()


def exact_ref(spec, state, maps):
    """The float64 reference of the exact construction.  The running variance is the float32 value 1 - 1e-5; the
    float64 net adds its eps to it in float64, where the sum is 1 only up to float32's rounding of rv, so the
    reference folds the scale as the issue states it: eps chosen so that rv + eps is exactly 1 in float64."""
    rv = np.float64(np.float32(1.0 - 1e-5))
    eps = float(1.0 - rv)
    assert rv + eps == 1.0
    return ref(spec, state, maps, torch.float64, eps)


def abs_bound(spec, state, maps):
    """An upper bound of every partial sum anywhere in the net, whatever the order: the net of |weights| and
    |biases| on |maps| (ReLU and max-pooling are monotone).  Returns the largest activation of that net."""
    s = np.abs(np.asarray(state, np.float64))
    _bn = np.asarray(state, np.float64)
    for lay in spec.layers:  # BatchNorm stays the identity
        if lay["bn"]:
            for key in ("g", "be", "rm", "rv"):
                s[lay[key]:lay[key] + lay["cout"]] = _bn[lay[key]:lay[key] + lay["cout"]]
    rv = np.float64(np.float32(1.0 - 1e-5))
    net = R.build(spec, spec.unpack(s), torch.float64).eval()
    big = [float(np.abs(maps).max())]
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.eps = float(1.0 - rv)
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            m.register_forward_hook(lambda mod, i, o: big.append(float(o.abs().max())))
    x = torch.from_numpy(np.ascontiguousarray(np.abs(np.asarray(maps)).transpose(0, 3, 1, 2))).to(torch.float64)
    with torch.no_grad():
        net(x)
    return max(big)
