"""The fused InvertedResidual (MBCONV record, csrc/layers.hip mbconv_kernel), bit for bit.

Every case of tests/mbconv_cases.py (odd geometries of every instantiation, maps smaller than the
window, and three batches large enough that each workgroup of the persistent grid runs two or three
tiles) under three constructions:
  L  dense integer-lattice weights, RE and R6: the float64 torch chain is a float32 number and no
     summation order can miss it, so the device must return it exactly;
  S  generic float32 values under selection 1x1 weights, RE, R6 and HS: the device must return the
     numpy restatement of its own arithmetic (taps in (kh, kw) order as one fmaf chain from +0, the
     expanded tensor zero outside the image, y = (sel2 + b2) + x);
  W  S with one +-2^e of w2 in every wave's 16 columns: the partial projections, one exact product
     each, must be added in wave order, ((p0 + p1) + p2) + ...
Each record runs twice inside a canary frame (mbconv_cases.run_record).  test_mbconv_cases.py shows
on the CPU which defects each construction sees.
"""
import numpy as np
import pytest
import torch

from tests import mbconv_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("act", M.L_ACTS)
@pytest.mark.parametrize("name", list(M.CASES))
def test_lattice_bitwise(name, act):
    case = M.CASES[name]
    t = M.lattice_case(name, act)
    want = M.chain(t, case, act, torch.float64)
    assert torch.equal(want.float().double(), want)
    M.assert_same_bits(M.run_record(t, case, act), want.float().numpy(), f"{name} L {act}")


# the small cases run all their rounds in one test; a loop case's restatement takes a second or two
# per round, so each of its rounds is a test of its own
S_RUNS = [(n, a, (r,)) for n in M.LOOP_CASES for a in M.S_ACTS for r in range(M.sel_rounds(n))] + \
         [(n, a, tuple(range(M.sel_rounds(n)))) for n in M.CASES if n not in M.LOOP_CASES for a in M.S_ACTS]


@pytest.mark.parametrize("name,act,rounds", S_RUNS, ids=lambda v: "r" + "".join(map(str, v)) if isinstance(v, tuple) else v)
def test_selection_bitwise(name, act, rounds):
    case = M.CASES[name]
    for r in rounds:
        t = M.selection_case(name, r)
        M.assert_same_bits(M.run_record(t, case, act), M.restate(t, case, act), f"{name} S {act} round {r}")


@pytest.mark.parametrize("act", M.S_ACTS)
@pytest.mark.parametrize("name", list(M.CASES))
def test_wave_order_bitwise(name, act):
    """Construction W: one exact product per wave, the partials added in wave order."""
    case = M.CASES[name]
    for r in range(M.W_ROUNDS):
        t = M.wave_case(name, r)
        M.assert_same_bits(M.run_record(t, case, act), M.restate(t, case, act), f"{name} W {act} round {r}")


def test_refused_geometry_is_a_clean_error():
    """K = 5, stride 2, Cin 32, Cexp 128 needs 169,728 bytes of LDS: mbconv_launch refuses it on the
    host (mbconv_fits, the predicate the lowering uses too) before any launch, names its domain, and
    leaves the output alone."""
    from edgeml_amd import ops
    case = M.REFUSED
    assert M.geom(case)["lds"] > M.LDS_MAX
    B, H, W, Cin, Cexp, Cout, K, S = case
    rng = np.random.default_rng(3)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    t = dict(x=f(B, H, W, Cin), w1=f(Cexp, Cin), b1=f(Cexp), wd=f(Cexp, K, K), bd=f(Cexp), w2=f(Cout, Cexp), b2=f(Cout))
    rc, buf, ys = M.launch(t, case, "RE", fill=M.CANARY)
    assert rc == -1, rc   # EDGEDET_REQUIRE's code: a host-side refusal, not a launch or runtime error
    with pytest.raises(ops.EdgeDetError, match=r"mbconv: .*Cexp <= 128.*160 KiB"):
        ops.check(rc)
    assert (buf == np.float32(M.CANARY)).all()
