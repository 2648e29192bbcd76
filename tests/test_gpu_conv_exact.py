"""Selection convs on every conv tile: exact, no tolerance.

The inputs (tests/conv_cases.py, checked on the CPU by test_conv_cases.py) make every output element
one product of a generic float32 value with +-2^e, so the float64 conv is representable in float32
and every kernel family must return it bit for bit (a sign-flipped zero counts as equal): the split
planes sum to the value exactly in any order, a bf16 x bf16 product has 16 bits and adding zeros is
exact.  Bias 0, no activation, no residual.
  direction A (weights select) checks the activation side to the last bit: the in-loop split,
      split_act_kernel (tile 25, presplit), the direct A loads of the fp32 kernels, the tap walk,
      the padding and the sign of every K block;
  direction B (pixels select) checks all three weight planes of ops.split_bf16x3, the low plane
      and the negated odd K blocks included.
A mismatch is a finding about that kernel, never a reason for a tolerance here.
"""
import pytest
import torch

from tests import conv_cases as C

pytestmark = pytest.mark.gpu

GENERAL = C.LDS_TILES + C.X6_TILES + C.X6B_TILES + C.AUTO
# (tile, shape): each tile on the shapes its launcher accepts.  Tile 26 halves K and needs Kpad >= 64
# (P has 32); the pointwise tiles 10-17 need 1x1 stride 1; the stream tiles Cin <= 72, Cout <= 96 and
# tile 33 NB x KJ <= 18 (W72 has 27).
CASES = ([(t, n) for t in GENERAL for n in ("Q", "S", "T", "STEM", "P") if (t, n) != (26, "P")] +
         [(t, n) for t in C.PW_TILES for n in ("P", "K520")] + [(26, "K520")] +
         [(t, "W20") for t in C.STREAM_TILES] + [(34, "W72"), (35, "W72")])
# the SE variant: one direction-A shape per family
SE_CASES = ([(t, "Q") for t in C.LDS_TILES + C.X6_TILES + C.X6B_TILES] + [(t, "P") for t in C.PW_TILES] +
            [(t, "K520") for t in (13, 14, 16, 17)] + [(t, "W20") for t in C.STREAM_TILES] +
            [(34, "W72"), (35, "W72")])


def _exact(name, direction, tile, se=False, presplit=False):
    shape = C.SEL_SHAPES[name]
    sc = C.sel_scale(name) if se else None
    for r in range(C.sel_rounds(name, direction)):
        x, w, ref = C.sel_case(name, direction, r, se)
        got = C.gpu_conv(x, w, shape, tile, sc=sc, presplit=presplit).double()
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            first = tuple(bad[0].tolist())
            raise AssertionError(f"{name} {direction} tile {tile} round {r}: {len(bad)} of {ref.numel()} outputs "
                                 f"differ, max |d| {(got - ref).abs().max().item():.3e}; first at (b, h, w, co) = "
                                 f"{first}: got {got[first].item()!r}, want {ref[first].item()!r}")


@pytest.mark.parametrize("direction", ["A", "B"])
@pytest.mark.parametrize("tile,name", CASES)
def test_conv_selection_exact(tile, name, direction):
    _exact(name, direction, tile)


@pytest.mark.parametrize("tile,name", SE_CASES)
def test_conv_selection_exact_se_scale(tile, name):
    """in_scale of powers of two per (b, ci) keeps every product exact and pins the scale's indexing."""
    _exact(name, "A", tile, se=True)


@pytest.mark.parametrize("direction,se", [("A", False), ("A", True), ("B", False)])
def test_conv_selection_exact_presplit(direction, se):
    """Tile 25 with the input split up front (split_act_kernel into the x3 scratch; Cin % 32 == 0)."""
    _exact("Q32", direction, 25, se=se, presplit=True)
    _exact("Q32", direction, 25, se=se)
