"""The constructions of tests/conv_cases.py, checked on the CPU: the selection cases are what the
exact GPU test assumes (representable, one term per output, every K index covered), and a float64
emulation of the bf16x6 product shows that the GPU tests have teeth: the designed arithmetic sits
far inside the RMS budget, the same arithmetic less any one of its three smallest kept products
breaks it on every budget shape, and fails the equality of a selection case where that product is
not zero by construction."""
import pytest
import torch

from tests import conv_cases as C

SEL = [(n, d) for n in C.SEL_SHAPES for d in "AB"]
BUDGET = list(C.BUDGET_SHAPES)


def test_planes_sum_to_the_value():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(5, 77, generator=g) * 10.0 ** torch.randint(-6, 6, (5, 77), generator=g)
    p = C.planes64(v)
    assert torch.equal(p.sum(0), v.double())
    assert torch.equal(p[2] + p[1] + p[0], v.double())
    one = C.planes64(torch.tensor(C.VALS))
    assert torch.equal(one[0], torch.tensor(C.VALS).double()) and not one[1:].any()


@pytest.mark.parametrize("name,direction", SEL)
def test_selection_case_is_exact_with_one_term(name, direction):
    """Every round (and the SE variant of direction A): the float64 conv equals its float32 rounding,
    no output has more than one nonzero term, and some output has one."""
    for r in range(C.sel_rounds(name, direction)):
        for se in (False, True) if direction == "A" else (False,):
            x, w, ref = C.sel_case(name, direction, r, se)
            assert torch.equal(ref, ref.float().double()), (r, se)
            terms = C.sel_terms(x, w, C.SEL_SHAPES[name])
            assert terms.max().item() == 1.0, (r, terms.max().item())
            assert ref.abs().max().item() > 0
    if direction == "A":
        sc = C.sel_scale(name)
        assert torch.equal(torch.exp2(torch.log2(sc).round()), sc) and sc.unique().numel() > 1


@pytest.mark.parametrize("name,direction", SEL)
def test_selection_rounds_cover_k(name, direction):
    """Over the rounds every K index (kh, kw, ci) is selected by some output: always in direction A,
    and in direction B for the stride-1 cases (a stride-2 window meets a lattice pixel at the taps
    of one parity only where the lattice period is even; both strided cases have odd periods and
    are reported)."""
    cov = C.sel_coverage(name, direction)
    print(f"{name} {direction}: K coverage {100 * cov:.1f} % over {C.sel_rounds(name, direction)} rounds")
    if direction == "A" or C.SEL_SHAPES[name][6] == 1:
        assert cov == 1.0, cov


@pytest.mark.parametrize("name,direction", SEL)
def test_emulation_is_exact_on_selection_cases(name, direction):
    """The emulated bf16x6 conv with the designed drops returns the selection value exactly."""
    r = C.sel_rounds(name, direction) - 1
    x, w, ref = C.sel_case(name, direction, r)
    assert torch.equal(C.emulate_x6(x, w, C.SEL_SHAPES[name]), ref)


@pytest.mark.parametrize("name", BUDGET)
def test_emulation_designed_drops_sit_far_inside_the_budget(name):
    """Only mid.lo, lo.mid and lo.lo dropped, exact sums: under a tenth of the float32 CPU conv's RMS
    error, and no bias to speak of."""
    c = C.budget_case(name)
    r, b = C.ratios(C.emulate_x6(c["x"], c["w"], C.BUDGET_SHAPES[name], c["b"]), c)
    print(f"{name}: designed drops rms {r:.4f} bias {b:+.4f} of the CPU's rms {C.rms(c['e_ref']) / c['scale']:.2e}")
    assert r < 0.1 and abs(b) < 0.01, (r, b)


@pytest.mark.parametrize("drop", list(C.SMALLEST_KEPT))
@pytest.mark.parametrize("name", BUDGET)
def test_emulation_dropped_product_breaks_the_budget(name, drop):
    """Any one of the three smallest kept products removed as well: over the RMS budget of the bf16x6
    kernels on every budget shape (it reads 10 to 25 where torch's CPU conv errs as in
    profiles/conv_budget.txt, so over the plain chain's factor 8 as well)."""
    c = C.budget_case(name)
    r, b = C.ratios(C.emulate_x6(c["x"], c["w"], C.BUDGET_SHAPES[name], c["b"], drop=C.SMALLEST_KEPT[drop]), c)
    print(f"{name} without {drop}: rms {r:.1f} bias {b:+.2f}")
    assert C.RMS_FACTOR < C.RMS_FACTOR_CHAIN
    assert r > C.RMS_FACTOR, r


@pytest.mark.parametrize("name", ["Q", "S", "K520"])
def test_emulation_dropped_product_fails_a_selection_case(name):
    """hi.lo is the whole low plane of a selected weight (direction B), lo.hi that of a selected
    activation (direction A): without it the equality fails.  mid.mid is zero in both directions by
    construction (the selecting operand has a high plane only), so it is the budget that holds it."""
    shape = C.SEL_SHAPES[name]
    for direction, drop, other in (("A", "lo.hi", "hi.lo"), ("B", "hi.lo", "lo.hi")):
        x, w, ref = C.sel_case(name, direction, 0)
        bad = C.emulate_x6(x, w, shape, drop=C.SMALLEST_KEPT[drop])
        assert not torch.equal(bad, ref) and (bad != ref).float().mean().item() > 0.25
        assert torch.equal(C.emulate_x6(x, w, shape, drop=C.SMALLEST_KEPT[other]), ref)
        assert torch.equal(C.emulate_x6(x, w, shape, drop=C.SMALLEST_KEPT["mid.mid"]), ref)
