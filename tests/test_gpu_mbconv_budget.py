"""RMS and bias budget of the fused InvertedResidual (mbconv_kernel) against a float64 chain.

Probe-style inputs (x = randn, weights randn * sqrt(2 / K), biases 0.1 randn, fixed seeds;
tests/mbconv_cases.py budget_case) on four shapes of 9,600 to 38,400 outputs.  The reference is the
block as three F.conv2d calls in float64; the yardstick e_ref is the error of the same three calls
in float32 on the CPU (contiguous NCHW), never an engine kernel.  With e = y - ref:
  rms(e) <= 4 rms(e_ref)         the project's factor for fp32 MFMA stage-sum kernels (conv_cases.py)
  |mean(e)| <= 0.1 rms(e_ref)
Each test prints its ratios; tools/mbconv_budget.py writes them to profiles/mbconv_budget.txt.
"""
import pytest

from tests import mbconv_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(M.BUDGET_SHAPES))
def test_mbconv_budget(name):
    case, act = M.BUDGET_SHAPES[name]
    c = M.budget_case(name)
    y = M.run_record(c["t"], case, act)
    r, b = M.ratios(y, c)
    print(f"{name} {case} {act}: rms(e) / rms(e_ref) {r:.3f} (<= {M.RMS_FACTOR:g}), mean(e) / rms(e_ref) {b:+.4f} "
          f"(|.| <= {M.BIAS_FACTOR:g}), rms(e_ref) / |ref|max {M.rms(c['e_ref']) / c['scale']:.2e}, N {y.size}")
    assert y.size >= M.BUDGET_MIN_N
    assert r <= M.RMS_FACTOR, (r, M.RMS_FACTOR)
    assert abs(b) <= M.BIAS_FACTOR, (b, M.BIAS_FACTOR)
