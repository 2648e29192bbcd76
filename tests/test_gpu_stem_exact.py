"""Bit-exactness of the SSD stem (csrc/layers.hip ssd_stem_kernel) at the small shapes the 320 x 320 tests
lack: partial tiles on both edges, one tile that is nearly all halo, scale 1, up- and downscaling.

1. The fused stem (transform folded into its input loads) equals the transform record followed by the
   non-fused stem, bit for bit, for uint8 and float sources, with the SSD normalisation (0.5: exact
   divisions) and the ImageNet one (divisions that are not exact: the fast division where u8_fast_div
   accepts it, the IEEE-division instantiation where it does not).
2. Both equal the outputs recorded from the library of an earlier commit (tests/golden/g10_stem_exact.npz,
   written by tests/golden/make_golden_stem.py; its `commit` entry names the commit): identity 1 cannot see
   a change that moves both sides together, and the halo GEMM, the depthwise and the projection are shared
   by the fused and non-fused forms.
"""
import os

import numpy as np
import pytest
import torch

from tests import stem_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_stem_exact.npz")
_outs = {}


def _run(case, u8, norm):
    """One device run per (case, source type, normalisation), shared by the tests and left unchanged."""
    key = (case[0], u8, norm)
    if key not in _outs:
        _outs[key] = SC.run(case, u8, norm)
    return _outs[key]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


IDS = [c[0] for c in SC.CASES]
FORMS = [(True, "ssd"), (False, "ssd"), (True, "imagenet"), (False, "imagenet")]
FORM_IDS = ["u8-ssd", "f32-ssd", "u8-imagenet", "f32-imagenet"]


@pytest.mark.parametrize("u8,norm", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_fused_equals_transform_then_stem(case, u8, norm):
    plain, fused = _run(case, u8, norm)
    assert torch.isfinite(plain).all() and torch.isfinite(fused).all()
    assert torch.equal(plain, fused), int((plain != fused).sum())


@pytest.mark.parametrize("u8,norm", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_stem_equals_recorded_commit(case, u8, norm, golden):
    key = f"{case[0]}/{norm}"
    for got in _run(case, u8, norm):
        assert torch.isfinite(got).all()
        assert SC.digest(got) == str(golden[key + "/sha256"]), (key, str(golden["commit"]))
        if case[0] not in SC.DIGEST_ONLY:
            ref = torch.from_numpy(golden[key + "/y"])
            assert torch.equal(got.cpu(), ref), (key, int((got.cpu() != ref).sum()))


def test_fixture_names_its_commit(golden):
    assert len(str(golden["commit"])) >= 7
    assert os.path.getsize(GOLDEN) < 1 << 20
