"""GPU parity of the full detectors against the CPU oracle (oracle/ssdlite.py, oracle/frcnn.py).

Raw head outputs must agree to fp32 tolerance; final detections are compared with the decision
replay protocol of tests/parity_models.py: rows are paired by candidate identity and agree within
1e-3 (north_star), and every candidate whose fate differs is a boundary flip (its deciding
quantity within EPS of a threshold, a top-k / output cut or an NMS IoU threshold).
"""
import pytest
import torch

from tests import parity_models as PM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssd():
    from edgeml_amd import models, synthetic
    sd = synthetic.synthetic_state_dict("ssd", 91, True, seed=0)
    return sd, models.SSDLite320(sd, 91, True).to("cuda")


@pytest.fixture(scope="module")
def frcnn():
    from edgeml_amd import models, synthetic
    sd = synthetic.synthetic_state_dict("faster_rcnn", 91, seed=0)
    return sd, models.FasterRCNNFPNv2(sd, 91).to("cuda")


def _run(model, imgs):
    B, _, H, W = imgs.shape
    plan = model.plan(B, H, W)
    plan.input.tensor().copy_(imgs.cuda())
    plan.run()
    torch.cuda.synchronize()
    return plan


@pytest.mark.parametrize("h,w,n", [(640, 640, 2), (480, 640, 1), (612, 612, 3)])
def test_ssd_detections_match_oracle(ssd, h, w, n):
    from edgeml_amd import synthetic
    sd, model = ssd
    imgs = synthetic.make_batch(n, h, w, seed=21 + h)
    rep = PM.ssd_check(_run(model, imgs), sd, 91, True, imgs, f"ssd {n}x{h}x{w}")
    print(rep)
    assert rep["rows"] > 0


# 427x640, 375x500 and 333x500 resize to 799 rows under the fp32 scale rule of [TV]'s transform
#  and to 800 under a double one: the plan's size is checked against the oracle's
# transform inside frcnn_check, and the expected size is pinned here.
RESIZED = {(427, 640): (799, 1199), (375, 500): (799, 1066), (333, 500): (799, 1201)}


@pytest.mark.parametrize("h,w,n", [(640, 640, 1), (480, 640, 2), (427, 640, 1), (375, 500, 2)])
def test_frcnn_detections_match_oracle(frcnn, h, w, n):
    from edgeml_amd import synthetic
    sd, model = frcnn
    imgs = synthetic.make_batch(n, h, w, seed=31 + h)
    plan = _run(model, imgs)
    if (h, w) in RESIZED:
        assert tuple(plan.resized[:2]) == RESIZED[(h, w)]
    rep = PM.frcnn_check(plan, sd, 91, imgs, f"frcnn {n}x{h}x{w}")
    print(rep)
    assert rep["box"]["rows"] > 0


def test_model_call_equals_plan_outputs(ssd):
    """model(images) (the detect.py:78 contract) returns exactly the plan's output rows."""
    from edgeml_amd import synthetic
    sd, model = ssd
    imgs = synthetic.make_batch(2, 480, 640, seed=9)
    got = model(imgs.cuda())
    plan = model.plan(2, 480, 640)
    for j, g in enumerate(got):
        n = int(plan.out_count.tensor()[j])
        assert torch.equal(g["boxes"], plan.out_box.tensor()[j, :n])
        assert torch.equal(g["scores"], plan.out_score.tensor()[j, :n])
        assert torch.equal(g["labels"], plan.out_label.tensor()[j, :n])
        assert bool((g["scores"][:-1] >= g["scores"][1:]).all())


def test_ssd_batch_chains_agree(ssd, monkeypatch):
    """A batch lowered as concurrent sub-batch chains (stream lanes) against one chain: tile choices
    depend on the per-chain batch, so summation orders (not results) may differ.  Both run against
    the oracle with the full protocol."""
    from edgeml_amd import synthetic
    sd, model = ssd
    imgs = synthetic.make_batch(16, 640, 640, seed=61)
    from edgeml_amd import native
    reps = {}
    for n in (1, 2):
        monkeypatch.setenv("EDGEDET_SSD_CHAINS", str(n))  # read by the library's lowering, part of its plan key
        model.plans.clear()
        plan = _run(model, imgs)
        assert plan.chains == n
        reps[n] = PM.ssd_check(plan, sd, 91, True, imgs, f"ssd b=16 chains={n}", own_check=0)
        print(reps[n])
    native.release("ssd", 16, 640, 640)
    model.plans.clear()
    assert reps[1]["rows"] == reps[2]["rows"] == 16 * 300


