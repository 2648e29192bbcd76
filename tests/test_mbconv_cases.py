"""The constructions of tests/mbconv_cases.py, checked on the CPU: what test_gpu_mbconv_exact.py
assumes (L exact in any order, the S restatement a float32 evaluation of the float64 chain, every
register slot selected), that each construction sees the defects it is meant to see, and that the
loop cases still make every workgroup of mbconv_kernel run more than two tiles."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mbconv_cases as M

NAMES = list(M.CASES)
SMALL = [n for n in NAMES if n not in M.LOOP_CASES]
U = 2.0 ** -24


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------- L
@pytest.mark.parametrize("act", M.L_ACTS)
@pytest.mark.parametrize("name", NAMES)
def test_lattice_is_exact_in_any_order(name, act):
    """torch's float32 chain equals its float64 chain bit for bit, so does the chain with both K axes
    (Cin, Cexp) permuted, and so does the restatement; the sums stay where the module says."""
    case = M.CASES[name]
    t = M.lattice_case(name, act)
    y64 = M.chain(t, case, act, torch.float64)
    y32 = M.chain(t, case, act, torch.float32)
    assert torch.equal(y64.float().double(), y64) and _bits_equal(y32, y64.float())
    rng = np.random.default_rng(5)
    pi, pe = rng.permutation(case[3]), rng.permutation(case[4])
    tp = dict(t, x=t["x"][..., pi], w1=t["w1"][pe][:, pi], b1=t["b1"][pe], wd=t["wd"][pe], bd=t["bd"][pe],
              w2=t["w2"][:, pe])
    yp = M.chain(tp, case, act, torch.float32)
    if M.residual(case):   # the permuted input is added back in the permuted order: undo it
        yp = yp - torch.from_numpy(tp["x"]) + torch.from_numpy(t["x"])
    assert _bits_equal(yp, y64.float())
    assert y64.abs().max().item() < (3.4e6 if act == "RE" else 2.0 ** 11) and y64.abs().max().item() > 0
    assert (y64 * (1 if act == "RE" else 128) % 1 == 0).all()
    if name not in M.LOOP_CASES or act == "RE":
        M.assert_same_bits(M.restate(t, case, act), y64.float().numpy(), "restatement")


# ------------------------------------------------------------------------------------- S
@pytest.mark.parametrize("name", NAMES)
def test_selection_rounds_cover_every_slot(name):
    """Over the rounds: one nonzero +-2^e per row of w1 and of w2; every input channel is selected by
    some expanded channel and every expanded channel by some output channel (so every w2r slot of
    every live wave); in every full wave every input channel, that is every w1r slot (s, q)."""
    B, H, W, Cin, Cexp, Cout, K, S = M.CASES[name]
    R = M.sel_rounds(name)
    seen1, seen2 = np.zeros((Cexp, Cin), bool), np.zeros((Cout, Cexp), bool)
    for r in range(R):
        t = M.selection_case(name, r)
        for w in (t["w1"], t["w2"]):
            assert ((w != 0).sum(1) == 1).all()
            assert np.isin(np.abs(w[w != 0]), (0.5, 1.0, 2.0)).all()
        seen1 |= t["w1"] != 0
        seen2 |= t["w2"] != 0
    assert seen1.any(0).all() and seen2.any(0).all()
    for w in range(Cexp // 16):
        assert seen1[16 * w:16 * w + 16].any(0).all(), w
    print(f"{name}: {R} rounds")


def _rounding_bound(t, case, act):
    """|float32 evaluation - float64 chain| of a selection case, one rounding error u = 2^-24 per
    float32 operation, propagated stage by stage (first order, the caller adds 1 % for the rest):
    the 1x1 stages are exact products; an activation is Lipschitz L (1.5 for HS, else 1) and HS adds
    three roundings of its own (v + 3, the product, the division); the depthwise chain errs by at most
    K^2 u sum|terms|."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    L, ca = (1.5, 3.0) if act == "HS" else (1.0, 0.0)
    c = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in t.items()}
    xc = c["x"].permute(0, 3, 1, 2)
    pre1 = F.conv2d(xc, c["w1"].reshape(Cexp, Cin, 1, 1), c["b1"])
    e = M._tact(pre1, act)
    de = L * U * pre1.abs() + ca * U * e.abs()
    dw = lambda v, w: F.conv2d(v, w.reshape(Cexp, 1, K, K), None, S, (K - 1) // 2, 1, Cexp)  # noqa: E731
    terms = dw(e.abs() + de, c["wd"].abs())
    dchain = dw(de, c["wd"].abs()) + K * K * U * terms
    pre2 = dw(e, c["wd"]) + c["bd"][None, :, None, None]
    dpre2 = dchain + U * (pre2.abs() + dchain)
    d = M._tact(pre2, act)
    dd = L * dpre2 + ca * U * d.abs()
    w2 = c["w2"].reshape(Cout, Cexp, 1, 1)
    s2 = F.conv2d(d, w2, c["b2"])
    y = s2 + xc if M.residual(case) else s2
    nnz = int((c["w2"] != 0).sum(1).max().item())   # partials of a row that are not zero: nnz - 1 rounded adds
    dy = F.conv2d(dd, w2.abs()) + (nnz - 1) * U * F.conv2d(d.abs() + dd, w2.abs()) + U * s2.abs() + U * y.abs()
    return dy.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("name", NAMES)
def test_wave_case_has_one_term_per_wave(name):
    B, H, W, Cin, Cexp, Cout, K, S = M.CASES[name]
    nw = -(-Cexp // 16)
    cols = set()
    for r in range(M.W_ROUNDS):
        w2 = M.wave_case(name, r)["w2"]
        per_wave = np.stack([(w2[:, 16 * w:16 * w + 16] != 0).sum(1) for w in range(nw)])
        assert (per_wave == 1).all() and np.isin(np.abs(w2[w2 != 0]), (0.5, 1.0, 2.0)).all()
        cols.add(w2.tobytes())
    assert len(cols) == M.W_ROUNDS


@pytest.mark.parametrize("act", M.S_ACTS)
@pytest.mark.parametrize("construction", ["S", "W"])
@pytest.mark.parametrize("name", NAMES)
def test_selection_restatement_is_the_float64_chain_in_float32(name, construction, act):
    """Every round of the small cases, round 0 of the loop cases."""
    case = M.CASES[name]
    make, rounds = (M.selection_case, M.sel_rounds(name)) if construction == "S" else (M.wave_case, M.W_ROUNDS)
    for r in range(1 if name in M.LOOP_CASES else rounds):
        t = make(name, r)
        y = torch.from_numpy(M.restate(t, case, act)).double()
        bound, y64 = _rounding_bound(t, case, act)
        y64 = M.chain(t, case, act, torch.float64)   # the reference itself; the bound's copy differs by ~1e-16
        err = (y - y64).abs()
        assert (err <= 1.01 * bound + 1e-30).all(), (r, (err / (bound + 1e-30)).max().item())
        assert err.max().item() > 0 and y64.abs().max().item() > 1.0


# ------------------------------------------------------------------------------------- defects
def _tensors(name, construction):
    return {"L": lambda: M.lattice_case(name, "RE"), "S": lambda: M.selection_case(name, 0),
            "W": lambda: M.wave_case(name, 0)}[construction]()


@pytest.mark.parametrize("construction", ["L", "S", "W"])
@pytest.mark.parametrize("name", SMALL)
def test_constructions_see_the_defects(name, construction):
    """Each emulated defect changes the restated output: the padding leak and a dropped wave in every
    case, the shifted residual where there is one (and the map is wider than a pixel), the tap order
    under S and W (L is order-free by design), the wave order under W alone and only where three or
    more waves are live (two partials commute)."""
    case = M.CASES[name]
    t = _tensors(name, construction)
    acts = M.L_ACTS if construction == "L" else M.S_ACTS
    for act in acts:
        if construction == "L":
            t = M.lattice_case(name, act)
        good = M.restate(t, case, act)
        wave = int(np.flatnonzero(t["w2"][0])[0]) // 16
        frac = {}
        for defect in M.DEFECTS:
            if defect == "residual_off" and not (M.residual(case) and case[2] > 1):
                continue
            bad = M.same_bits(M.restate(t, case, act, defect, wave), good)
            frac[defect] = bad.mean()
        print(f"{name} {construction} {act}: outputs changed " + ", ".join(f"{k} {100 * v:.0f} %" for k, v in frac.items()))
        for defect, f in frac.items():
            if defect == "wave_order":
                assert (f > 0) == (construction == "W" and case[4] > 32), (act, defect, f)
            elif defect != "tap_order":
                assert f > 0, (act, defect)
            elif construction == "L":
                assert f == 0, (act, f)
            elif case[1] >= case[6] and case[2] >= case[6]:   # a smaller map has one to six live taps per output
                assert f > 0, (act, defect)


@pytest.mark.parametrize("construction", ["L", "S"])
@pytest.mark.parametrize("name", M.LOOP_CASES)
def test_loop_cases_see_a_stale_halo_slot(name, construction):
    """One halo pixel left over from the tile the workgroup ran before: the second tile's outputs change."""
    good, bad, tile = M.stale_halo(_tensors(name, construction), M.CASES[name], "RE")
    g = M.geom(M.CASES[name])
    assert g["grid"] <= tile < g["ntiles"]
    assert M.same_bits(bad, good).any()


# ------------------------------------------------------------------------------------- geometry
def test_loop_cases_loop_and_every_case_fits():
    """MbwGeom::smem and the launcher's grid rule restated (mbconv_cases.geom).  A change of the
    kernel's geometry that fails this names the cases to move."""
    want = {"loop1": (1300, 512), "loop2": (1300, 512), "loop5": (700, 256)}
    for name, case in M.CASES.items():
        g = M.geom(case)
        assert g["lds"] <= M.LDS_MAX and g["NPXP"] <= 256, (name, g)
        if name in M.LOOP_CASES:
            assert (g["ntiles"], g["grid"]) == want[name] and g["ntiles"] > 2 * g["grid"], (name, g)
        else:
            assert g["ntiles"] <= g["grid"], (name, g)
    assert M.geom(M.CASES["k5s2"])["lds"] == 152320        # the largest K5 / S2 geometry that fits
    assert M.geom(M.REFUSED)["lds"] == 169728 > M.LDS_MAX   # test_gpu_mbconv_exact.py: refused cleanly
    waves = {n: M.geom(c)["nw"] for n, c in M.CASES.items()}
    assert waves["b03"] == 5 and waves["c20"] == 4 and waves["c28"] == 7 and waves["w8k5"] == 8
    assert {M.geom(c)["cinp"] for c in M.CASES.values()} == {16, 24, 32}


def test_budget_shapes_have_enough_outputs():
    for name, (case, act) in M.BUDGET_SHAPES.items():
        pad, Ho, Wo = M.out_dims(case)
        assert case[0] * Ho * Wo * case[5] >= M.BUDGET_MIN_N, name
        assert M.geom(case)["lds"] <= M.LDS_MAX
