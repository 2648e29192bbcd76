"""CONV record addressing on every tile: one conv run dense, then again through a strided view.

The plans never run a conv the way ops.conv2d_nhwc does: the SSD / RetinaNet heads write one buffer
shared by all levels (a batch stride larger than the level, an odd y_off), the FRCNN predictor writes
padded rows, the FPN top-down convs add a nearest-upsampled residual.  That addressing lives in the
epilogue's conv_row_offset (its linear fast paths against the fastdiv path) and in each kernel's
A-loader (lin_x against the general branch).  Addressing changes no arithmetic, so the view run must
equal the dense run of the same tile bit for bit (the dense run is held to torch by
test_gpu_kernels.py); where a view legitimately changes the kernel (tile 0's automatic choice, the
x6b kernels leaving their P1 loader for a lin_x-false input) the run is held to torch fp32 conv2d
under the project's bound instead.  Output parents are larger than the view and filled with a canary
bit pattern: every element outside the view must still hold it afterwards.  The residual parent's
slack holds the same (NaN) pattern and the input's slack NaN, so a stray read poisons the result.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0x7FC5A5A5  # a quiet NaN with a payload: compared as int32, and poison when read as data
SLACK = 64           # floats before the view's first element and after its last row

# name: (B, H, W, Cin, Cout, k, stride, act); M = B * Ho * Wo.  The smallest shapes that put a batch
# boundary inside a 32-row MFMA block, leave M and Cout ragged against every tile and (P, Q: M = 297)
# span two M tiles of the 256-row tiles.
SHAPES = {
    "P": (3, 11, 9, 24, 40, 1, 1, "HS"),
    "Q": (3, 11, 9, 16, 136, 3, 1, "RE"),
    "S": (2, 13, 10, 8, 24, 3, 2, None),
    "P2x": (3, 12, 10, 24, 40, 1, 1, "HS"),    # P / Q at 12 x 10: the exact 2x upsample of a 6 x 5 residual
    "Q2x": (3, 12, 10, 16, 136, 3, 1, "RE"),
    "FC": (5, 1, 1, 24, 40, 1, 1, "HS"),       # P as a fully connected layer (the predictor's form)
    "Q32": (3, 11, 9, 32, 136, 3, 1, "RE"),    # Q with Cin = 32: the pre-split input path needs Cin % 32 == 0
}
LDS_TILES = [1, 2, 3, 4, 5, 6]
X6_TILES = [21, 22, 23, 24, 25, 27, 28, 29, 30, 31, 32, 38, 39]
X6B_TILES = (25, 29, 30, 31, 32, 38, 39)
PW_TILES = [10, 11, 12, 13, 14, 15, 16, 17]
STREAM_TILES = [33, 34, 35]
# (tile, shape): 1-6 and the bf16x6 tiles on P, Q, S; the direct pointwise tiles on P only.  "0" / "0w"
# is the automatic choice without / with the split weight planes.
TILE_SHAPES = [(t, s) for t in ["0", "0w"] + LDS_TILES + X6_TILES for s in "PQS"] + [(t, "P") for t in PW_TILES]


def _tile(t):
    """(tile number, with split planes)."""
    if isinstance(t, str):
        return 0, t.endswith("w")
    return t, t in X6_TILES


def _dims(name):
    B, H, W, Cin, Cout, k, s, act = SHAPES[name]
    pad = (k - 1) // 2
    return B, H, W, Cin, Cout, k, s, act, pad, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


# ------------------------------------------------------------------------------------- views
def _y_view(name, kind):
    """(pixel stride, batch stride, y_off) of an output view."""
    B, H, W, Cin, Cout, k, s, act, pad, Ho, Wo = _dims(name)
    if kind == "dense":
        return Cout, Ho * Wo * Cout, 0
    if kind == "head":    # lin_y false, odd offset: the SSD / RetinaNet class heads
        return Cout, Ho * Wo * Cout + 52, 7
    if kind == "rows":    # lin_y true with gaps between rows: the predictor
        return Cout + 11, Ho * Wo * (Cout + 11), 0
    if kind == "both":
        return Cout + 11, Ho * Wo * (Cout + 11) + 52, 7
    raise KeyError(kind)


def _res_view(name, kind):
    """(pixel stride, batch stride, res_H, res_W) of a residual view (None: no residual)."""
    B, H, W, Cin, Cout, k, s, act, pad, Ho, Wo = _dims(name)
    if kind is None:
        return None
    if kind == "dense":
        return Cout, Ho * Wo * Cout, Ho, Wo
    if kind == "strided":
        return Cout + 5, Ho * Wo * (Cout + 5) + 36, Ho, Wo
    if kind == "rows":    # padded rows, linear batches: lin_res stays true
        return Cout + 5, Ho * Wo * (Cout + 5), Ho, Wo
    if kind == "up":      # FPN top-down: nearest upsample of a 6 x 5 residual
        return Cout, 6 * 5 * Cout, 6, 5
    raise KeyError(kind)


def _x_view(name, kind):
    """(pixel stride, batch stride) of an input view."""
    B, H, W, Cin = SHAPES[name][:4]
    if kind == "dense":
        return Cin, H * W * Cin
    if kind == "xps":     # padded pixels, linear batches: lin_x stays true
        return Cin + 8, H * W * (Cin + 8)
    if kind == "xbs":     # padded batches: lin_x false
        return Cin, H * W * Cin + 20
    if kind == "xboth":
        return Cin + 8, H * W * (Cin + 8) + 20
    raise KeyError(kind)


def _index(B, npix, C, ps, bs, off):
    b = torch.arange(B).view(B, 1, 1) * bs
    p = torch.arange(npix).view(1, npix, 1) * ps
    c = torch.arange(C).view(1, 1, C)
    return (SLACK + off + b + p + c).reshape(-1)


def _parent(vals, ps, bs, off, fill):
    """vals [B, npix, C] laid into a parent of fill (an int32 bit pattern) with SLACK floats on both
    sides -> (device parent as float32, flat indices of the view)."""
    B, npix, C = vals.shape
    idx = _index(B, npix, C, ps, bs, off)
    n = SLACK + off + (B - 1) * bs + (npix - 1) * ps + C + SLACK
    par = torch.full((n,), fill, dtype=torch.int32)
    if vals.dtype == torch.float32:
        par[idx] = vals.reshape(-1).view(torch.int32)
    return par.view(torch.float32).to(DEV), idx


# ------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _data(name, se=False):
    """Host tensors of a shape (fixed per shape, shared by every test), the device weights and the
    torch fp32 references with and without a residual."""
    from edgeml_amd import ops
    from edgeml_amd.plan import pack_conv_weight
    B, H, W, Cin, Cout, k, s, act, pad, Ho, Wo = _dims(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Ho, Wo, Cout, generator=g)
    small = torch.randn(B, 6, 5, Cout, generator=g)
    sc = torch.rand(B, Cin, generator=g) if se else None
    wp = torch.from_numpy(pack_conv_weight(w.numpy())[0]).to(DEV)
    d = dict(x=x, res=res, small=small, sc=sc, wp=wp, w3=ops.split_bf16x3(wp), b=b.to(DEV))
    up = F.interpolate(small.permute(0, 3, 1, 2), size=(Ho, Wo), mode="nearest").permute(0, 2, 3, 1).contiguous()
    d["up"] = up
    xin = x.permute(0, 3, 1, 2) * (sc[:, :, None, None] if se else 1)
    y = F.conv2d(xin, w, b, s, pad).permute(0, 2, 3, 1)
    a = {None: lambda t: t, "RE": F.relu, "HS": F.hardswish}[act]
    d["ref"] = {None: a(y), "full": a(y + res), "up": a(y + up)}
    return d


def _run(name, tile, yv="dense", rv=None, xv="dense", se=False, presplit=False):
    """One CONV record of shape `name` on `tile` with output view yv, residual view rv (None, "dense",
    "strided", "up", or "full-up": the upsampled residual handed over full-size and dense) and input
    view xv.  Returns the view's values [B, Ho, Wo, Cout] on the host after checking that nothing
    outside the view changed."""
    from edgeml_amd import ops
    B, H, W, Cin, Cout, k, s, act, pad, Ho, Wo = _dims(name)
    d = _data(name, se)
    tnum, x6 = _tile(tile)
    x_ps, x_bs = _x_view(name, xv)
    xpar, _ = _parent(d["x"].reshape(B, H * W, Cin), x_ps, x_bs, 0, 0x7FC00000)
    y_ps, y_bs, y_off = _y_view(name, yv)
    ypar, yidx = _parent(torch.empty(B, Ho * Wo, Cout, dtype=torch.int32), y_ps, y_bs, y_off, CANARY)
    rpar, r_ps, r_bs, rH, rW = None, Cout, Ho * Wo * Cout, Ho, Wo
    if rv is not None:
        src = {"dense": d["res"], "strided": d["res"], "rows": d["res"], "up": d["small"], "full-up": d["up"]}[rv]
        r_ps, r_bs, rH, rW = _res_view(name, "dense" if rv == "full-up" else rv)
        rpar, _ = _parent(src.reshape(B, rH * rW, Cout), r_ps, r_bs, 0, CANARY)
    sc = d["sc"].to(DEV) if se else None
    x3 = torch.empty(3 * B * H * W * Cin + 32, dtype=torch.int16, device=DEV) if presplit else None
    # x / y / res point at the parent's element SLACK (256 bytes in: the alignment is kept)
    inside = lambda t: None if t is None else t.data_ptr() + 4 * SLACK  # noqa: E731
    rec = ops.conv_record((B, H, W, Cin), Cout, k, s, pad, act, inside(xpar), d["wp"], d["b"], inside(ypar),
                          res=inside(rpar), in_scale=sc, w3=d["w3"] if x6 else None, x3=x3, x_pstride=x_ps,
                          y_pstride=y_ps, res_pstride=r_ps, x_bstride=x_bs, y_bstride=y_bs, res_bstride=r_bs,
                          y_off=y_off, res_hw=(rH, rW), tile=tnum)
    try:
        ops.check(ops.lib().edgedet_plan_run(rec.ctypes.data_as(ctypes.c_void_p), 1, ops.stream_handle()))
    finally:
        torch.cuda.synchronize()
        out = ypar.cpu().view(torch.int32)
        outside = torch.ones(out.numel(), dtype=torch.bool)
        outside[yidx] = False
        bad = int((out[outside] != CANARY).sum())
        assert bad == 0, f"{bad} elements outside the output view were written"
    got = out[yidx].view(torch.float32).reshape(B, Ho, Wo, Cout)
    assert int((out[yidx] == CANARY).sum()) == 0, "elements of the output view were never written"
    return got


def _close(got, ref):
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all() and err < 1e-4 * max(1.0, ref.abs().max().item()), err


def _same(name, tile, view, dense, ref_key):
    """The view run equals the dense run bit for bit; tile 0 may resolve to another kernel for a view
    and is held to torch instead."""
    got = _run(name, tile, **view)
    if _tile(tile)[0] == 0:
        _close(got, _data(name, False)["ref"][ref_key])
    else:
        want = _run(name, tile, **dense)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
            (int((got != want).sum()), (got - want).abs().max().item())


# ------------------------------------------------------------------------------------- output views
@pytest.mark.parametrize("yv", ["head", "rows", "both"])
@pytest.mark.parametrize("tile,name", TILE_SHAPES)
def test_conv_output_view(tile, name, yv):
    _same(name, tile, dict(yv=yv), dict(), None)


@pytest.mark.parametrize("tile", LDS_TILES + X6_TILES + PW_TILES + STREAM_TILES)
def test_conv_rows_view_fc(tile):
    """The predictor's form: B = 5 rows of a 1 x 1 map written with a padded row stride (lin_y true;
    the streaming tiles 33-35 accept it too)."""
    _same("FC", tile, dict(yv="rows"), dict(), None)


# ------------------------------------------------------------------------------------- residual views
@pytest.mark.parametrize("yv", ["dense", "head"])
@pytest.mark.parametrize("tile,name", TILE_SHAPES)
def test_conv_residual_strided(tile, name, yv):
    _same(name, tile, dict(yv=yv, rv="strided"), dict(rv="dense"), "full")


@pytest.mark.parametrize("yv", ["dense", "head"])
@pytest.mark.parametrize("tile,name", [(t, s + x) for t, s in TILE_SHAPES if s != "S" for x in ("", "2x")])
def test_conv_residual_upsampled(tile, name, yv):
    """The FPN top-down add: an 11 x 9 (and, exactly 2x, a 12 x 10) output takes its residual from a
    6 x 5 map by nearest index; the dense counterpart gets F.interpolate(mode="nearest") full-size."""
    _same(name, tile, dict(yv=yv, rv="up"), dict(rv="full-up"), "up")


# ------------------------------------------------------------------------------------- input views
X_CASES = [(t, "P") for t in (3, 5, 13, 16, 23, 25, 29, 31, 38, 39)] + [(t, "Q") for t in (3, 21, 25, 31)]


@pytest.mark.parametrize("xv", ["xps", "xbs", "xboth"])
@pytest.mark.parametrize("tile,name", X_CASES)
def test_conv_input_view(tile, name, xv):
    """Input views (record fields conv_prepare accepts; no lowering uses them), the slack NaN.  A
    padded pixel stride keeps lin_x; a padded batch stride clears it, and the kernels take their
    general loaders: the direct pointwise tiles refuse (test_conv_pointwise_refuses_nonlinear_input),
    the x6b tiles leave their P1 loader (another summation order) and are held to torch."""
    from edgeml_amd import ops
    lin_x = name == "P" and xv == "xps"
    if name == "P" and not lin_x and tile in PW_TILES:
        with pytest.raises(ops.EdgeDetError):
            _run(name, tile, xv=xv)
        return
    got = _run(name, tile, xv=xv)
    if name == "P" and not lin_x and tile in X6B_TILES:
        _close(got, _data(name, False)["ref"][None])
    else:
        want = _run(name, tile)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got - want).abs().max().item()


@pytest.mark.parametrize("xv", ["xbs", "xboth"])
@pytest.mark.parametrize("tile", PW_TILES + STREAM_TILES)
def test_conv_pointwise_refuses_nonlinear_input(tile, xv):
    """Tiles 10-17 and 33-35 address pixel m at m * x_pstride: a padded batch stride (lin_x false) is
    the launchers' documented refusal, and nothing is written."""
    from edgeml_amd import ops
    with pytest.raises(ops.EdgeDetError):
        _run("P", tile, xv=xv)


# ------------------------------------------------------------------------------------- input transform
def test_conv_presplit_se_scale_head_view():
    """Tile 25 with the SE input scale and the input split up front (the x3 scratch) through the head
    view: bit-identical to its dense run, and both match torch."""
    dense = _run("Q32", 25, se=True, presplit=True)
    got = _run("Q32", 25, yv="head", se=True, presplit=True)
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32))
    _close(got, _data("Q32", True)["ref"][None])


# ------------------------------------------------------------------------------------- streaming tiles
@pytest.mark.parametrize("view", [dict(yv="head"), dict(yv="both"), dict(rv="strided"), dict(rv="up"),
                                  dict(yv="head", rv="dense")], ids=lambda v: "-".join(f"{k}={v[k]}" for k in v))
@pytest.mark.parametrize("tile", STREAM_TILES)
def test_conv_pointwise_stream_refuses_views(tile, view):
    """Tiles 33-35 keep a lean epilogue (one base address per lane, uniform row stride): an output or
    residual whose batches are not linear is refused by the launcher, and the canary stays intact
    (checked by _run on the way out)."""
    from edgeml_amd import ops
    with pytest.raises(ops.EdgeDetError):
        _run("P", tile, **view)


@pytest.mark.parametrize("tile", STREAM_TILES)
def test_conv_pointwise_stream_linear_views(tile):
    """What tiles 33-35 do accept: padded rows with linear batches, for the output and the residual."""
    d = _data("P", False)
    got = _run("P", tile, yv="rows")
    assert torch.equal(got.view(torch.int32), _run("P", tile).view(torch.int32))
    _close(got, d["ref"][None])
    got = _run("P", tile, yv="rows", rv="rows")
    assert torch.equal(got.view(torch.int32), _run("P", tile, rv="dense").view(torch.int32))
    _close(got, d["ref"]["full"])
