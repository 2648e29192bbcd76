"""Host-side checks of the cascade's hidden-layer decision (edgeml_amd.tapnet / maps, csrc/tapnet.hip's fit rule,
csrc/lower.hip's stage table): the table against arch.ssdlite_table, load_estimator(stage=), the fit rule at its
boundary, the exports and the CLI refusals.  No device needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# H = W of every stage's map for the 320 x 320 input (the strides of mobilenet_v3_large and the extra blocks)
SIDE = {1: 160, 2: 80, 3: 80, 4: 40, 5: 40, 6: 40, 7: 20, 8: 20, 9: 20, 10: 20, 11: 20, 12: 20, 13: 10, 14: 10, 15: 10,
        16: 10, 17: 5, 18: 3, 19: 2, 20: 1}


def _table_channels(table, buffer):
    """Output channels of the layer whose output the buffer holds, from the state-dict table."""
    key = buffer + ".0.weight"
    if key not in table:  # a whole block's output (the fused stem + block, an MBCONV record): its last conv
        keys = [k for k in table if k.startswith(buffer + ".block.") and k.endswith(".0.weight")]
        key = sorted(keys, key=lambda k: int(k[len(buffer) + 7:].split(".")[0]))[-1]
    return int(table[key][0])


@pytest.mark.parametrize("reduced", [True, False])
def test_stage_table_against_the_state_dict_table(reduced):
    from edgeml_amd import arch, tapnet
    table = arch.ssdlite_table(91, reduced)
    taps = tapnet.stage_table(91, reduced)
    assert [t.stage for t in taps] == list(range(1, 21))
    by = {t.stage: t for t in taps}
    for s, t in by.items():
        assert (t.H, t.W) == (SIDE[s], SIDE[s]), t
        assert t.C == _table_channels(table, t.buffer), t
        assert t.token == ("IR" if s <= 15 else "Conv" if s == 16 else "Extra")
        assert (t.chain, t.image0, t.images) == (0, 0, 1)
    assert [by[s].buffer for s in (17, 18, 19, 20)] == [f"backbone.extra.{e}.2" for e in range(4)]
    assert by[13].buffer == "backbone.features.1.0.3" and by[16].buffer == "backbone.features.1.3"
    assert all(by[s].buffer.startswith(f"backbone.features.0.{s}") for s in range(1, 13))
    assert (by[1].C, by[1].H) == (16, 160) and (by[7].C, by[7].H) == (80, 20)
    assert (by[13].C, by[13].H) == (80 if reduced else 160, 10)
    assert by[16].C == (480 if reduced else 960)
    assert tapnet.ssd_names(91, reduced) == {s: by[s].token for s in by}


def test_stage_table_chains_tile_the_batch():
    from edgeml_amd import tapnet
    for B in (32, 37, 4):
        for s in (1, 7, 20):
            taps = tapnet.stage_table(91, True, B=B, H=480, W=640, u8=True, stage=s)
            assert [t.chain for t in taps] == list(range(len(taps)))
            pos = 0
            for t in taps:
                assert t.image0 == pos and t.images >= 1 and t.stage == s
                pos += t.images
            assert pos == B
            assert len({t.buffer for t in taps}) == len(taps)
    assert len(tapnet.stage_table(91, True, B=32, stage=7)) == 2 and len(tapnet.stage_table(91, True, B=4, stage=7)) == 1


def test_stage_refusals():
    from edgeml_amd import tapnet
    with pytest.raises(ValueError, match="EDGEDET_SSD_STEM_FUSE"):
        tapnet.stage_table(stage=0)
    for s in (21, 24, -2):
        with pytest.raises(ValueError, match="stage table"):
            tapnet.stage_table(stage=s)


def _save(tmp_path, cin, channels, kernels, pools, hidden, S):
    from edgeml_amd import convnet
    spec = convnet.ConvSpec(cin, channels, kernels, pools, hidden, (S, S) if S else None, bool(S))
    state = spec.init_state(np.random.default_rng(0))
    convnet.save_state(str(tmp_path), spec, state, 0)
    return spec, state, str(tmp_path / "wts1.pth")


def test_load_estimator_with_a_stage(tmp_path):
    from edgeml_amd import offload
    spec, state, path = _save(tmp_path, 80, [8, 4], [3, 3], [True, True], [16, 16], 8)
    with pytest.raises(ValueError, match="conv_stacks"):  # no stage: refused exactly as before
        offload.load_estimator(path, 205)
    est = offload.load_estimator(path, 205, stage=7, resize=8)
    assert est.kind == "convnet" and est.stage == 7 and est.resize == 8 and est.map_shape == (80, 20, 20)
    sp = est.net.spec
    assert (sp.cin, sp.channels, sp.kernels, sp.pools, sp.dims) == (80, [8, 4], [3, 3], [True, True], [16, 16, 16, 1])
    assert est.net.state.tobytes() == state.tobytes() and est.net.fits
    assert est.net.use_fused() is False  # the layered forward is the default
    assert offload.load_estimator(path, 205, stage=7, resize=8, fused=True).net.use_fused() is True
    # a wrong Cin: stage 6 has 40 channels; the message names both numbers
    with pytest.raises(ValueError, match=r"80 channels.*40"):
        offload.load_estimator(path, 205, stage=6, resize=8)
    # a wrong pooled width: S = 12 gives 4 * 3 * 3 = 36 inputs, the file has 16
    with pytest.raises(ValueError, match=r"takes 16 inputs.*gives 36"):
        offload.load_estimator(path, 205, stage=7, resize=12)
    with pytest.raises(ValueError, match=r"--stage N and --resize S"):
        offload.load_estimator(path, 205, stage=7)
    with pytest.raises(ValueError, match="stage table"):
        offload.load_estimator(path, 205, stage=24, resize=8)


def test_load_estimator_takes_a_resize_0_file_as_layered(tmp_path):
    from edgeml_amd import offload
    spec, state, path = _save(tmp_path, 80, [8, 4], [3, 3], [True, False], [16], 0)
    est = offload.load_estimator(path, 205, stage=7, resize=0, pools=[1, 0])
    assert est.kind == "convnet" and est.resize == 0 and not est.net.spec.resize and not est.net.fits
    assert est.net.spec.dims == [4, 16, 1] and est.net.state.tobytes() == state.tobytes()
    with pytest.raises(ValueError, match="fused kernel does not take"):
        est.net.use_fused(True)
    assert est.net.use_fused() is False
    with pytest.raises(ValueError, match="--fused"):
        offload.load_estimator(path, 205, stage=7, resize=0, pools=[1, 0], fused=True)


def _net(S, cin, channels, kernels, pools, hidden):
    from edgeml_amd import convnet
    spec = convnet.ConvSpec(cin, channels, kernels, pools, hidden, (S, S), True)
    i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(x) for x in v])  # noqa: E731
    return spec, (S, cin, len(channels), i32(channels), i32(kernels), i32(pools), len(spec.dims) - 1, i32(spec.dims))


def test_fit_rule_agrees_with_the_launcher_at_its_boundary():
    """The planes of [S][S][C] -> conv -> [S][S][C] are two regions of S S (C + 1) floats: at S = 8 that is
    512 (C + 1) bytes, within 160 KiB up to C = 316 and beyond it from C = 320.  The launcher answers
    EDGEDET_TAPNET_NOFIT exactly where the rule says no, before it looks at a pointer (null here)."""
    from edgeml_amd import ops
    L = ops.lib()
    codes = {}
    for C in (312, 316, 320, 324):
        spec, net = _net(8, C, [C], [3], [False], [16])
        lds = L.edgedet_tapnet_lds(*net)
        assert lds == 2 * 4 * 64 * (C + 1)
        fits = L.edgedet_tapnet_fits(*net)
        assert fits == int(lds <= 160 * 1024)
        codes[C] = (fits, L.edgedet_tapnet_infer(None, 1, *net, None, spec.ns, 0.0, None, None, None))
    assert codes == {312: (1, -1), 316: (1, -1), 320: (0, ops.TAPNET_NOFIT), 324: (0, ops.TAPNET_NOFIT)}
    # the regions alternate: input (region 0), conv output (1), pooled map (0), hidden vectors (1, 0, ...)
    spec, net = _net(8, 40, [64, 32], [3, 3], [True, True], [16, 16, 16, 16])
    assert L.edgedet_tapnet_lds(*net) == 4 * (64 * 41 + 64 * 65) and L.edgedet_tapnet_fits(*net) == 1
    # what is not such a net at all: an even kernel, channels not a multiple of 4, a pool on a 1 x 1 map
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    for S, cin, ch, k, pool, dims in ((8, 40, 8, 2, 0, [512, 1]), (8, 40, 6, 3, 0, [384, 1]), (8, 42, 8, 3, 0, [512, 1]),
                                      (1, 16, 4, 3, 1, [4, 1]), (8, 40, 8, 3, 0, [500, 1])):
        net = (S, cin, 1, i32([ch]), i32([k]), i32([pool]), 1, i32(dims))
        assert L.edgedet_tapnet_fits(*net) == 0 and L.edgedet_tapnet_lds(*net) == -1
        assert L.edgedet_tapnet_infer(None, 1, *net, None, 0, 0.0, None, None, None) == ops.TAPNET_NOFIT


def test_exports_declared_defined_and_bound():
    from edgeml_amd import ops
    names = [n for n in ops.EXPORTS if n.startswith("edgedet_tapnet_")] + ["edgedet_ssdlite_taps"]
    assert sorted(names) == ["edgedet_ssdlite_taps", "edgedet_tapnet_finish", "edgedet_tapnet_fits",
                             "edgedet_tapnet_infer", "edgedet_tapnet_lds"]
    assert "edgedet_ssdlite_taps" in ops.EXPORTS
    header = open(os.path.join(ROOT, "include", "edgedet.h")).read()
    csrc = os.path.join(ROOT, "edgeml-object-detection_amd", "csrc")
    src = open(os.path.join(csrc, "tapnet.hip")).read() + open(os.path.join(csrc, "lower.hip")).read()
    opsrc = open(os.path.join(ROOT, "edgeml-object-detection_amd", "ops.py")).read()
    L = ops.lib()
    for n in names:
        assert re.search(rf"\b(int|int64_t) {n}\(", header), n
        assert re.search(rf'extern "C" (int|int64_t) {n}\(', src), n
        assert f"L.{n}.argtypes" in opsrc, n
        assert hasattr(L, n), n
    assert not any(n.startswith("edgedet_cnn_") for n in names)


def test_cli_refusals(tmp_path):
    from edgeml_amd import convnet, maps, offload
    with pytest.raises(SystemExit, match="EDGEDET_SSD_STEM_FUSE"):
        maps.main(maps.getargs(["i", str(tmp_path / "f"), "--stages", "7", "0"]))
    with pytest.raises(SystemExit, match="stage_table"):
        maps.main(maps.getargs(["i", str(tmp_path / "f"), "--stages", "21"]))
    with pytest.raises(SystemExit, match="--model ssd"):
        maps.main(maps.getargs(["i", str(tmp_path / "f"), "--stages", "7", "--model", "faster_rcnn"]))
    assert not (tmp_path / "f").exists()
    args = lambda *e: convnet.getargs(["d", "r", "s", "o", "--channels", "8", *e])  # noqa: E731
    with pytest.raises(SystemExit, match="stage_table"):
        convnet.main(args("--weak", "ssd", "--stage", "22"))
    with pytest.raises(SystemExit, match="stage_table"):
        convnet.main(args("--weak", "ssd"))  # --stage 24, the default, is not an SSDLite stage
    with pytest.raises(SystemExit, match="EDGEDET_SSD_STEM_FUSE"):
        convnet.main(args("--weak", "ssd", "--stage", "0"))
    assert convnet.check_args(args("--weak", "ssd", "--stage", "20")) == ([3], [True])
    assert args().weak == "yolov5"
    with pytest.raises(SystemExit, match="YOLOv5 stages are 0-23"):
        convnet.main(args("--stage", "30"))
    # the offload CLI: a conv-stack file without --stage / --resize names both
    spec, state, path = _save(tmp_path, 80, [8, 4], [3, 3], [True, True], [16], 8)
    base = ["i", str(tmp_path / "o"), "--estimator", path, "--threshold", "0"]
    with pytest.raises(SystemExit, match=r"--stage N.*--resize S"):
        offload.main(offload.getargs(base))
    with pytest.raises(SystemExit, match=r"--stage N and --resize S"):
        offload.main(offload.getargs(base + ["--stage", "7"]))
    with pytest.raises(SystemExit, match=r"80 channels.*40"):
        offload.main(offload.getargs(base + ["--stage", "6", "--resize", "8"]))


def test_load_maps_takes_a_name_table(tmp_path):
    from edgeml_amd import convnet, tapnet
    for i in range(2):
        d = tmp_path / f"im{i}"
        d.mkdir()
        np.save(d / "stage7_IR_features.npy", np.full((4, 2, 2), i, np.float32))
        np.save(d / "stage7_Conv_features.npy", np.full((4, 2, 2), 10 + i, np.float32))
    assert [float(m[0, 0, 0]) for m in convnet.load_maps(str(tmp_path), 7, tapnet.ssd_names())] == [0.0, 1.0]
    assert [float(m[0, 0, 0]) for m in convnet.load_maps(str(tmp_path), 7)] == [10.0, 11.0]  # YOLOv5's stage 7: Conv
