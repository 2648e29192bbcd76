"""Host side of edgeml_amd.baseline (the drop-in for baseline.py): the argument parser, get_area, the
output / model paths, the (conf, area) packing and the area grid.  No device needed."""
import os

import numpy as np
import pytest


def test_parser_defaults_are_the_references():
    from edgeml_amd import baseline
    o = baseline.getargs(["data", "reward.npz", "split.npy", "save"])
    assert (o.data_dir, o.reward_path, o.split_path, o.save_dir) == ("data", "reward.npz", "split.npy", "save")
    assert o.baseline == "af" and o.positive_weight == 3.0 and isinstance(o.positive_weight, float)
    assert o.label_dir == "" and o.model_dir == ""
    o = baseline.getargs(["d", "r", "s", "o", "--baseline", "dcsb", "--positive_weight", "2", "--label_dir", "L",
                          "--model_dir", "M"])
    assert (o.baseline, o.positive_weight, o.label_dir, o.model_dir) == ("dcsb", 2.0, "L", "M")
    with pytest.raises(SystemExit):
        baseline.getargs(["d", "r", "s", "o", "--baseline", "svm"])


def test_get_area_is_float64_xyxy():
    from edgeml_amd import baseline
    b = np.array([[0.1, 0.2, 0.7, 0.5], [0.0, 0.0, 1.0, 1.0], [0.3, 0.3, 0.3, 0.9]])
    a = baseline.get_area(b)
    assert a.dtype == np.float64
    np.testing.assert_array_equal(a, (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    assert a[1] == 1.0 and a[2] == 0.0


def test_output_and_model_paths():
    from edgeml_amd import baseline
    assert baseline.result_dir("save", "af", 3.0) == os.path.join("save", "3.0")
    assert baseline.result_dir("save", "af", 0.5) == os.path.join("save", "0.5")
    assert baseline.result_dir("save", "dcsb", 3.0) == "save"
    assert baseline.model_save_dir("m", "af", 3.0) == os.path.join("m", "3.0")
    assert baseline.model_save_dir("m", "dcsb", 3.0) == "m"
    assert baseline.model_path(os.path.join("m", "3.0"), 0) == os.path.join("m", "3.0", "wts1.pickle")


def test_conf_area_packing_with_empty_images():
    from edgeml_amd import baseline
    xyxy = np.array([[0.0, 0.0, 0.5, 0.5], [0.25, 0.25, 1.0, 0.75]])
    weak = [(), (np.array([1, 2]), xyxy, np.array([0.9, 0.4])), (), (np.array([3]), xyxy[:1], np.array([0.5]))]
    dets = baseline.dcsb_inputs(weak)
    assert len(dets) == 4
    for i in (0, 2):
        assert dets[i][0].shape == (0,) and dets[i][1].shape == (0,)
    np.testing.assert_array_equal(dets[1][0], [0.9, 0.4])
    np.testing.assert_array_equal(dets[1][1], [0.25, 0.375])
    conf, area, off = baseline.pack_dets(dets)
    assert conf.dtype == area.dtype == np.float64 and off.dtype == np.int64
    np.testing.assert_array_equal(off, [0, 0, 2, 2, 3])
    np.testing.assert_array_equal(conf, [0.9, 0.4, 0.5])
    np.testing.assert_array_equal(area, [0.25, 0.375, 0.25])
    conf, area, off = baseline.pack_dets([(np.array([]), np.array([]))] * 3)
    assert conf.shape == area.shape == (0,) and off.tolist() == [0, 0, 0, 0]


def test_area_grid_is_numpys_arange():
    from edgeml_amd import baseline
    g = baseline.area_grid()
    assert g.dtype == np.float64 and g.shape == (70,)
    np.testing.assert_array_equal(g, np.arange(0.2, 0.9, 0.01))
    assert g[0] == 0.2 and g[-1] == 0.8900000000000006


def test_feature_padding_to_the_matrix_tile():
    from edgeml_amd import baseline
    x = np.arange(3 * 145, dtype=np.float64).reshape(3, 145)
    xt, d = baseline.pad_features(x)
    assert d == 145 and xt.shape == (3, 160) and xt.dtype == np.float64
    np.testing.assert_array_equal(xt[:, :145], x)
    assert np.all(xt[:, 145] == 1.0) and np.all(xt[:, 146:] == 0.0)
    assert baseline.pad_features(np.zeros((2, 15)))[0].shape == (2, 16)
    assert baseline.pad_features(np.zeros((2, 16)))[0].shape == (2, 32)


def test_there_is_no_cpu_path():
    import torch
    from edgeml_amd import baseline
    if torch.cuda.is_available():
        return  # the refusal only exists where no device does
    split = np.array([[True, False, False], [False, True, False]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        baseline.fit_af_folds(np.zeros((3, 4)), np.array([0, 1, 0]), split)
    with pytest.raises(RuntimeError, match="no CPU path"):
        baseline.fit_dcsb_folds([(np.array([]), np.array([]))] * 3, np.zeros(3, int), np.array([0, 1, 0]), split)
