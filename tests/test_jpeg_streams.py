"""Crafted-stream conformance of the JPEG ingest on the host (csrc/jpeg.hip: the entropy decoder's
packet, reconstructed by the host checker that shares csrc/jpeg_core.hpp and chroma() with the kernels),
byte for byte against PIL's libjpeg-turbo on files PIL's own encoder never writes (tests/jpeg_streams.py):
several scans, restart intervals 1 and 5, 16-bit tables under SOF1, a table redefined between scans,
components never scanned, sizes from 1 x 1, and the files the decoder must refuse instead of decoding
differently from libjpeg.  tests/test_gpu_jpeg_streams.py runs the same files through the kernels.

On the commit before the fixes 98 of the 624 streams of HOST_SIZES differed (46 of the 4:2:2 / 4:2:0
images up to 4 pixels wide, where libjpeg replicates chroma; all 52 redefined-table files) and all 12 reject
cases were decoded without complaint."""
import numpy as np
import pytest

from edgeml_amd import jpeg, ops
from tests import jpeg_streams as J

_ids = lambda hw: f"{hw[0]}x{hw[1]}"


# ------------------------------------------------------------------------------------ the writer checks itself
@pytest.mark.parametrize("hw", J.HOST_SIZES, ids=_ids)
def test_pil_reads_every_stream(hw):
    """A stream PIL cannot read, or reads with another size, is a bug of the writer."""
    for (name, data), ref in zip(J.variants(*hw), J.references(*hw)):
        assert ref.shape == (3, *hw), name


@pytest.mark.parametrize("sampling", ["444", "422", "420"])
@pytest.mark.parametrize("hw", [(1, 1), (9, 4), (9, 17), (17, 33), (37, 29)], ids=_ids)
def test_scan_structure_does_not_change_pil_pixels(hw, sampling):
    """The same coefficients in one interleaved scan, one scan per component, and chrominance before
    luminance, with and without restart markers, are one image."""
    geo = J.Geometry(*hw, J.SAMPLINGS[sampling])
    coefs = J.quantise(J.make_planes(geo, 5, 2), [J.MID[0], J.MID[1], J.MID[1]])
    tabs = {0: J.MID[0], 1: J.MID[1]}
    want = J.pil_rgb(J.write(geo, coefs, [[0, 1, 2]], tabs, [0, 1, 1]))
    for scans in ([[0], [1], [2]], [[1, 2], [0]], [[2], [0], [1]]):
        for restart in (0, 1, 5):
            got = J.pil_rgb(J.write(geo, coefs, scans, tabs, [0, 1, 1], restart=restart, fill=restart % 2))
            np.testing.assert_array_equal(got, want, err_msg=f"{scans} restart {restart}")


def test_redefined_table_file_is_legitimate():
    """PIL decodes 'DQT 0 = A, scan Y, DQT 0 = B, scans Cb Cr' as its two-table twin."""
    for hw in [(24, 40), (9, 5)]:
        one, two = J.redefined_table_pair(*hw, "420", seed=1, noise=2)
        assert one != two
        np.testing.assert_array_equal(J.pil_rgb(one), J.pil_rgb(two))


def test_streams_reach_every_block_kind():
    """The content gives DC-only blocks, blocks with zero runs of 16 and more (ZRL) and blocks whose
    last coefficient is coded (no EOB), under the quantisers the variants use."""
    geo = J.Geometry(37, 29, J.SAMPLINGS["420"])
    q = lambda t: [t[0], t[1], t[1]]
    assert J.block_kinds(J.quantise(J.make_planes(geo, 1, 0), q((J.flat(255),) * 2)))["dc_only"] > 0
    assert J.block_kinds(J.quantise(J.make_planes(geo, 1, 1), q((J.flat(48),) * 2)))["zrl"] > 0
    assert J.block_kinds(J.quantise(J.make_planes(geo, 1, 2), q((J.flat(1),) * 2)))["full"] > 0


# ------------------------------------------------------------------------------------ decode = PIL
@pytest.mark.parametrize("hw", J.HOST_SIZES, ids=_ids)
def test_host_decode_of_crafted_streams_is_byte_exact(hw):
    wrong = []
    for (name, data), ref in zip(J.variants(*hw), J.references(*hw)):
        pk, got_hw = jpeg.packet(data)
        assert pk is not None, (name, got_hw)
        assert got_hw == hw, name
        got = jpeg.reconstruct_host(pk, got_hw)
        if not np.array_equal(got, ref):
            d = np.abs(got.astype(int) - ref)
            wrong.append(f"{name}: {int((d > 0).sum())} of {d.size} bytes differ, max {int(d.max())}")
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------ rejects
def _restart_file(info):
    return J.stream(40, 56, "420", "il", "mid", 2, seed=3, restart=2, info=info)


def _without_rst(k):
    info = {}
    data = _restart_file(info)
    at = info["rst"][k]
    assert data[at] == 0xFF and 0xD0 <= data[at + 1] <= 0xD7
    return data[:at] + data[at + 2:]


def _renumbered_rst(k, step):
    info = {}
    data = bytearray(_restart_file(info))
    at = info["rst"][k]
    data[at + 1] = 0xD0 + (data[at + 1] - 0xD0 + step) % 8
    return bytes(data)


def _cut(frac, eoi, scans="il"):
    data = J.stream(40, 56, "420", scans, "mid", 2, seed=4)
    sos = data.index(b"\xff\xda")
    at = int(len(data) * frac)
    assert at > sos + 64  # inside entropy data
    return data[:at] + (b"\xff\xd9" if eoi else b"")


def _late_table():
    """Cb is scanned before its table 1 is defined (libjpeg: 'quantization table 0x01 was not defined')."""
    geo = J.Geometry(24, 40, J.SAMPLINGS["420"])
    A, B = J.MID
    coefs = J.quantise(J.make_planes(geo, 6, 1), [A, B, B])
    return J.write(geo, coefs, [[0], [1], [2]], {0: A}, [0, 1, 1], dqt_before={2: {1: B}})


REJECTS = {
    "cut-50": lambda: _cut(0.5, False),
    "cut-80": lambda: _cut(0.8, False),
    "cut-50-eoi": lambda: _cut(0.5, True),
    "cut-80-eoi": lambda: _cut(0.8, True),
    "cut-50-per-component-scans": lambda: _cut(0.5, False, "ni"),
    "cut-80-eoi-per-component-scans": lambda: _cut(0.8, True, "ni"),
    "rst-missing-first": lambda: _without_rst(0),
    "rst-missing-later": lambda: _without_rst(3),
    "rst-out-of-sequence": lambda: _renumbered_rst(2, 2),
    "rst-repeated-number": lambda: _renumbered_rst(4, -1),
    "scan-components-out-of-order": lambda: J.stream(24, 40, "420", [[0, 2, 1]], "mid", 1, seed=5),
    "sos-before-its-table": _late_table,
}


@pytest.mark.parametrize("kind", sorted(REJECTS))
def test_damaged_and_nonconforming_files_are_rejected(kind, tmp_path):
    """Files libjpeg decodes only with a warning (or refuses) never become a packet: packet() raises or
    reports unsupported, and a batch holding one goes to the host decoder (batch_packets None)."""
    data = REJECTS[kind]()
    try:
        pk, _ = jpeg.packet(data)
    except ops.EdgeDetError:
        pk = None
    assert pk is None
    h, w = (40, 56) if kind.startswith(("cut", "rst")) else (24, 40)
    good = J.stream(h, w, "420", "il", "mid", 1, seed=9)
    assert jpeg.packet(good)[0] is not None
    paths = []
    for k, d in enumerate([good, data, good]):
        p = tmp_path / f"{k}.jpg"
        p.write_bytes(d)
        paths.append(str(p))
    assert jpeg.batch_packets([paths[0], paths[2]], 2, pinned=False) is not None
    assert jpeg.batch_packets(paths, 2, pinned=False) is None
    assert jpeg.batch_packets(paths, 1, pinned=False) is None


def test_intact_twins_of_the_rejects_decode():
    """The files the rejects were made from are accepted: the reject rules do not fire on the reader's
    look-ahead into a closing marker, on fill bytes before RSTn, or on eight and more restarts."""
    for data in (_restart_file({}), J.stream(40, 56, "420", "il", "mid", 2, seed=3, restart=2, fill=2),
                 J.stream(40, 56, "420", "ni", "mid", 2, seed=4, restart=1)):
        pk, hw = jpeg.packet(data)
        assert pk is not None and hw == (40, 56)
        np.testing.assert_array_equal(jpeg.reconstruct_host(pk, hw), J.pil_rgb(data))
