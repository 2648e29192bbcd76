"""The device JPEG reconstruction (csrc/jpeg.hip jpeg_idct_kernel + jpeg_color_kernel) byte-exact
against PIL's libjpeg-turbo on the crafted streams of tests/jpeg_streams.py, at the sizes PIL-written
pictures never bring to the kernels: fewer than one wave's worth of blocks up to a few workgroups, one
block, one row, one column, ch == 1, cw <= 2 (replicated chroma) and the first width above it.  One
BatchDecoder.decode launch per size holds every variant of that size, so packets of gray (one plane),
4:4:4, 4:2:2 and 4:2:0, of one and of several scans, with restart intervals, 16-bit tables, blocks
without a coefficient (chroma never scanned) and a redefined table share one grid.
tests/test_jpeg_streams.py checks the same files on the host."""
import numpy as np
import pytest
import torch

from tests import jpeg_streams as J

pytestmark = pytest.mark.gpu


def _packets(hw, pinned=False):
    from edgeml_amd import jpeg
    pks = []
    for name, data in J.variants(*hw):
        pk, got = jpeg.packet(data, pinned=pinned)
        assert pk is not None and got == hw, name
        pks.append(pk)
    return pks


def _decode_and_check(dec, hw, pks):
    out = torch.full((len(pks), 3, *hw), 0x5A, dtype=torch.uint8, device="cuda")
    dec.decode(pks, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    wrong = []
    for b, ((name, _), ref) in enumerate(zip(J.variants(*hw), J.references(*hw))):
        if not np.array_equal(got[b], ref):
            d = np.abs(got[b].astype(int) - ref)
            wrong.append(f"{name}: {int((d > 0).sum())} of {d.size} bytes differ, max {int(d.max())}")
    assert not wrong, f"{hw}\n" + "\n".join(wrong)


@pytest.mark.parametrize("hw", J.DEVICE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_gpu_decode_of_crafted_streams_is_byte_exact(hw):
    from edgeml_amd import jpeg
    pks = _packets(hw)
    assert len({jpeg.plane_bytes(p) for p in pks}) > 1  # block counts differ within the launch
    _decode_and_check(jpeg.BatchDecoder("cuda"), hw, pks)


def test_gpu_decoder_reused_across_sizes():
    """Largest batch, smallest, largest again through one BatchDecoder: the staging, device and plane
    buffers are then larger than the batch needs and hold the previous batch's bytes."""
    from edgeml_amd import jpeg
    dec = jpeg.BatchDecoder("cuda")
    for hw in ((37, 29), (1, 1), (37, 29)):
        _decode_and_check(dec, hw, _packets(hw))


def test_gpu_decode_of_pinned_packets():
    """packet(..., pinned=True): decode()'s direct upload, every packet copied from its own pinned block."""
    from edgeml_amd import jpeg
    hw = (17, 33)
    pks = _packets(hw, pinned=True)
    assert all(torch.is_tensor(p) and p.is_pinned() for p in pks)
    _decode_and_check(jpeg.BatchDecoder("cuda"), hw, pks)
