"""G10: the SSD stem's outputs as the library of one commit computes them (csrc/layers.hip ssd_stem_kernel
through SSD_STEM records), the fixture of tests/test_gpu_stem_exact.py: a later change to the stem that keeps
its arithmetic must reproduce these bytes.

Run once on an MI355X with libedgedet.so built from the commit that is to be the reference (or that library
named by EDGEDET_LIB), passing the commit's hash:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stem.py COMMIT [OUT.npz]

Inputs and weights: tests/stem_cases.py (seeded).  For every case, with the SSD and the ImageNet
normalisation, the fused stem on the uint8 source is run; it must equal the non-fused stem behind the
transform record and the fused stem on the float image / 255 (asserted here, so the fixture stands for all
forms).  Stored (only data): the full output array of the small cases, the SHA-256 of the output bytes of
every case, and the producing commit.  Writes tests/golden/g10_stem_exact.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import stem_cases as SC  # noqa: E402


def main():
    if len(sys.argv) < 2:
        raise SystemExit("usage: make_golden_stem.py COMMIT [OUT.npz]")
    out = {"commit": np.array(sys.argv[1]), "library": np.array(os.path.basename(os.environ.get("EDGEDET_LIB", "libedgedet.so")))}
    for case in SC.CASES:
        for norm in SC.NORMS:
            plain, fused = SC.run(case, True, norm)
            plain_f, fused_f = SC.run(case, False, norm)
            assert torch.isfinite(fused).all()
            assert torch.equal(plain, fused) and torch.equal(plain_f, fused) and torch.equal(fused_f, fused), (case, norm)
            key = f"{case[0]}/{norm}"
            out[key + "/sha256"] = np.array(SC.digest(fused))
            if case[0] not in SC.DIGEST_ONLY:
                out[key + "/y"] = fused.cpu().numpy()
            print(key, tuple(fused.shape), out[key + "/sha256"])
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "g10_stem_exact.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
