"""Digests of what the library's lowering (csrc/lower.hip) produces, for refactors meant to keep it.

    python tools/plan_dump.py > before.txt      (at the old commit)
    python tools/plan_dump.py > after.txt       (at the new one; the files must be identical)

For each (model, nc, tail, B, H, W, u8) configuration under each setting of the lowering switches
(EDGEDET_*), one sha256 per artefact: the packed weight blob of a seeded state dict, workspace_size,
the records resolved against fixed fake weight / workspace bases, edgedet_model_buffers and the op
names.  Every line is lowered in a fresh child process, so no plan cache is shared.  CPU only.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("EDGEDET_SSD_STEM_FUSE=0", "EDGEDET_MB_BLOCK=0", "EDGEDET_CONV_MATH=f32", "EDGEDET_CONV_TUNED=0",
            "EDGEDET_RPN_SPLIT=0", "EDGEDET_SSD_CHAINS=1")
# (model, nc, reduced tail, B, H, W, u8)
CONFIGS = (("ssd", 91, True, 4, 480, 640, False), ("ssd", 91, True, 32, 480, 640, False),
           ("ssd", 91, False, 1, 480, 640, True), ("ssd", 101, True, 4, 480, 640, False),
           ("faster_rcnn", 91, True, 2, 427, 640, False), ("faster_rcnn", 91, True, 1, 640, 640, False),
           ("retinanet", 91, True, 1, 640, 640, False))
CASES = [(c, "") for c in CONFIGS] + [(c, s) for c in (CONFIGS[0], CONFIGS[4]) for s in SWITCHES]
WEIGHTS, WORKSPACE = 0x7000000000, 0x8000000000


def child(cfg):
    from edgeml_amd import native, synthetic
    kind, nc, rt, B, H, W, u8 = cfg
    sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()  # noqa: E731
    sd = synthetic.synthetic_state_dict(kind, nc, rt, seed=3, calibrated=False)
    out = {"blob": sha(native.pack_state_dict(kind, sd, nc, rt).tobytes()),
           "workspace_size": native.workspace_size(kind, B, H, W, nc, rt, u8),
           "records": sha(native.records(kind, B, H, W, WEIGHTS, WORKSPACE, nc, rt, u8).tobytes()),
           "buffers": sha(native.buffers(kind, B, H, W, nc, rt, u8).tobytes()),
           "op_names": sha("\n".join(native.op_names(kind, B, H, W, nc, rt, u8)).encode())}
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1:
        return child(json.loads(sys.argv[1]))
    for cfg, switch in CASES:
        env = {k: v for k, v in os.environ.items() if not k.startswith("EDGEDET_") or k == "EDGEDET_LIB"}
        if switch:
            env.update([switch.split("=")])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(cfg)], env=env, capture_output=True,
                           text=True)
        if r.returncode != 0:
            sys.exit(f"{cfg} {switch}: lowering failed\n{r.stderr}")
        tag = "{} nc={} tail={} B={} {}x{} {}".format(cfg[0], cfg[1], "reduced" if cfg[2] else "full", cfg[3], cfg[4],
                                                      cfg[5], "u8" if cfg[6] else "f32") + (" " + switch if switch else "")
        for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
            print(f"{tag}: {k} {v}", flush=True)


if __name__ == "__main__":
    main()
