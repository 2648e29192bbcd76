"""Timing of the cascade's hidden-layer decision on the device: the fused launch (csrc/tapnet.hip)
against the layered eval forward, alone and inside the weak stage of edgeml_amd.offload.

    python tools/tapnet_bench.py [--out FILE] [--images 1024] [--rounds 5] [--kernels-only]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/tapnet_bench.py --kernels-only   # the kernels' own durations

Kernel alone: the same device tensors, B = 32 pooled stage-7 maps (80 channels), S = 8, channels 64 32, hidden
16 16 16 16; after a warm-up the two paths alternate, `--rounds` windows of 200 calls each, timed by device events
(and by the host clock around the window, which ends in a synchronise).  Weak stage: edgeml_amd.offload.run on
`--images` seeded synthetic JPEGs with a threshold no estimate exceeds (nothing reaches the strong model), the
convnet estimator fused and layered and a stage-24 MLP estimator alternating, the first round of each as warm-up;
the figure is run()'s "engine" host seconds (decode, weak model, hook, result copies).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_alone(rounds, calls, say):
    from edgeml_amd import convnet, tapnet
    from tests import tapnet_cases as T
    spec = convnet.ConvSpec(80, [64, 32], [3, 3], [True, True], [16, 16, 16, 16], (8, 8), True)
    net = tapnet.TapNet(spec, T.trained_state(spec, 3))
    x = torch.from_numpy(T.trained_maps(spec, 4, 32)).to("cuda:0")
    est = torch.empty(32, dtype=torch.float64, device="cuda:0")
    flag = torch.empty(32, dtype=torch.uint8, device="cuda:0")
    say(f"kernel alone: B 32, Cin 80, S 8, channels 64 32, hidden 16 16 16 16; fits {net.fits}, LDS {net.lds_bytes()} B; "
        f"{calls} calls per window")
    got = {}
    for fused in (True, False):  # warm-up: code objects, the Trainer's buffers
        for _ in range(20):
            net.infer(x, 0.0, est, flag, fused=fused)
        torch.cuda.synchronize()
        got[fused] = est.cpu().numpy().copy()
    say(f"  max |fused - layered| = {np.abs(got[True] - got[False]).max():.3e} (estimates of std {got[True].std():.3e})")
    res = {True: [], False: []}
    for r in range(rounds):
        for fused in (True, False):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                net.infer(x, 0.0, est, flag, fused=fused)
            b.record()
            enq = (time.perf_counter() - t0) / calls * 1e6  # the host's enqueue alone: equal to the rest = host-bound
            torch.cuda.synchronize()
            host = (time.perf_counter() - t0) / calls * 1e6
            dev = a.elapsed_time(b) / calls * 1e3
            res[fused].append((dev, host))
            say(f"  round {r} {'fused  ' if fused else 'layered'}: {dev:8.2f} us/call device events, {host:8.2f} us/call host "
                f"to the synchronise, {enq:8.2f} us/call host enqueue")
    for fused in (True, False):
        d = sorted(v[0] for v in res[fused])
        say(f"  {'fused  ' if fused else 'layered'} median {d[len(d) // 2]:8.2f} us/call (min {d[0]:.2f}, max {d[-1]:.2f})")


def weak_stage(images, rounds, say):
    from PIL import Image
    from edgeml_amd import convnet, detect, estimator, offload, synthetic, tapnet
    from tests import tapnet_cases as T
    spec = convnet.ConvSpec(80, [64, 32], [3, 3], [True, True], [16, 16, 16, 16], (8, 8), True)
    state = T.trained_state(spec, 3)
    dims = [205, 16, 16, 16, 16, 1]
    ms = estimator.MlpSpec(dims)
    ests = {"convnet fused": offload.Estimator("convnet", 205, net=tapnet.TapNet(spec, state, fused=True), stage=7, resize=8,
                                               map_shape=(80, 20, 20)),
            "convnet layered": offload.Estimator("convnet", 205, net=tapnet.TapNet(spec, state), stage=7,
                                                 resize=8, map_shape=(80, 20, 20)),
            "stage-24 mlp": offload.Estimator("mlp", 205, dims=dims, state=ms.init_state(np.random.default_rng(1)))}
    with tempfile.TemporaryDirectory() as d:
        scenes = [Image.fromarray(synthetic.make_scene(9000 + i, 480, 640).transpose(1, 2, 0)) for i in range(16)]
        for i in range(images):
            scenes[i % 16].save(os.path.join(d, f"{i:012d}.jpg"))
        weak = detect.load_weak_models("ssd", "", 91).to("cuda:0")
        say(f"weak stage: {images} JPEGs of 480 x 640, weak batch 32, threshold above every estimate; engine seconds of "
            f"offload.run, round 0 is the warm-up")
        res = {k: [] for k in ests}
        for r in range(rounds + 1):
            for k, e in ests.items():
                out = offload.run(d, e, 1e30, weak=weak, weak_batch=32)
                assert not out["offloaded"].any()
                s = out["seconds"]["engine"]
                if r:
                    res[k].append(s)
                say(f"  round {r} {k:16s}: {s * 1e3:9.2f} ms  ({images / s:9.1f} img/s)")
        for k, v in res.items():
            v = sorted(v)
            say(f"  {k:16s} median {v[len(v) // 2] * 1e3:9.2f} ms (min {v[0] * 1e3:.2f}, max {v[-1] * 1e3:.2f}), "
                f"{v[len(v) // 2] / (images / 32) * 1e3:.3f} ms per weak batch")


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--out", default="")
    a.add_argument("--images", type=int, default=1024)
    a.add_argument("--rounds", type=int, default=5)
    a.add_argument("--calls", type=int, default=200)
    a.add_argument("--kernels-only", action="store_true", help="the kernel-alone part only (for a profiler run)")
    opts = a.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/tapnet_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}")
    kernel_alone(opts.rounds, opts.calls, say)
    if not opts.kernels_only:
        weak_stage(opts.images, opts.rounds, say)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
