"""Time the device fits of the two comparison baselines (edgeml_amd.baseline: every fold at once) at
COCO-val scale on synthetic data: N images, 80 classes + 5 x 25 box values = 205 stage-24 features.

    python tools/baseline_bench.py [--n 5000] [--folds 5] [--dump data.npz]

--dump writes the data (features, detections, label counts, rewards, split) so that the reference's
fit_af / fit_dcsb can be timed on the same arrays on a CPU; --dump-only does that without a device.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NUM_CLASS, K = 80, 25


def synth(n, folds, seed=0):
    rng = np.random.default_rng(seed)
    feats = np.zeros((n, NUM_CLASS + 5 * K))
    dets, lab, rew = [], np.zeros(n, int), np.zeros(n, int)
    for i in range(n):
        nh, nm, nl = rng.poisson(3), rng.poisson(4), rng.poisson(11)
        conf = np.sort(np.concatenate([rng.uniform(0.5, 0.95, nh), rng.uniform(0.25, 0.5, nm),
                                       rng.uniform(0.05, 0.25, nl)]))[::-1]
        m = len(conf)
        w, h = rng.uniform(0.5, 1.0, m), rng.uniform(0.5, 1.0, m)
        x, y = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
        cls = rng.integers(0, NUM_CLASS, m)
        area = ((x + w / 2) - (x - w / 2)) * ((y + h / 2) - (y - h / 2))
        dets.append((conf, area))
        lab[i] = nh + rng.binomial(nm, 0.55)
        rows = np.stack([x, y, w, h, conf], 1)[:K]
        np.add.at(feats[i], cls[:K], 1)
        feats[i, NUM_CLASS:NUM_CLASS + rows.size] = rows.reshape(-1)
        above = conf > 0.36
        hard = above.sum() != nh and (above.sum() > 5 or area[above].min() < 0.40)
        rew[i] = int(hard != (rng.uniform() < 0.08))
    fold = rng.permutation(np.arange(n) % folds)
    return feats, dets, lab, rew, np.stack([fold == f for f in range(folds)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--dump", type=str, default="")
    ap.add_argument("--dump-only", action="store_true")
    a = ap.parse_args()
    feats, dets, lab, rew, split = synth(a.n, a.folds)
    if a.dump:
        off = np.concatenate([[0], np.cumsum([len(d[0]) for d in dets])])
        np.savez_compressed(a.dump, features=feats, conf=np.concatenate([d[0] for d in dets]),
                            area=np.concatenate([d[1] for d in dets]), det_off=off, label_num=lab, reward=rew,
                            split=split)
    if a.dump_only:
        return
    import torch
    from edgeml_amd import baseline
    baseline.fit_af_folds(feats[:300], rew[:300], split[:, :300])  # warm: library load, allocator
    baseline.fit_dcsb_folds(dets[:300], lab[:300], rew[:300], split[:, :300])
    torch.cuda.synchronize()
    for name, fit in (("af", lambda: baseline.fit_af_folds(feats, rew, split)),
                      ("dcsb", lambda: baseline.fit_dcsb_folds(dets, lab, rew, split))):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            res, models = fit()
            times.append(time.perf_counter() - t0)
        acc = [float(np.mean(rew[~m] == r["train_est"])) for m, r in zip(split, res)]
        extra = (f"Newton steps {[m['n_iter'] for m in models]}, |grad| {[float('%.2g' % m['grad_norm']) for m in models]}"
                 if name == "af" else f"models {[(m[0], m[1], float(m[2])) for m in models]}")
        print(f"{name}: {a.folds} folds, N={a.n}: {min(times):.4f} s (runs {[round(t, 4) for t in times]}, host packing and "
              f"copies included); train accuracy {np.round(acc, 3).tolist()}; {extra}")


if __name__ == "__main__":
    main()
