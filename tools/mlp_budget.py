"""Writes profiles/mlp_budget.txt: how far tests/mlp_ref.py Fit32 (the float32 restatement of mlp_fit_kernel that the
device is held to bit for bit) stands from torch float64 autograd, one training step per case, on the CPU.

    python tools/mlp_budget.py > profiles/mlp_budget.txt

Per case the worst quantity by its ratio to 4 E (E = max |torch32 - torch64|) and, over all cases, every quantity above
4 E with its class (mlp_ref.floor_class) and its error in float32 ulps of max |ref64|: each class's ulp floor in
tests/test_mlp_ref_host.py is the smallest power of two that covers twice the worst of its class.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import mlp_ref as R  # noqa: E402


def main():
    print("Fit32 (tests/mlp_ref.py) against torch float64 autograd, one training step (tools/mlp_budget.py;")
    print("tests/test_mlp_ref_host.py).  ratio = max|Fit32 - ref64| / (4 E), E = max|torch32 - ref64|; ulps = the same")
    print("error in float32 ulps of max|ref64|.  limit: ratio <= 1; a one-element quantity, or one of at most "
          f"{R.FEW} elements")
    print(f"in a step of at most {R.FEW} rows, may stand within its class's ulp floor instead")
    print()
    print(f"{'case':22s} {'worst quantity':>14s} {'n':>5s} {'ratio':>7s} {'E':>9s} {'ulps':>7s}   zero-gradient biases: "
          "max |G32| / bound")
    over, worst_plain = [], 0.0
    for c in R.anchor_cases():
        rows, zero = R.measure(c)
        name, size, ratio, E, ulps = max(rows, key=lambda r: r[2])
        zr = max([float((g / (b + 1e-300)).max()) for _, g, b in zero] or [0.0])
        print(f"{c.name:22s} {name:>14s} {size:5d} {ratio:7.3f} {E:9.2e} {ulps:7.2f}   {zr:.4f}")
        over += [(c.name, R.floor_class(c, r[1])) + r for r in rows if r[2] > 1.0]
        worst_plain = max([worst_plain] + [r[2] for r in rows if R.floor_class(c, r[1]) is None])
    print()
    print("quantities above 4 E:")
    for cname, cls, name, size, ratio, E, ulps in sorted(over, key=lambda r: -r[6]):
        print(f"{cname:22s} {name:>14s} {size:5d} {ratio:7.3f} {E:9.2e} {ulps:7.2f}   {cls}")
    print()
    print(f"worst ratio of a quantity held to plain 4 E: {worst_plain:.3f}")
    for cls in ("one", "few"):
        worst = max([r[6] for r in over if r[1] == cls] or [0.0])
        floor = 1
        while floor < 2 * worst:
            floor *= 2
        print(f"class {cls}: worst above 4 E {worst:.2f} ulps; twice that needs a floor of {floor} ulps")


if __name__ == "__main__":
    main()
