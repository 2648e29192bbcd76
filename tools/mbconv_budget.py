"""The float64 error budget of the fused InvertedResidual kernel as a table (needs a GPU).

    python tools/mbconv_budget.py [out.txt]      (default: profiles/mbconv_budget.txt)

Runs every case of tests/test_gpu_mbconv_budget.py (shapes, seeds and factors from
tests/mbconv_cases.py) and writes, per shape, the error of torch's float32 CPU chain against the
float64 chain (the yardstick) and the kernel's RMS error and bias as ratios of that yardstick.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch

    from tests import mbconv_cases as M
    lines = ["mbconv_kernel error budget against a float64 chain (tools/mbconv_budget.py; tests/test_gpu_mbconv_budget.py)",
             "e = y - ref; e_ref = torch float32 CPU chain (three F.conv2d) - ref on the same tensors; errors relative to "
             "|ref|max",
             f"limits: rms(e) / rms(e_ref) <= {M.RMS_FACTOR:g}; |mean(e)| / rms(e_ref) <= {M.BIAS_FACTOR:g}", "",
             f"{'shape':<6} {'(B,H,W,Cin,Cexp,Cout,K,S)':<34} {'act':<4} {'N':>6} {'|ref|max':>9} {'CPU rms':>9} "
             f"{'rms(e)':>9} {'bias':>9} {'rms ratio':>10} {'bias ratio':>11}"]
    for name, (case, act) in M.BUDGET_SHAPES.items():
        c = M.budget_case(name)
        y = M.run_record(c["t"], case, act)
        e = torch.as_tensor(y).double() - c["ref"]
        r, b = M.ratios(y, c)
        ok = r <= M.RMS_FACTOR and abs(b) <= M.BIAS_FACTOR
        lines.append(f"{name:<6} {str(case):<34} {act:<4} {y.size:>6} {c['scale']:>9.3f} "
                     f"{M.rms(c['e_ref']) / c['scale']:>9.2e} {M.rms(e) / c['scale']:>9.2e} "
                     f"{e.mean().item() / c['scale']:>+9.1e} {r:>10.3f} {b:>+11.4f}{'' if ok else '  OVER'}")
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mbconv_budget.txt"))
