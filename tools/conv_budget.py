"""The float64 error budget of every conv tile as a table (needs a GPU).

    python tools/conv_budget.py [out.txt]      (default: profiles/conv_budget.txt)

Runs every case of tests/test_gpu_conv_budget.py (shapes, seeds, tiles and factors from
tests/conv_cases.py) and writes, per shape, torch's float32 CPU conv error against the float64 conv
(the yardstick) and per tile its RMS error and its bias as ratios of that yardstick.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    from tests import conv_cases as C
    lines = ["conv tile error budget against a float64 conv (tools/conv_budget.py; tests/test_gpu_conv_budget.py)",
             "e = y - ref; e_ref = torch float32 CPU conv - ref on the same tensors; errors relative to |ref|max",
             f"limits: rms(e) / rms(e_ref) <= {C.RMS_FACTOR:g} ({C.RMS_FACTOR_CHAIN:g} for the plain-chain tiles 3, 4);"
             f" |mean(e)| / rms(e_ref) <= {C.BIAS_FACTOR:g} (not 3, 4)", ""]
    worst = {}
    last = None
    for name, tile, se, presplit in C.BUDGET_RUNS:
        shape = C.BUDGET_SHAPES[name]
        c = C.budget_case(name, se)
        if (name, se) != last:
            last = (name, se)
            B, H, W, Cin, Cout, k, s = shape
            lines += ["", f"{name}{' with in_scale = rand(B, Cin)' if se else ''}: (B,H,W,Cin,Cout,k,s) = {shape} "
                          f"K = {k * k * Cin} N = {c['ref'].numel()} |ref|max {c['scale']:.3f} "
                          f"CPU float32: rms {C.rms(c['e_ref']) / c['scale']:.2e} "
                          f"bias {c['e_ref'].mean().item() / c['scale']:+.1e}",
                      f"  {'tile':<12} {'rms(e)':>9} {'bias':>9} {'rms ratio':>10} {'bias ratio':>11} {'limit':>6}"]
        y = C.gpu_conv(c["x"], c["w"], shape, tile, bias=c["b"], sc=c["sc"], presplit=presplit)
        e = y.double() - c["ref"]
        r, b = C.ratios(y, c)
        f_rms, f_bias = C.budget_factors(C.tile_of(tile)[0])
        ok = r <= f_rms and (f_bias is None or abs(b) <= f_bias)
        tag = f"{tile}" + (" presplit" if presplit else "")
        lines.append(f"  {tag:<12} {C.rms(e) / c['scale']:>9.2e} {e.mean().item() / c['scale']:>+9.1e} {r:>10.3f} "
                     f"{b:>+11.4f} {f_rms:>6g}{'' if ok else '  OVER'}")
        key = "chain (3, 4)" if tile in C.CHAIN_TILES else "stream (33-35)" if tile in C.STREAM_TILES else "stage sum"
        w = worst.setdefault(key, [0.0, 0.0])
        w[0], w[1] = max(w[0], r), max(w[1], abs(b))
    lines += ["", "largest ratios: " + "; ".join(f"{k}: rms {v[0]:.3f} bias {v[1]:.4f}" for k, v in worst.items())]
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_budget.txt"))
