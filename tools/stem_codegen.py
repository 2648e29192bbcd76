"""Codegen table of the SSD stem instantiations (csrc/layers.hip ssd_stem_kernel), counted in the gfx950
assembly that build.py's flags produce.

    python tools/stem_codegen.py [layers.hip ...]      (default: the tree's csrc/layers.hip)

Per instantiation: global loads / s_waitcnt with a vmcnt / of those vmcnt(0) / branches (s_cbranch +
s_branch), all four in the input phase; of those waits and branches, the ones between the first and the last
global load; static VALU instructions per phase (input, halo GEMM, depthwise, projection: they end at the
last three s_barrier); VGPRs / scratch bytes / LDS bytes / occupancy as the compiler reports them.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "edgeml-object-detection_amd")
sys.path.insert(0, PKG)
import build as B  # noqa: E402


def assembly(src):
    """The gfx950 assembly of one csrc file (the tree's or a copy elsewhere) under build.py's flags for its name."""
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    B.write_tile_table(objdir)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "kernels.s")
        cmd = [B.hipcc(), *B.FLAGS, *B.FILE_FLAGS.get(os.path.basename(src), []), "-I", objdir, "-I",
               os.path.join(PKG, "csrc"), "--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr)
        return open(out).read()


def kernels(asm, name=r"_ZN7edgedet15ssd_stem_kernel\w+"):
    """mangled name -> (instruction lines, trailing metadata comment lines) of every function whose name matches."""
    out = {}
    for m in re.finditer(r"^(%s):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; COMPUTE_PGM_RSRC2" % name, asm, re.S | re.M):
        body = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
        out[m.group(1)] = ([ln for ln in body if ln and not ln.endswith(":") and not ln.startswith(".")], m.group(3))
    return out


def demangle(name):
    t = {"h": "uint8_t", "f": "float"}[name[len("_ZN7edgedet15ssd_stem_kernelI")]]
    flags = re.findall(r"Lb([01])E", name)
    return f"<{t}, {', '.join('true' if f == '1' else 'false' for f in flags)}>"


def is_valu(op):
    return op.startswith("v_") and not op.startswith(("v_mfma", "v_nop", "v_accvgpr"))


def row(ins, meta):
    # the phases end at the last three barriers (the fused forms have one more, in the input phase, behind
    # the coordinate table)
    bars = [i for i, ln in enumerate(ins) if ln.startswith("s_barrier")][-3:]
    p1 = ins[: bars[0]]
    op = lambda ln: ln.split()[0]  # noqa: E731
    loads = [i for i, ln in enumerate(p1) if op(ln).startswith("global_load")]
    wait = [i for i, ln in enumerate(p1) if op(ln) == "s_waitcnt" and "vmcnt" in ln]
    wait0 = [i for i in wait if "vmcnt(0)" in p1[i]]
    br = [i for i, ln in enumerate(p1) if op(ln).startswith(("s_cbranch", "s_branch"))]
    inside = lambda idx: sum(loads[0] < i < loads[-1] for i in idx)  # noqa: E731
    edges = [0] + bars + [len(ins)]
    valu = [sum(is_valu(op(ln)) for ln in ins[a:b]) for a, b in zip(edges, edges[1:])]
    g = lambda k: int(re.search(k + r":\s*(\d+)", meta).group(1))  # noqa: E731
    return (f"{len(loads):3d} / {len(wait):2d} / {len(wait0):2d} / {len(br):2d}   between the loads: vmcnt(0) {inside(wait0)}, "
            f"branches {inside(br)}   VALU {' + '.join(map(str, valu))} = {sum(valu)}   {g('TotalNumVgprs')} VGPRs / "
            f"{g('ScratchSize')} scratch / {g('LDSByteSize')} LDS / occupancy {g('Occupancy')}")


def main():
    for src in sys.argv[1:] or [os.path.join(PKG, "csrc", "layers.hip")]:
        print(src)
        for name, (ins, meta) in sorted(kernels(assembly(src)).items()):
            print(f"  ssd_stem_kernel{demangle(name):24s} {row(ins, meta)}")


if __name__ == "__main__":
    main()
