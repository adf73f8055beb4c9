"""Register record of the SpMM kernels: compiles spmm.hip and spmm_bf16.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage (device side only, no GPU needed) and prints VGPRs,
SGPRs, scratch and occupancy of every instantiated spmm_csr_kernel / spmm_items_kernel /
spmm_fixup_kernel.

    python tools/kernel_resources.py [-D GNN_SPMM_TASK_U=8 ...] [--all] [--out FILE]

The template arguments of spmm_csr_kernel are <VW, LPR, NCH, U, NT, HUB, TASKS, CPL, XT, HT>;
the flagship pass 2 (fp32, F = 128, packed tasks over hub ids) is
<4, 32, 1, 4, true, true, true, 1, float, float>; those of spmm_items_kernel (pass 1 under
ops.SPMM_ITEMS_KERNEL) are <LPR, U>: <32, 16> at F = 128, <64, 8> at F = 256.
"""
import argparse
import re
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILES = ["spmm.hip", "spmm_bf16.hip"]
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds")]


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if filt is None:  # the mangled names still carry every template argument
        return names
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n") if r.returncode == 0 else names


def resources(src: Path, defines):
    from graphneuralnetwork_amd.build import HIPCC_FLAGS, _hipcc
    cmd = [_hipcc(), *HIPCC_FLAGS, *[f"-D{d}" for d in defines], "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            out.append(cur)
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    for k, n in zip(out, demangle([k["name"] for k in out])):
        k["name"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--all", action="store_true", help="every kernel, not only the SpMM ones")
    ap.add_argument("--out", default="")
    ap.add_argument("--files", default=",".join(FILES))
    args = ap.parse_args()
    lines = [f"# defines: {' '.join(args.defines) or '(none)'}",
             f"# {'file':14s} {'vgpr':>4s} {'agpr':>4s} {'sgpr':>4s} {'scratch':>7s} {'occ':>3s}  kernel"]
    scratch = 0
    for f in args.files.split(","):
        for k in resources(ROOT / "graphneuralnetwork_amd" / "csrc" / f, args.defines):
            if not args.all and "spmm_" not in k["name"]:
                continue
            name = re.sub(r"^void gnn::", "", k["name"])
            name = re.sub(r"\(.*\)$", "", name).replace("gnn::", "").replace("true", "1").replace("false", "0")
            lines.append(f"  {f:14s} {k.get('vgpr', -1):4d} {k.get('agpr', 0):4d} {k.get('sgpr', -1):4d} "
                         f"{k.get('scratch', -1):7d} {k.get('occ', -1):3d}  {name}")
            scratch += k.get("scratch", 0) > 0
    lines.append(f"# kernels with scratch: {scratch}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
