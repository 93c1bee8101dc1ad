#!/usr/bin/env python3
"""Static count of the vector-ALU instructions of every kernel variant's gfx950 machine code (hipcc cross-compiles: no GPU).

    python scripts/valu_static.py [--group 0..3 ...] [--match SUBSTRING] [extra hipcc flags]

Per kernel: all instructions, those that start with v_ (what issues to the vector ALU, matrix instructions included), and of
these the selects (v_cndmask), the binary64 arithmetic (v_*_f64 without the conversions) and the matrix instructions.  A
static count weighs an instruction inside a loop once: it compares two builds of the same source, it is not a cycle count."""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hector_simulation_amd import build as hip_build  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_counts(groups=None, extra=()):
    groups = list(range(hip_build.VARIANT_GROUPS)) if not groups else groups
    out = {}
    with tempfile.TemporaryDirectory(prefix="hmpc_valu_") as td:
        def one(g):
            co, elf = os.path.join(td, f"g{g}.bundle"), os.path.join(td, f"g{g}.elf")
            subprocess.check_call(["/opt/rocm/bin/hipcc"] + hip_build.CFLAGS + list(extra) +
                                  [f"-DHMPC_VARIANT_GROUP={g}", "--cuda-device-only", "-c",
                                   os.path.join(hip_build.CSRC, "hmpc_variants.hip"), "-o", co], stderr=subprocess.DEVNULL)
            subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={co}",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"])
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf],
                                 capture_output=True, text=True, check=True).stdout
            res, name = {}, None
            for line in dis.splitlines():
                m = re.match(r"^<(\S+)>:$", line.strip())
                if m:
                    name = m.group(1)
                    res[name] = dict(all=0, valu=0, cndmask=0, f64=0, mfma=0, ds=0)
                    continue
                op = line.split()[0] if name and line.strip() else ""
                if not op or op.startswith("//"):
                    continue
                r = res[name]
                r["all"] += 1
                if op.startswith("ds_"):
                    r["ds"] += 1
                if op.startswith("v_"):
                    r["valu"] += 1
                    if op.startswith("v_cndmask"):
                        r["cndmask"] += 1
                    elif op.startswith("v_mfma"):
                        r["mfma"] += 1
                    elif "_f64" in op and not op.startswith("v_cvt"):
                        r["f64"] += 1
            return res

        with concurrent.futures.ThreadPoolExecutor(max_workers=len(groups)) as ex:
            for r in ex.map(one, groups):
                out.update(r)
    short = {}
    for k, v in out.items():
        d = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        short[re.sub(r"^void hmpc::", "", d).replace("(hmpc::KernelArgs)", "")] = v
    return short


def main():
    args, groups, extra, match = sys.argv[1:], [], [], ""
    i = 0
    while i < len(args):
        if args[i] == "--group":
            groups.append(int(args[i + 1])); i += 2
        elif args[i] == "--match":
            match = args[i + 1]; i += 2
        else:
            extra.append(args[i]); i += 1
    for k, r in sorted(kernel_counts(groups, extra).items()):
        if match in k:
            print(f"{k:64s} all {r['all']:6d}  v_* {r['valu']:6d}  cndmask {r['cndmask']:5d}  f64 {r['f64']:5d}  mfma {r['mfma']:4d}  ds_* {r['ds']:5d}")


if __name__ == "__main__":
    main()
