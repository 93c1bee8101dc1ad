#!/usr/bin/env python3
"""Generates tests/golden/ref_pod_layout.json: size and field offsets of the reference's own PODs (update_data_t,
problem_setup of ConvexMPC/convexMPC_interface.h), as the compiler lays them out on this ABI (x86-64 SysV).
tests/test_source_dropin.py checks include/hector_mpc.h against them with static_asserts, without the reference's sources.
Run from the repo root with the reference checkout's root:  python tests/golden/make_pod_layout_golden.py REFERENCE_ROOT"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = {"update_data_t": ["p", "v", "q", "w", "r", "joint_angles", "yaw", "weights", "traj", "Alpha_K", "gait", "hack_pad",
                            "max_iterations", "rho", "sigma", "solver_alpha", "terminate"],
          "problem_setup": ["dt", "mu", "f_max", "horizon"]}


def main(ref_root: str) -> None:
    header = os.path.join(ref_root, "Hector_ROS_Simulation", "hector_control", "ConvexMPC", "convexMPC_interface.h")
    body = [f'#include "{header}"', "#include <cstddef>", "#include <cstdio>", "int main() {", '  std::printf("{");']
    for i, (struct, fields) in enumerate(FIELDS.items()):
        body.append(f'  std::printf("%s\\"{struct}\\": {{\\"sizeof\\": %zu", "{", " if i else ""}", sizeof({struct}));')
        for f in fields:
            body.append(f'  std::printf(", \\"{f}\\": %zu", offsetof({struct}, {f}));')
        body.append('  std::printf("}");')
    body += ['  std::printf("}\\n");', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "layout.cpp"), os.path.join(td, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(body) + "\n")
        subprocess.check_call(["g++", "-std=gnu++17", src, "-o", exe])
        layout = json.loads(subprocess.check_output([exe], text=True))
    path = os.path.join(ROOT, "tests", "golden", "ref_pod_layout.json")
    with open(path, "w") as fh:
        json.dump(layout, fh, indent=1)
        fh.write("\n")
    print(path, layout)


if __name__ == "__main__":
    main(sys.argv[1])
