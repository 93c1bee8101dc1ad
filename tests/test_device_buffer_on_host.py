"""The owner types of the handle's device memory (csrc/hmpc_device_buffer.h: DeviceBuffer, OutputBuffer) on the CPU, no GPU needed: a
stand-alone program (tests/src/device_buffer_on_host.cpp) compiled with g++ against a stand-in hip_runtime.h whose hipMalloc / hipFree /
hipMemset are malloc / free / memset, which counts live allocations and synchronisations and can make the N-th allocation or fill fail
(tests/src/hip_alloc_shim).  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly: a double free or a use after free
in the types ends the run, a leak fails it at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_buffer_types_on_the_host(tmp_path):
    exe = str(tmp_path / "device_buffer_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "tests", "src", "hip_alloc_shim"), "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "src", "device_buffer_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
