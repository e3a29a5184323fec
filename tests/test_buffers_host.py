"""The owning buffers over the resource pool (reservoir_amd/csrc/rsv_buffers.h) against stub pool
functions that count live blocks and fail a chosen allocation: no allocation within the capacity, kept
contents across growths, a group's capacity never above a member's after any failed allocation, move and
swap, and no block left behind; then the sampler handle's landing zone (each form, a failed allocation, the
block given away), its event owner (taken at first use, returned once) and its work clock, as rules
(tests/cpp/test_buffers.cpp, a stand-alone host program built with AddressSanitizer +
UndefinedBehaviorSanitizer; CPU only, no HIP library linked)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffers_over_stub_pool(tmp_path):
    exe = tmp_path / "test_buffers"
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "reservoir_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_buffers.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
