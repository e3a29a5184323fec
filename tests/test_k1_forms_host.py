"""The host's choice of K1 kernel per launch (tests/cpp/test_k1_forms.cpp): launches planned through k1_plan on both
sides of 2^33 and 2^40 pick the FAST instantiation exactly where the launch-uniform flag selected the FAST body
when one kernel held both.  A stand-alone program with the element kernels' translation unit included whole (so
its device code is compiled too, ~20 s), its host code built with AddressSanitizer + UndefinedBehaviorSanitizer;
CPU only, no GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_k1_form_choice(tmp_path):
    exe = tmp_path / "test_k1_forms"
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "reservoir_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_k1_forms.cpp"), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
