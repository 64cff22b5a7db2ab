"""The once-per-device mask behind the dynamic-LDS guard (csrc/ff_device_once.h), on the host: tests/device_once_tsan.cpp is built with the
host compiler and run -- 8 threads, device indices 0, 1, 63 and 64, no HIP and no GPU.  Its header comment gives the ThreadSanitizer build."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    from isr2_amd.build import HIPCC
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "clang++")
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", rocm_clang):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler found")


def test_device_once_mask_under_threads(tmp_path):
    exe = str(tmp_path / "device_once")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "image-super-resolution-2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "device_once_tsan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "device_once: ok" in r.stdout, r.stdout + r.stderr
