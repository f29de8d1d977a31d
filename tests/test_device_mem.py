"""copra_amd/csrc/device_mem.hpp, the owners of device and pinned memory, on the host: tests/cpp/test_device_mem.cpp drives them with a
counting allocator (what is released and when, what a failed attempt leaves behind; for DevArg, the borrowed-or-copied input array, which
pointer is in force and when its copy grows) under AddressSanitizer and UBSan.  The program is an
executable of its own: g++ only, no HIP, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_against_a_counting_allocator(tmp_path):
    exe = str(tmp_path / "test_device_mem")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "cpp", "test_device_mem.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_mem ok" in r.stdout and "none live" in r.stdout


def test_the_header_is_host_only():
    text = open(os.path.join(ROOT, "copra_amd", "csrc", "device_mem.hpp")).read()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
