"""The grouped lane-form launch of the commitment scheduler (csrc/hash_service.cpp) on the CPU, under ThreadSanitizer and under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/lane_group_pool_main.cpp against the stand-in device of csrc/host_only_stubs.cc.  A
pool of eight big contexts, groups of 2, 3 and 4 under all three commit policies: one launch per group, every member's `done` recorded, a
member whose `ready` fails fails alone (`make lane-group-test` runs the same two programs)."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {
    "thread": (["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1"}, "ThreadSanitizer"),
    "address": (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1"}, "AddressSanitizer"),
}


@pytest.mark.slow
@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_lane_groups_go_out_as_one_launch_each(tmp_path, sanitizer):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags, env, name = SANITIZERS[sanitizer]
    exe = str(tmp_path / "lane_group_pool")
    srcs = sorted(glob.glob(os.path.join(ROOT, "starky_bls12_381_amd", "csrc", "*.cpp"))) + [os.path.join(ROOT, "starky_bls12_381_amd", "csrc", "host_only_stubs.cc")]
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + flags + ["-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "lane_group_pool_main.cpp")] + srcs + ["-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "cannot find" in b.stderr.lower() and ("tsan" in b.stderr.lower() or "asan" in b.stderr.lower()):
        pytest.skip("the sanitizer's runtime is not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert name not in r.stderr
    for policy in (0, 1, 2):
        assert f"policy {policy}: ok" in r.stdout
