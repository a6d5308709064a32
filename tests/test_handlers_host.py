"""The host-only parts of the struct path's handlers (csrc/sf_plan_cache.h, sf_placement.h) without a GPU: the
stand-alone program tools/handlers_host_sanitize.cpp under ASan + UBSan -- the pattern key, the LRU plan cache, the in-core /
out-of-core decision, every branch of the retry ladder round plan creation, the host fingerprints.  Nothing is loaded into this
process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc")


def test_headers_need_no_hip():
    """the key, the cache and the placement include no HIP header, and of the library's only the schedule's"""
    allowed = {"sf_plan_cache.h": {"sf_schedule.h"}, "sf_placement.h": {"sf_schedule.h"}, "sf_plan_cache.cpp": {"sf_plan_cache.h"},
               "sf_placement.cpp": {"sf_placement.h", "sf_symbolic.h"}}
    for name, own in allowed.items():
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert "#include <hip" not in text, name
        assert set(re.findall(r'#include "([^"]+)"', text)) == own, name


def test_handlers_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "handlers_host_sanitize")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (no runtime to find or to order at load time)
           f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", os.path.join(ROOT, "tools", "handlers_host_sanitize.cpp"),
           os.path.join(CSRC, "sf_plan_cache.cpp"), os.path.join(CSRC, "sf_placement.cpp"), os.path.join(CSRC, "sf_symbolic.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for knob in ("SF_VERIFY_THREADS", "SF_DEVICE_BUDGET_MB", "SF_TRACE"):      # the program sets what it varies itself
        env.pop(knob, None)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "handlers_host_sanitize: ok" in r.stdout
    for word in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"):
        assert word not in r.stdout, r.stdout
