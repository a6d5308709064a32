"""The GPU-free half of the overlapped download (csrc/sf_download.h), without a GPU: the stand-alone program
tools/download_sanitize.cpp -- the gate between the enqueue thread and the copy workers with 1, 4 and 16 workers, and the
unpacking of a staging slot against an element-by-element reference -- built with the host compiler once under ThreadSanitizer
and once under ASan + UBSan.  Every scenario of the program runs under its own watchdog, so a lost wake-up is a failure here,
not a hang.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc")
BAD_WORDS = ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "TIMEOUT")


def test_header_needs_no_hip():
    """sf_download.h compiles with nothing but the host compiler's own headers on the include path"""
    with open(os.path.join(CSRC, "sf_download.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and '#include "' not in text


@pytest.mark.parametrize("flags", [
    ("-fsanitize=thread", "-static-libtsan"),
    ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"),
], ids=["tsan", "asan_ubsan"])
def test_download_program_is_clean(tmp_path, flags):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "download_sanitize")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-pthread", *flags,       # (static runtimes: none to find or to order at load time)
           f"-I{CSRC}", os.path.join(ROOT, "tools", "download_sanitize.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=0")
    run = [exe]
    setarch = shutil.which("setarch")
    if "-fsanitize=thread" in flags and setarch:
        # a ThreadSanitizer runtime older than the kernel's mmap_rnd_bits setting stops at start with "unexpected memory mapping":
        # this one program runs without address randomisation
        run = [setarch, os.uname().machine, "-R", exe]
    r = subprocess.run(run, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "download_sanitize: ok" in r.stdout
    for word in BAD_WORDS:
        assert word not in r.stdout, r.stdout
