"""The life-cycle of a plan's factor (csrc/sf_factor_state.h), without a GPU: the stand-alone program
tools/factor_state_sanitize.cpp under ASan + UBSan, and the rule that nothing in csrc/ outside that header writes or compares the
state's members."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc")
HEADER = "sf_factor_state.h"


def test_state_program_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "factor_state_sanitize")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",      # (no runtime to find or to order at load time)
           f"-I{CSRC}", os.path.join(ROOT, "tools", "factor_state_sanitize.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "factor_state_sanitize: ok" in r.stdout
    for word in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"):
        assert word not in r.stdout, r.stdout


def _members():
    """the data members of SfFactorState, read from the header"""
    with open(os.path.join(CSRC, HEADER)) as f:
        body = _code(f.read()).split("struct SfFactorState {", 1)[1]
    names = []
    for line in body.splitlines():
        m = re.match(r"\s+(?:bool|int|int64_t) ([^;()]*);", line)
        if m:
            names += [d.split("=")[0].strip() for d in m.group(1).split(",")]
    return names


def _code(text):
    """the text without // comments"""
    return "\n".join(line.split("//", 1)[0] for line in text.splitlines())


def test_only_the_header_writes_or_compares_the_state():
    names = _members()
    assert sorted(names) == sorted(["values_set", "factor_gen", "fact_gen", "ok_gen", "sel_gen", "rf_anorm_gen", "fact_done",
                                    "upd_failed", "epoch", "hash_epoch", "last_status"]), names
    alt = "|".join(names)
    member = r"(?:\b(?:%s)\b)" % alt
    # an assignment (plain or compound), an increment or a decrement of a member, however it is reached
    written = re.compile(r"%s\s*(?:=(?!=)|[-+*/%%&|^]=|<<=|>>=|\+\+|--)|(?:\+\+|--)\s*(?:[\w\]\[]+\s*(?:->|\.)\s*)*%s" % (member, member))
    compared = re.compile(r"\b(?:sel_gen|ok_gen|fact_gen)\b\s*(?:[=!<>]=|[<>])|(?:[=!<>]=|[<>])\s*(?:[\w\]\[]+\s*(?:->|\.)\s*)*\b(?:sel_gen|ok_gen|fact_gen)\b")
    seen = 0
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".cpp", ".inc")) or name == HEADER:
            continue
        with open(os.path.join(CSRC, name)) as f:
            code = _code(f.read())
        assert "/*" not in code or not re.search(member, code), name
        for rx in (written, compared):
            m = rx.search(code)
            assert not m, f"{name}: {code[max(0, m.start() - 60):m.end() + 20]!r}"
        seen += 1
    assert seen > 40
    # the rule finds what it is meant to find
    for bad in ("p->ok_gen = p->factor_gen;", "++p->factor_gen;", "dst->ok_gen = ++dst->factor_gen;", "p->fs.epoch += 1;", "q->fs.fact_done=true;",
                "R.epoch = 3;", "s.hash_epoch--;"):
        assert written.search(bad), bad
    for bad in ("p->ok_gen >= p->fact_gen", "p->sel_gen != p->factor_gen", "x == p->fs.ok_gen", "0 < p->fact_gen"):
        assert compared.search(bad), bad
    for good in ("int epoch, int* info", "p->fs.factor_epoch() != R.plan_epoch", "flags, epoch, info", "part_epochs.push_back(q->fs.factor_epoch());"):
        assert not written.search(good) and not compared.search(good), good
