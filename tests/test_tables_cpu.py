"""TableBook (simfire_amd/csrc/sf_tables.h): what a handle knows about its terrain tables, and the only code that changes it.

The header is plain C++17, so it is checked on its own: ``tests/tables_check.cpp`` (a program with its own ``main``) drives a 3-table
and a 1-table book through scripted sequences and compares every flag after every operation with literals; it is built here with the
address and undefined-behaviour sanitizers and run as a child process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")


def test_table_book_sequences(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    exe = str(tmp_path / "tables_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "tables_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan", r.stderr):
        print("sanitizer runtime missing, building without:", r.stderr.strip().splitlines()[-1])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def test_no_per_table_flag_outside_the_book():
    """The six per-table vectors and the stored have_rt are gone from the host code; what is left of their names is TableBook's."""
    old = re.compile(r"\b(rt_set|rd_lay|rd_fbfm|rd_stale)\b|(?<![\w.])(rtc_stale|wt_stale|have_rt)\s*(\[|=[^=]|\.assign)")
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "sf_tables.h":
            for no, line in enumerate(open(os.path.join(CSRC, name)), 1):
                code = line.split("//")[0]
                assert not old.search(code), f"{name}:{no}: {line.strip()}"
    book = open(os.path.join(CSRC, "sf_tables.h")).read()
    assert re.findall(r"#include\s*(\S+)", book) == ["<cstddef>", "<cstdint>", "<vector>"]      # no HIP include: it compiles on its own
    assert re.search(r"private:\s*std::vector<Table> t_;", book)
