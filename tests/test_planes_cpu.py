"""PlaneBook (simfire_amd/csrc/sf_planes.h): which cell layout of a handle is current, which structures derived from it still match
it, and the only code that changes either.

The header is plain C++17, so it is checked on its own: ``tests/planes_check.cpp`` (a program with its own ``main``) drives a book
through scripted sequences of host events and compares every query after every operation with literals; it is built here with the
address and undefined-behaviour sanitizers and run as a child process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")
OLD_FIELDS = ("bl_cur", "vbits_valid", "vbits_fl_valid", "tiles_valid", "tdirty_all", "status_fresh", "committed", "fire_rows", "last_kind",
              "was_reset")


def test_plane_book_sequences(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    exe = str(tmp_path / "planes_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "planes_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan", r.stderr):
        print("sanitizer runtime missing, building without:", r.stderr.strip().splitlines()[-1])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def _code(path):
    """A source file without its comments."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), open(path).read(), flags=re.S)
    return [line.split("//")[0] for line in text.split("\n")]


def test_no_plane_flag_outside_the_book():
    """The ten fields are gone from the handle and the host code: what is left of their names outside ``sf_planes.h`` is a call of
    the book's query of that name.  ``fire_rows`` of ``StateHeader`` (the bound a state blob carries: ``sf_state_kernels.h``,
    ``state_header`` / ``sf_load_state``) is another thing and is exempted by name."""
    old = re.compile(r"\b(%s)\b(?!\()" % "|".join(OLD_FIELDS))
    blob = re.compile(r"\b(h|hdr\[i\])\.fire_rows\b|\bint32_t has_parents, fire_rows, has_arrival, reserved1;")
    ternaries = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")) or name == "sf_planes.h":
            continue
        for no, code in enumerate(_code(os.path.join(CSRC, name)), 1):
            if name in ("sf_state_kernels.h", "sf_host_state.h"):
                code = blob.sub("", code)
            assert not old.search(code), f"{name}:{no}: {code.strip()}"
            for m in re.finditer(r"\b(%s)\(" % "|".join(OLD_FIELDS), code):      # a query: the book's, read through the handle
                assert code[:m.start()].endswith("planes."), f"{name}:{no}: {code.strip()}"
            if re.search(r"\?\s*s->cells\s*:\s*nullptr", code):
                ternaries.append((name, code.strip()))
    assert len(ternaries) == 1 and ternaries[0][0] == "sf_handle.h" and ternaries[0][1].startswith("static uint8_t *cur_cells("), ternaries
    book = open(os.path.join(CSRC, "sf_planes.h")).read()
    assert re.findall(r"#include\s*(\S+)", book) == ["<algorithm>"]      # standard headers only, no HIP include: it compiles on its own
    public, private = book.split("private:")
    members = re.findall(r"\b(\w+_)\s*=\s*[-\w]+\s*[,;]", private)
    assert sorted(members) == sorted(["blocked_", "bits_valid_", "bits_fl_valid_", "tiles_valid_", "hist_all_stale_", "row_fresh_", "committed_",
                                      "was_reset_", "fire_rows_", "last_kind_"]), members
    assert not re.search(r"^\s*(bool|int)\s+\w+_\b[^()]*;", public, flags=re.M), "a data member of PlaneBook is public"
    handle = open(os.path.join(CSRC, "sf_handle.h")).read()
    assert '#include "sf_planes.h"' in handle and re.search(r"^\s*PlaneBook planes;", handle, flags=re.M)
