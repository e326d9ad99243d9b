"""The blocked cell plane has one reader (simfire_amd/csrc/sf_cells.h), and the queries one device frame (sf_query_dev.h).

``sf_cells.h`` is plain C++17, so its layout arithmetic and its accessors are checked on their own: ``tests/cells_check.cpp`` (a
program with its own ``main``) restates the layout from its definition and compares, for every grid of H in {1, 2, 3, 4, 5, 9} and W
in {1, 15, 16, 17, 33, 64}; it is built here with the address and undefined-behaviour sanitizers and run as a child process.  The
``Geo`` forwards of ``sf_common.h`` need HIP: the program checks the accessors on a struct with Geo's fields instead, a
``static_assert`` beside the forwards compares them with the PV forms in every build, and the source test below holds both in place."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")
STEP_PATH = ("sf_step_kernels.h", "sf_run_kernels.h", "sf_win_kernels.h")
GONE = ("PerimGeo", "beh_wave_sum", "beh_wave_max", "perim_wave_sum", "beh_status_ptr", "dist_status", "reach_status", "travel_status")


def test_cell_layout_and_accessors(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    exe = str(tmp_path / "cells_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cells_check.cpp")]
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


def test_blocked_layout_known_in_one_place():
    """Outside ``sf_cells.h``, ``sf_common.h`` (the ``Geo`` field and the two forwards) and the three step-path headers no code line
    under ``csrc/`` names ``kBlStatus`` or ``cells_env`` - but for the host lines of ``simfire_hip.hip`` that fill, allocate and list
    by ``g.cells_env`` - or carries the sector arithmetic written out, and the per-query copies of the shared device idioms are gone."""
    names = re.compile(r"\b(kBlStatus|cells_env)\b")
    sector = re.compile(r"\*\s*128\s*\+\s*\(\(\s*\w+\s*>>\s*1\s*\)\s*&\s*1\s*\)\s*\*\s*64")
    gone = re.compile(r"\b(%s)\b" % "|".join(GONE))
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        for no, code in enumerate(_code(os.path.join(CSRC, name)), 1):
            assert not gone.search(code), f"{name}:{no}: {code.strip()}"
            if name == "sf_cells.h":
                continue
            assert not sector.search(code), f"{name}:{no}: {code.strip()}"
            if name == "simfire_hip.hip":      # host code: sf_create fills Geo's field, the blocked plane is allocated and listed by it
                assert "kBlStatus" not in code and ("cells_env" not in code or re.search(r"\bg\.cells_env\b", code)), f"{name}:{no}: {code.strip()}"
            elif name != "sf_common.h" and name not in STEP_PATH:
                assert not names.search(code), f"{name}:{no}: {code.strip()}"
    cells = open(os.path.join(CSRC, "sf_cells.h")).read()
    assert re.findall(r"#include\s*(\S+)", cells) == ["<cstdint>"]      # no HIP include: it compiles on its own
    assert sum(1 for code in _code(os.path.join(CSRC, "sf_cells.h")) if sector.search(code)) == 1
    # sf_common.h keeps the Geo field and forwards the offsets, one line each
    common = "\n".join(_code(os.path.join(CSRC, "sf_common.h")))
    assert '#include "sf_cells.h"' in common
    assert re.search(r"int bl_vec\(const Geo &g, int y, int v\) \{ return bl_vec\(g\.PV, y, v\); \}", common)
    assert re.search(r"int bl_cell\(const Geo &g, int y, int x\) \{ return bl_cell\(g\.PV, y, x\); \}", common)
    assert re.search(r"static_assert\(bl_vec\(bl_check_geo\(\), \d+, \d+\) == bl_vec\(3, .*bl_cell\(bl_check_geo\(\), \d+, \d+\) == bl_cell\(3, ", common)      # and the build checks them
    assert len(names.findall(common)) == 1 and re.search(r"long long cells_env;", common)
    # the byte-permute tables of the status masks are applied in sf_query_dev.h alone (sf_common.h: the step path's elig01_perm)
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name not in ("sf_query_dev.h", "sf_common.h") + STEP_PATH:
            for no, code in enumerate(_code(os.path.join(CSRC, name)), 1):
                assert "__builtin_amdgcn_perm" not in code, f"{name}:{no}: {code.strip()}"
