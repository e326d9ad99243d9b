"""The band scheme of the two bit-plane searches has one header (simfire_amd/csrc/sf_bands.h): geometry, the fill along a row, the
halo, the round of the flood fill and the level of the breadth-first search.

The header is plain C++17, so it is checked on its own: ``tests/bands_check.cpp`` (a program with its own ``main``) emulates a
workgroup on the host - every band reads its halo, then every band runs its round or level, then every band publishes - and compares
with a flood fill and a breadth-first search over a byte grid that it states itself, for H in {1, 15, 16, 17, 33} x W in {1, 63, 64,
65, 130}, both connectivities, random maps of three densities, the empty grid, an all-open grid with a corner seed and a serpentine;
the edge cases of ``band_fill``, ``band_edges`` / ``band_halo`` and ``band_at`` are literals.  It is built here with the address and
undefined-behaviour sanitizers and run as a child process.  The source tests below hold the sharing in place."""
import os
import re
import shutil
import subprocess

import pytest

from test_cells_cpu import _code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")
GONE = ("reach_fill", "reach_halo", "walk_plane_bits", "perim_bytes4")


def test_band_searches_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    exe = str(tmp_path / "bands_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "bands_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan", r.stderr):
        print("sanitizer runtime missing, building without:", r.stderr.strip().splitlines()[-1])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def _text(name):
    return "\n".join(_code(os.path.join(CSRC, name)))


def test_band_header_stands_alone():
    """``sf_bands.h`` includes ``<cstdint>`` only, and both searches include it."""
    assert re.findall(r"#include\s*(\S+)", open(os.path.join(CSRC, "sf_bands.h")).read()) == ["<cstdint>"]
    for name in ("sf_reach_kernels.h", "sf_walk_kernels.h"):
        assert re.findall(r"#include\s*(\S+)", _text(name)) == ['"sf_bands.h"', '"sf_query_dev.h"'], name


def test_walk_does_not_lean_on_reach():
    walk = _text("sf_walk_kernels.h")
    assert "sf_reach_kernels.h" not in walk and not re.search(r"\bReachArgs\b", walk)
    host = _text("sf_host_query.h")
    assert re.search(r"struct WalkArgs \{\s*BandArgs band;", walk) and re.search(r"struct ReachArgs \{\s*BandArgs band;", _text("sf_reach_kernels.h"))
    sig = host[host.index("static int band_search("):]
    sig = sig[:sig.index("\n{")]
    assert not re.search(r"\bReachArgs\b|\bBandArgs\b", sig), "band_search reaches the BandArgs through its Args"
    assert "static_assert" not in host


def test_no_open_coded_wave_reduction_in_the_queries():
    for name in ("sf_reach_kernels.h", "sf_walk_kernels.h", "sf_dist_kernels.h", "sf_travel_kernels.h"):
        for no, code in enumerate(_code(os.path.join(CSRC, name)), 1):
            assert "__shfl_xor" not in code, f"{name}:{no}: {code.strip()}"
    dev = _text("sf_query_dev.h")
    for fn in ("wave_sum", "wave_max", "wave_min"):
        assert re.search(r"T %s\(T v\)" % fn, dev), fn


def test_old_spellings_are_gone():
    gone = re.compile(r"\b(%s)\b" % "|".join(GONE))
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            for no, code in enumerate(_code(os.path.join(CSRC, name)), 1):
                assert not gone.search(code), f"{name}:{no}: {code.strip()}"
