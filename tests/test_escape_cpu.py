"""Escape routes (``sf_escape``) without a GPU: the oracle against a search over the states (cell, move
index), what every hand-made scene claims, the refusals of ``EscapeSpec``, the scratch arithmetic, the text of the ABI, where the
kernel is named, and ``band_grow`` of ``sf_bands.h`` in a stand-alone program that emulates a workgroup on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _escape_oracle as eo
import _escape_worlds as ew
import _reach_oracle as ro
from test_cells_cpu import _code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")


def test_oracle_against_the_states():
    assert eo.self_test() == 24 * 12 * 14


def test_deadlines():
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.5, 63.99, 64.0, 65.0, np.inf, np.nan, -1.0, -0.0], dtype=np.float32)
    N = eo.NEVER
    assert eo.deadlines(t, 1.0, 0.0, 64.0).tolist() == [0, 1, 1, 2, 3, 64, N, N, N, N, N, 0]
    assert eo.deadlines(t, 1.0, 0.5, 64.0).tolist() == [0, 0, 1, 1, 2, 64, N, N, N, N, N, 0]
    assert eo.deadlines(np.float32(0.3), 0.1, 0.0, 6.0).tolist() == 4 and eo.deadlines(np.float32(2.5), 1.0, 0.5, 64.0).tolist() == 2
    assert eo.move_bound(1.0, 0.0, 32768.0) == 32768 and eo.move_bound(0.5, 1.0, 9.0) == 16


@pytest.mark.parametrize("shape", ew.SCENE_SHAPES[:4], ids=["%dx%d" % s for s in ew.SCENE_SHAPES[:4]])
def test_what_the_scenes_claim(shape):
    names = set()
    for s in ew.scenes(*shape):
        r = eo.answer(s["map"], s["minutes"], ro.mask_of(s["target"]) if s["target"] else 0, ro.mask_of(s["through"]), s["conn"], s["passable"],
                      s["targets"], s["points"], s["per_move"], s["margin"], s["horizon"], s["flag"])
        assert r["safe"] + r["escapable"] + r["lost"] == int(((r["slack"] != eo.BLOCKED) & (r["slack"] != eo.SAFE)).sum()) + r["safe"]
        if s["claim"] is not None:
            s["claim"](r)
        names.add(s["name"])
    assert len(names) == 18


def test_a_front_only_search_misses_the_late_opener():
    """The scene is there for a reason: dilating only the cells the last level added leaves the late cell LOST."""
    s = ew.late_opener(9, 9)
    D = eo.deadlines(s["minutes"], 1.0, 0.0, s["horizon"])
    tgt, walk = eo.cell_sets(s["map"], 4, 1, None, None, D)
    front, A, S = tgt.copy(), tgt.copy(), np.where(tgt, eo.SAFE, np.where(walk, eo.LOST, eo.BLOCKED))
    for v in range(int(D[walk].max()) - 1, -1, -1):
        new = eo._grow(front, 4) & walk & ~A & (D > v)
        S[new] = v
        A |= new
        front = new if new.any() else front
    assert S[2, 1] == eo.LOST and eo.slack_plane(tgt, walk, D, 4)[2, 1] == 2


def test_spec_refusals():
    from simfire_amd import escape
    ok = dict(target=("BURNED",), horizon_minutes=64.0)
    assert escape.request(**ok) == (4, 1, 4, 1.0, 0.0, 64.0, 0, 0)
    assert escape.request(target=(), targets=True, horizon_minutes=8, minutes_per_move=0.5, margin_minutes=1, unreached_safe=True,
                          connectivity=8, scratch_bytes=7)[2:] == (8, 0.5, 1.0, 8.0, 1, 7)
    bad = [dict(target=()), dict(target=None), dict(target=0), dict(target=64), dict(target=("ASH",)), dict(through=()), dict(through=0),
           dict(connectivity=6), dict(connectivity=True), dict(connectivity=4.0), dict(horizon_minutes=None), dict(horizon_minutes=0),
           dict(horizon_minutes=-1.0), dict(horizon_minutes=float("inf")), dict(horizon_minutes=float("nan")), dict(horizon_minutes="8"),
           dict(horizon_minutes=True), dict(minutes_per_move=0), dict(minutes_per_move=-2.0), dict(minutes_per_move=float("nan")),
           dict(minutes_per_move=None), dict(margin_minutes=-0.1), dict(margin_minutes=float("inf")), dict(margin_minutes=None),
           dict(unreached_safe=1), dict(unreached_safe=None), dict(scratch_bytes=-1), dict(scratch_bytes=1.5),
           dict(horizon_minutes=32769.0), dict(horizon_minutes=64.0, minutes_per_move=0.001)]
    for kw in bad:
        with pytest.raises(ValueError, match="escape"):
            escape.request(**dict(ok, **kw))
    assert escape.request(target=("BURNED",), horizon_minutes=32768.0)[5] == 32768.0
    assert escape.request(target=("BURNED",), horizon_minutes=32769.0, margin_minutes=1.0)[5] == 32769.0      # (the bound counts from the margin)
    assert escape.move_bound(1.0, 0.0, 64.0) == 64 and escape.move_bound(0.1, 0.0, 6.0) == eo.move_bound(0.1, 0.0, 6.0)
    # what needs no tensor: the list, the flags, the outputs
    for kw in (dict(envs=[0, 5]), dict(envs=[[0]]), dict(envs=[0.5]), dict(plane=1), dict(summary="yes"), dict(plane=False), dict(step=True, plane=True),
               dict(plane=True, scratch_bytes=1)):
        with pytest.raises(ValueError, match="escape"):
            escape.EscapeSpec(5, 24, 40, None, **dict(dict(ok, plane=True), **kw))
    with pytest.raises(ValueError, match="wider than 8192"):
        escape.EscapeSpec(1, 4, 8200, None, plane=True, **ok)
    with pytest.raises(ValueError, match="minutes"):
        escape.EscapeSpec(5, 24, 40, np.zeros((5, 24, 40), np.float32), plane=True, **ok)      # (a host array is no CUDA tensor)


def test_scratch_need():
    from simfire_amd import _args, escape, walk
    bounds = ((2 * 32768 + 3) * 4 + 255) // 256 * 256
    assert bounds == 262400
    for H, W in ((9, 9), (24, 40), (977, 1030), (1024, 1024), (2048, 2048)):
        assert escape.scratch_need(H, W) == walk.scratch_need(H, W) + (4 * H * W + 255) // 256 * 256 + bounds
        assert escape.scratch_need(H, W) % 256 == 0
    assert _args.band_count(1024, 1024) == 1024 and _args.band_count(977, 1030) == 1054
    one = escape.scratch_need(1024, 1024)
    assert one == 4890880 and 256 * one <= 1280 << 20 < 280 * one          # the default budget holds 256 environments of 1024 x 1024 in one chunk
    src = open(os.path.join(CSRC, "sf_escape_kernels.h")).read()
    assert "kEscapeScratchDefault = 1280ll << 20" in src and "kEscapeMaxMoves = 32768" in src


def test_abi_text():
    from simfire_amd import _lib
    h = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int sf_escape\(sf_sim \*sim, const sf_escape_params \*params, int32_t n, const int32_t \*envs[^)]*, const sf_escape_out \*out\);", h)
    for name, val in (("SF_ESCAPE_SAFE", "2147483647"), ("SF_ESCAPE_LOST", "(-1)"), ("SF_ESCAPE_BLOCKED", "(-2)"), ("SF_ESCAPE_MAX_MOVES", "32768"),
                      ("SF_ESCAPE_UNREACHED_SAFE", "1")):
        assert re.search(r"#define %s %s\n" % (name, re.escape(val)), h), name
    assert (_lib.SF_ESCAPE_SAFE, _lib.SF_ESCAPE_LOST, _lib.SF_ESCAPE_BLOCKED, _lib.SF_ESCAPE_MAX_MOVES, _lib.SF_ESCAPE_UNREACHED_SAFE) == (2 ** 31 - 1, -1, -2, 32768, 1)
    body = h[h.index("typedef struct sf_escape_params {"):h.index("} sf_escape_params;")]
    flat = []
    for decl in re.findall(r"\n\s+([^;/]+);", body):            # "int32_t a, b" / "const uint8_t *p" / "int32_t reserved[2]"
        flat += [re.sub(r"\[\d+\]", "", name.split()[-1].lstrip("*")) for name in decl.split(",")]
    assert [f[0] for f in _lib.SfEscapeParams._fields_] == flat, flat
    assert "int32_t reserved[2];" in body
    out = h[h.index("typedef struct sf_escape_out {"):h.index("} sf_escape_out;")]
    assert [f[0] for f in _lib.SfEscapeOut._fields_] == re.findall(r"int32_t \*(\w+);", out)
    assert "sf_escape" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_escape"]) == 5
    host = "\n".join(_code(os.path.join(CSRC, "sf_host_query.h")))
    assert 'extern "C" int sf_escape(' in host and "k_escape<true>, k_escape<false>" in host


def test_only_the_query_names_the_kernel():
    """The step path, the enqueue layer and the other features' kernels do not know the search: ``k_escape`` is named in its own
    header and in the host code of the queries, ``band_grow`` in ``sf_bands.h`` and the kernel."""
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        text = "\n".join(_code(os.path.join(CSRC, name)))
        if name not in ("sf_escape_kernels.h", "sf_host_query.h"):
            assert "k_escape" not in text and "EscapeArgs" not in text, name
        if name not in ("sf_escape_kernels.h", "sf_bands.h"):
            assert "band_grow" not in text, name
        if name != "simfire_hip.hip":
            assert "sf_escape_kernels.h" not in text, name
    kernel = open(os.path.join(CSRC, "sf_escape_kernels.h")).read()
    assert "asm" not in "\n".join(_code(os.path.join(CSRC, "sf_escape_kernels.h"))) and "band_grow(" in kernel and "band_round(" in kernel


def test_band_grow_on_the_host(tmp_path):
    """``tests/escape_check.cpp`` once plainly and once under the address and undefined-behaviour sanitizers, each its own program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    src = os.path.join(ROOT, "tests", "escape_check.cpp")
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / ("escape_check_" + tag))
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src] + extra, capture_output=True, text=True)
        if r.returncode != 0 and tag == "san" and re.search(r"cannot find|libasan|libubsan", r.stderr):
            pytest.fail("the sanitizer runtimes (libasan, libubsan) are missing: the sanitizer build is part of this test: " + r.stderr.strip().splitlines()[-1])
        assert r.returncode == 0, r.stderr
        run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (tag, run.stdout + run.stderr)
