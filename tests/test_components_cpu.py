"""Connected components without a GPU (``sf_components``): the oracle against ``scipy.ndimage.label`` and against
what the scenes claim, the shared header's arithmetic in a program of its own under the sanitizers, the request checks, the scratch
arithmetic, and the texts that have to agree."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _components_oracle as co
import _components_worlds as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simfire_amd", "csrc")
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1]] * 3}


def _against_scipy(sel, conn, tag):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(sel, structure=STRUCTURE[conn])
    got, c = co.label(sel, conn)
    assert c == n and (got == lab).all(), tag


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("density", [0.3, 0.5, 0.6])
@pytest.mark.parametrize("conn", [4, 8])
def test_oracle_against_scipy_on_random_maps(density, conn):
    """Same labels in the same order; 0.6 lies near the percolation threshold of the 4-neighbourhood: long winding components."""
    rng = np.random.default_rng(int(density * 10) * 10 + conn)
    for H, W in ((9, 9), (33, 17), (40, 130), (64, 64), (120, 200)):
        _against_scipy(rng.random((H, W)) < density, conn, (H, W, density, conn))


@pytest.mark.parametrize("shape", cw.SHAPES, ids=["%dx%d" % s for s in cw.SHAPES])
def test_scenes_on_the_oracle(shape):
    """Every scene: the oracle's labels equal scipy's, the count is the one the scene claims, its claim holds, and the rows fit
    together (sizes sum to the selected cells, the first cell carries its number, boxes hold their cells)."""
    H, W = shape
    names = set()
    for s in cw.scenes(H, W):
        assert s["name"] not in names
        names.add(s["name"])
        member = cw.per_env_member(4, H, W)[1] if isinstance(s["member"], str) else s["member"]
        mask = co.mask_of(s["select"])
        _against_scipy(co.selected(s["map"], mask, member), s["conn"], (shape, s["name"]))
        r = co.components(s["map"], mask, s["conn"], member=member, cap=cw.CAP, points=s["points"])
        C = int(r["count"])
        if s["count"] is not None:
            assert C == s["count"], (shape, s["name"], C)
        if s["claim"] is not None:
            s["claim"](r)
        big = co.components(s["map"], mask, s["conn"], member=member, cap=max(C, 1))
        assert int(big["cells"].sum()) == int(r["selected"]) == int((r["labels"] > 0).sum())
        for j in range(min(C, cw.CAP)):
            y, x = divmod(int(r["first"][j]), W)
            x0, y0, x1, y1 = r["bbox"][j].tolist()
            assert r["labels"][y, x] == j + 1 and y == y0 and x0 <= x <= x1 and (r["labels"][y0:y1 + 1, x0:x1 + 1] == j + 1).sum() == r["cells"][j]
        assert (r["cells"][C:] == 0).all() and (r["first"][C:] == -1).all() and (r["touch"][C:] == 0).all()
        if C:
            assert r["largest"][1] == big["cells"].max() and big["cells"][r["largest"][0] - 1] == r["largest"][1]
            assert not (big["cells"][:r["largest"][0] - 1] == r["largest"][1]).any()            # ties go to the lower number
    assert {"checkerboard_4", "comb_8", "ring_4", "points_8", "member_per_env_4", "wall_to_the_last_column_8", "diagonal_touch_4"} <= names
    if W >= 130:
        assert {"gaps_a_4", "gaps_b_8", "gaps_c_4", "spiral_4"} <= names


def test_oracle_touch_and_values_by_hand():
    m = np.array([[1, 1, 0, 3],
                  [0, 0, 0, 3],
                  [2, 0, 1, 1]], dtype=np.uint8)
    vals = np.arange(12, dtype=np.int32).reshape(3, 4) - 3
    r = co.components(m, 2, 4, values=vals, cap=3, points=np.array([(0, 0, 1), (2, 0, 1), (3, 2, 5), (3, 2, 0), (4, 0, 1)]))
    assert int(r["count"]) == 2 and r["cells"].tolist() == [2, 2, 0] and r["first"].tolist() == [0, 10, -1]
    assert r["touch"].tolist() == [64 | 1, 64 | 1 | 8, 0] and r["value"].tolist() == [-3 - 2, 7 + 8, 0]
    assert r["bbox"].tolist() == [[0, 0, 1, 0], [2, 2, 3, 2], [-1] * 4] and r["largest"].tolist() == [1, 2]
    assert r["point_label"].tolist() == [1, 0, 2, -1, -1]
    r8 = co.components(m, 1 | 2, 8, cap=1)
    assert int(r8["count"]) == 1 and r8["touch"].tolist() == [64 | 4 | 8] and r8["cells"].tolist() == [9]
    member = np.ones((3, 4), dtype=np.uint8)
    member[0, 1] = 0
    assert co.components(m, 2, 4, member=member)["touch"][0] == 64 | 1 | 2            # (the cell the member plane took out is BURNING and not selected)


# ---------------------------------------------------------------------------------------------- the shared header
def test_components_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) on this machine")
    exe = str(tmp_path / "components_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "components_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan", r.stderr):
        # only a machine WITHOUT the runtimes may fall back: where the compiler can name both, the sanitizer build has to link
        have = [subprocess.run([cxx, "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip() for lib in ("libasan.so", "libubsan.so")]
        assert not all(os.path.isabs(h) for h in have), "the sanitizer runtimes are here (%s) but the build failed:\n%s" % (have, r.stderr)
        print("sanitizer runtime missing, building without:", r.stderr.strip().splitlines()[-1])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def test_header_stands_alone_and_the_kernels_use_it():
    """``sf_components.h`` includes ``<cstdint>`` only; the kernel file includes it and the queries' device header, is part of the
    translation unit the build compiles, and touches the label plane in the merge through agent-scope atomics only."""
    from simfire_amd import build
    assert re.findall(r"#include\s*(\S+)", open(os.path.join(CSRC, "sf_components.h")).read()) == ["<cstdint>"]
    kern = open(os.path.join(CSRC, "sf_components_kernels.h")).read()
    assert re.findall(r"#include\s*(\S+)", kern) == ['"sf_components.h"', '"sf_query_dev.h"']
    unit = open(os.path.join(CSRC, "simfire_hip.hip")).read()
    assert '#include "sf_components_kernels.h"' in unit and "simfire_hip.hip" in build.SOURCES
    assert unit.index('"sf_components_kernels.h"') < unit.index('"sf_handle.h"')
    merge = kern[kern.index("void k_comp_merge("):kern.index("void k_comp_heads(")]
    assert "cc_unite(plane" in merge and "cc_contacts(" in merge and not re.search(r"\blab\[", merge)
    plane = kern[kern.index("struct CompPlane {"):kern.index("};", kern.index("struct CompPlane {"))]
    assert plane.count("__HIP_MEMORY_SCOPE_AGENT") == 3 and "__hip_atomic_load" in plane and "__hip_atomic_fetch_min" in plane
    assert not re.search(r"\basm\b|__asm", kern)
    for fn in ("cc_first_col", "cc_carry_col", "cc_seg_sum", "cc_seg_write", "cc_next_run", "cc_touch_run", "cc_touch_from", "cc_border", "cc_largest_key"):
        assert fn + "(" in kern, fn
    host = open(os.path.join(CSRC, "sf_host_query.h")).read()
    assert "cc_env_bytes(g.H, g.W, out->labels != nullptr)" in host and "s->components" in host


# ---------------------------------------------------------------------------------------------- the request
def test_request_refusals():
    from simfire_amd import components
    from simfire_amd.enums import BurnStatus
    assert components.request() == (2, 0, 64, 0)
    assert components.request(("UNBURNED", BurnStatus.BURNED), 8, 4096, 1 << 20) == (1 | 4, 8, 4096, 1 << 20)
    assert components.request(63, 4, 1)[:3] == (63, 4, 1)
    for kwargs in (dict(select=()), dict(select=0), dict(select=64), dict(select=("EMBERS",)), dict(connectivity=6), dict(connectivity=True),
                   dict(connectivity=4.0), dict(max_components=0), dict(max_components=4097), dict(max_components=2.0),
                   dict(max_components=True), dict(scratch_bytes=-1), dict(scratch_bytes=1.5)):
        with pytest.raises(ValueError, match="components"):
            components.request(**kwargs)
    assert components.mask_of(("BURNING",)) == 2 and components.TOUCH_BORDER == 64


def test_spec_refusals_and_outputs():
    from simfire_amd.components import ComponentsSpec
    s = ComponentsSpec(4, 24, 40, False, envs=[3, 1, 1], labels=True, cells=True, first=True, bbox=True, touch=True, largest=True, selected=True,
                       max_components=7)
    assert list(s.outputs) == ["count", "selected", "labels", "cells", "first", "bbox", "touch", "largest"]
    assert s.outputs["labels"] == ((3, 24, 40), "int32") and s.outputs["bbox"] == ((3, 7, 4), "int32") and s.outputs["largest"] == ((3, 2), "int32")
    assert ComponentsSpec(4, 24, 40, True, value=True).outputs["value"] == ((4, 64), "int64")
    p = s.params()
    assert (p.select_mask, p.connectivity, p.k, p.max_components, p.member_per_env, p.reserved0) == (2, 0, 0, 7, 0, 0) and not p.member and not p.points
    for kwargs in (dict(count=False), dict(value=True), dict(labels=1), dict(envs=[4]), dict(envs=[-1]), dict(scratch_bytes=100),
                   dict(member=np.ones((24, 40), dtype=np.uint8)), dict(points=np.zeros((4, 2, 3), dtype=np.int32))):
        with pytest.raises(ValueError, match="components"):
            ComponentsSpec(4, 24, 40, False, **kwargs)
    with pytest.raises(ValueError, match="8192"):
        ComponentsSpec(1, 2, 8200, False)


def test_scratch_need_arithmetic():
    """Head, bits in whole words, a counter per row, the second plane, the label plane unless labels is one - each rounded to 256; at
    most 4 + 4 bytes and a bit per cell, plus the rows and the rounding."""
    from simfire_amd.components import scratch_need
    assert scratch_need(1, 1) == 256 + 256 + 256 + 256 + 256 and scratch_need(1, 1, labels=True) == 256 * 4
    assert scratch_need(24, 40) == 256 + 256 + 256 + 3840 + 3840
    assert scratch_need(70, 1030) == 256 + (70 * 17 * 8 + 255) // 256 * 256 + 512 + 2 * ((4 * 70 * 1030 + 255) // 256 * 256)
    n = 1024 * 1024
    assert scratch_need(1024, 1024) == 256 + n // 8 + (4 * 1025 + 255) // 256 * 256 + 8 * n
    assert scratch_need(1024, 1024, labels=True) == scratch_need(1024, 1024) - 4 * n
    text = open(os.path.join(CSRC, "sf_components.h")).read()
    assert "kCompHeadBytes + cc_round((long long)H * cc_words(W) * 8) + cc_round(4ll * (H + 1)) + cc_round(4 * n) + (labels_out ? 0 : cc_round(4 * n))" in text


# ---------------------------------------------------------------------------------------------- the texts
def test_abi_comment_lists_every_refusal():
    """The table in the header names every refusal of the host function, in its order, and the function refuses nothing else with
    SF_EINVAL; the binding declares the call and structures of the header's size."""
    import ctypes as C
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    doc = header[header.index("sf_components_out;"):header.index("int sf_components(")]
    rows = re.findall(r"^ \*   \| (.*?)\s*\|$", doc, flags=re.M)
    assert rows[0] == "refused" and len(rows) == 13
    host = open(os.path.join(CSRC, "sf_host_query.h")).read()
    body = host[host.index('extern "C" int sf_components('):]
    body = body[:body.index("QueryState &q")]
    marks = ["select_mask %d", "connectivity %d", "check_points(who, p->k, p->points, true)", "max_components %d", "point_label needs k > 0",
             "check_reserved(who, p->reserved0 | p->reserved[0] | p->reserved[1])", "every output is null", "check_aligned(who", "check_scratch(who",
             "check_envs(s, who, n, envs)", "value needs a value plane"]
    at = [body.index(m) for m in marks]
    assert at == sorted(at)
    keys = ["select_mask", "connectivity", "k outside", "points", "max_components", "point_label", "reserved", "every output null", "aligned", "scratch_bytes",
            "environment out of range", "value without a value plane"]
    for row, key in zip(rows[1:], keys):
        assert key in row, (row, key)
    assert body.count("SF_EINVAL") == 9 and body.count("SF_ENOTSUP") == 2 and "SF_ESTATE" not in body
    assert _lib.SIGNATURES["sf_components"][1]._type_ is _lib.SfComponentsParams and _lib.SF_COMPONENTS_MAX == 4096
    assert C.sizeof(_lib.SfComponentsParams) == 56 and C.sizeof(_lib.SfComponentsOut) == 80
    decl = r"^ +(?:const )?\w+ \*?(\w+)(?:\[2\])?;"
    fields = re.findall(decl, header[header.index("typedef struct sf_components_out {"):header.index("} sf_components_out;")], flags=re.M)
    assert fields == [f[0] for f in _lib.SfComponentsOut._fields_]
    fields = re.findall(decl, header[header.index("typedef struct sf_components_params {"):header.index("} sf_components_params;")], flags=re.M)
    assert fields == [f[0] for f in _lib.SfComponentsParams._fields_]


def test_documents_name_the_query():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 31\. ", design, flags=re.M) and "sf_components.h" in design[design.index("21a"):]
    for name in ("README.md", "INTEGRATION.md"):
        assert "components(" in open(os.path.join(ROOT, name)).read(), name
