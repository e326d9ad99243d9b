"""The vector pass of k_run requests the rows of a wave's NEXT batch before it works on the current one.  That only pays if nothing
between the request and the current batch's work waits for those rows - and a wait there changes no result, so only the compiled code
can show it (NOTEBOOK.md 5.13: a select on the loaded rows once put `s_waitcnt vmcnt(0)` right behind the prefetch).

The flagship kernel, k_run<1, 0, 1, 0, 2>, is compiled to gfx950 assembly with the product flags (no GPU needed) and the instructions
between the four row loads of the prefetch and the first `wave_shr:1` DPP - the start of a batch's work - are walked with
profiles/isa_waits.py, the same walk as a tool."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGSHIP = "1,0,1,0,2"


def _tool():
    spec = importlib.util.spec_from_file_location("isa_waits", os.path.join(ROOT, "profiles", "isa_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def flagship_body(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not installed")
    iw = _tool()
    asm = iw.compile_asm("simfire_hip_run2.hip", str(tmp_path_factory.mktemp("isa") / "simfire_hip_run2.s"))
    with open(asm) as f:
        return iw, iw.kernel_lines(f.read(), FLAGSHIP)


def test_prefetch_is_found(flagship_body):
    """The walk looks at the right place: four consecutive 16-byte row loads, then the batch's first DPP, a short way on."""
    iw, body = flagship_body
    load, dpp = iw.find_prefetch(body)
    assert all(iw.ROW_LOAD in body[load - k] for k in range(4))
    assert iw.DPP_START in body[dpp] and 0 < dpp - load < 400


def test_no_wait_for_next_rows_on_the_plain_path(flagship_body):
    """A wave without an edge lane and without a boundary row (every s_cbranch_execz taken) meets no wait that names vmcnt between
    the prefetch and the current batch's work."""
    iw, body = flagship_body
    load, dpp = iw.find_prefetch(body)
    waits = iw.vm_waits_on_skip_path(body, load, dpp)
    assert not waits, "the prefetch of the next batch's rows is waited for in front of the current batch: %s" % waits


def test_no_wait_for_next_rows_on_any_path(flagship_body):
    """Nor does any other wave: the halo rows of a team's boundary rows are put in where the rows are consumed, and the edge words are
    only loaded, not looked at, in front of the batch's work."""
    iw, body = flagship_body
    load, dpp = iw.find_prefetch(body)
    waits = iw.vm_waits_between(body, load, dpp)
    assert not waits, "a wait that names vmcnt lies between the prefetch and the batch's first DPP: %s" % waits
