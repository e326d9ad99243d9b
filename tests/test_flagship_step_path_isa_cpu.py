"""What NOTEBOOK.md 5.18 took off the step path of the flagship kernel, k_run<1, 0, 1, 0, 2>, shows only in the compiled code - none of it
changes a result.  The kernel is compiled to gfx950 assembly with the product flags (no GPU needed) and read with
profiles/isa_step_path.py, the same reading as a tool (profiles/r08_isa_step_path.txt is its output for the parent and for this source).

  * registers: no scratch, at most 128 VGPRs, 4 waves per SIMD - what the kernel had, kept;
  * spilled SGPRs: 334 in the parent (the argument block by value, 228 of them stored in the entry block); 252 with the block split
    (by value what a step looks at, through the kernel-argument segment what only a cut, a join or the way out needs).  The bound is
    this source's own number + 10, so that the test guards the result and not the parent;
  * the batch loop is unrolled by two: no block of register moves - "this batch's rows = the rows requested during the batch before",
    8 v_mov_b64 + 7 v_mov_b32 in the parent - between the loop's header and the prefetch, and no scalar load inside the loop (read
    through the segment as a whole, the loop reloaded 13 argument words per batch);
  * the kernel with the statistics, k_run<1, 0, 1, 0, 3>, exists beside it (the host launches it when the counters are on)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGSHIP, COUNTED = "1,0,1,0,2", "1,0,1,0,3"
SPILLED_SGPRS = 252          # this source's cross-compile (profiles/r08_isa_step_path.txt); the parent: 334


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "profiles", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not installed")
    sp = _tool("isa_step_path")
    asm = sp.iw.compile_asm("simfire_hip_run2.hip", str(tmp_path_factory.mktemp("isa") / "simfire_hip_run2.s"))
    with open(asm) as f:
        text = f.read()
    return sp, text, sp.analyse(text, FLAGSHIP)


def test_registers_of_the_flagship(unit):
    _, _, a = unit
    r = a["resources"]
    assert r["ScratchSize"] == 0 and r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["NumVgprs"] <= 128 and r["Occupancy"] == 4, r


def test_spilled_sgprs_of_the_flagship(unit):
    _, _, a = unit
    n = a["resources"]["sgpr_spill_count"]
    assert n < 334, "no fewer spilled SGPRs than the parent: %d" % n
    assert n <= SPILLED_SGPRS + 10, "the flagship spills %d SGPRs; this source was committed with %d" % (n, SPILLED_SGPRS)


def test_no_row_copy_at_the_head_of_the_batch_loop(unit):
    _, _, a = unit
    hm = a["header_moves"]
    assert hm["v_mov_b64"] == 0 and hm["longest_run"] < 4, "register moves between the batch loop's header and the prefetch: %s" % hm


def test_no_scalar_load_in_the_batch_loop(unit):
    _, _, a = unit
    assert a["batch_loop"]["SMEM"] == 0, a["batch_loop"]
    assert a["batch_loop"]["lane"] <= 8, a["batch_loop"]          # (spill traffic inside the loop: 3 in the parent's one batch, 4 in this one's two)


def test_the_counting_kernel_is_built_beside_it(unit):
    sp, text, _ = unit
    c = sp.analyse(text, COUNTED)
    assert c["resources"]["Occupancy"] == 4 and c["resources"]["ScratchSize"] == 0, c["resources"]
