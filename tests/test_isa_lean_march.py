"""The generated code of the lean form of the Cartesian march: stage_fused_kernel_lean leaves
the internal-energy equation out, so its plane loop must hold fewer vector instructions and less LDS traffic than the
full instantiation of the same row, within the same budget -- no scratch, two workgroups per CU, the 80 KiB tile -- and
under the same condition on exposed LDS waits as tests/test_isa_lds_waits.py holds the full instantiations to.  The
counts are scripts/lds_wait_audit.py's; the comparisons are relations between two kernels of one compilation, not
fixed numbers.  Compiles kernels_fused.hip to gfx950 assembly once; no GPU needed."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MAX_EXPOSED = 8  # (a condition, not a measurement: tests/test_isa_lds_waits.py)
RIEMANN = {0: "hllc", 1: "hlle", 2: "llf"}
# <RIEMANN, RECON = plm, HAS_U1, WRITE_CONS, WITH_DT, D3, CURV, FLUXES>: what launch_fused picks for the stages of rk2
STAGES = {"stage 1": "false, false, false", "stage 2": "true, false, true"}


@pytest.fixture(scope="module")
def fused_table():
    from artemis_amd import build
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip("hipcc not found")
    import lds_wait_audit
    return dict(lds_wait_audit.table("kernels_fused.hip"))


@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("riemann", sorted(RIEMANN))
def test_lean_march_is_leaner_within_the_same_budget(fused_table, riemann, stage):
    args = "%d, 1, %s, true, false, false" % (riemann, STAGES[stage])
    lean_name, full_name = "void stage_fused_kernel_lean<%s>" % args, "void stage_fused_kernel<%s>" % args
    assert lean_name in fused_table, "instantiation not found in the assembly: %s" % lean_name
    assert full_name in fused_table, "instantiation not found in the assembly: %s" % full_name
    lean, full = fused_table[lean_name], fused_table[full_name]
    print("%s %s: lean %s" % (RIEMANN[riemann], stage, lean))
    print("%s %s: full %s" % (RIEMANN[riemann], stage, full))
    assert lean["loop"] and full["loop"], "no plane loop found"
    assert lean["ScratchSize"] == 0
    assert lean["Occupancy"] == 2
    assert lean["LDSByteSize"] <= 81920
    assert lean["exposed"] <= MAX_EXPOSED, "%d exposed LDS waits in the plane loop" % lean["exposed"]
    for what in ("valu", "ds_read", "ds_write"):
        assert 0 < lean[what] < full[what], "%s: lean %d, full %d" % (what, lean[what], full[what])
