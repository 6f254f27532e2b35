"""The generated code of the tuned Cartesian march keeps its LDS reads ahead of the arithmetic that uses them.

A store to the `__shared__` tile orders every later load of the tile behind it (the compiler cannot tell the members
apart through run-time indices), so a phase that reads, computes and stores strip by strip waits for a whole LDS round
trip per strip: 28 times per plane before `plane_sweeps` requested each phase's reads first (DESIGN.md section 3.9,
pattern 5).  This test compiles kernels_fused.hip to gfx950 assembly once (about 100 s, no GPU needed) and holds the
headline instantiations -- HLLC / HLLE / LLF with PLM on 3-D blocks, both stages of rk2 -- to their budget and to at
most 8 exposed waits in the plane loop, counted as scripts/lds_wait_audit.py defines them.  The 8 is a condition, not a
measurement: one unavoidable first wait per phase entry (P1, the two P1 duties, P2, the P2 perimeter pass, the plane
flag) plus two of slack."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MAX_EXPOSED = 8
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
def test_headline_march_exposes_few_lds_round_trips(fused_table, riemann, stage):
    name = "void stage_fused_kernel<%d, 1, %s, true, false, false>" % (riemann, STAGES[stage])
    assert name in fused_table, "instantiation not found in the assembly: %s" % name
    r = fused_table[name]
    print("%s %s: %s" % (RIEMANN[riemann], stage, r))
    assert r["loop"], "no plane loop found"
    assert r["ScratchSize"] == 0
    assert r["Occupancy"] == 2
    assert r["NumVgprs"] <= 256
    assert r["LDSByteSize"] <= 81920
    assert r["ds_read"] > 0 and r["waits"] > 0  # (the audit saw the loop's LDS traffic at all)
    assert r["exposed"] <= MAX_EXPOSED, "%d exposed LDS waits in the plane loop" % r["exposed"]
