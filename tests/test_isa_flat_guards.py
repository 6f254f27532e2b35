"""The generated code of the tile march's flat-wave guards: the default form must spend fewer
guard branches in the plane loop than one wave-uniform guard per slope (-DARTEMIS_FLAT_SKIP=1) does.  A per-slope guard
is a vector compare, a scalar compare of the mask against exec and a scalar conditional branch; the count below is of
those branches (`s_cbranch_scc1`) in the largest loop of the headline HLLC + PLM instantiations, lean and full, as
scripts/lds_wait_audit.py delimits it.  A relation between two compilations of one source, not a fixed number.
Compiles kernels_fused.hip to gfx950 assembly twice; no GPU needed."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# <RIEMANN = hllc, RECON = plm, HAS_U1, WRITE_CONS, WITH_DT, D3, CURV, FLUXES>: what launch_fused picks for the stages of rk2
STAGES = {"stage 1": "false, false, false", "stage 2": "true, false, true"}
KERNELS = ("stage_fused_kernel_lean", "stage_fused_kernel")
BRANCH = "s_cbranch_scc1"


def _guard_branches(extra):
    """{demangled kernel name: count of BRANCH in the kernel's largest loop} for one compilation."""
    import lds_wait_audit as audit
    ks = audit.kernels(audit.compile_asm("kernels_fused.hip", extra))
    out = {}
    for name, short in zip(ks, audit.demangle(ks)):
        lines = ks[name]["lines"]
        lo, hi = audit.main_region(lines)
        out[short] = sum(1 for ln in lines[lo:hi + 1] if ln.split() and ln.split()[0] == BRANCH)
    return out


@pytest.fixture(scope="module")
def counts():
    from artemis_amd import build
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip("hipcc not found")
    return {"default": _guard_branches(()), "per slope": _guard_branches(("-DARTEMIS_FLAT_SKIP=1",))}


@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_default_form_has_fewer_guard_branches_than_one_per_slope(counts, kernel, stage):
    name = "void %s<0, 1, %s, true, false, false>" % (kernel, STAGES[stage])
    for build_ in counts:
        assert name in counts[build_], "instantiation not found in the assembly (%s): %s" % (build_, name)
    default, per_slope = counts["default"][name], counts["per slope"][name]
    print("%s %s: %s in the plane loop: default %d, one guard per slope %d" % (kernel, stage, BRANCH, default, per_slope))
    assert per_slope > 0
    assert default < per_slope
