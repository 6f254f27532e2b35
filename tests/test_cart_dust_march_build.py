"""CPU-side checks of the Cartesian dust / shearing-box instantiations of the tile march (kernels_curv.hip) and of its
species index: the library exports artemis_hip_stage_general_dust_variant and the header documents it, the switch
NO_CART_DUST_MARCH is one the library knows, and the two queries -- which touch no device -- send exactly the packs
the march now covers to it (gas variant 3; dust variant 3, or 5 with the drag finish inside the march)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = (b"NO_CART_DUST_MARCH", b"NO_CURV_DUST_MARCH", b"NO_DRAG_IN_MARCH", b"NO_CART_MARCH")


@pytest.fixture
def lib():
    """The library with the switches this file sets put back afterwards (NO_CART_DUST_MARCH is not in the list the
    suite-wide fixture restores)."""
    from artemis_amd import capi
    L = capi.load()
    before = {n: L.artemis_hip_get_option(n) for n in SWITCHES}
    yield L
    for n, v in before.items():
        if v >= 0:
            L.artemis_hip_set_option(n, v)


def _drag(capi, ntau, damping=False):
    """capi.Drag of simple_dust drag with constant stopping times (pack.drag_params without its torch import)."""
    d = capi.Drag()
    d.type, d.model, d.scale, d.grain_density = capi.DRAG_SIMPLE_DUST, capi.DRAG_CONSTANT, 1.0, 1.0
    for n in range(ntau):
        d.tau[n] = 0.05 * (n + 1)
    big = 1.7976931348623157e308
    for f in (d.gas, d.dust):
        f.ix[:], f.ox[:], f.irate[:], f.orate[:] = [-big] * 3, [big] * 3, [0.0] * 3, [0.0] * 3
    if damping:
        d.dust.irate[0] = 1.0
    d.xmin[:], d.xmax[:] = [0.0] * 3, [1.0] * 3
    return d


def _variants(L, capi, nx=(40, 20, 36), ng=2, coords=None, recon=None, riemann=None, ns_dust=1, drecon=None, driemann=None,
              **args):
    p = capi.Pack()
    p.nblocks, p.nghost = 1, ng
    p.nx1, p.nx2, p.nx3 = nx
    p.coords = capi.CARTESIAN if coords is None else coords
    p.gm1 = 0.4
    p.gas.nspecies, p.gas.recon, p.gas.riemann = 1, capi.PLM if recon is None else recon, capi.HLLC if riemann is None else riemann
    p.dust.nspecies, p.dust.recon = ns_dust, capi.PLM if drecon is None else drecon
    p.dust.riemann = capi.HLLE if driemann is None else driemann
    a = capi.StageGeneralArgs()
    a.gam0, a.gam1, a.beta_dt, a.bdt = 0.0, 1.0, 1e-3, 1e-3
    keep = []
    for k, v in args.items():
        if k in ("drag", "cooling"):
            keep.append(v)
            v = C.pointer(v)
        setattr(a, k, v)
    return (L.artemis_hip_stage_general_variant(C.byref(p), C.byref(a)),
            L.artemis_hip_stage_general_dust_variant(C.byref(p), C.byref(a)))


def test_the_symbol_is_exported_and_documented(lib):
    from artemis_amd import capi
    assert "artemis_hip_stage_general_dust_variant" in capi.EXPORTS_HIP
    fn = getattr(lib, "artemis_hip_stage_general_dust_variant")  # AttributeError: the library lacks it
    assert fn.restype is C.c_int
    header = open(os.path.join(ROOT, "include", "artemis_hip.h")).read()
    assert re.search(r"int artemis_hip_stage_general_dust_variant\(const artemis_pack_t \*p, const artemis_stage_general_args_t \*a\);",
                     header)
    for code in ("-1 = the pack has no dust", "0 = the\n * cell-centred dust kernels", "1 = the 2-D row", "3 = the dust instantiations",
                 "5 = the same march with the drag finish"):
        assert code in header, code
    assert "gas on any non-Cartesian system, geometry in LDS tables" not in header  # (variant 3's old description)
    # the host driver does not call it (the CPU double implements the ABI the driver links against, and lacks it)
    drv = os.path.join(ROOT, "artemis_amd", "csrc", "driver")
    for f in os.listdir(drv):
        assert "stage_general_dust_variant" not in open(os.path.join(drv, f), errors="ignore").read(), f
    assert "stage_general_dust_variant" not in open(os.path.join(ROOT, "artemis_amd", "driver.py")).read()


def test_the_switch_is_known_and_documented(lib):
    assert lib.artemis_hip_get_option(b"NO_CART_DUST_MARCH") == 0
    assert lib.artemis_hip_get_option(b"artemis_no_cart_dust_march") == 0
    assert "NO_CART_DUST_MARCH" in open(os.path.join(ROOT, "include", "artemis_hip.h")).read()
    assert "X(NO_CART_DUST_MARCH)" in open(os.path.join(ROOT, "artemis_amd", "csrc", "options.hpp")).read()


def test_march_for_cartesian_dust_and_the_shearing_box(lib):
    """(fails on the parent commit at the first assertion: it answers 0, and lacks the dust query)"""
    from artemis_amd import capi
    L = lib
    for ns in (1, 2, 16):
        assert _variants(L, capi, ns_dust=ns) == (3, 3), ns
    assert _variants(L, capi, driemann=capi.LLF) == (3, 3)
    assert _variants(L, capi, ns_dust=2, riemann=capi.LLF, driemann=capi.LLF) == (3, 3)
    assert _variants(L, capi, pcm=1) == (3, 3)
    assert _variants(L, capi, rf_omega=1.0, rf_qshear=1.5) == (3, 3)
    assert _variants(L, capi, rf_omega=1.0) == (3, 3)
    assert _variants(L, capi, ns_dust=0, rf_omega=1.0, rf_qshear=1.5) == (3, -1)  # the shearing box on gas alone
    assert _variants(L, capi, ns_dust=0) == (3, -1)
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=3) == (3, 3)                # 2-D, more species than the row march takes
    assert _variants(L, capi, nx=(8, 4, 4), ns_dust=1) == (3, 3)                  # a block smaller than a tile
    assert _variants(L, capi, defer_finish=1) == (3, 3) and _variants(L, capi, defer_finish=2) == (3, 3)
    # several species on the curvilinear systems: the gas march is no longer refused, the dust marches beside it
    assert _variants(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL, ns_dust=2) == (3, 3)
    assert _variants(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL, ns_dust=1) == (3, 3)  # (as before)


def test_drag_finish_inside_the_march_for_one_species_only(lib):
    from artemis_amd import capi
    L = lib
    assert _variants(L, capi, drag=_drag(capi, 1)) == (3, 5)
    assert _variants(L, capi, drag=_drag(capi, 1), rf_omega=1.2, rf_qshear=1.5, cfl_gas=0.3, cfl_dust=0.4, dt_dev=8) == (3, 5)
    assert _variants(L, capi, drag=_drag(capi, 1), defer_finish=2) == (3, 5)
    assert _variants(L, capi, drag=_drag(capi, 1), defer_finish=1) == (3, 3)      # stops at the conserved state
    assert _variants(L, capi, drag=_drag(capi, 1, damping=True)) == (3, 3)        # damping: the finish launch
    assert _variants(L, capi, ns_dust=2, drag=_drag(capi, 2)) == (3, 3)
    assert _variants(L, capi, ns_dust=3, drag=_drag(capi, 3)) == (3, 3)
    L.artemis_hip_set_option(b"NO_DRAG_IN_MARCH", 1)
    assert _variants(L, capi, drag=_drag(capi, 1)) == (3, 3)


def test_dust_the_march_does_not_take_stays_on_its_cell_kernel(lib):
    from artemis_amd import capi
    L = lib
    assert _variants(L, capi, drecon=capi.PPM, ng=3) == (3, 0)    # dust PPM: the gas still marches
    assert _variants(L, capi, drecon=capi.PPM, ng=3, pcm=1) == (3, 3)
    L.artemis_hip_set_option(b"NO_CURV_DUST_MARCH", 1)
    assert _variants(L, capi) == (3, 0)
    assert _variants(L, capi, ns_dust=3, drag=_drag(capi, 3)) == (3, 0)
    assert _variants(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL) == (3, 0)


def test_what_stays_on_the_kernels_it_had(lib):
    from artemis_amd import capi
    L = lib
    assert _variants(L, capi, nbody_n=1) == (0, 0)                          # N-body on a Cartesian pack
    assert _variants(L, capi, ns_dust=0, nbody_n=1) == (0, -1)
    cool = capi.Cooling()
    assert _variants(L, capi, cooling=cool) == (0, 0)
    assert _variants(L, capi, nx=(131, 1, 1), ns_dust=2) == (0, 0)          # 1-D
    assert _variants(L, capi, nx=(131, 1, 1), ns_dust=0, rf_omega=1.0) == (0, -1)
    assert _variants(L, capi, recon=capi.PPM, ng=3) == (0, 0)               # PPM gas with dust
    assert _variants(L, capi, defer_finish=3) == (0, 0)                     # (artemis_hip_stage_general refuses it: EINVAL)
    # the 2-D row march still wins first for what it takes
    for ns in (0, 1, 2):
        assert _variants(L, capi, nx=(61, 40, 1), ns_dust=ns, rf_omega=1.0, rf_qshear=1.5) == (1, 1 if ns else -1), ns
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=2, drag=_drag(capi, 2)) == (1, 1)
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=2, strat_faces=15) == (1, 1)
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=3, strat_faces=15) == (0, 0)  # strat_faces: the row march only
    # NO_CART_MARCH keeps its meaning, and so does the new switch: the parent's kernels
    L.artemis_hip_set_option(b"NO_CART_MARCH", 1)
    assert _variants(L, capi) == (0, 0) and _variants(L, capi, ns_dust=0, rf_omega=1.0) == (0, -1)
    L.artemis_hip_set_option(b"NO_CART_MARCH", 0)
    L.artemis_hip_set_option(b"NO_CART_DUST_MARCH", 1)
    for ns in (1, 2, 16):
        assert _variants(L, capi, ns_dust=ns) == (0, 0), ns
    assert _variants(L, capi, ns_dust=0, rf_omega=1.0, rf_qshear=1.5) == (0, -1)
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=3) == (0, 0)
    assert _variants(L, capi, drag=_drag(capi, 1)) == (0, 0)
    assert _variants(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL, ns_dust=2) == (0, 0)
    # ... and what marched before this switch existed still marches under it
    assert _variants(L, capi, ns_dust=0) == (3, -1)                                          # Cartesian gas
    assert _variants(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL, ns_dust=1) == (3, 3)  # curvilinear, one species
    assert _variants(L, capi, nx=(61, 40, 1), ns_dust=2) == (1, 1)
    L.artemis_hip_set_option(b"NO_CART_DUST_MARCH", 0)
    assert _variants(L, capi) == (3, 3)
