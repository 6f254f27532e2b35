"""CPU-side checks of the PPM tile march (kernels_ppm.hip): it is part of the library that is built, its switch is one
the library knows and the public header documents, and artemis_hip_stage_general_variant -- which touches no device --
sends exactly the packs the march covers to it (variant 4)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_march_is_a_unit_of_the_library():
    from artemis_amd import build, capi
    assert "kernels_ppm.hip" in build.HIP_SOURCES
    assert os.path.isfile(os.path.join(build.CSRC, "kernels_ppm.hip"))
    capi.load()
    sha = build.object_hashes()["kernels_ppm"]
    assert re.fullmatch(r"[0-9a-f]{64}", sha) and capi.object_sha("kernels_ppm") == sha


def test_the_switch_is_known_and_documented():
    from artemis_amd import capi
    L = capi.load()
    assert L.artemis_hip_get_option(b"NO_PPM_MARCH") == 0
    assert L.artemis_hip_get_option(b"NO_SUCH_MARCH") < 0
    header = open(os.path.join(ROOT, "include", "artemis_hip.h")).read()
    assert "NO_PPM_MARCH" in header
    assert "NO_PPM_MARCH" in open(os.path.join(ROOT, "artemis_amd", "csrc", "options.hpp")).read()
    assert re.search(r"4 = the PPM tile march", header)


def _variant(L, capi, nx=(40, 20, 36), ng=3, coords=None, recon=None, ns_gas=1, ns_dust=0, **args):
    p = capi.Pack()
    p.nblocks, p.nghost = 1, ng
    p.nx1, p.nx2, p.nx3 = nx
    p.coords = capi.CARTESIAN if coords is None else coords
    p.gm1 = 0.4
    p.gas.nspecies, p.gas.recon, p.gas.riemann = ns_gas, capi.PPM if recon is None else recon, capi.HLLC
    p.dust.nspecies, p.dust.recon, p.dust.riemann = ns_dust, capi.PPM, capi.HLLE
    a = capi.StageGeneralArgs()
    a.gam0, a.gam1, a.beta_dt, a.bdt = 0.0, 1.0, 1e-3, 1e-3
    for k, v in args.items():
        setattr(a, k, v)
    return L.artemis_hip_stage_general_variant(C.byref(p), C.byref(a))


def test_variant_4_for_what_the_march_covers_and_nothing_else():
    from artemis_amd import capi
    L = capi.load()
    L.artemis_hip_stage_general_variant.restype = C.c_int
    assert _variant(L, capi) == 4
    assert _variant(L, capi, nx=(8, 4, 4), ng=4) == 4        # a block smaller than a tile
    assert _variant(L, capi, nx=(33, 9, 17)) == 4            # ragged
    assert _variant(L, capi, cfl_gas=0.3, dt_dev=8) == 4     # (the pointer is not followed)
    # not covered: as on the parent commit
    assert _variant(L, capi, ns_dust=1) == 0                 # a dust species beside the gas
    assert _variant(L, capi, pcm=1) == 3                     # vl2's predictor stage: the Cartesian tile march of PCM / PLM
    assert _variant(L, capi, nx=(61, 40, 1)) == 0            # 2-D
    assert _variant(L, capi, nx=(16, 8, 6), coords=capi.CYLINDRICAL) == 0
    assert _variant(L, capi, defer_finish=1) == 0
    assert _variant(L, capi, defer_finish=2) == 0
    assert _variant(L, capi, rf_omega=1.0) == 0
    assert _variant(L, capi, recon=capi.PLM) == 3            # PLM keeps its own march
    assert _variant(L, capi, defer_finish=3) == 0            # (artemis_hip_stage_general refuses it: EINVAL)
    before = L.artemis_hip_get_option(b"NO_PPM_MARCH")
    try:
        L.artemis_hip_set_option(b"NO_PPM_MARCH", 1)
        assert _variant(L, capi) == 0
    finally:
        L.artemis_hip_set_option(b"NO_PPM_MARCH", before)
    assert _variant(L, capi) == 4

