#!/usr/bin/env python3
"""Which kernels a general stage runs, as a table: the answers of artemis_hip_stage_general_variant and
artemis_hip_stage_general_dust_variant over the full product of the axes below, one character per row.  The queries
touch no device and validate nothing, so no pointer in the packs is real; rows that artemis_hip_stage_general itself
would refuse are kept.  Uses the two queries and artemis_hip_set_option only, so it runs in a checkout of any commit
that has them:
    python scripts/stage_plan_table.py > tests/golden/stage_plan_table.json
tests/test_stage_plan.py holds the library to the committed table (recorded from the commit before the stage plan)."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1.7976931348623157e308

SWITCHES = ["none", "NO_PPM_MARCH", "NO_STAGE2D", "NO_FUSED_CURV", "NO_CURV_MARCH", "NO_CART_MARCH", "NO_CART_DUST_MARCH",
            "NO_CURV_DUST_MARCH", "NO_DRAG_IN_MARCH"]
BLOCKS = ["cartesian 40x20x36", "cartesian 61x40x1", "cartesian 131x1x1", "cylindrical 16x8x6", "cylindrical 16x8x1",
          "spherical1D 32x1x1", "spherical2D 16x8x1", "spherical3D 16x8x6", "axisymmetric 16x8x1", "axisymmetric 16x1x1"]
GAS_RECON = ["plm", "ppm", "plm pcm=1"]  # (gas Riemann solver: HLLC)
# n species with the gas's reconstruction; the last entry is one species whose own reconstruction is PPM whatever the gas has
DUST = ["none"] + ["%d %s" % (n, r) for n in (1, 2, 3) for r in ("hlle", "llf")] + ["1 hlle ppm"]
TASKS = ["none", "uniform gravity", "rf_omega rf_qshear", "drag", "drag damping", "diffusion flux arrays", "diffusion sums",
         "cooling", "nbody_n=1", "strat_faces=15"]
DEFER = ["0", "1", "2"]
AXES = [("switch", SWITCHES), ("block", BLOCKS), ("gas_recon", GAS_RECON), ("dust", DUST), ("task", TASKS),
        ("defer_finish", DEFER)]  # outermost first: the order of the rows
DUST_CODES = [-1, 0, 1, 3, 5]
ALPHABET = "abcdefghijklmnopqrstuvwxy"  # the pair (gas code 0..4, dust code): ALPHABET[5 * gas + DUST_CODES.index(dust)]
NGHOST = 3


def decode(ch):
    n = ALPHABET.index(ch)
    return n // 5, DUST_CODES[n % 5]


def _call(capi, block, gas_recon, dust, task, defer):
    """(pack, args, objects the two point to) of one row"""
    p, a, keep = capi.Pack(), capi.StageGeneralArgs(), []
    system, shape = block.split()
    p.nblocks, p.nghost, p.gm1 = 1, NGHOST, 0.4
    p.nx1, p.nx2, p.nx3 = (int(n) for n in shape.split("x"))
    p.coords = {"cartesian": capi.CARTESIAN, "cylindrical": capi.CYLINDRICAL, "spherical1D": capi.SPHERICAL1D,
                "spherical2D": capi.SPHERICAL2D, "spherical3D": capi.SPHERICAL3D, "axisymmetric": capi.AXISYMMETRIC}[system]
    p.gas.nspecies, p.gas.riemann = 1, capi.HLLC
    p.gas.recon = capi.PPM if gas_recon == "ppm" else capi.PLM
    a.pcm = 1 if gas_recon.endswith("pcm=1") else 0
    d = dust.split()
    p.dust.nspecies = 0 if dust == "none" else int(d[0])
    p.dust.recon = capi.PPM if d[-1] == "ppm" else p.gas.recon
    p.dust.riemann = capi.LLF if "llf" in d else capi.HLLE
    a.gam0, a.gam1, a.beta_dt, a.bdt, a.defer_finish = 0.0, 1.0, 1e-3, 1e-3, int(defer)
    if task == "uniform gravity":
        g = capi.Gravity()
        g.type, g.tstart, g.tstop = capi.GRAVITY_UNIFORM, -BIG, BIG
        g.g[:] = [0.0, -1.0, 0.0]
        keep.append(g)
        a.gravity = C.pointer(g)
    elif task == "rf_omega rf_qshear":
        a.rf_omega, a.rf_qshear = 1.0, 1.5
    elif task in ("drag", "drag damping"):
        dr = capi.Drag()
        dr.type, dr.model, dr.scale, dr.grain_density = capi.DRAG_SIMPLE_DUST, capi.DRAG_CONSTANT, 1.0, 1.0
        for n in range(max(1, p.dust.nspecies)):
            dr.tau[n] = 0.05 * (n + 1)
        for f in (dr.gas, dr.dust):
            f.ix[:], f.ox[:], f.irate[:], f.orate[:] = [-BIG] * 3, [BIG] * 3, [0.0] * 3, [0.0] * 3
        if task == "drag damping":
            dr.dust.irate[0] = 1.0
        dr.xmin[:], dr.xmax[:] = [0.0] * 3, [1.0] * 3
        keep.append(dr)
        a.drag = C.pointer(dr)
    elif task in ("diffusion flux arrays", "diffusion sums"):
        df = capi.Diffusion()
        df.visc.type, df.visc.coeff, df.cv = capi.VISCOSITY_PLAW, 1e-3, 2.5
        keep.append(df)
        a.diffusion = C.pointer(df)
        if task == "diffusion sums":
            a.diffusion_sums = 8  # (any non-null address: it is not read)
    elif task == "cooling":
        c = capi.Cooling()
        c.cv = 2.5
        keep.append(c)
        a.cooling = C.pointer(c)
    elif task == "nbody_n=1":
        a.nbody_n = 1
    elif task == "strat_faces=15":
        a.strat_faces = 15
    return p, a, keep


def sweep(L, capi):
    """The table as one string, rows in the order of AXES.  Every switch is set alone and cleared again."""
    calls = [_call(capi, *row) for row in itertools.product(*(values for _, values in AXES[1:]))]
    out = []
    for sw in SWITCHES:
        if sw != "none":
            L.artemis_hip_set_option(sw.encode(), 1)
        try:
            for p, a, _ in calls:
                gas = L.artemis_hip_stage_general_variant(C.byref(p), C.byref(a))
                dust = L.artemis_hip_stage_general_dust_variant(C.byref(p), C.byref(a))
                out.append(ALPHABET[5 * gas + DUST_CODES.index(dust)])
        finally:
            if sw != "none":
                L.artemis_hip_set_option(sw.encode(), 0)
    return "".join(out)


def table(L, capi):
    return {"axes": [name for name, _ in AXES], **{name: values for name, values in AXES},
            "codes": "one character per row, rows in the order of `axes` (outermost first): "
                     "'%s'[5 * gas_code + %s.index(dust_code)]" % (ALPHABET, DUST_CODES),
            "answers": sweep(L, capi)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from artemis_amd import capi
    json.dump(table(capi.load(), capi), sys.stdout, indent=1)
    print()
