"""Every march gives the same bits however its launch is cut (csrc/options.hpp: "every path a switch selects gives the
same bits").  The launchers cut x3 into chunks of planes (the tile marches) or x2 into chunks of rows (the 2-D row march)
with a heuristic that, on one small block, always lands on its shortest legal piece; the workloads run 16 .. 128 planes a
chunk.  Here the tuning knobs force the cuts the heuristic never takes at test sizes -- chunks of one plane, of nghost
planes, a last chunk of a single plane, one chunk holding the whole column -- and every cut is held, bit for bit, against
the CPU oracle's task chain.

Every case
  * forms the oracle's result once and runs the kernel once per knob value,
  * writes into output buffers filled with NaN beforehand (a plane no chunk writes cannot pass),
  * asserts the cut that really ran (artemis_hip_last_launch_cut: a knob a launcher ignored or clamped would make the
    sweep vacuous) against numbers written out here, and the kernel that ran.

Shapes: (40, 17, 21) with two ghost zones and (40, 17, 24) with three -- two ragged 32-zone tiles in x1, three 8-zone
tiles in x2 (the last of one row), and x3 extents that leave remainders.  Legal knob ranges (read from the launchers and
kernels; values outside are clamped by the launcher): FUSED_KCHUNK >= 1 (no per-plane table; a chunk reads planes
k0 - 2 .. k1 + 2), CURV_KCHUNK 1 .. 64 (x3 tables in LDS), VISC_KCHUNK 1 .. nx3, PPM_KCHUNK 1 .. 64 (reads k0 - 3 .. k1 + 3),
STAGE2D_ROWS 1 .. nx2 (the exact pass already marches single rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from test_parity_cart_dust_march import source_pack
from test_parity_diffusion import VSRC, pair
from test_parity_flat_guards import _flat, _mild, _same_bits
from test_parity_fused import fused_step, setup
from test_parity_ops import face_slices, make_pair, push, random_state, same
from test_parity_ppm_march import make_oracle, make_pack
from test_parity_stage_general import CASES as GENERAL

pytestmark = pytest.mark.gpu

BIG = 1.7976931348623157e308
NAN = float("nan")
KEEP = [0, 1, 2, 3, 5]  # (the general stage does not write the pressure slot)
NX2, NX3 = (40, 17, 21), (40, 17, 24)
TILES = 2 * 3  # 32 x 8 tiles of a 40 x 17 plane

# (planes per chunk, chunks) by knob value -- the launchers' arithmetic worked out by hand:
# kernels_fused.hip: n = max(1, planes / knob); chunk = ceil(planes / n); chunks = ceil(planes / chunk)
FUSED_CUT = {21: {1: (1, 21), 2: (3, 7), 4: (5, 5), 7: (7, 3), 16: (21, 1)},  # 21 x 1, 7 x 3, 5+5+5+5+1, 3 x 7, one chunk
             24: {2: (2, 12)}}                                                 # 12 chunks of nghost planes
# kernels_curv.hip / the viscous source / kernels_ppm.hip: n = ceil(planes / knob); chunk = ceil(planes / n); ...
MARCH_CUT = {1: (1, 21), 2: (2, 11), 3: (3, 7), 4: (4, 6), 5: (5, 5), 64: (21, 1)}  # 10 x 2 + 1, 5 x 4 + 1, 4 x 5 + 1


def interior(o):
    return (slice(None), slice(o.ks, o.ke + 1), slice(o.js, o.je + 1), slice(o.is_, o.ie + 1))


def cut_of(launcher):
    from artemis_amd import capi
    c = capi.last_launch_cut()
    assert c.launcher == launcher, (c.launcher, launcher)
    return c


def dt_word():
    return torch.full((1,), BIG, dtype=torch.float64, device="cuda")


# The per-XCD id remap of the headline kernel splits the bulk ids as 8 q + rem: the sweeps below launch bulk counts below 8
# (q = 0), multiples of 8 (rem = 0) and counts with a remainder (checked where the table is read, with or without a GPU;
# the sweeps assert the counts that really ran)
BULK_COUNTS = sorted({TILES * n for cuts in FUSED_CUT.values() for _, n in cuts.values()})
assert BULK_COUNTS == [6, 18, 30, 42, 72, 126]
assert any(c < 8 for c in BULK_COUNTS) and any(c % 8 == 0 for c in BULK_COUNTS) and any(c > 8 and c % 8 for c in BULK_COUNTS)


# ---- a: the headline stage, artemis_hip_stage_fused -------------------------------------------------------------------
def oracle_fused_stage(o, g0, g1, be, dt):
    """One stage of the reference's task chain on the oracle's state, then what the fused launch also leaves: the
    conserved state of the new primitives and their timestep limit."""
    o.CalculateFluxes(0, False)
    o.ApplyUpdate(g0, g1, be * dt)
    o.FluxSource(be * dt, 0)
    o.SetAuxillaryFields()
    o.ConsToPrim()
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    return o.new_dt()


def fused_reference(nx, ng, recon, riem, stage2):
    """(oracle after the stage, pack, buffers, the stage's arguments, the oracle's new dt)"""
    bc = ("outflow",) * 6
    o, mb, bufs = setup(nx, ng, recon, riem, bc, seed=11)
    A, B, U = bufs
    o.DeepCopyConservedData()
    u1 = A
    if stage2:  # rk2 stage-2 weights with a start-of-step state of its own
        o2, _, _ = setup(nx, ng, recon, riem, bc, seed=77)
        o.gu1[:] = o2.gu0
        U[0][0].copy_(torch.from_numpy(o2.gprim.copy()))
        u1 = U
    g0, g1, be = (0.5, 0.5, 0.5) if stage2 else (0.0, 1.0, 1.0)
    dt = o.new_dt()
    want_dt = oracle_fused_stage(o, g0, g1, be, dt)
    return o, mb, (A, u1, B), (g0, g1, be * dt, be * dt), want_dt


@pytest.mark.parametrize("nx,ng,knobs", [(NX2, 2, (1, 2, 4, 7, 16)), (NX3, 3, (2,))])
@pytest.mark.parametrize("riem,recon", [("hllc", "plm"), ("hlle", "plm"), ("llf", "pcm")])
@pytest.mark.parametrize("stage2", [False, True])
def test_headline_stage_at_every_cut(hiplib, nx, ng, knobs, riem, recon, stage2):
    """New primitives, the conserved output and the atomic-min timestep of one launch, per FUSED_KCHUNK and with the
    per-XCD id remap on and off."""
    from artemis_amd import capi
    o, mb, (A, u1, B), w, want_dt = fused_reference(nx, ng, recon, riem, stage2)
    I = interior(o)
    for knob in knobs:
        chunk, nchunk = FUSED_CUT[nx[2]][knob]
        for no_swizzle in (0, 1):
            with capi.option("fused_kchunk", knob), capi.option("fused_no_swizzle", no_swizzle):
                B[0].fill_(NAN), mb.gas_u0.fill_(NAN)
                dtd = dt_word()
                mb.stage_fused(*w, A[1], u1[1], B[1], cons_out=mb.pack.gas.cons0, cfl=0.3, dt_dev=C.c_void_p(dtd.data_ptr()))
                c = cut_of(capi.CUT_STAGE_FUSED)
            what = "kchunk %d, no_swizzle %d" % (knob, no_swizzle)
            print(what, "-> chunk", c.chunk, "chunks", c.nchunk, "workgroups", c.workgroups, "shell", c.shell_workgroups)
            assert (c.chunk, c.nchunk, c.workgroups, c.shell_workgroups) == (chunk, nchunk, TILES * nchunk, 0), what
            same(B[0][0][I], o.gprim[I], "prim, " + what)
            same(mb.gas_u0[0][I], o.gu0[I], "cons_out, " + what)
            assert dtd.item() == want_dt, what


def scaled_velocities(o, seed, choices, prob):
    rng = np.random.default_rng(seed)
    scale = rng.choice(choices, size=o.gprim[1].shape, p=prob)
    for v in (1, 2, 3):
        o.gprim[v] *= scale
    o.ApplyBoundaryConditions()
    o.PrimToCons()


def rk2_step_at_cuts(o, mb, bufs, bc, knobs, check):
    """The oracle's rk2 step once; the fused step once per knob from the same start, intermediate buffers NaN-filled."""
    from artemis_amd import capi
    start = torch.from_numpy(o.gprim.copy())
    dt = o.new_dt()
    o.dt = dt
    o.step()
    for knob in knobs:
        mb.gas_prim[0].copy_(start)
        bufs[1][0].fill_(NAN), bufs[2][0].fill_(NAN), mb.gas_u0.fill_(NAN)
        capi.redo_totals(reset=True)
        with capi.option("fused_kchunk", knob):
            fused_step(mb, bufs, "rk2", dt, [bc])
            c = cut_of(capi.CUT_STAGE_FUSED)
        assert (c.chunk, c.nchunk) == FUSED_CUT[21][knob], knob
        mb.PrimToCons()  # materialise P in the ghosts and the conserved state for comparison
        check(knob, capi.redo_totals())


@pytest.mark.parametrize("riem", ["hllc", "llf"])
def test_redo_list_at_short_chunks(hiplib, riem):
    """The state of test_fused_step_with_vanishing_velocities (velocities of 1e-300 .. 1e-40 next to zeros): chunks
    recompute their priming planes, and the zones they defer to the exact pass must come out right whichever chunk lists
    them -- chunks of one plane and 5+5+5+5+1."""
    bc = ("outflow",) * 6
    o, mb, bufs = setup(NX2, 2, "plm", riem, bc, seed=13)
    scaled_velocities(o, 3, [1.0, 0.0, 1e-300, 1e-306, 1e-250, 1e-160, 1e-150, 1e-100, 1e-40],
                      [0.3, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.08, 0.08])

    def check(knob, redone):
        assert redone[0] > 0, "the exact pass recomputed nothing: the state does not reach the redo list"
        same(mb.gas_prim[0], o.gprim, "prim, kchunk %d" % knob)
        same(mb.gas_u0[0], o.gu0, "cons, kchunk %d" % knob)
    rk2_step_at_cuts(o, mb, bufs, bc, (1, 4), check)


@pytest.mark.parametrize("past", [0, 1])
def test_flat_slab_ending_on_a_seam(hiplib, past):
    """Gas at rest, bitwise uniform, in the x3 planes below interior plane 10 (+ past), random gas above: with chunks of
    five planes the slab ends exactly on the seam between the second and the third chunk (past = 0) or one plane beyond
    it -- the flat-wave guards of a chunk's priming slope and of its first and last trips decide on either side of it;
    with chunks of one plane every trip is a priming trip.  Bits, a zero's sign included."""
    bc = ("outflow",) * 6
    o, mb, bufs = setup(NX2, 2, "plm", "hllc", bc, seed=17)
    _mild(o.gprim, np.random.default_rng(31))
    m = np.zeros(o.gprim[0].shape, bool)
    m[:o.ks + 10 + past] = True
    _flat(o.gprim, m)
    o.ApplyBoundaryConditions()
    o.PrimToCons()

    def check(knob, _):
        same(mb.gas_prim[0], o.gprim, "prim, kchunk %d" % knob)
        _same_bits(mb.gas_prim[0], o.gprim, "prim, kchunk %d" % knob)
        _same_bits(mb.gas_u0[0], o.gu0, "cons, kchunk %d" % knob)
    rk2_step_at_cuts(o, mb, bufs, bc, (1, 4), check)


# faces -> {knob: [(chunk, chunks, workgroups) of the region-1 launch, ... of the region-2 launch]}: zt = nghost = 2
# x3 (48): shell = two boxes of 2 planes on all six tiles, bulk = 17 planes on six tiles
# x2 (12): shell = the two outer tile rows (2 x 2 tiles) over 21 planes, bulk = the middle row (2 tiles) over 21 planes
# x2 + x3 (60): shell = the x3 boxes, then the outer tile rows over the 17 middle planes; bulk = 2 tiles x 17 planes
REGION_CUT = {
    48: {1: [(1, 2, 24), (1, 17, 102)], 4: [(2, 1, 12), (5, 4, 24)], 16: [(2, 1, 12), (17, 1, 6)]},
    12: {1: [(1, 21, 84), (1, 21, 42)], 4: [(5, 5, 20), (5, 5, 10)], 16: [(21, 1, 4), (21, 1, 2)]},
    60: {1: [(1, 17, 24 + 68), (1, 17, 34)], 4: [(5, 4, 12 + 16), (5, 4, 8)], 16: [(17, 1, 12 + 4), (17, 1, 2)]},
}


@pytest.mark.parametrize("knob", [1, 4, 16])
def test_shell_then_bulk_at_every_cut(hiplib, knob):
    """region 1 (boundary shell) + region 2 (bulk) == region 0 == the oracle, per FUSED_KCHUNK: the knob cuts the shell
    boxes and the bulk box separately.  (Two tiles in x1 cannot lose both to a shell: the x1 faces stay out of the masks.)"""
    from artemis_amd import capi
    o, mb, (A, u1, B), w, _ = fused_reference(NX2, 2, "plm", "hllc", True)
    I = interior(o)
    Cc = mb.new_prim_buffer("shell+bulk")
    with capi.option("fused_kchunk", knob):
        B[0].fill_(NAN)
        mb.stage_fused(*w, A[1], u1[1], B[1], region=0)
        same(B[0][0][I], o.gprim[I], "region 0")
        for faces, cuts in REGION_CUT.items():
            Cc[0].fill_(NAN)
            for region in (1, 2):
                mb.stage_fused(*w, A[1], u1[1], Cc[1], region=region, shell_faces=faces)
                c = cut_of(capi.CUT_STAGE_FUSED)
                print("faces", bin(faces), "region", region, "-> chunk", c.chunk, "chunks", c.nchunk, "workgroups", c.workgroups)
                assert (c.chunk, c.nchunk, c.workgroups) == cuts[knob][region - 1], (bin(faces), region)
            torch.cuda.synchronize()
            assert torch.equal(B[0][0][I], Cc[0][0][I]), bin(faces)


# knob -> (x3 shell thickness zt = max(nghost, min(knob, nx3 / 3)), (chunk, chunks) of the bulk box, workgroups, of them shell)
SHELL_FIRST_CUT = {1: (2, (1, 17), 24 + 102, 24), 4: (4, (5, 3), 12 + 18, 12), 16: (7, (7, 1), 12 + 6, 12)}


@pytest.mark.parametrize("knob", [1, 4, 16])
def test_shell_first_launch_at_every_cut(hiplib, knob):
    """The one-launch shell-first order (artemis_stage_args_t.shell_done): there the knob also sets the thickness of the
    x3 shell.  The launch equals the oracle, its shell workgroups all count themselves in, and the target it reports is
    their number."""
    from artemis_amd import capi
    o, mb, (A, u1, B), w, _ = fused_reference(NX2, 2, "plm", "hllc", True)
    I = interior(o)
    zt, bulk, wgs, shell = SHELL_FIRST_CUT[knob]
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    target = C.c_uint(0)
    a = capi.StageArgs()
    a.gam0, a.gam1, a.beta_dt, a.bdt = w
    a.prim_in, a.prim_u1, a.prim_out = A[1], u1[1], B[1]
    a.shell_done, a.shell_target, a.shell_faces = done.data_ptr(), C.pointer(target), 48
    B[0].fill_(NAN)
    with capi.option("fused_kchunk", knob):
        mb._call(mb.L.artemis_hip_stage_fused, C.byref(a))
        c = cut_of(capi.CUT_STAGE_FUSED)
        mb._call(mb.L.artemis_hip_stage_fused_redo_shell, C.byref(a))  # (the shell's list: the waiting stream's duty)
    torch.cuda.synchronize()
    print("kchunk", knob, "-> zt", zt, "chunk", c.chunk, "chunks", c.nchunk, "workgroups", c.workgroups, "shell", c.shell_workgroups)
    assert (c.chunk, c.nchunk) == bulk and (c.workgroups, c.shell_workgroups) == (wgs, shell)
    assert target.value == shell and int(done.item()) == shell
    same(B[0][0][I], o.gprim[I], "shell-first launch")


# ---- b: Gas::CalculateFluxes through the tile march -------------------------------------------------------------------
@pytest.mark.parametrize("nx,ng", [(NX2, 2), (NX3, 3)])
@pytest.mark.parametrize("riem,recon", [("hllc", "plm"), ("hlle", "plm"), ("llf", "pcm")])
def test_flux_task_at_every_cut(hiplib, nx, ng, riem, recon):
    """The same knob values as the headline stage: 1, 2, 4, 7, 16 on 21 planes, 2 on 24 planes (12 chunks of nghost)."""
    from artemis_amd import capi
    (o,), mb = make_pair(nx, ng=ng, recon=recon, riem=riem, seed=21)
    o.CalculateFluxes(0, False)
    for knob, (chunk, nchunk) in FUSED_CUT[nx[2]].items():
        for d in range(3):
            mb.gas_flux[d].fill_(NAN), mb.gas_pflux[d].fill_(NAN), mb.gas_vface[d].fill_(NAN)
        with capi.option("fused_kchunk", knob):
            mb.CalculateFluxes(0, False)
            c = cut_of(capi.CUT_FLUX_FUSED)
        assert (c.chunk, c.nchunk, c.workgroups) == (chunk, nchunk, TILES * nchunk), ("cut", knob, c.chunk, c.nchunk, c.workgroups)
        for d in range(3):
            sl = face_slices(o, d)
            same(mb.gas_flux[d][0][sl], o.gflux(d)[sl], "flux x%d, kchunk %d" % (d + 1, knob))
            same(mb.gas_pflux[d][0][sl], o.gpflux(d)[sl], "pflux x%d, kchunk %d" % (d + 1, knob))
            same(mb.gas_vface[d][0][sl], o.gvface(d)[sl], "vface x%d, kchunk %d" % (d + 1, knob))


# ---- c, d: the general stage's tile marches -----------------------------------------------------------------------------
def general_pair(nx, lo, hi, recon, riem, coords, ng, seed, omega_frame=0.0, shock=True):
    from artemis_amd.pack import MeshBlockPack
    kw = dict(ng=ng, ns_gas=1, ns_dust=0, reconstruct=recon, riemann=riem, dust_reconstruct=recon, dust_riemann="hlle",
              gamma=1.4, dfloor=1e-10, siefloor=1e-10, dust_dfloor=1e-10, coordinates=coords)
    o = Oracle(nx, lo, hi, bc=("outflow",) * 6, cfl=0.3, dust_cfl=0.3, **kw)
    if shock:
        random_state(o, np.random.default_rng(seed), shock=True)
    else:
        random_state(o, np.random.default_rng(seed), shock=False, mach=0.5, contrast=10.0)
    mb = MeshBlockPack(1, nx, [lo], [hi], with_fluxes=False, omega_frame=omega_frame, **kw)
    push([o], mb)
    return o, mb


def gas_stage_reference(o, mb, nx, lo, hi, recon, riem, coords, ng, stage2, sources=None):
    """The oracle's stage (hydro, or with point-mass gravity and the rotating frame); returns the stage's keyword
    arguments for mb.stage_general and the timestep limit of the new state."""
    from artemis_amd.pack import gravity_point
    o.DeepCopyConservedData()
    gin = gu1 = mb.gas_prim_table
    if stage2:
        o2, mb2 = general_pair(nx, lo, hi, recon, riem, coords, ng, 77, shock=sources is None)
        o.gu1[:] = o2.gu0
        t, gu1 = mb.new_prim_buffer("u1")
        t.copy_(mb2.gas_prim)
    g0, g1, be = (0.5, 0.5, 0.5) if stage2 else (0.0, 1.0, 1.0)
    dt, time = 1.0e-4, 0.25
    kw = {}
    if sources:  # (ahead of the fluxes: the frame velocity enters FluxSource's coordinate sources)
        om, pos = sources
        o.set_gravity_point(1.3, soft=0.05, x=pos[0], y=pos[1], z=pos[2])
        o.set_rotating_frame(om, 0.0)
        kw = dict(time=time, gravity=gravity_point(1.3, soft=0.05, pos=pos), rotating_frame=(om, 0.0))
    o.CalculateFluxes(0, False)
    o.ApplyUpdate(g0, g1, be * dt)
    o.FluxSource(be * dt, 0)
    if sources:
        o.ExternalGravity(time, be * dt)
        o.RotatingFrameForce(be * dt)
    o.SetAuxillaryFields()
    o.ConsToPrim()
    return (g0, g1, be * dt, be * dt), (gin, gu1), kw, o.EstimateTimestepMesh(0)


def sweep_gas_march(o, mb, w, tables, kw, want_dt, option_name, knobs, launcher, variant, tiles):
    from artemis_amd import capi
    I = interior(o)
    gbuf, gout = mb.new_prim_buffer("o")
    for knob in knobs:
        chunk, nchunk = FUSED_CUT[21][knob] if option_name == "fused_kchunk" else MARCH_CUT[knob]
        gbuf.fill_(NAN)
        dtd = dt_word()
        with capi.option(option_name, knob):
            mb.stage_general(*w, gas=(tables[0], tables[1], gout), cfl=(0.3, 0.3), dt_dev=dtd.data_ptr(), **kw)
            c = cut_of(launcher)
        assert mb.last_stage_variant == variant
        assert (c.chunk, c.nchunk, c.workgroups) == (chunk, nchunk, tiles * nchunk), ("cut", (option_name, knob), c.chunk, c.nchunk, c.workgroups)
        assert np.array_equal(gbuf[0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP]), (option_name, knob)
        assert dtd.item() == want_dt, (option_name, knob)


@pytest.mark.parametrize("case,tiles", [(15, 2 * 3), (16, 2 * 2)])
@pytest.mark.parametrize("stage2", [False, True])
def test_curvilinear_instantiation_of_the_headline_kernel_at_every_cut(hiplib, option, case, tiles, stage2):
    """NO_CURV_MARCH sends one gas species on a curvilinear block to launch_stage_fused_curv (variant 2), which reads the
    raw FUSED_KCHUNK: spherical (40, 19, 21) and cylindrical (35, 10, 21)."""
    from artemis_amd import capi
    nx, lo, hi, _, _, recon, riem, _, coords, ng = GENERAL[case]
    nx = (nx[0], nx[1], 21)
    option("no_curv_march", 1)
    o, mb = general_pair(nx, lo, hi, recon, riem, coords, ng, 31)
    w, tables, kw, want_dt = gas_stage_reference(o, mb, nx, lo, hi, recon, riem, coords, ng, stage2)
    sweep_gas_march(o, mb, w, tables, kw, want_dt, "fused_kchunk", (1, 4, 16), capi.CUT_STAGE_FUSED_CURV, 2, tiles)


CURV_KNOBS = (1, 2, 5, 64)  # 21 x 1, 10 x 2 + 1, 4 x 5 + 1, one chunk
SPH = ("spherical", (40, 19, 21), (0.9, 1.06, -3.1), (5.6, 2.08, 3.1))


@pytest.mark.parametrize("which", ["spherical", "spherical+sources", "cartesian"])
@pytest.mark.parametrize("stage2", [False, True])
def test_tile_march_gas_at_every_cut(hiplib, which, stage2):
    """stage_curv_kernel, gas alone: a spherical block (PLM_G: the x3 weight tables in LDS are filled per chunk), the same
    with point-mass gravity off the axis and the rotating frame, and the Cartesian instantiation."""
    from artemis_amd import capi
    if which == "cartesian":
        coords, nx, lo, hi, riem = "cartesian", NX2, (-1, -0.5, 0.25), (1, 0.8, 0.95), "hlle"
    else:
        (coords, nx, lo, hi), riem = SPH, "hllc"
    src = (0.8, (0.1, 0.05, 0.0)) if which.endswith("sources") else None
    o, mb = general_pair(nx, lo, hi, "plm", riem, coords, 2, 31, omega_frame=src[0] if src else 0.0, shock=src is None)
    w, tables, kw, want_dt = gas_stage_reference(o, mb, nx, lo, hi, "plm", riem, coords, 2, stage2, sources=src)
    sweep_gas_march(o, mb, w, tables, kw, want_dt, "curv_kchunk", CURV_KNOBS, capi.CUT_STAGE_CURV, 3, TILES)


def test_tile_march_dust_with_the_drag_finish_at_every_cut(hiplib):
    """Gas + one dust species on a Cartesian block with point-mass gravity, the shearing box and simple_dust drag: the dust
    march finishes both fluids (dust variant 5) and reduces both timestep limits."""
    from artemis_amd import capi
    from artemis_amd.pack import drag_params, gravity_point
    from test_parity_cart_dust_march import HI3, LO3, TAU
    nx = (40, 19, 21)
    mb, ref = source_pack(nx, 1)
    # (source_stage of test_parity_cart_dust_march.py with output buffers of this test's own, NaN-filled before every launch)
    grav = gravity_point(0.7, soft=0.1, pos=(0.1, 0.05, 0.0))
    drag = drag_params("simple_dust", "constant", tau=TAU[:1], mesh_min=LO3, mesh_max=HI3)
    dt = 2.0e-4
    gbuf, gout = mb.new_prim_buffer("o")
    dbuf, dout = mb.new_dust_prim_buffer("o")
    for knob in CURV_KNOBS:
        chunk, nchunk = MARCH_CUT[knob]
        gbuf.fill_(NAN), dbuf.fill_(NAN)
        dtd = dt_word()
        with capi.option("curv_kchunk", knob):
            mb.stage_general(0.0, 1.0, dt, dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout),
                             dust=(mb.dust_prim_table, mb.dust_prim_table, dout), time=0.25, gravity=grav,
                             rotating_frame=(1.2, 1.5), drag=drag, cfl=(0.3, 0.4), dt_dev=dtd.data_ptr())
            c = cut_of(capi.CUT_STAGE_CURV)
        assert mb.last_stage_variant == 3 and mb.last_dust_stage_variant == 5
        assert (c.chunk, c.nchunk, c.workgroups) == (chunk, nchunk, TILES * nchunk), ("cut", knob, c.chunk, c.nchunk, c.workgroups)
        assert np.array_equal(gbuf[0][ref["I"]].cpu().numpy()[KEEP], ref["g"]), knob
        same(dbuf[0][ref["I"]], ref["d"], "dust prim, kchunk %d" % knob)
        assert dtd.item() == ref["dt"], knob


# ---- e: the viscous source march ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coordinates,nx,lo,hi", VSRC)
def test_viscous_source_at_every_cut(hiplib, coordinates, nx, lo, hi):
    from artemis_amd import capi
    from artemis_amd.pack import diffusion_params
    nx = (nx[0], nx[1], 21)
    o, mb = pair(nx, ns_gas=1, seed=63, coordinates=coordinates, lo=lo, hi=hi)
    visc = dict(type="alpha", alpha=2e-2, eta_bulk=0.3, r0=0.9, Omega0=1.2, averaging="arithmetic")
    o.set_viscosity("alpha", alpha=2e-2, eta_bulk=0.3, r0=0.9, Omega0=1.2, averaging="arithmetic")
    D = diffusion_params(1.4, viscosity=visc)
    mb.viscosity_radial_table(D)
    assert mb.viscous_source_covers()
    dt = 2.0e-4
    o.ZeroDiffusionFlux(), o.ViscousFlux()
    before = o.gu0.copy()
    o.DiffusionUpdate(dt)
    I = (slice(o.ks, o.ke + 1), slice(o.js, o.je + 1), slice(o.is_, o.ie + 1))
    mb.distance_table(D)
    narrow = nx[0] % 32 != 0 and (nx[0] % 16 == 0 or nx[0] < 32)
    vtx = 16 if narrow else 32
    tiles = -(-nx[0] // vtx) * -(-nx[1] // (256 // vtx))
    sums, _ = mb.viscous_source(D, dt)  # (allocates the sums)
    for knob in (1, 2, 5, 64):  # 64: clamped to the column, one chunk
        chunk, nchunk = MARCH_CUT[knob]
        sums.fill_(NAN)
        with capi.option("visc_kchunk", knob):
            mb.viscous_source(D, dt)
            c = cut_of(capi.CUT_VISCOUS_SOURCE)
        assert (c.chunk, c.nchunk, c.workgroups) == (chunk, nchunk, tiles * nchunk), ("cut", knob, c.chunk, c.nchunk, c.workgroups)
        got = sums[0].cpu().numpy()
        for q in range(5):
            assert np.array_equal(before[1 + q][I] - got[q][I], o.gu0[1 + q][I]), (knob, q)


# ---- f: the PPM march ---------------------------------------------------------------------------------------------------
PPM_KNOBS = (1, 3, 4, 64)


@pytest.mark.parametrize("ng", [3, 4])
@pytest.mark.parametrize("stage2", [False, True])
def test_ppm_march_at_every_cut(hiplib, ng, stage2):
    """PPM_KCHUNK 1, 3 (= nghost at ng = 3), 4 (5 x 4 + 1) and 64 (one chunk)."""
    from artemis_amd import capi
    from test_parity_stage_general import oracle_stage
    o = make_oracle(NX2, ng, "hllc", ("outflow",) * 6, 11)
    mb = make_pack([o], NX2, ng, "hllc")
    gin = gu1 = mb.gas_prim_table
    o.DeepCopyConservedData()
    if stage2:
        o2 = make_oracle(NX2, ng, "hllc", ("outflow",) * 6, 77)
        o.gu1[:] = o2.gu0
        u1_t, gu1 = mb.new_prim_buffer("u1")
        u1_t[0].copy_(torch.from_numpy(o2.gprim.copy()))
    g0, g1, be = (0.5, 0.5, 0.5) if stage2 else (0.0, 1.0, 1.0)
    dt = 1.0e-4
    oracle_stage(o, g0, g1, be, dt, False, 0.0, False, False, False)
    want = o.gprim[interior(o)][KEEP].copy()
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    want_dt = o.new_dt()
    gbuf, gout = mb.new_prim_buffer("o")
    for knob in PPM_KNOBS:
        chunk, nchunk = MARCH_CUT[knob]
        gbuf.fill_(NAN)
        dtd = dt_word()
        with capi.option("ppm_kchunk", knob):
            mb.stage_general(g0, g1, be * dt, be * dt, gas=(gin, gu1, gout), cfl=(0.3, 0.0), dt_dev=C.c_void_p(dtd.data_ptr()))
            c = cut_of(capi.CUT_STAGE_PPM)
        assert mb.last_stage_variant == 4
        assert (c.chunk, c.nchunk, c.workgroups) == (chunk, nchunk, TILES * nchunk), ("cut", knob, c.chunk, c.nchunk, c.workgroups)
        assert np.array_equal(gbuf[0][interior(o)].cpu().numpy()[KEEP], want), knob
        assert dtd.item() == want_dt, knob


# ---- g: the 2-D row march -----------------------------------------------------------------------------------------------
# STAGE2D_ROWS -> (rows, chunks): 37 rows: 37 x 1, 12 x 3 + 1, 36 + 1, one chunk, one chunk (clamped); 33 rows likewise
ROWS_CUT = {37: {1: (1, 37), 3: (3, 13), 36: (36, 2), 37: (37, 1), 64: (37, 1)},
            33: {1: (1, 33), 3: (3, 11), 36: (33, 1), 37: (33, 1), 64: (33, 1)}}
STRIPS = 3  # 60 owned columns a wave: 130 and 121 columns alike


def row_march_pair(case, seed):
    from artemis_amd.pack import MeshBlockPack
    nx, lo, hi, nsg, nsd, recon, riem, driem, coords, ng = GENERAL[case]
    kw = dict(ng=ng, ns_gas=nsg, ns_dust=nsd, reconstruct=recon, riemann=riem, dust_reconstruct=recon, dust_riemann=driem,
              gamma=1.4, dfloor=1e-10, siefloor=1e-10, dust_dfloor=1e-10, coordinates=coords)
    o = Oracle(nx, lo, hi, bc=("outflow",) * 6, cfl=0.3, dust_cfl=0.4, **kw)
    random_state(o, np.random.default_rng(seed), shock=True)
    mb = MeshBlockPack(1, nx, [lo], [hi], with_fluxes=False, **kw)
    push([o], mb)
    return o, mb, nx, nsd


def row_march_outputs(mb, nsd):
    gbuf, gout = mb.new_prim_buffer("o")
    dbuf, dout = mb.new_dust_prim_buffer("o") if nsd else (None, None)
    return gbuf, gout, dbuf, dout


@pytest.mark.parametrize("case", [6, 9])  # (130, 37, 1) gas alone; (121, 33, 1) with two dust species
@pytest.mark.parametrize("stage2", [False, True])
def test_row_march_at_every_cut(hiplib, case, stage2):
    from artemis_amd import capi
    from test_parity_stage_general import oracle_stage
    o, mb, nx, nsd = row_march_pair(case, 31)
    gin, din = mb.gas_prim_table, mb.dust_prim_table
    gu1, du1 = gin, din
    o.DeepCopyConservedData()
    if stage2:
        o2, mb2, _, _ = row_march_pair(case, 77)
        o.gu1[:] = o2.gu0
        t, gu1 = mb.new_prim_buffer("u1")
        t.copy_(mb2.gas_prim)
        if nsd:
            o.du1[:] = o2.du0
            t, du1 = mb.new_dust_prim_buffer("u1")
            t.copy_(mb2.dust_prim)
    g0, g1, be = (0.5, 0.5, 0.5) if stage2 else (0.0, 1.0, 1.0)
    dt = 1.0e-4
    oracle_stage(o, g0, g1, be, dt, False, 0.0, False, False, False)
    want_dt = min(o.EstimateTimestepMesh(0), o.EstimateTimestepMesh(1)) if nsd else o.EstimateTimestepMesh(0)
    I = interior(o)
    gbuf, gout, dbuf, dout = row_march_outputs(mb, nsd)
    for knob, (rows, nchunk) in ROWS_CUT[nx[1]].items():
        gbuf.fill_(NAN)
        if nsd:
            dbuf.fill_(NAN)
        dtd = dt_word()
        with capi.option("stage2d_rows", knob):
            mb.stage_general(g0, g1, be * dt, be * dt, gas=(gin, gu1, gout), dust=(din, du1, dout), cfl=(0.3, 0.4),
                             dt_dev=dtd.data_ptr())
            c = cut_of(capi.CUT_STAGE2D)
        assert mb.last_stage_variant == 1
        assert (c.chunk, c.nchunk, c.workgroups) == (rows, nchunk, (STRIPS * nchunk + 3) // 4), ("cut", knob, c.chunk, c.nchunk, c.workgroups)
        assert np.array_equal(gbuf[0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP]), ("gas", knob)
        if nsd:
            same(dbuf[0][I], o.dprim[I], "dust prim, rows %d" % knob)
        assert dtd.item() == want_dt, knob


@pytest.mark.parametrize("case", [6, 9])
def test_row_march_exact_pass_strides_over_its_list(hiplib, case):
    """The state of test_row_march_kernel_with_vanishing_velocities with STAGE2D_RGRID 1 and 2: the four or eight waves of
    the exact pass take several trips over the listed rows."""
    from artemis_amd import capi
    from test_parity_stage_general import oracle_stage
    o, mb, nx, nsd = row_march_pair(case, 33)
    rng = np.random.default_rng(9)
    choices, prob = [1.0, 0.0, 1e-300, 1e-306, 1e-250, 1e-160, 1e-150, 1e-100, 1e-40], [0.3, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.08, 0.08]
    for arr, ns in ((o.gprim, 1), (o.dprim if nsd else None, nsd)):
        if arr is None:
            continue
        scale = rng.choice(choices, size=arr[0].shape, p=prob)
        for v in range(ns, 4 * ns):
            arr[v] *= scale
    o.PrimToCons()
    push([o], mb)
    # The main launch lists (block, strip, row) at least where the row's own zones of the strip hold a gas velocity that is
    # not zero and below 2^-200 (kernels_stage2d.hip: tiny_vel3 over the wave's lanes of row j; the window's other rows and
    # the dust only add to the list).  Counted here from the state: far more rows than the 4 (RGRID 1) or 8 (RGRID 2)
    # waves of the exact pass, which therefore take several trips each.
    v = np.abs(o.gprim[1:4, o.ks, o.js:o.je + 1, o.is_:o.ie + 1])
    tiny = ((v > 0.0) & (v < 2.0 ** -200)).any(axis=0)  # [row, column]
    listed = sum(int(tiny[:, 60 * strip:60 * (strip + 1)].any(axis=1).sum()) for strip in range(STRIPS))
    print("rows listed at least:", listed, "of", STRIPS * nx[1])
    assert listed >= 4 * 8, listed
    gin, din = mb.gas_prim_table, mb.dust_prim_table
    o.DeepCopyConservedData()
    dt = 1.0e-4
    oracle_stage(o, 0.0, 1.0, 1.0, dt, False, 0.0, False, False, False)
    I = interior(o)
    gbuf, gout, dbuf, dout = row_march_outputs(mb, nsd)
    for rgrid in (1, 2):
        gbuf.fill_(NAN)
        if nsd:
            dbuf.fill_(NAN)
        with capi.option("stage2d_rgrid", rgrid):
            mb.stage_general(0.0, 1.0, dt, dt, gas=(gin, gin, gout), dust=(din, din, dout))
            c = cut_of(capi.CUT_STAGE2D)
        assert mb.last_stage_variant == 1 and c.redo_workgroups == rgrid
        got = gbuf[0][I].cpu().numpy()[KEEP]
        bad = got != o.gprim[I][KEEP]
        assert not bad.any(), "gas, rgrid %d: %d entries differ" % (rgrid, np.count_nonzero(bad))
        if nsd:
            same(dbuf[0][I], o.dprim[I], "dust prim, rgrid %d" % rgrid)
