"""GPU parity of the PPM tile march (kernels_ppm.hip, variant 4 of artemis_hip_stage_general): one gas species on
Cartesian 3-D blocks, PPM4, HLLC / HLLE / LLF -- against the CPU oracle with reconstruct="ppm", against the cell-centred
kernel it replaces (NO_PPM_MARCH), through the host driver, and what it does not cover.  BIT-EXACT everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from pins import LINWAVE, linwave_waves
from test_driver_gpu import DECK, linwave_overrides
from test_parity_fused import COEFF
from test_parity_ops import push, random_state, same
from test_parity_stage_general import oracle_stage

pytestmark = pytest.mark.gpu

LO, HI = (-1.0, -0.7, 0.1), (1.0, 0.9, 1.3)
KW = dict(gamma=1.4, dfloor=1e-10, siefloor=1e-10)
CASES = [
    ((40, 20, 36), 3, "hllc", "outflow"),
    ((40, 20, 36), 3, "hlle", "periodic"),
    ((40, 20, 36), 3, "llf", "reflecting"),
    ((33, 9, 17), 3, "hllc", "outflow"),    # ragged against the tile in every direction
    ((64, 16, 70), 4, "hllc", "periodic"),  # several chunks along x3
    ((8, 4, 4), 4, "hllc", "periodic"),     # a block smaller than its own halo (linwave.py's block size at N = 16)
]
KEEP = [0, 1, 2, 3, 5]  # the pressure slot of the output is not written (variant 0 does not write it either)


def make_oracle(nx, ng, riem, bc, seed, integ="rk2", lo=LO, hi=HI, recon="ppm"):
    o = Oracle(nx, lo, hi, cfl=0.3, bc=bc, integrator=integ, ng=ng, reconstruct=recon, riemann=riem, **KW)
    random_state(o, np.random.default_rng(seed), mach=1.0, contrast=30.0)
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    return o


def make_pack(oracles, nx, ng, riem, recon="ppm", **extra):
    from artemis_amd.pack import MeshBlockPack
    mb = MeshBlockPack(len(oracles), nx, [LO] * len(oracles), [HI] * len(oracles), with_fluxes=False, ng=ng,
                       reconstruct=recon, riemann=riem, **KW, **extra)
    push(oracles, mb)
    return mb


def interior(o):
    return np.s_[:, o.ks:o.ke + 1, o.js:o.je + 1, o.is_:o.ie + 1]


def apply_bc(mb, table, bc):
    from artemis_amd import capi
    flat = [capi.BCS[x] for x in bc]
    mb.call_on(mb.pack_with_prim(table), mb.L.artemis_hip_apply_bc, (C.c_int * len(flat))(*flat), None)


def one_stage(oracles, mb, stage2, seed_u1=77, **kw):
    """One call of the general stage on every block of the pack and the same stage on each block's oracle: RK stage-1
    weights with u1 = in, or RK2 stage-2 weights with a distinct u1; the device dt with cfl 0.3.  Returns the output
    tensor and the device dt."""
    gin = mb.gas_prim_table
    gout_t, gout = mb.new_prim_buffer("o")
    gu1 = gin
    for o in oracles:
        o.DeepCopyConservedData()
    if stage2:
        u1_t, gu1 = mb.new_prim_buffer("u1")
        for b, o in enumerate(oracles):
            o2 = make_oracle((o.cfg.nx1, o.cfg.nx2, o.cfg.nx3), o.cfg.ng, "hllc", ("outflow",) * 6, seed_u1 + b)
            o.gu1[:] = o2.gu0
            u1_t[b].copy_(torch.from_numpy(o2.gprim.copy()))
    g0, g1, be = (0.5, 0.5, 0.5) if stage2 else (0.0, 1.0, 1.0)
    dt = 1.0e-4
    for o in oracles:
        oracle_stage(o, g0, g1, be, dt, False, 0.0, False, False, False)
    dt_dev = torch.full((1,), torch.finfo(torch.float64).max, dtype=torch.float64, device="cuda")
    mb.stage_general(g0, g1, be * dt, be * dt, gas=(gin, gu1, gout), cfl=(0.3, 0.0),
                     dt_dev=C.c_void_p(dt_dev.data_ptr()), **kw)
    torch.cuda.synchronize()
    return gout_t, dt_dev.item()


# ---- 1 (a): one stage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ng,riem,bcname", CASES)
@pytest.mark.parametrize("stage2", [False, True])
def test_ppm_march_one_stage(hiplib, nx, ng, riem, bcname, stage2):
    """The march runs (variant 4; the parent commit reports 0 here) and one stage equals the oracle's task chain:
    interior primitives except P, and the timestep limit reduced on the device."""
    o = make_oracle(nx, ng, riem, (bcname,) * 6, 11)
    mb = make_pack([o], nx, ng, riem)
    out, dt_dev = one_stage([o], mb, stage2)
    assert mb.last_stage_variant == 4
    I = interior(o)
    assert np.array_equal(out[0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP]), "gas prim"
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    assert dt_dev == o.new_dt(), "EstimateTimestepMesh inside the march"


@pytest.mark.parametrize("stage2", [False, True])
def test_ppm_march_pack_of_blocks(hiplib, stage2):
    """Four (16, 8, 8) blocks in one pack, each with its own state: every block equals its own oracle, and the device dt
    is the smallest of the blocks' limits."""
    nx, ng = (16, 8, 8), 3
    oracles = [make_oracle(nx, ng, "hllc", ("outflow",) * 6, 11 + 7 * b) for b in range(4)]
    mb = make_pack(oracles, nx, ng, "hllc")
    out, dt_dev = one_stage(oracles, mb, stage2)
    assert mb.last_stage_variant == 4
    dts = []
    for b, o in enumerate(oracles):
        I = interior(o)
        assert np.array_equal(out[b][I].cpu().numpy()[KEEP], o.gprim[I][KEEP]), f"gas prim, block {b}"
        o.ApplyBoundaryConditions()
        o.PrimToCons()
        dts.append(o.new_dt())
    assert dt_dev == min(dts)


# ---- 1 (b): full steps -----------------------------------------------------------------------------------------------
def general_step(mb, bufs, integ, dt, bc, variants):
    """test_parity_fused.fused_step with artemis_hip_stage_general per stage: bufs[0] holds the start-of-step
    primitives (ghost zones filled) and receives the end-of-step primitives."""
    A, B, Cc = bufs
    cur = A
    stages = COEFF[integ]
    for s, (g0, g1, be) in enumerate(stages):
        out = A if s == len(stages) - 1 else (B if cur is not B else Cc)  # (may alias u1: cell-wise access only)
        mb.stage_general(g0, g1, be * dt, be * dt, gas=(cur[1], A[1], out[1]), pcm=(integ == "vl2" and s == 0))
        variants.append(mb.last_stage_variant)
        apply_bc(mb, out[1], bc)
        cur = out


@pytest.mark.parametrize("nx,ng,riem,bcname", CASES)
@pytest.mark.parametrize("integ", ["rk2", "rk3", "vl2"])
def test_ppm_march_steps_match_oracle(hiplib, nx, ng, riem, bcname, integ):
    """Three full steps driven stage by stage: primitives and conserved state equal the oracle's after every step;
    every PPM stage runs on the march, the PCM predictor stage of vl2 where it ran before (variant 3)."""
    bc = (bcname,) * 6
    o = make_oracle(nx, ng, riem, bc, 11, integ=integ)
    mb = make_pack([o], nx, ng, riem)
    expect = {"rk2": [4, 4], "rk3": [4, 4, 4], "vl2": [3, 4]}[integ]
    run_steps(o, mb, integ, 3, expect, bc)


def run_steps(o, mb, integ, nsteps, expect, bc):
    bufs = [(mb.gas_prim, mb.pack.gas.prim), mb.new_prim_buffer("B"), mb.new_prim_buffer("C")]
    for step in range(nsteps):
        dt = o.new_dt()
        o.dt = dt
        o.step()
        variants = []
        general_step(mb, bufs, integ, dt, bc, variants)
        assert variants == expect, variants
        mb.PrimToCons()
        for got, ref, what in ((mb.gas_prim[0].cpu().numpy(), o.gprim, "prim"), (mb.gas_u0[0].cpu().numpy(), o.gu0, "cons")):
            bad = got != ref
            assert not bad.any(), (f"{what}, step {step}: {np.count_nonzero(bad)} entries differ, the largest of magnitude "
                                   f"{np.abs(ref[bad]).max():.3e} (gpu {got[bad][0]:.17e} ref {ref[bad][0]:.17e})")


# ---- 2: vanishing velocities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
def test_ppm_march_with_vanishing_velocities(hiplib, riem):
    """Velocities scaled zone by zone by 1, 0, 1e-300 .. 1e-40 (test_parity_fused's construction): momenta and PPM's
    numerators (sums of velocities) leave the window in which the shared-reciprocal divisions give the bits of `/`; the
    march takes the IEEE forms where that can matter (kernels_ppm.hip).  Two RK2 steps, every bit equal.
    Observed once during development: a build with all of the kernel's tiny-value guards compiled out fails this test
    for every solver (36 entries of the primitives differ after the first step); a build with only the reconstruction's
    per-plane / x3 guards compiled out still passes it -- in PPM4 a numerator small enough to leave the window belongs
    to a stencil whose limiter product qc * qd underflows to zero, which flattens the zone whatever the quotient's last
    bit was.  The guards the test exercises are therefore the update's (momenta over volume and over density)."""
    nx, ng, bc = (40, 20, 36), 3, ("outflow",) * 6
    o = Oracle(nx, LO, HI, cfl=0.3, bc=bc, integrator="rk2", ng=ng, reconstruct="ppm", riemann=riem, **KW)
    random_state(o, np.random.default_rng(13), mach=1.0, contrast=30.0)
    rng = np.random.default_rng(3)
    w = o.gprim
    scale = rng.choice([1.0, 0.0, 1e-300, 1e-306, 1e-250, 1e-160, 1e-150, 1e-100, 1e-40], size=w[1].shape,
                       p=[0.3, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.08, 0.08])
    for v in (1, 2, 3):
        w[v] *= scale
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    mb = make_pack([o], nx, ng, riem)
    run_steps(o, mb, "rk2", 2, [4, 4], bc)


@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
def test_ppm_march_with_subnormal_velocities(hiplib, riem):
    """The same construction one step further down: velocities scaled by 1, 0, 1e-300, 1e-310, 1e-315, 3e-320, so that
    momenta, face values and PPM's numerators are subnormal numbers in a good part of the block.  Two RK2 steps, every
    bit equal."""
    nx, ng, bc = (40, 20, 36), 3, ("outflow",) * 6
    o = Oracle(nx, LO, HI, cfl=0.3, bc=bc, integrator="rk2", ng=ng, reconstruct="ppm", riemann=riem, **KW)
    random_state(o, np.random.default_rng(13), mach=1.0, contrast=30.0)
    rng = np.random.default_rng(3)
    w = o.gprim
    scale = rng.choice([1.0, 0.0, 1e-300, 1e-310, 1e-315, 3e-320], size=w[1].shape, p=[0.3, 0.1, 0.15, 0.15, 0.15, 0.15])
    for v in (1, 2, 3):
        w[v] *= scale
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    mb = make_pack([o], nx, ng, riem)
    run_steps(o, mb, "rk2", 2, [4, 4], bc)


# ---- 3: path against path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ng,riem,bcname", [CASES[0], CASES[3], CASES[5]])
def test_ppm_march_equals_cell_kernel(hiplib, nx, ng, riem, bcname):
    """NO_PPM_MARCH sends the same call back to the cell-centred kernel (variant 0): the same bits in every zone of the
    output, ghost zones and the pressure slot (which neither path writes) included."""
    outs, dts, variants = [], [], []
    L = hiplib
    before = L.artemis_hip_get_option(b"NO_PPM_MARCH")
    try:
        for off in (0, 1):
            L.artemis_hip_set_option(b"NO_PPM_MARCH", off)
            oo = make_oracle(nx, ng, riem, (bcname,) * 6, 11)
            mb = make_pack([oo], nx, ng, riem)
            out, dt_dev = one_stage([oo], mb, True)
            variants.append(mb.last_stage_variant)
            outs.append(out.cpu().numpy().copy())
            dts.append(dt_dev)
    finally:
        L.artemis_hip_set_option(b"NO_PPM_MARCH", before)
    assert variants == [4, 0]
    assert np.array_equal(outs[0], outs[1]) and dts[0] == dts[1]


# ---- 4: what is not covered stays where it was -------------------------------------------------------------------------
def test_ppm_march_does_not_take_what_it_does_not_cover(hiplib):
    from artemis_amd.pack import MeshBlockPack
    from test_parity_stage_general import build
    dt = 1.0e-4
    # PPM with a dust species beside the gas: the cell-centred kernels, results as before (equal to the oracle)
    o, mb = build((20, 8, 6), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 1, "ppm", "hllc", "hlle", "cartesian", 3, seed=31)
    _, gout = mb.new_prim_buffer("o")
    dbuf, dout = mb.new_dust_prim_buffer("o")
    o.DeepCopyConservedData()
    oracle_stage(o, 0.0, 1.0, 1.0, dt, False, 0.0, False, False, False)
    mb.stage_general(0.0, 1.0, dt, dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout), dust=(mb.dust_prim_table, mb.dust_prim_table, dout))
    assert mb.last_stage_variant == 0
    I = interior(o)
    assert np.array_equal(mb._extra_prim["o"][0][0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP])
    same(dbuf[0][I], o.dprim[I], "dust prim")
    # the PCM predictor stage (pcm = 1) of a PPM pack: the Cartesian instantiation of the curvilinear march, as before
    o = make_oracle((40, 20, 36), 3, "hllc", ("outflow",) * 6, 11)
    mb = make_pack([o], (40, 20, 36), 3, "hllc")
    _, gout = mb.new_prim_buffer("o")
    o.DeepCopyConservedData()
    oracle_stage(o, 0.0, 1.0, 0.5, dt, True, 0.0, False, False, False)
    mb.stage_general(0.0, 1.0, 0.5 * dt, 0.5 * dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout), pcm=True)
    assert mb.last_stage_variant == 3
    I = interior(o)
    assert np.array_equal(mb._extra_prim["o"][0][0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP])
    # defer_finish = 1 (a refined mesh's fix-up follows): the cell-centred kernel, conserved state in cons0
    mb.stage_general(0.0, 1.0, dt, dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout), defer_finish=1)
    assert mb.last_stage_variant == 0
    # defer_finish outside 0 .. 2: refused
    with pytest.raises(Exception, match="defer_finish"):
        mb.stage_general(0.0, 1.0, dt, dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout), defer_finish=3)
    # a 2-D block and a cylindrical block with PPM: as before
    for nx, lo, hi, coords, want in (((61, 40, 1), (-1, -0.5, -0.5), (1, 0.8, 0.5), "cartesian", 0),
                                     ((16, 8, 6), (0.5, 0.0, -1.0), (2.0, 6.0, 1.0), "cylindrical", 0)):
        o, mb = build(nx, lo, hi, 1, 0, "ppm", "hlle", "hlle", coords, 3, seed=31)
        _, gout = mb.new_prim_buffer("o")
        o.DeepCopyConservedData()
        oracle_stage(o, 0.0, 1.0, 1.0, dt, False, 0.0, False, False, False)
        mb.stage_general(0.0, 1.0, dt, dt, gas=(mb.gas_prim_table, mb.gas_prim_table, gout))
        assert mb.last_stage_variant == want, (coords, nx)
        I = interior(o)
        assert np.array_equal(mb._extra_prim["o"][0][0][I].cpu().numpy()[KEEP], o.gprim[I][KEEP]), (coords, nx)


# ---- 5: the host driver ----------------------------------------------------------------------------------------------
def gather(sim, name, N):
    """The mesh's interior zones of a field from every block of a uniform mesh (blocks placed by their bounds)."""
    nx = (N, N // 2, N // 2)
    dx = (3.0 / nx[0], 1.5 / nx[1], 1.5 / nx[2])
    out = None
    for b in range(sim.nblocks):
        f = sim.interior(sim.field(name, b))
        if out is None:
            out = np.empty((f.shape[0], nx[2], nx[1], nx[0]))
        x = sim.block_bounds(b)
        i0, j0, k0 = (int(round(x[0] / dx[0])), int(round(x[2] / dx[1])), int(round(x[4] / dx[2])))
        out[:, k0:k0 + f.shape[1], j0:j0 + f.shape[2], i0:i0 + f.shape[3]] = f
    return out


@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
def test_driver_linwave_ppm_on_the_march(hiplib, riem):
    """The reference's linear-wave regression with PPM through the host driver: the general stage takes the march
    (stage_kernel says so), one block equals the oracle bit for bit, the mesh split into 8 x 4 x 4 blocks (linwave.py's
    decomposition) equals the one-block run, and the error norms meet the reference's thresholds."""
    from artemis_amd.driver import Simulation
    thr = (LINWAVE["ppm"]["rms_err_n32_max"], LINWAVE["ppm"]["n32_over_n16_max"])
    e32 = []
    for wi, (wave, vflow) in enumerate(linwave_waves()):
        errs = {}
        for N in (16, 32):
            sim = Simulation(DECK("linwave", "linear_wave.in"), linwave_overrides(N, "ppm", riem, wave, vflow))
            assert sim.uses_fused_path and not sim.uses_tuned_kernel
            sim.evolve()
            assert sim.stage_kernel == "stage_ppm_kernel", sim.stage_kernel
            errs[N] = sim.errors()[0]
            if N == 32:
                o = Oracle((N, N // 2, N // 2), (0, 0, 0), (3.0, 1.5, 1.5), ng=4, reconstruct="ppm",
                           riemann=riem, gamma=1.66666666667, cfl=0.9, bc=("periodic",) * 6)
                tlim = o.pgen_linear_wave(wave, 1.0e-6, vflow)
                o.evolve(tlim, 1000)
                assert sim.ncycle == o.ncycle and sim.time == o.time and sim.dt == o.dt
                I = interior(o)
                one_prim, one_cons = sim.field("gas.prim")[I], sim.field("gas.cons")[I]
                assert np.array_equal(one_prim, o.gprim[I])
                assert np.array_equal(one_cons, o.gu0[I])
                assert errs[N] == o.linear_wave_errors()[0]
                split = Simulation(DECK("linwave", "linear_wave.in"),
                                   linwave_overrides(N, "ppm", riem, wave, vflow, mb=(N // 4, N // 8, N // 8)))
                assert split.uses_fused_path and not split.uses_tuned_kernel
                split.evolve()
                assert split.stage_kernel == "stage_ppm_kernel", split.stage_kernel
                assert split.nblocks == 64
                assert (split.ncycle, split.time, split.dt) == (sim.ncycle, sim.time, sim.dt)
                assert np.array_equal(gather(split, "gas.prim", N), one_prim)
                assert np.array_equal(gather(split, "gas.cons", N), one_cons)
                # (the norm is a sum over the mesh taken block by block: equal fields, another order of additions -- it
                #  meets the reference's threshold like the one-block run's and agrees with it within 8192 zones x 2^-53 < 1e-12)
                assert split.errors()[0] <= thr[0][wi] and abs(split.errors()[0] - errs[N]) <= 1e-12 * errs[N]
                split.close()
            sim.close()
        e32.append(errs[32])
        assert errs[32] <= thr[0][wi] and errs[32] / errs[16] <= thr[1][wi]
    assert "%e" % e32[0] == "%e" % e32[1]  # linwave.py:135-143
