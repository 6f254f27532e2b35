"""Checkpoint and restart through the HIP driver (artemis_sim_save / artemis_sim_restore), on every family of stage
kernels and mesh the driver runs.

The pattern of every case: run A does evolve(n1); evolve(n2).  Run B does evolve(n1); save; close; restore; evolve(n2).
1. Directly after the restore every zone of field(...) of every block equals the saved simulation's (the whole arrays
   are stored: ghost zones included).
2. After n2: time, dt, ncycle, stage_kernel and the INTERIOR of gas.prim, gas.cons, dust.* of every block equal A's.
   (Only the interior: edge and corner ghost zones and the pressure slot of a ping-pong buffer hold whatever that buffer
   held before, and B starts on buffer 0 where A may be on another.)
All comparisons are np.array_equal.  The host logic and the refusals are tests/test_restart_cpu.py."""
import os

import numpy as np
import pytest

import amr_cases
from pins import DISK
from test_driver_gpu import BLAST3D, disk_overrides, linwave_overrides

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)


def fields_of(s):
    return ["gas.prim", "gas.cons"] + (["dust.prim", "dust.cons"] if s.ns_dust else [])


def clock(s):
    return dict(time=s.time, dt=s.dt, ncycle=s.ncycle, remeshes=s.remeshes, nblocks=s.nblocks, nglobal=s.nblocks_global)


def tree(s):
    return [(s.block_level(b), tuple(s.block_bounds(b))) for b in range(s.nblocks)]


def whole(s):
    return {f: [s.field(f, b) for b in range(s.nblocks)] for f in fields_of(s)}


def interiors(s):
    return {f: [s.interior(s.field(f, b)).copy() for b in range(s.nblocks)] for f in fields_of(s)}


def go(s, n):
    if n != 0:
        s.evolve(n)


def pattern(deck, ov, n1, n2, tmp_path, setup=None, save_ov=(), restore_ov=(), comm=None, lib=None, nbody=False, errors=False):
    """Runs A and B; returns what the caller may check further: A's and B's final clocks, stage kernels, density of A at
    the start and at the end (interiors), and the checkpoint directory."""
    from artemis_amd.driver import Simulation
    setup = setup or (lambda s: None)
    ck = str(tmp_path / "ck")
    a = Simulation(deck, list(ov), comm=comm, lib=lib)
    setup(a)
    d0 = [a.interior(a.field("gas.prim", b))[0].copy() for b in range(a.nblocks)]
    r0 = a.remeshes
    go(a, n1), go(a, n2)
    A = dict(clock=clock(a), kernel=a.stage_kernel, tree=tree(a), fields=interiors(a), errors=list(a.errors()) if errors else None,
             nbody=a.nbody_force() if nbody else None)
    a.close()
    b = Simulation(deck, list(ov) + list(save_ov), comm=comm, lib=lib)
    setup(b)
    go(b, n1)
    S = dict(clock=clock(b), tree=tree(b), fields=whole(b))
    assert S["clock"]["ncycle"] == n1
    b.save(ck)
    zones = (b.ni * b.nj * b.nk, b.nblocks_global, b.ns_gas, b.ns_dust)
    b.close()
    r = Simulation.restore(ck, list(restore_ov), comm=comm, lib=lib)
    setup(r)
    assert clock(r) == S["clock"] and tree(r) == S["tree"]
    for f in fields_of(r):  # 1. every zone, directly after the restore
        for blk in range(r.nblocks):
            assert np.array_equal(r.field(f, blk), S["fields"][f][blk]), ("after restore", f, blk)
    go(r, n2)
    assert clock(r) == A["clock"], (clock(r), A["clock"])  # 2. after n2
    assert r.stage_kernel == A["kernel"] and tree(r) == A["tree"]
    for f in fields_of(r):
        for blk in range(r.nblocks):
            assert np.array_equal(r.interior(r.field(f, blk)), A["fields"][f][blk]), ("after n2", f, blk)
    if errors:
        assert list(r.errors()) == A["errors"]
    if nbody:
        assert np.array_equal(r.nbody_force(), A["nbody"]) and np.abs(A["nbody"]).max() > 0.0
    r.close()
    return dict(A=A, S=S, d0=d0, remeshes=(r0, S["clock"]["remeshes"], A["clock"]["remeshes"]), ck=ck, zones=zones)


BLAST_8 = [o for o in BLAST3D if "meshblock" not in o] + ["parthenon/meshblock/nx1=24", "parthenon/meshblock/nx2=20",
                                                          "parthenon/meshblock/nx3=16"]


@pytest.mark.parametrize("integ,path", [("rk2", "fused"), ("vl2", "fused"), ("rk3", "fused"), ("rk2", "unfused")])
def test_tuned_kernel_blast3d_on_eight_blocks(hiplib, tmp_path, integ, path):
    """blast.in in 3-D (the overrides of test_blast3d_fused_equals_unfused_equals_oracle) on 8 blocks; 5 + 6 cycles: past
    the three plain steps of an evolve(), so B's second half replays a captured graph as A's does.  Also on the per-task
    chain (set_path is a runtime setting: the caller re-applies it after the restore)."""
    res = pattern(DECK("blast", "blast.in"), BLAST_8 + [f"parthenon/time/integrator={integ}"], 5, 6, tmp_path,
                  setup=lambda s: s.set_path(path))
    assert res["A"]["clock"]["nblocks"] == 8 and res["A"]["clock"]["ncycle"] == 11
    assert res["A"]["kernel"] == ("stage_fused_kernel" if path == "fused" else "per-task chain")


@pytest.mark.parametrize("mb", [None, (4, 2, 2)])
def test_ppm_march_linwave_to_tlim(hiplib, tmp_path, mb):
    """The PPM march on one block and on 4 x 2 x 2-zone blocks; saved after 7 cycles, then to tlim: the tlim clamp of the
    last step and the error norms are part of the check."""
    res = pattern(DECK("linwave", "linear_wave.in"), linwave_overrides(16, "ppm", "hllc", 0, 0.0, mb=mb), 7, -1, tmp_path, errors=True)
    assert res["A"]["clock"]["ncycle"] > 7 and res["A"]["errors"][0] > 0.0
    assert res["A"]["clock"]["nblocks"] == (1 if mb is None else 64)


def test_row_march_shearing_sheet_with_dust_and_drag(hiplib, tmp_path):
    """ssheet.in at 64 x 64 on one block: two dust species, drag, the `extrap` / `inflow` conditions of the strat problem."""
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=64", "parthenon/meshblock/nx1=64", "parthenon/meshblock/nx2=64",
          "physics/dust=true", "physics/drag=true", "dust/nspecies=2", "dust/cfl=0.3", "dust/reconstruct=plm", "dust/riemann=hlle",
          "dust/dfloor=1.0e-10", "dust/stopping_time/type=constant", "dust/stopping_time/tau=0.01, 2.0", "drag/type=simple_dust",
          "gravity/point/mass=1.0e-3", "parthenon/time/nlim=25"]
    res = pattern(DECK("ssheet", "ssheet.in"), ov, 6, 6, tmp_path)
    assert res["A"]["clock"]["ncycle"] == 12 and res["A"]["clock"]["nblocks"] == 1 and res["zones"][3] == 2


def check_disk_bounds(res):
    """tst/scripts/disk/disk.py:118-187: density error <= 6e-3, 1e-4 < dt < 3e-2, positive density and temperature"""
    num = den = 0.0
    for b, P in enumerate(res["A"]["fields"]["gas.prim"]):  # (== B's, bit for bit: checked by pattern())
        d, T = P[0], P[5] * 0.4
        assert not np.isnan(P).any() and d.min() > 0.0 and T.min() > 0.0
        num += (res["d0"][b] * (d - res["d0"][b]) ** 2).sum()
        den += res["d0"][b].sum()
    assert DISK["dt_low"] < res["A"]["clock"]["dt"] < DISK["dt_high"]
    err = np.sqrt(num) / den
    assert err <= DISK["density_err_max"], err


@pytest.mark.parametrize("g,gam,b,one_block", [("axi", 1.0, "ic", True), ("axi", 1.4, "extrap", True), ("cyl", 1.0, "ic", True),
                                               ("cyl", 1.4, "extrap", True), ("sph", 1.4, "ic", True), ("sph", 1.0, "extrap", True),
                                               ("cyl", 1.0, "ic", False)])
def test_reference_disk_regression_across_a_restart(hiplib, tmp_path, g, gam, b, one_block):
    """tst/scripts/disk/disk.py:54,83-97: 5 cycles, restart with nlim = 10 on the command line, on to cycle 10.  Equal to
    the straight 10-cycle run bit for bit (`extrap` too: both halves run on the device), within disk.py's bounds.  One
    geometry also on the deck's own 32-zone blocks."""
    ov = disk_overrides(g, gam, b, one_block=one_block)  # (carries nlim = 10)
    res = pattern(DECK("disk", f"disk_{g}.in"), ov, 5, -1, tmp_path, save_ov=["parthenon/time/nlim=5"],
                  restore_ov=["parthenon/time/nlim=10"])
    assert res["A"]["clock"]["ncycle"] == 10 and (res["A"]["clock"]["nblocks"] == 1) == one_block
    check_disk_bounds(res)


def test_static_refinement_disk_cart(hiplib, tmp_path):
    """disk_cart.in (static level-1 region) at the 64^3 root tests/test_multilevel.py runs: 64 coarse + 512 fine blocks,
    5 + 5 cycles across the restart; the tree comes from the file."""
    ov = ["parthenon/time/nlim=%d" % DISK["cycles"]] + ["parthenon/mesh/nx%d=%d" % (d + 1, n) for d, n in enumerate(DISK["cart_mesh_override"])]
    res = pattern(DECK("disk", "disk_cart.in"), ov + ["problem/polytropic_index=1.40", "gas/de_switch=0.0"], 5, -1, tmp_path,
                  save_ov=["parthenon/time/nlim=5"], restore_ov=["parthenon/time/nlim=10"])
    assert res["A"]["clock"]["nblocks"] == 576 and [l for l, _ in res["A"]["tree"]].count(1) == 512
    assert res["A"]["clock"]["ncycle"] == 10


@pytest.mark.parametrize("name", ["blast_amr", "disk_planet_dust_3d"])
def test_adaptive_mesh(hiplib, tmp_path, name):
    """Leaves in Z-order, levels, bounds and the remesh count equal A's (pattern() compares them), and so do the n-body
    sums.  The mesh changes at least twice in EACH half, so the restored derefinement counters decide merges of B."""
    if name == "blast_amr":
        # (the shock reaches the edge of the level-2 patch after 60 cycles: the tree changes at cycles 61, 66, 67 and then
        #  every fifth and sixth cycle -- 70 + 20 puts three changes before the save and seven after it)
        case, n1, n2, nbody = amr_cases.blast_amr(n=128, derefine_count=5), 70, 20, False
    else:
        # (18 cycles as tests/test_adaptive.py runs this case; the tree changes after cycles 4, 11, 13, 14, 16 and 17: a save
        #  after 13 has three changes behind it and three ahead -- after 9 there would be one behind)
        case, n1, n2, nbody = amr_cases.disk_planet_dust_amr(n=16, planet=3e-2, thr=2.5, nz=8, zlim=0.01), 13, 5, True
    res = pattern(DECK(*case["deck"]), case["overrides"], n1, n2, tmp_path, nbody=nbody)
    r0, r1, r2 = res["remeshes"]
    assert r1 >= r0 + 2 and r2 >= r1 + 2, res["remeshes"]
    assert res["A"]["clock"]["ncycle"] == n1 + n2


def test_binary_gravity_positions_come_from_the_restored_clock(hiplib, tmp_path):
    """binary_cyl.in at 64 x 128 (the orbit is evaluated on the host from the simulation time), 4 + 4 cycles."""
    res = pattern(DECK("disk", "binary_cyl.in"), ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=128", "parthenon/time/nlim=20"], 4, 4, tmp_path)
    assert res["A"]["clock"]["ncycle"] == 8 and res["A"]["clock"]["time"] > 0.0


def test_save_at_cycle_zero(hiplib, tmp_path):
    """Before the first step dt is still DBL_MAX: the restored run derives its first dt like a fresh one."""
    res = pattern(DECK("blast", "blast.in"), BLAST_8, 0, 5, tmp_path)
    assert res["S"]["clock"]["ncycle"] == 0 and res["S"]["clock"]["dt"] > 1e300 and res["A"]["clock"]["ncycle"] == 5


def test_rccl_loopback(hiplib, tmp_path, option):
    """Every ghost slab through the native RCCL transport as a message to self (the option of
    test_rccl_loopback_halo_exchange): save and restore are collective over the communicator."""
    from artemis_amd.driver import RcclComm
    ov = linwave_overrides(32, "plm", "hllc", 0, 0.0, mb=(16, 8, 8)) + ["parthenon/time/nlim=12"]
    option("loopback_comm", 1)
    comm = RcclComm(0, 1)
    try:
        res = pattern(DECK("linwave", "linear_wave.in"), ov, 5, -1, tmp_path, comm=comm)
    finally:
        comm.close()
    assert res["A"]["clock"]["ncycle"] == 12 and res["A"]["clock"]["nblocks"] == 8


def test_file_size_is_what_the_format_says(hiplib, tmp_path):
    """At most nblocks (6 ns_gas + 4 ns_dust) ni nj nk 8 bytes + the deck text + 64 B per block + 4 KB: from the format
    (32 B of directory and at most 20 B of derefinement counter per block; headers, overrides and n-body rows in the 4 KB)."""
    from artemis_amd.driver import Simulation
    case = amr_cases.disk_planet_dust_amr()
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    s.evolve(2)
    ck = str(tmp_path / "ck")
    s.save(ck)
    size = sum(os.path.getsize(os.path.join(ck, f)) for f in os.listdir(ck))
    deck = len(open(DECK(*case["deck"])).read())
    assert s.ns_dust == 1 and s.nblocks_global > 16
    assert size <= s.nblocks_global * (6 * s.ns_gas + 4 * s.ns_dust) * s.ni * s.nj * s.nk * 8 + deck + 64 * s.nblocks_global + 4096
    d = Simulation.describe_checkpoint(ck)
    assert d["bytes"] == size and d["nblocks"] == s.nblocks_global and d["ncycle"] == 2 and d["adaptive"] and d["nparticles"] == 2
    s.close()
