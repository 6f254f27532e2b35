"""GPU tests of the deck-driven outputs (artemis_sim_enable_outputs) and of the device history sums
(artemis_hip_history_sums through Simulation.history_device): only repository code runs here.

The bound of the sum comparison is derived, not tuned.  history_device() and history() add the same n per-zone terms
(each term the same double: PrimToCons's expressions times Coords::Volume()) in a different order; a sum of n terms t in
any order is off by at most gamma_{n-1} * sum|t|, gamma_m = m u / (1 - m u), u = 2^-53, so the two differ by at most
2 gamma_{n-1} S with S >= sum|t|: the host value itself for mass and the energies (positive terms), max|M_d / D| * mass
for a momentum.  A dropped or doubled zone moves a sum by about 1/n of it, ten and more orders of magnitude above that."""
import os

import numpy as np
import pytest

from pins import ADVECTION, advection_history
from test_driver_gpu import linwave_overrides
from test_multilevel import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)
PI = 3.141592653589793

# mesh 24 x 20 x 12 in 8 blocks of 12 x 10 x 6: no extent is a multiple of the 64 x 4 tile
BLAST_CART = ["parthenon/mesh/nx1=24", "parthenon/mesh/nx2=20", "parthenon/mesh/nx3=12", "parthenon/mesh/x3min=-1.0",
              "parthenon/mesh/x3max=1.0", "parthenon/meshblock/nx1=12", "parthenon/meshblock/nx2=10",
              "parthenon/meshblock/nx3=6", "gas/riemann=hllc", "problem/symmetry=spherical", "problem/radius=0.3",
              "problem/samples=0"]


def advection_overrides(N, riem="hlle"):
    ov = linwave_overrides(N, "plm", riem, 0, 1.0, mb=(N // 4, N // 4, N // 4))  # test_advection_history_pins
    return [o for o in ov if "wave_flag" not in o] + ["dust/reconstruct=plm", f"dust/riemann={riem}"]


SUM_CASES = {
    "cart3d": (("blast", "blast.in"), BLAST_CART + ["parthenon/time/nlim=3"]),
    "advection": (("advection", "advection.in"), advection_overrides(16)),
    # the spherical 64 x 1 blast of smoke()
    "sph1d": (("blast", "blast.in"),
              ["artemis/coordinates=spherical", "parthenon/mesh/nx1=64", "parthenon/mesh/nx2=1", "parthenon/mesh/x1min=0.0",
               "parthenon/mesh/x1max=1.0", "parthenon/mesh/x2min=0.0", "parthenon/mesh/x2max=3.141592653589793",
               "parthenon/mesh/ix1_bc=reflecting", "parthenon/meshblock/nx1=64", "parthenon/meshblock/nx2=1",
               "problem/symmetry=spherical", "problem/radius=0.1", "problem/samples=0", "parthenon/time/nlim=5"]),
    # the cylindrical disk deck on the 16 x 8 x 6 block of tests/test_parity_disk.py (its smallest 3-D curvilinear one)
    "disk_cyl": (("disk", "disk_cyl.in"),
                 ["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=8", "parthenon/mesh/nx3=6", "parthenon/meshblock/nx1=16",
                  "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=6", "parthenon/mesh/x1min=0.8",
                  "parthenon/mesh/x1max=4.3", "parthenon/mesh/x3min=-1.0", "parthenon/mesh/x3max=1.0",
                  "parthenon/time/nlim=3"]),
    # the smallest statically refined case of tests/test_multilevel.py: 12 coarse + 16 fine blocks of 8 x 8
    "refined": (CASES["blast2d"]["deck"], CASES["blast2d"]["ov"]),
}


def gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def sum_bounds(s, host):
    """S of every entry of the history layout, from the conserved fields of all blocks."""
    S = np.abs(np.array(host, dtype=np.float64))
    nsg, nsd = s.ns_gas, s.ns_dust
    gas = [s.interior(s.field("gas.cons", b)) for b in range(s.nblocks)] if nsg else []
    dust = [s.interior(s.field("dust.cons", b)) for b in range(s.nblocks)] if nsd else []
    for n in range(nsg):
        for d in range(3):
            S[6 * n + 1 + d] = max(np.abs(g[nsg + 3 * n + d] / g[n]).max() for g in gas) * host[6 * n]
    for n in range(nsd):
        for d in range(3):
            S[6 * nsg + 4 * n + 1 + d] = max(np.abs(g[nsd + 3 * n + d] / g[n]).max() for g in dust) * host[6 * nsg + 4 * n]
    return S


@pytest.mark.parametrize("case", list(SUM_CASES))
def test_device_history_sums_equal_the_host_sums(hiplib, case):
    from artemis_amd.driver import Simulation
    deck, ov = SUM_CASES[case]
    s = Simulation(DECK(*deck), ov)
    s.evolve(3)
    assert s.ncycle == 3
    dev, again = s.history_device(), s.history_device()
    assert dev.tobytes() == again.tobytes()  # no atomics, a fixed number of partial rows: the same bits every time
    host = s.history()
    assert len(dev) == 6 * s.ns_gas + 4 * s.ns_dust == len(host)
    n = s.total_zones
    if case == "cart3d":
        assert s.nblocks == 8 and n == 24 * 20 * 12
    if case == "refined":
        assert s.nblocks == 28 and {s.block_level(b) for b in range(s.nblocks)} == {0, 1}
    S = sum_bounds(s, host)
    err = np.abs(dev - host)
    bound = 2.0 * gamma(n - 1) * S
    print(case, "n =", n, "max err / bound =", np.max(err / np.where(bound > 0, bound, 1.0)), "err", err, "bound", bound)
    assert host[0] > 0.0 and np.all(err <= bound), (case, err, bound)
    if case == "advection":  # the two dust species stream against each other: S is not the value there
        assert host[7] == pytest.approx(-host[11], rel=1e-9) and S[7] > 0.0
    s.close()


def equiv(a, b, tol=ADVECTION["equiv_rel_tol"]):  # advection.py:95-99
    return 2.0 * abs(a - b) / (abs(a) + abs(b)) <= tol


def test_reference_history_pins_through_the_file(hiplib, tmp_path):
    """The advection deck at N = 32 with an `hst` block every 0.1: the last row of the file satisfies the reference's pins
    (tests/golden/reference_pins.json), and the rows sit at cycle 0, at the first cycle with time >= m * 0.1 for every
    multiple the run reaches, and at the end of the run, one row per cycle: 11 rows, the number the reference's own
    regression test demands of this file (advection.py:123).  The tenth multiple and the end of the run share the last
    row: the problem generator's time limit is one unit in the last place below 1.0, so the run ends at t =
    0.9999999999999998 < 10 * 0.1 and the row of cycle 56 is the end-of-run row (were the limit exactly 1.0 it would be the
    row of the tenth multiple, again written once).  The issue that asked for this test counted twelve rows for the same
    list -- cycle 0, ten multiples, the end merged with the last -- which is eleven.  The cycles are checked against a
    second run of the deck stepped with evolve(1) and no outputs."""
    from artemis_amd.driver import Simulation
    from artemis_amd.history import read_history
    ov = advection_overrides(32)
    s = Simulation(DECK("advection", "advection.in"), ov + ["parthenon/output0/file_type=hst", "parthenon/output0/dt=0.1"])
    s.enable_outputs(tmp_path)
    s.evolve()
    h = read_history(tmp_path / "advection.out0.hst")
    H = ADVECTION["history_n32"]
    assert h["cycle"][-1] == H["cycle"] == s.ncycle and h["nbtotal"][-1] == H["nbtotal"]
    assert equiv(h["time"][-1], H["time"]) and equiv(h["dt"][-1], H["dt"])
    assert h["time"][-1] == s.time and h["dt"][-1] == s.dt  # %.16e reads back to the same doubles
    labels = (["gas_mass_0"] + ["gas_momentum_x%d_0" % d for d in (1, 2, 3)] + ["gas_energy_0", "gas_internal_energy_0"] +
              ["dust_mass_0"] + ["dust_momentum_x%d_0" % d for d in (1, 2, 3)] +
              ["dust_mass_1"] + ["dust_momentum_x%d_1" % d for d in (1, 2, 3)])
    assert list(h)[:4] == ["time", "dt", "cycle", "nbtotal"] and set(list(h)[4:]) == set(labels) and len(h) == 18
    assert list(h)[4:10] == labels[:6] and list(h)[10:12] == ["dust_mass_0", "dust_mass_1"]  # the species is the inner index
    for lab, want in zip(labels, advection_history()):
        assert equiv(h[lab][-1], want), (lab, h[lab][-1], want)
    assert np.array_equal(np.array([h[lab][-1] for lab in labels]), s.history_device())
    # where the rows sit
    r = Simulation(DECK("advection", "advection.in"), ov)
    want_cycles, want_times, m = [0], [0.0], 1
    while r.evolve(1) == 1:
        if r.time >= m * 0.1:
            want_cycles.append(r.ncycle), want_times.append(r.time)
            m += 1
    assert r.ncycle == s.ncycle and r.time == s.time and r.dt == s.dt
    if want_cycles[-1] != r.ncycle:  # the end of the run has a row of its own unless its cycle was due anyway
        want_cycles.append(r.ncycle), want_times.append(r.time)
    assert list(h["cycle"]) == want_cycles and list(h["time"]) == want_times
    assert len(want_cycles) == 11 and m in (10, 11)
    s.close(), r.close()


# The values used.  12 cycles of this blast end at t = 0.0521 (dt falls from 4.8e-3 to 4.0e-3):
#   hst 0.002 / rst 0.005   both shorter than every step: a row after each cycle, a numbered dump after ten of the twelve;
#   hst 0.02  / rst 0.021   rows at cycles 0, 5 (t = 0.0230), 10 (t = 0.0440) and 12 (the end), numbered dumps at cycles 0, 5
#                           and 10 -- two of each kind strictly inside the run, and the first two cycles fit into one
#                           unsynchronised batch of the time loop.
# Where the rows and dumps have to sit is worked out from the clock of a third run stepped with evolve(1).
INTERVALS = {"every_cycle": (0.002, 0.005), "sparse": (0.02, 0.021)}


def out_blocks(hst_dt, rst_dt):
    return ["parthenon/output0/file_type=hst", "parthenon/output0/dt=%r" % hst_dt,
            "parthenon/output1/file_type=rst", "parthenon/output1/dt=%r" % rst_dt,
            "parthenon/output2/file_type=hdf5", "parthenon/output2/dt=0.001"]


def due_cycles(clock, dt_out):
    """Cycles after which a block with interval dt_out is written: time >= next_time, next_time the smallest multiple of
    dt_out above the time of the last write (0 at the start)."""
    out, nxt = [], 0.0
    for cycle, time in clock:
        if time >= nxt:
            out.append(cycle)
            m = int(np.floor(time / dt_out)) + 1
            while m * dt_out <= time:
                m += 1
            while m > 1 and (m - 1) * dt_out > time:
                m -= 1
            nxt = m * dt_out
    return out


def state_of(s):
    """The clock and, per block, the state: density, velocities and internal energy of every zone, ghost zones included,
    and all six primitives of the interior.  (The pressure of a ghost zone is no state: the one-kernel stages keep it on
    interior zones only, and a ghost zone shows whatever the last whole-block PrimToCons left there -- the convention of
    smoke() and tests/test_multilevel.py.)"""
    fields = []
    for b in range(s.nblocks):
        p = s.field("gas.prim", b)
        fields += [p[[0, 1, 2, 3, 5]], s.interior(p).copy(), s.interior(s.field("gas.cons", b)).copy()]
    return (s.time, s.dt, s.ncycle, s.stage_kernel), fields


@pytest.fixture(scope="module", params=[("tlim", "every_cycle"), ("no_tlim", "every_cycle"), ("tlim", "sparse"), ("no_tlim", "sparse")],
                ids=lambda p: "-".join(p))
def blast_with_outputs(request, tmp_path_factory):
    import torch
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    capi.load()
    assert torch.cuda.is_available()
    mode, which = request.param
    hst_dt, rst_dt = INTERVALS[which]
    out = tmp_path_factory.mktemp("outputs")
    ov = BLAST_CART + out_blocks(hst_dt, rst_dt) + ["parthenon/time/nlim=12"] + (["parthenon/time/tlim=-1.0"] if mode == "no_tlim" else [])
    a = Simulation(DECK("blast", "blast.in"), ov)
    a.enable_outputs(out)
    a.evolve()
    b = Simulation(DECK("blast", "blast.in"), ov)
    b.evolve()
    c = Simulation(DECK("blast", "blast.in"), ov)
    clock = [(0, 0.0)]
    while c.evolve(1) == 1:
        clock.append((c.ncycle, c.time))
    res = dict(with_outputs=state_of(a), without=state_of(b), stepped=state_of(c), out=out, describe=a.outputs(), tlim=b.tlim,
               mode=mode, hst_dt=hst_dt, rst_dt=rst_dt, clock=clock)
    a.close(), b.close(), c.close()
    return res


def test_outputs_do_not_move_the_trajectory(hiplib, blast_with_outputs):
    from artemis_amd.driver import Simulation
    from artemis_amd.history import read_history
    R = blast_with_outputs
    (ca, fa), (cb, fb), out = R["with_outputs"], R["without"], R["out"]
    assert (R["tlim"] < 0.0) == (R["mode"] == "no_tlim")
    assert ca == cb == R["stepped"][0] and ca[2] == 12
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    h = read_history(out / "blast_cart.out0.hst")
    files = sorted(os.listdir(out))
    dumps = [f for f in files if f.endswith(".rst")]
    rows, numbered = due_cycles(R["clock"], R["hst_dt"]), due_cycles(R["clock"], R["rst_dt"])
    print(R["mode"], "rows at cycles", h["cycle"], "times", h["time"], "dumps", dumps, "expected", rows, numbered)
    # two rows and two dumps (or more) strictly inside the run, next to the ones of cycle 0 and of the end
    assert len([c for c in rows if 0 < c < 12]) >= 2 and len([c for c in numbered if 0 < c < 12]) >= 2
    if rows[-1] != 12:
        rows = rows + [12]  # the end of the run, unless that cycle had its row already
    assert list(h["cycle"]) == rows and list(h["time"]) == [dict(R["clock"])[c] for c in rows]
    assert dumps == ["blast_cart.out1.%05d.rst" % q for q in range(len(numbered))] + ["blast_cart.out1.final.rst"]
    assert [Simulation.describe_checkpoint(out / d)["ncycle"] for d in dumps] == numbered + [12]
    # the hdf5 block is listed and never written
    blocks = {b["index"]: b for b in R["describe"]["blocks"]}
    assert blocks[2]["status"] == "skipped: hdf5 is not built" and blocks[2]["written"] == 0
    assert not [f for f in files if ".out2." in f]
    assert blocks[0]["status"] == "active" and blocks[0]["written"] == len(h["cycle"])


def test_a_dump_continues_the_run(hiplib, blast_with_outputs, tmp_path):
    """Simulation.restore of the second numbered dump, evolved to the end with outputs enabled in a copy of the directory:
    bit for bit the straight run; the history file gains a second header section and read_history returns the later one."""
    import shutil
    from artemis_amd.driver import Simulation
    from artemis_amd.history import HEADER, read_history
    R = blast_with_outputs
    (cb, fb) = R["without"]
    out = tmp_path / "continued"  # (a copy: the directory of the fixture stays as the first run left it)
    shutil.copytree(R["out"], out)
    hst = out / "blast_cart.out0.hst"
    first = read_history(hst)
    r = Simulation.restore(out / "blast_cart.out1.00001.rst")
    assert 0 < r.ncycle < 12 and r.time >= R["rst_dt"]
    start = r.ncycle
    r.enable_outputs(out)
    assert all(b["next_time"] is None or b["next_time"] > r.time for b in r.outputs()["blocks"])
    r.evolve()
    (cr, fr) = state_of(r)
    assert cr == cb
    for x, y in zip(fr, fb):
        assert np.array_equal(x, y)
    assert open(hst).read().count(HEADER) == 2
    later = read_history(hst)
    assert later["cycle"][0] > start and later["cycle"][-1] == 12  # no cycle-0 row, no row of the restored cycle
    keep = first["cycle"] > start
    assert np.array_equal(later["cycle"], first["cycle"][keep])
    for k in first:
        assert np.array_equal(later[k], first[k][keep]), k
    r.close()
