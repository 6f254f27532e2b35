"""What the recorder tests (tests/test_record.py on the GPU, tests/test_record_cpu.py and tests/record_worker.py on the CPU double)
share: the points, the stepping loop that defines a time series -- evolve(1), then ncycle, time, dt and plan.values -- and
the bitwise comparison of a Recorder's rows with it.  `make` is a callable that returns a fresh Simulation."""
import numpy as np

from fields_sample_ref import same_bits

VARS = ["gas.prim.density", "gas.cons.momentum"]
DERIVED = VARS + ["gas.derived.vorticity"]


def mesh_box(sim):
    sim._refresh_dims()
    bounds = np.array([sim.block_bounds(b) for b in range(sim.nblocks)]).reshape(-1, 6)
    nx = (sim.ie - sim.is_ + 1, sim.je - sim.js + 1, sim.ke - sim.ks + 1)
    return bounds, nx, bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)


def probe_points(sim):
    """a 16 x 16 lattice slice of the mesh (through x3 a little above its middle), two points outside the mesh, and the mesh's
    upper corner, which the closed upper edge puts into the last zone: [259, 3]"""
    from artemis_amd import sample as smp
    _, _, lo, hi = mesh_box(sim)
    z = lo[2] + 0.53 * (hi[2] - lo[2])
    slice_ = smp.lattice((lo[0], lo[1], z), (hi[0], hi[1], z), (16, 16, 1))
    outside = np.array([[lo[0] - 0.5 * (hi[0] - lo[0]), 0.5 * (lo[1] + hi[1]), z], [0.5 * (lo[0] + hi[0]), hi[1] + 0.25 * (hi[1] - lo[1]), z]])
    return np.ascontiguousarray(np.concatenate([slice_, outside, hi[None, :]]))


def stepping(make, points, variables, cycles, single=False, start=0, prepare=None):
    """Run A: prepare(sim) if given and `start` cycles, then up to `cycles` times (evolve(1); ncycle, time, dt; values) --
    until the run ends.  Returns cycle [n], time [n], dt [n], values [n, ncomp, npoints], the final state, the final clock
    and the remeshes of the recorded cycles."""
    sim = make()
    try:
        if prepare:
            prepare(sim)
        if start:
            assert sim.evolve(start) == start
        plan = sim.sample_plan(points)
        r0 = sim.remeshes
        cyc, tim, dts, val = [], [], [], []
        for _ in range(cycles):
            if sim.evolve(1) != 1:
                break
            cyc.append(sim.ncycle), tim.append(sim.time), dts.append(sim.dt), val.append(plan.values(variables, single=single))
        out = dict(cycle=np.array(cyc, dtype=np.int64), time=np.array(tim), dt=np.array(dts), values=np.stack(val), final=final_state(sim),
                   clock=(sim.ncycle, sim.time, sim.dt), remeshes=sim.remeshes - r0)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out
    finally:
        sim.close()


def split_a_coarsest_leaf(sim):
    """force_refine of a coarsest leaf (one rank: the local index is the global one): the criterion does not want the new
    blocks, so with derefine_count = 2 they merge again two cycles later -- a remesh inside a short run"""
    levels = [sim.block_level(b) for b in range(sim.nblocks)]
    assert sim.force_refine(int(np.argmin(levels)))


def final_state(sim):
    return sim.gather(["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"])


def same_series(ts, A, rows=None, tag=""):
    """the rows of a TimeSeries against rows `rows` (indices; default all) of the stepping loop's, every array bit for bit"""
    rows = np.arange(len(A["cycle"])) if rows is None else np.asarray(rows, dtype=np.int64)
    assert ts.cycle.dtype == np.int64 and np.array_equal(ts.cycle, A["cycle"][rows]), (tag, ts.cycle, A["cycle"][rows])
    assert same_bits(ts.time, A["time"][rows]) and same_bits(ts.dt, A["dt"][rows]), (tag, ts.time, A["time"][rows], ts.dt, A["dt"][rows])
    assert ts.values.shape == A["values"][rows].shape and ts.values.dtype == A["values"].dtype, (tag, ts.values.shape, A["values"][rows].shape)
    for r in range(len(rows)):
        assert same_bits(ts.values[r], A["values"][rows[r]]), (tag, "row", r, "cycle", int(ts.cycle[r]))


def same_run(sim, A, tag=""):
    """the run was not disturbed: clock and state equal the stepping loop's, bit for bit"""
    assert (sim.ncycle, sim.time, sim.dt) == A["clock"], (tag, sim.ncycle, sim.time, sim.dt, A["clock"])
    assert same_bits(final_state(sim), A["final"]), tag
