"""What the integral-recorder tests (tests/test_record_integrals.py on the GPU, tests/test_record_integrals_cpu.py and
tests/record_integrals_worker.py on the CPU double) share: the windows of a set of blocks, their zone membership in numpy, the
stepping loop that defines the series -- evolve(1), then ncycle, time, dt and history_device() -- and the derived bound of a
sum comparison.  `make` is a callable that returns a fresh Simulation.

The bound (tests/test_outputs.py): a sum of n terms t in any order is off by at most gamma_{n-1} * sum|t|, gamma_m = m u /
(1 - m u), u = 2^-53, so two such sums differ by at most 2 gamma_{n-1} S with S >= sum|t|.  A dropped or doubled zone moves a
sum by about 1/n of it; for a window of one zone the bound is 0 and the comparison is bitwise."""
import math

import numpy as np

from fields_sample_ref import same_bits
from record_cases import final_state


def gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def centres(bounds_b, nx, d):
    lo, hi = bounds_b[2 * d], bounds_b[2 * d + 1]
    return lo + (np.arange(nx[d]) + 0.5) * ((hi - lo) / nx[d])


def membership(bounds, nx, windows):
    """mask [nb, nwin, nz, ny, nx] of the zones whose centre lies in [lo, hi) along every direction with more than one zone"""
    bounds, windows = np.asarray(bounds, dtype=np.float64).reshape(-1, 6), np.asarray(windows, dtype=np.float64).reshape(-1, 3, 2)
    out = np.ones((len(bounds), len(windows), nx[2], nx[1], nx[0]), dtype=bool)
    for b in range(len(bounds)):
        for w in range(len(windows)):
            for d in range(3):
                if nx[d] == 1:
                    continue
                c = centres(bounds[b], nx, d)
                m = (c >= windows[w, d, 0]) & (c < windows[w, d, 1])
                out[b, w] &= m.reshape([-1 if a == 2 - d else 1 for a in range(3)])
    return out


def zone_table(bounds, nx, windows):
    """[nb, nwin, 6] int32 {i0, i1, j0, j1, k0, k1}: per direction the range of the zones whose centre lies in the window,
    half-open; all zeros where the window holds no zone of the block"""
    bounds, windows = np.asarray(bounds, dtype=np.float64).reshape(-1, 6), np.asarray(windows, dtype=np.float64).reshape(-1, 3, 2)
    out = np.zeros((len(bounds), len(windows), 6), dtype=np.int32)
    for b in range(len(bounds)):
        for w in range(len(windows)):
            r = []
            for d in range(3):
                if nx[d] == 1:
                    r += [0, 1]
                    continue
                c = centres(bounds[b], nx, d)
                at = np.nonzero((c >= windows[w, d, 0]) & (c < windows[w, d, 1]))[0]
                r += [int(at[0]), int(at[-1]) + 1] if len(at) else [0, 0]
            if all(r[2 * d] < r[2 * d + 1] for d in range(3)):
                out[b, w] = r
    return out


def mask_of_table(table, nx):
    """the membership a zone table describes, [nb, nwin, nz, ny, nx]"""
    nb, nwin = table.shape[:2]
    out = np.zeros((nb, nwin, nx[2], nx[1], nx[0]), dtype=bool)
    for b in range(nb):
        for w in range(nwin):
            i0, i1, j0, j1, k0, k1 = table[b, w]
            out[b, w, k0:k1, j0:j1, i0:i1] = True
    return out


def seven_windows(bounds, nx):
    """(a) the whole mesh, (b) no zone, (c) an x1 edge a quarter zone off a face in the middle of block 0 (it cuts a tile in
    mid-wave), (d) cuts along x2 and x3, (e) exactly the last block, (f) one zone of block 0, (g) the upper third of the last
    block along x1 (it misses every block below it).  The edges are measured in zones of the last block, the smallest: they
    lie a quarter of such a zone off its faces and at least an eighth of a zone from every zone centre of a coarser block."""
    bounds = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    lo, hi = bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)
    dx = np.array([(bounds[-1, 2 * d + 1] - bounds[-1, 2 * d]) / nx[d] for d in range(3)])
    dx0 = np.array([(bounds[0, 2 * d + 1] - bounds[0, 2 * d]) / nx[d] for d in range(3)])
    big = 4.0 * (hi - lo) + 1.0
    all_ = np.stack([lo - big, hi + big], axis=1)
    a, b = all_.copy(), np.stack([hi + big, hi + 2.0 * big], axis=1)
    c = all_.copy()
    c[0, 0] = bounds[0, 0] + (nx[0] // 2 + 0.25) * dx0[0]
    d = all_.copy()
    d[1] = [lo[1] + 1.25 * dx[1], hi[1] - 1.25 * dx[1]]
    d[2] = [lo[2] + 0.25 * dx[2], hi[2] - 1.25 * dx[2]]
    e = bounds[-1].reshape(3, 2).copy()
    zone = [min(3, nx[0] - 1), min(2, nx[1] - 1), min(1, nx[2] - 1)]
    f = np.array([[bounds[0, 2 * q] + (zone[q] + 0.25) * dx0[q], bounds[0, 2 * q] + (zone[q] + 0.75) * dx0[q]] for q in range(3)])
    g = all_.copy()
    g[0, 0] = bounds[-1, 1] - (nx[0] // 3 + 0.25) * dx[0]
    return np.ascontiguousarray(np.stack([a, b, c, d, e, f, g]))


def window_sums(terms, mask):
    """terms [nq][nb, nz, ny, nx] and a mask [nb, nz, ny, nx]: (the float64 numpy sums [nq], S >= sum|t| [nq], zones)"""
    sums = np.array([np.sum(t[mask]) for t in terms])
    S = np.array([math.fsum(np.abs(t[mask])) for t in terms]) * (1.0 + 2.0 ** -50)
    return sums, S, int(mask.sum())


def within_bound(got, want, S, n, tag=""):
    err, bound = np.abs(np.asarray(got) - want), 2.0 * gamma(max(n - 1, 0)) * S
    print(tag, "n =", n, "max err / bound =", float(np.max(err / np.where(bound > 0, bound, 1.0))) if n > 1 else float(np.max(err)))
    assert np.all(err <= bound), (tag, n, err, bound)


def stepping(make, cycles, start=0, prepare=None):
    """Run A: prepare(sim) if given and `start` cycles, then up to `cycles` times (evolve(1); ncycle, time, dt;
    history_device()) -- until the run ends.  Returns cycle [n], time [n], dt [n], set0 [n, nq], the final state and clock and
    the remeshes of the recorded cycles."""
    sim = make()
    try:
        if prepare:
            prepare(sim)
        if start:
            assert sim.evolve(start) == start
        r0 = sim.remeshes
        cyc, tim, dts, val = [], [], [], []
        for _ in range(cycles):
            if sim.evolve(1) != 1:
                break
            cyc.append(sim.ncycle), tim.append(sim.time), dts.append(sim.dt), val.append(sim.history_device())
        out = dict(cycle=np.array(cyc, dtype=np.int64), time=np.array(tim), dt=np.array(dts), set0=np.stack(val), final=final_state(sim),
                   clock=(sim.ncycle, sim.time, sim.dt), remeshes=sim.remeshes - r0)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out
    finally:
        sim.close()


def same_series(ts, A, rows=None, tag=""):
    """cycle, time, dt and set 0 of an IntegralSeries against rows `rows` (indices; default all) of the stepping loop's, bit
    for bit"""
    rows = np.arange(len(A["cycle"])) if rows is None else np.asarray(rows, dtype=np.int64)
    assert ts.cycle.dtype == np.int64 and np.array_equal(ts.cycle, A["cycle"][rows]), (tag, ts.cycle, A["cycle"][rows])
    assert same_bits(ts.time, A["time"][rows]) and same_bits(ts.dt, A["dt"][rows]), (tag, ts.time, A["time"][rows], ts.dt, A["dt"][rows])
    assert ts.integrals.ndim == 3 and ts.integrals.shape[0] == len(rows) and ts.integrals.shape[2] == A["set0"].shape[1], (tag, ts.integrals.shape)
    for r in range(len(rows)):
        assert same_bits(ts.integrals[r, 0], A["set0"][rows[r]]), (tag, "row", r, "cycle", int(ts.cycle[r]), ts.integrals[r, 0], A["set0"][rows[r]])


def sim_blocks(sim):
    """bounds [nb, 6] and zones (nx1, nx2, nx3) of a simulation's local blocks"""
    sim._refresh_dims()
    bounds = np.array([sim.block_bounds(b) for b in range(sim.nblocks)]).reshape(-1, 6)
    return bounds, (sim.ie - sim.is_ + 1, sim.je - sim.js + 1, sim.ke - sim.ks + 1)


def sim_terms(sim, volumes):
    """the per-zone terms of the history layout from the conserved fields of every block, [nq][nb, nz, ny, nx]; volumes:
    [nb, nz, ny, nx]"""
    nsg, nsd = sim.ns_gas, sim.ns_dust
    gas = np.stack([sim.interior(sim.field("gas.cons", b)) for b in range(sim.nblocks)]) if nsg else None
    dust = np.stack([sim.interior(sim.field("dust.cons", b)) for b in range(sim.nblocks)]) if nsd else None
    return layout_terms(gas, dust, nsg, nsd, volumes)


def layout_terms(gas, dust, nsg, nsd, volumes):
    """gas [nb, 6 nsg, ...] and dust [nb, 4 nsd, ...] conserved arrays in the driver's order -> [nq][nb, ...] terms"""
    out = []
    for n in range(nsg):
        out += [gas[:, n] * volumes] + [gas[:, nsg + 3 * n + q] * volumes for q in range(3)] + [gas[:, 4 * nsg + n] * volumes, gas[:, 5 * nsg + n] * volumes]
    for n in range(nsd):
        out += [dust[:, n] * volumes] + [dust[:, nsd + 3 * n + q] * volumes for q in range(3)]
    return out


def box_about_leaf(bounds, nx, leaf):
    """a window [1, 3, 2] that strictly contains block `leaf`: its bounds widened by 1.125 of its zones along every direction
    with more than one zone, so every edge lies a quarter of a zone of the next finer level off a face and at least a
    quarter of such a zone from every zone centre of this level, of the next finer one (the block's children, and by 2:1
    balance the finest a neighbour can be) and of every coarser one"""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)[leaf]
    box = np.array([[-1e3, 1e3]] * 3)
    for d in range(3):
        if nx[d] > 1:
            dx = (b[2 * d + 1] - b[2 * d]) / nx[d]
            box[d] = [b[2 * d] - 1.125 * dx, b[2 * d + 1] + 1.125 * dx]
    return box[None]


def window_across_remeshes(sim, cycles=8):
    """Item: a window's mass across a remesh that only splits or merges blocks inside it.  One cycle, then force_refine of a
    coarsest leaf that a proper window strictly contains, then cycles - 1 more, one evolve(1) at a time so that the mesh of
    every row is known.  After every cycle window_zones() is the numpy table of the mesh of that moment.  The window lies in
    gas at rest (asserted: its momentum integrals vanish against its mass to 1e-13, and its mass does not move between rows
    on one mesh beyond the same bound), so across a remesh the two masses are sums of n1 and n2 terms of one total:
    restriction and prolongation are conservative, each forming a zone from at most 8 others (gamma_8).  The bound is
    (gamma_{n1 - 1} + gamma_{n2 - 1} + gamma_8) S, S the larger mass (positive terms).  Returns the number of remeshes that
    changed the window's zones."""
    bounds, nx = sim_blocks(sim)
    levels = [sim.block_level(b) for b in range(sim.nblocks)]
    leaf = int(np.argmin(levels))
    win = box_about_leaf(bounds, nx, leaf)
    rec = sim.record_integrals(windows=win)
    zones = []
    for c in range(cycles):
        if c == 1:
            assert sim.force_refine(leaf)
        assert sim.evolve(1) == 1
        bounds, nx = sim_blocks(sim)
        table = rec.window_zones()
        assert table.shape == (sim.nblocks, 1, 6) and np.array_equal(table, zone_table(bounds, nx, win)), ("cycle", c)
        zones.append(int(mask_of_table(table, nx).sum()))
    ts = rec.read()
    mass, mom = ts.integrals[:, 1, 0], np.abs(ts.integrals[:, 1, 1:4]).max(axis=1)
    whole = ts.integrals[:, 0, 0]
    assert (mass > 0.0).all() and (mass < whole).all() and 0 < min(zones)  # a proper window
    assert (mom <= 1e-13 * mass).all(), (mom, mass)  # at rest
    changed = 0
    for r in range(1, cycles):
        n1, n2 = zones[r - 1], zones[r]
        S = max(mass[r - 1], mass[r])
        bound = (gamma(n1 - 1) + gamma(n2 - 1) + gamma(8)) * S
        print("rows", r - 1, r, "zones", n1, n2, "mass", mass[r - 1], mass[r], "diff", abs(mass[r] - mass[r - 1]), "bound", bound)
        assert abs(mass[r] - mass[r - 1]) <= bound, (r, n1, n2, mass[r - 1], mass[r], bound)
        changed += n1 != n2
    rec.close()
    return changed
