"""GPU tests of the recorded history integrals and n-body force sums (include/artemis_hip_record.h:
artemis_hip_record_integrals and artemis_hip_record_nbody; include/artemis_driver.h: artemis_sim_record_integrals_*;
Simulation.record_integrals).  Only repository code runs here.

The kernels on packs with random primitives in every zone: set 0 of the row the tick opened has the bits of
artemis_hip_history_sums, a window that holds every zone has the bits of set 0, an empty one is +0.0, every other window is
within the derived bound of tests/record_integrals_cases.py of a float64 numpy sum over the zones numpy puts into it (bitwise
for the window of one zone), a due row that finds the buffers full is counted and written nowhere, and nothing behind the
buffers is touched.  The driver against the stepping loop -- evolve(1), then ncycle, time, dt and history_device() --
through the plain steps, the captured graphs and their replays, the drains, the loop near tlim, the forced synchronous loop,
curvilinear, refined and adaptive meshes; the n-body rows against nbody_force() of fresh runs.  Set 0, the clock and the
n-body rows are compared bitwise."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import amr_cases
import record_cases as rc
import record_integrals_cases as ric
from fields_reduce_ref import oracle_volumes
from fields_sample_ref import same_bits
from test_fields import BLAST32
from test_fields_sample import NG, PACKS, make_pack
from test_record import tick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)
CANARY = 64
NAN = float("nan")
PACK_NAMES = ["three", "cyl3d", "sph3d", "mixed3d"]
CAPS = (1, 3)  # GRID_CAP as tests/test_grid_stride.py sets it


# ---- the kernels on packs -----------------------------------------------------------------------------------------------
def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nq_of(mb):
    return 6 * mb.nsg + 4 * mb.nsd


def scratch_of(mb, nwin):
    import torch
    nbytes = mb.L.artemis_hip_record_integrals_scratch_bytes(C.byref(mb.pack), nwin)
    rows = mb.L.artemis_hip_history_scratch_bytes(C.byref(mb.pack)) // (8 * nq_of(mb))
    assert nbytes == rows * (1 + nwin) * nq_of(mb) * 8 and rows >= 1, (nbytes, rows)
    return torch.full((nbytes // 8 + CANARY,), NAN, dtype=torch.float64, device=mb.dev), nbytes // 8


def integrals(mb, nwin, table, scratch, ctl, capacity, rows):
    return mb.L.artemis_hip_record_integrals(C.byref(mb.pack), nwin, ptr(table), ptr(scratch), ptr(ctl), capacity, ptr(rows), mb._stream())


def history_sums(mb):
    import torch
    nq = nq_of(mb)
    scratch = torch.zeros(mb.L.artemis_hip_history_scratch_bytes(C.byref(mb.pack)) // 8, dtype=torch.float64, device=mb.dev)
    sums = torch.zeros(nq, dtype=torch.float64, device=mb.dev)
    mb._call(mb.L.artemis_hip_history_sums, ptr(sums), ptr(scratch))
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def pack_terms(name):
    """the per-zone terms of the history layout, [nq][nb, nz, ny, nx]: the conserved values artemis_hip_prim_to_cons leaves in
    a second pack of the same primitives, times the oracle's volumes"""
    import torch
    mb, bounds, _, _ = make_pack(name)
    mb.PrimToCons()
    torch.cuda.synchronize()
    coords = PACKS[name][4]
    vol = np.stack([oracle_volumes(mb.nx, bounds[b, 0::2], bounds[b, 1::2], NG, coords) for b in range(mb.nb)])
    inner = (slice(None), slice(None), slice(mb.ks, mb.ke + 1), slice(mb.js, mb.je + 1), slice(mb.is_, mb.ie + 1))
    gas = mb.gas_u0.cpu().numpy()[inner] if mb.nsg else None
    dust = mb.dust_u0.cpu().numpy()[inner] if mb.nsd else None
    return ric.layout_terms(gas, dust, mb.nsg, mb.nsd, vol)


@pytest.mark.parametrize("name", PACK_NAMES)
def test_slot_mechanics(hiplib, name):
    """tick and integrals nine times with every = 3 and capacity = 2, a few primitives changed before each call: rows 0 and 1,
    set 0, are artemis_hip_history_sums at calls 3 and 6; the third due row (call 9) is dropped, counted, and leaves the
    canary behind the rows untouched"""
    import torch
    mb, bounds, _, _ = make_pack(name)
    nq, nwin = nq_of(mb), 2
    win = ric.seven_windows(bounds, mb.nx)[[0, 2]]
    table = torch.from_numpy(ric.zone_table(bounds, mb.nx, win)).to(mb.dev)
    every, capacity, cycle0 = 3, 2, 100
    row = (1 + nwin) * nq
    ctl = torch.tensor([0, cycle0, 0, -1, 0], dtype=torch.int64, device=mb.dev)
    head = torch.zeros(3 * capacity + 3, dtype=torch.float64, device=mb.dev)
    rows = torch.full((capacity * row + CANARY,), NAN, dtype=torch.float64, device=mb.dev)
    scratch, nscratch = scratch_of(mb, nwin)
    rng = np.random.default_rng(5)
    want, slots = {}, []
    for call in range(1, 10):
        for prim in (mb.gas_prim, mb.dust_prim):  # a few primitives, ghost zones included
            flat = prim.view(-1)
            if flat.numel():
                at = torch.from_numpy(rng.integers(0, flat.numel(), size=257)).to(mb.dev)
                flat[at] = flat[at] * 1.03125 + 0.015625 * call
        assert tick(mb, ctl, head, None, 0.125 * call, 0.01, every, capacity) == 0
        assert integrals(mb, nwin, table, scratch, ctl, capacity, rows) == 0, mb.L.artemis_hip_last_error()
        torch.cuda.synchronize()
        slots.append(int(ctl[3].item()))
        if call % every == 0:
            want[call] = history_sums(mb)
    assert slots == [-1, -1, 0, -1, -1, 1, -1, -1, -1]
    assert ctl.cpu().tolist() == [9, cycle0 + 9, 2, -1, 1]  # seen, cycle, rows, slot, dropped
    raw = rows.cpu().numpy()
    assert np.isnan(raw[capacity * row:]).all() and np.isnan(scratch.cpu().numpy()[nscratch:]).all()  # the canaries
    got = raw[:capacity * row].reshape(capacity, 1 + nwin, nq)
    assert same_bits(got[0, 0], want[3]) and same_bits(got[1, 0], want[6]) and not same_bits(want[3], want[6])
    assert same_bits(got[:, 1], got[:, 0]) and not np.isnan(got).any()


@pytest.fixture(scope="module")
def terms_of():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pack_terms(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", PACK_NAMES)
def test_windows(hiplib, terms_of, name):
    """the seven windows of record_integrals_cases.seven_windows in one call"""
    import torch
    mb, bounds, _, _ = make_pack(name)
    nq, nwin = nq_of(mb), 7
    win = ric.seven_windows(bounds, mb.nx)
    table = ric.zone_table(bounds, mb.nx, win)
    mask = ric.membership(bounds, mb.nx, win)
    assert np.array_equal(ric.mask_of_table(table, mb.nx), mask)  # the table the test uploads is that membership
    zones = mask.reshape(mb.nb, nwin, -1).sum(axis=2)
    total = mb.nb * mb.nx[0] * mb.nx[1] * mb.nx[2]
    assert zones[:, 0].sum() == total and zones[:, 1].sum() == 0 and zones[:, 5].sum() == 1 and 0 < zones[:, 2].sum() < total
    assert zones[:, 4].sum() == total // mb.nb and (mb.nb == 1 or (zones[:-1, 4] == 0).all())
    assert mb.nb == 1 or ((zones[:, 6] == 0).any() and zones[:, 6].sum() > 0)
    tdev = torch.from_numpy(table).to(mb.dev)
    ctl = torch.tensor([0, 0, 0, -1, 0], dtype=torch.int64, device=mb.dev)
    head = torch.zeros(6, dtype=torch.float64, device=mb.dev)
    row = (1 + nwin) * nq
    scratch, _ = scratch_of(mb, nwin)
    out = []
    for _ in range(2):
        rows = torch.full((row + CANARY,), NAN, dtype=torch.float64, device=mb.dev)
        ctl.copy_(torch.tensor([0, 0, 0, -1, 0], dtype=torch.int64))
        assert tick(mb, ctl, head, None, 0.5, 0.25, 1, 1) == 0
        assert integrals(mb, nwin, tdev, scratch, ctl, 1, rows) == 0, mb.L.artemis_hip_last_error()
        torch.cuda.synchronize()
        raw = rows.cpu().numpy()
        assert np.isnan(raw[row:]).all() and not np.isnan(raw[:row]).any()
        out.append(raw[:row].reshape(1 + nwin, nq).copy())
    got = out[0]
    assert same_bits(out[0], out[1])  # the same call twice
    assert same_bits(got[0], history_sums(mb))
    assert same_bits(got[1], got[0])  # (a)
    assert same_bits(got[2], np.zeros(nq))  # (b): +0.0, the sign bit clear
    terms = terms_of(name)
    for w in range(2, 7):
        want, S, n = ric.window_sums(terms, mask[:, w])
        assert n == zones[:, w].sum() and n > 0
        ric.within_bound(got[1 + w], want, S, n, "%s window %d" % (name, w))


@pytest.mark.parametrize("cap", CAPS)
def test_launch_shape(hiplib, cap):
    """GRID_CAP makes the workgroups stride over several tiles: set 0 still is artemis_hip_history_sums under the same cap and
    the window of every zone still has its bits"""
    import torch
    from artemis_amd import capi
    mb, bounds, _, _ = make_pack("three")
    nq, nwin = nq_of(mb), 7
    win = ric.seven_windows(bounds, mb.nx)
    tdev = torch.from_numpy(ric.zone_table(bounds, mb.nx, win)).to(mb.dev)
    free = history_sums(mb)
    with capi.option("grid_cap", cap):
        want = history_sums(mb)
        ctl = torch.tensor([0, 0, 0, -1, 0], dtype=torch.int64, device=mb.dev)
        head = torch.zeros(6, dtype=torch.float64, device=mb.dev)
        rows = torch.full(((1 + nwin) * nq + CANARY,), NAN, dtype=torch.float64, device=mb.dev)
        scratch, nscratch = scratch_of(mb, nwin)
        assert nscratch == min(cap, 3 * 2 * 2 * 3) * (1 + nwin) * nq  # 64 x 4 tiles: 2 along x1, 2 along x2, 3 planes, 3 blocks
        assert tick(mb, ctl, head, None, 0.5, 0.25, 1, 1) == 0 and integrals(mb, nwin, tdev, scratch, ctl, 1, rows) == 0
        torch.cuda.synchronize()
    got = rows.cpu().numpy()[:(1 + nwin) * nq].reshape(1 + nwin, nq)
    assert same_bits(got[0], want) and same_bits(got[1], got[0]) and same_bits(got[2], np.zeros(nq))
    assert np.isnan(scratch.cpu().numpy()[nscratch:]).all() and np.isnan(rows.cpu().numpy()[(1 + nwin) * nq:]).all()
    assert cap >= 36 or not same_bits(want, free)  # (the cap did change the tree)


@pytest.mark.parametrize("n", [7, 7 * 128])
def test_nbody_rows(hiplib, n):
    """artemis_hip_record_nbody: bitwise base + acc in the opened row, the canary untouched, no store when slot < 0"""
    import torch
    from artemis_amd import capi
    L = capi.load()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n)
    base, acc = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, size=n), rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, size=n)
    bd, ad = torch.from_numpy(base).to(dev), torch.from_numpy(acc).to(dev)
    capacity = 3
    rows = torch.full((capacity * n + CANARY,), NAN, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for slot in (-1, 3):  # not due; past the buffer
        ctl = torch.tensor([5, 5, 1, slot, 0], dtype=torch.int64, device=dev)
        assert L.artemis_hip_record_nbody(ptr(bd), ptr(ad), n, ptr(ctl), capacity, ptr(rows), stream) == 0
        torch.cuda.synchronize()
        assert np.isnan(rows.cpu().numpy()).all()
    ctl = torch.tensor([5, 5, 2, 1, 0], dtype=torch.int64, device=dev)
    assert L.artemis_hip_record_nbody(ptr(bd), ptr(ad), n, ptr(ctl), capacity, ptr(rows), stream) == 0
    torch.cuda.synchronize()
    raw = rows.cpu().numpy()
    assert same_bits(raw[n:2 * n], base + acc) and np.isnan(raw[:n]).all() and np.isnan(raw[2 * n:]).all()
    assert ctl.cpu().tolist() == [5, 5, 2, 1, 0]
    for bad in (lambda: L.artemis_hip_record_nbody(None, ptr(ad), n, ptr(ctl), capacity, ptr(rows), stream),
                lambda: L.artemis_hip_record_nbody(ptr(bd), ptr(ad), n, None, capacity, ptr(rows), stream),
                lambda: L.artemis_hip_record_nbody(ptr(bd), ptr(ad), n, ptr(ctl), 0, ptr(rows), stream),
                lambda: L.artemis_hip_record_nbody(ptr(bd), ptr(ad), -1, ptr(ctl), capacity, ptr(rows), stream),
                lambda: L.artemis_hip_record_nbody(ptr(bd), ptr(ad), n, ptr(ctl), capacity, None, stream)):
        assert bad() == capi.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.int64), raw.view(np.int64))


def test_refusals(hiplib):
    """what artemis_hip_record_integrals refuses leaves every buffer and the control block as they were"""
    import torch
    from artemis_amd import capi
    mb, bounds, _, _ = make_pack("cyl3d")
    nq = nq_of(mb)
    tdev = torch.from_numpy(ric.zone_table(bounds, mb.nx, ric.seven_windows(bounds, mb.nx))).to(mb.dev)
    ctl = torch.tensor([4, 44, 1, 0, 0], dtype=torch.int64, device=mb.dev)
    rows = torch.full((2 * 8 * nq + CANARY,), NAN, dtype=torch.float64, device=mb.dev)
    scratch, _ = scratch_of(mb, 7)
    for bad in (lambda: integrals(mb, 7, tdev, scratch, None, 2, rows), lambda: integrals(mb, 7, tdev, scratch, ctl, 2, None),
                lambda: integrals(mb, 7, tdev, scratch, ctl, 0, rows), lambda: integrals(mb, 8, tdev, scratch, ctl, 2, rows),
                lambda: integrals(mb, -1, tdev, scratch, ctl, 2, rows), lambda: integrals(mb, 7, None, scratch, ctl, 2, rows),
                lambda: integrals(mb, 7, tdev, None, ctl, 2, rows)):
        assert bad() == capi.EINVAL
    assert mb.L.artemis_hip_record_integrals_scratch_bytes(C.byref(mb.pack), 8) == 0
    torch.cuda.synchronize()
    assert ctl.cpu().tolist() == [4, 44, 1, 0, 0] and np.isnan(rows.cpu().numpy()).all() and np.isnan(scratch.cpu().numpy()).all()


# ---- the driver, against the stepping loop ------------------------------------------------------------------------------
CYCLES = 9
RUN = BLAST32 + ["parthenon/time/tlim=-1.0", "parthenon/time/nlim=%d" % CYCLES]


def blast32(extra=()):
    from artemis_amd.driver import Simulation
    return lambda: Simulation(DECK("blast", "blast.in"), RUN + list(extra))


@pytest.fixture(scope="module")
def blast_run(hiplib):
    """the stepping loop of the 32^3 blast (2 x 2 x 2 blocks of 16^3, nine cycles), made once, shared, never modified"""
    A = ric.stepping(blast32(), CYCLES)
    assert np.array_equal(A["cycle"], np.arange(1, CYCLES + 1))
    return A


def test_one_evolve_equals_the_stepping_loop(blast_run):
    """nine cycles in one evolve(9): plain steps, one capture per ping-pong phase, replays.  cycle, time, dt and set 0 equal
    the stepping loop, the last row history_device() of the recorded run, and the run is that of the stepping loop; a sample
    recorder beside the integral recorder leaves both series what they are alone"""
    A = blast_run
    assert not same_bits(A["set0"][0], A["set0"][-1]) and A["set0"][0, 0] > 0.0
    b = blast32()()
    bounds, nx = ric.sim_blocks(b)
    win = ric.seven_windows(bounds, nx)
    rec = b.record_integrals(windows=win)
    table = rec.window_zones()
    assert table.shape == (8, 7, 6) and np.array_equal(table, ric.zone_table(bounds, nx, win))
    assert b.uses_tuned_kernel and rec.rows == 0 and b.evolve(CYCLES) == CYCLES and rec.rows == CYCLES
    ts = rec.read()
    ric.same_series(ts, A)
    assert same_bits(ts.integrals[-1, 0], b.history_device()) and ts.nbody is None
    assert same_bits(ts.integrals[:, 1], ts.integrals[:, 0]) and same_bits(ts.integrals[:, 2], np.zeros_like(ts.integrals[:, 2]))
    assert rec.labels == ["gas_mass_0", "gas_momentum_x1_0", "gas_momentum_x2_0", "gas_momentum_x3_0", "gas_energy_0", "gas_internal_energy_0"]
    rc.same_run(b, A, "recorder")
    b.close()
    d = blast32()()
    pts = rc.probe_points(d)
    B = rc.stepping(blast32(), pts, rc.VARS, CYCLES)
    samples, both = d.record(pts, rc.VARS, capacity=2), d.record_integrals(capacity=3)
    assert d.evolve(CYCLES) == CYCLES
    rc.same_series(samples.read(), B, tag="samples beside integrals")
    ric.same_series(both.read(), A, tag="integrals beside samples")
    rc.same_run(d, A, "both kinds")
    d.close()


@pytest.mark.parametrize("variant", ["every2", "every3", "capacity2", "two_calls", "sync_loop", "no_graph"])
def test_variants(blast_run, variant):
    from artemis_amd import capi
    A = blast_run
    with (capi.option(variant) if variant in ("sync_loop", "no_graph") else contextlib.nullcontext()):
        b = blast32()()
        try:
            if variant in ("every2", "every3"):
                every = int(variant[-1])
                rec = b.record_integrals(every=every)
                assert b.evolve(CYCLES) == CYCLES
                ric.same_series(rec.read(), A, list(range(every - 1, CYCLES, every)))
            elif variant == "two_calls":
                rec = b.record_integrals(capacity=4)
                assert b.evolve(4) == 4
                ric.same_series(rec.read(clear=True), A, [0, 1, 2, 3])
                assert rec.rows == 0 and b.evolve(5) == 5 and rec.rows == 5
                ric.same_series(rec.read(), A, [4, 5, 6, 7, 8])
            else:  # capacity 2: drains inside the loop, between replays
                rec = b.record_integrals(capacity=2)
                assert b.evolve(CYCLES) == CYCLES
                ric.same_series(rec.read(), A, tag=variant)
            rc.same_run(b, A, variant)
        finally:
            b.close()


def test_run_that_ends_by_time(blast_run):
    """tlim between the 5th and the 6th cycle's time: batches far from tlim, one cycle at a time near it, the last step clamped"""
    tlim = 0.5 * (blast_run["time"][4] + blast_run["time"][5])
    make = blast32(["parthenon/time/tlim=%r" % float(tlim)])
    A = ric.stepping(make, CYCLES)
    assert len(A["cycle"]) == 6 and A["time"][-1] == tlim and A["time"][-2] < tlim
    b = make()
    rec = b.record_integrals()
    assert b.evolve() == 6
    ts = rec.read()
    ric.same_series(ts, A)
    assert ts.time[-1] == tlim
    rc.same_run(b, A)
    b.close()


@pytest.mark.parametrize("case", ["disk_cyl", "refined"])
def test_curvilinear_and_refined(hiplib, case):
    """set 0 against the stepping loop, and an annulus (a box in the mesh's own coordinates) against numpy within the bound"""
    from artemis_amd.driver import Simulation
    from test_fields_reduce import block_volumes
    from test_outputs import SUM_CASES
    deck, ov = SUM_CASES[case]
    make = lambda: Simulation(DECK(*deck), list(ov))  # noqa: E731
    A = ric.stepping(make, 3)
    assert len(A["cycle"]) == 3
    b = make()
    try:
        bounds, nx = ric.sim_blocks(b)
        lo, hi = bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)
        dx = np.array([(bounds[:, 2 * d + 1] - bounds[:, 2 * d]).min() / nx[d] for d in range(3)])
        ring = np.array([[[lo[0] + 3.25 * dx[0], hi[0] - 4.25 * dx[0]], [lo[1] - 1.0, hi[1] + 1.0], [lo[2] - 1.0, hi[2] + 1.0]]])
        rec = b.record_integrals(windows=ring, capacity=2)
        assert b.evolve(3) == 3
        ts = rec.read()
        ric.same_series(ts, A)
        table = rec.window_zones()
        assert np.array_equal(table, ric.zone_table(bounds, nx, ring))
        mask = ric.membership(bounds, nx, ring)[:, 0]
        vol = np.stack(block_volumes(b, "cylindrical" if case == "disk_cyl" else "cartesian"))
        want, S, n = ric.window_sums(ric.sim_terms(b, vol), mask)
        assert 0 < n < mask.size
        ric.within_bound(ts.integrals[-1, 1], want, S, n, case)
        rc.same_run(b, A, case)
    finally:
        b.close()


def test_adaptive_mesh(hiplib):
    """the refined cylindrical blast at 64^2 root zones, a forced split that merges again inside the run: set 0 follows the
    stepping loop across the remesh, the window of every zone keeps the bits of set 0 on every mesh, and window_zones()
    has the new block count afterwards"""
    from artemis_amd.driver import Simulation
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    make = lambda: Simulation(DECK(*c["deck"]), list(c["overrides"]))  # noqa: E731
    A = ric.stepping(make, 8, prepare=rc.split_a_coarsest_leaf)
    assert A["remeshes"] >= 1, "the case shows nothing: no remesh within 8 cycles"
    b = make()
    try:
        whole = np.array([[[-1e3, 1e3]] * 3])
        rec = b.record_integrals(windows=whole, capacity=3)
        n0 = b.nblocks
        assert rec.window_zones().shape == (n0, 1, 6)
        rc.split_a_coarsest_leaf(b)
        assert b.nblocks != n0 and rec.window_zones().shape == (b.nblocks, 1, 6)
        r0 = b.remeshes
        assert b.evolve(8) == 8 and b.remeshes - r0 == A["remeshes"]
        ts = rec.read()
        ric.same_series(ts, A)
        assert same_bits(ts.integrals[:, 1], ts.integrals[:, 0]) and rec.window_zones().shape == (b.nblocks, 1, 6)
        bounds, nx = ric.sim_blocks(b)
        assert np.array_equal(rec.window_zones(), ric.zone_table(bounds, nx, whole))
        rc.same_run(b, A)
    finally:
        b.close()


def test_window_across_remeshes(hiplib):
    """the same adaptive case: a proper window that strictly contains the leaf a forced split refines.  Its index ranges are
    rebuilt on every new mesh (compared with numpy after every cycle), and its mass moves across the split and across the
    merge by no more than the bound record_integrals_cases.window_across_remeshes derives from the two sums' term counts"""
    from artemis_amd.driver import Simulation
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    b = Simulation(DECK(*c["deck"]), list(c["overrides"]))
    try:
        assert ric.window_across_remeshes(b) >= 2  # the split and the merge
    finally:
        b.close()


NBODY_NX = (64, 32, 16)


def nbody_maker(path):
    from artemis_amd.driver import Simulation
    ov = ["parthenon/time/nlim=4"] + ["parthenon/mesh/nx%d=%d" % (d + 1, n) for d, n in enumerate(NBODY_NX)] + \
         ["parthenon/meshblock/nx%d=%d" % (d + 1, n) for d, n in enumerate(NBODY_NX)]
    for d in ("x1", "x3"):
        ov += ["parthenon/mesh/i%s_bc=ic" % d, "parthenon/mesh/o%s_bc=ic" % d]

    def make():
        s = Simulation(DECK("disk", "disk_nbody_cyl.in"), ov)
        s.set_path(path)
        return s
    return make


@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_nbody(hiplib, path):
    """row k of one recorded evolve(4) is nbody_force() called once after evolve(k) on a fresh run, k = 1 .. 4, bit for bit;
    nbody_force() after the recorded run is that of an unrecorded run: recording flushed nothing"""
    make = nbody_maker(path)
    want = []
    for k in range(1, 5):
        s = make()
        assert s.uses_fused_path == (path == "fused") and s.evolve(k) == k
        want.append(s.nbody_force())
        s.close()
    b = make()
    rec = b.record_integrals(nbody=True)
    assert b.evolve(4) == 4
    ts = rec.read()
    assert ts.nbody.shape == (4, 1, 7) and np.abs(ts.nbody).max() > 0.0 and not same_bits(ts.nbody[0], ts.nbody[3])
    for k in range(4):
        assert same_bits(ts.nbody[k], want[k]), (k, ts.nbody[k], want[k])
    assert same_bits(b.nbody_force(), want[3])
    b.close()


def test_labels_name_the_entries_an_hst_file_names(hiplib, tmp_path):
    """the advection deck with one gas and two dust species and an `hst` block that writes every cycle: rec.labels has the
    strings read_history yields (as a set: the file's columns are quantity-outermost, rec.labels follows the history_device
    layout, species-outermost), and entry i of set 0 is, bit for bit, the file's column named rec.labels[i] at the same cycle
    (the file holds 17 digits)"""
    from artemis_amd.driver import Simulation
    from artemis_amd.history import read_history
    from test_outputs import SUM_CASES
    deck, ov = SUM_CASES["advection"]
    b = Simulation(DECK(*deck), list(ov) + ["parthenon/time/nlim=3", "parthenon/output1/file_type=hst", "parthenon/output1/dt=1e-9"])
    try:
        assert (b.ns_gas, b.ns_dust) == (1, 2)
        rec = b.record_integrals()
        b.enable_outputs(tmp_path)
        assert b.evolve() == 3
        ts = rec.read()
        hst = read_history(os.path.join(tmp_path, "advection.out1.hst"))
        assert len(rec.labels) == 14 == len(set(rec.labels)) and set(rec.labels) == set(hst) - {"time", "dt", "cycle", "nbtotal"}
        assert rec.labels[6:10] == ["dust_mass_0", "dust_momentum_x1_0", "dust_momentum_x2_0", "dust_momentum_x3_0"]
        assert [k for k in hst if k.startswith("dust_mass")] == ["dust_mass_0", "dust_mass_1"]  # (the file's own order)
        rows = {int(c): r for r, c in enumerate(hst["cycle"])}
        for r, cycle in enumerate(ts.cycle):
            at = rows[int(cycle)]
            for i, name in enumerate(rec.labels):
                assert same_bits(np.array([hst[name][at]]), ts.integrals[r, 0, i:i + 1]), (int(cycle), i, name)
            assert hst["time"][at] == ts.time[r]
    finally:
        b.close()


def test_the_header_and_the_library_agree(hiplib):
    """every function include/artemis_hip_record.h declares is in capi.EXPORTS_HIP_RECORD and exported, and nothing else is"""
    import re
    from artemis_amd import capi
    text = open(os.path.join(ROOT, "include", "artemis_hip_record.h")).read()
    declared = sorted(set(re.findall(r"\b(artemis_hip_record_\w+)\s*\(", text)))
    assert declared == sorted(capi.EXPORTS_HIP_RECORD) and len(declared) == 3
    for name in declared:
        assert hasattr(hiplib, name), name


def test_lifetime_and_refusals(blast_run):
    b = blast32()()
    try:
        bounds, nx = ric.sim_blocks(b)
        win = ric.seven_windows(bounds, nx)
        for kw in (dict(every=0), dict(capacity=0), dict(windows=np.zeros((8, 3, 2)))):
            with pytest.raises(ValueError):
                b.record_integrals(**kw)
        bad = win[:1].copy()
        bad[0, 1] = [0.5, 0.5]  # lo >= hi along x2
        with pytest.raises(RuntimeError, match="lo < hi"):
            b.record_integrals(windows=bad)
        with pytest.raises(RuntimeError, match="without particles"):
            b.record_integrals(nbody=True)
        rec = b.record_integrals(windows=win[:2])
        assert rec.capacity == min(4096, (64 << 20) // (3 * 6 * 8))
        b.history_device(), b.gather(rc.VARS)  # nothing but evolve records
        assert rec.rows == 0 and b.evolve(2) == 2 and rec.rows == 2
        rec.close()
        for use in (lambda: rec.read(), lambda: rec.rows, lambda: rec.window_zones()):
            with pytest.raises(RuntimeError, match="closed"):
                use()
        rec.close()  # (closing twice is no error)
    finally:
        b.close()
