"""GPU tests of the time series of point samples (include/artemis_hip_sample.h: artemis_hip_record_tick and
artemis_hip_record_samples; include/artemis_driver.h: artemis_sim_record_*; Simulation.record).  Only repository code runs here.

The kernels on packs with random primitives in every zone: the rows a recorder's buffers hold equal what
artemis_hip_sample_fields returns at the cycles that were due, the heads are the clock that was passed -- from device memory
and by value -- a due row that finds the buffers full is counted and written nowhere, and nothing behind the buffers is
touched.  The driver against the stepping loop of tests/record_cases.py -- evolve(1), then ncycle, time, dt and plan.values
-- through the plain steps, the captured graphs and their replays, the drains, the one-by-one loop near tlim, the forced
synchronous loop, refined and adaptive meshes.  Every comparison is bitwise."""
import ctypes as C
import os

import numpy as np
import pytest

import amr_cases
import fields_sample_ref as ref
import record_cases as rc
from fields_sample_ref import same_bits
from test_fields import BLAST32
from test_fields_derived import code_of
from test_fields_sample import NG, codes_of, device_sample, make_pack, ncomp_of_codes, pack_points, payload_nan, sorted_order

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)
CANARY = 64


# ---- the kernels on packs -----------------------------------------------------------------------------------------------
def tick(mb, ctl, head, tstate, time, dt, every, capacity):
    return mb.L.artemis_hip_record_tick(C.c_void_p(ctl.data_ptr()) if ctl is not None else None, C.c_void_p(head.data_ptr()) if head is not None else None,
                                        C.c_void_p(tstate.data_ptr()) if tstate is not None else None, time, dt, every, capacity, mb._stream())


def record(mb, n, ld, od, codes, single, ctl, capacity, rows, nsel=None):
    sel = (C.c_int * max(len(codes), 1))(*[code_of(c) for c in codes])
    return mb.L.artemis_hip_record_samples(C.byref(mb.pack), n, C.c_void_p(ld.data_ptr()), C.c_void_p(od.data_ptr()) if od is not None else None,
                                           len(codes) if nsel is None else nsel, sel, int(single), C.c_void_p(ctl.data_ptr()) if ctl is not None else None,
                                           capacity, C.c_void_p(rows.data_ptr()) if rows is not None else None, mb._stream())


def clock_of(call):
    return 0.125 * call + 1.0 / 3.0, 0.1 / (call + 2.0)


@pytest.mark.parametrize("clock", ["device_clock", "by_value"])
@pytest.mark.parametrize("derived", [False, True], ids=["plain", "derived"])
@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", ["cart3d", "three", "cyl3d", "sph3d", "mixed3d"])
def test_rows_are_the_samples_of_the_due_cycles(hiplib, name, single, derived, clock):
    """tick and record nine times with every = 3 and capacity = 2, a few primitives changed before each call: rows 0 and 1
    are artemis_hip_sample_fields at calls 3 and 6 and their heads the clock of those calls; the third due row (call 9) is
    dropped, counted, and leaves the canary behind the rows untouched"""
    import torch
    mb, bounds, lo, hi = make_pack(name)
    pts = pack_points(name, bounds, mb.nx, lo, hi)
    n = len(pts)
    assert n % 64 != 0
    loc = ref.locate(pts, bounds, mb.nx, NG, hi)
    assert (loc[:, 0] < 0).any() and (loc[:, 0] >= 0).sum() > 64
    order = sorted_order(loc)
    codes = [c for c in codes_of(mb.nsd) if derived or c < 16]
    ncomp = ncomp_of_codes(mb, codes)
    every, capacity, cycle0 = 3, 2, 100
    ld, od = torch.from_numpy(loc.reshape(-1).copy()).to(mb.dev), torch.from_numpy(order).to(mb.dev)
    ctl = torch.tensor([0, cycle0, 0, -1, 0], dtype=torch.int64, device=mb.dev)
    head = torch.zeros(3 * capacity + 3, dtype=torch.float64, device=mb.dev)
    rows = payload_nan(capacity * ncomp * n + CANARY, single, mb.dev)
    before = rows.cpu().numpy().copy()
    tstate = torch.zeros(6, dtype=torch.float64, device=mb.dev)
    rng = np.random.default_rng(5)
    want, slots = {}, []
    for call in range(1, 10):
        for prim in (mb.gas_prim, mb.dust_prim):  # a few primitives, ghost zones included
            flat = prim.view(-1)
            if flat.numel():
                at = torch.from_numpy(rng.integers(0, flat.numel(), size=257)).to(mb.dev)
                flat[at] = flat[at] * 1.03125 + 0.015625 * call
        t, dt = clock_of(call)
        if clock == "device_clock":
            tstate.copy_(torch.tensor([t, dt, 7.0, 8.0, 9.0, 10.0], dtype=torch.float64))
            assert tick(mb, ctl, head, tstate, -1.0, -1.0, every, capacity) == 0
        else:
            assert tick(mb, ctl, head, None, t, dt, every, capacity) == 0
        assert record(mb, n, ld, od, codes, single, ctl, capacity, rows) == 0, mb.L.artemis_hip_last_error()
        torch.cuda.synchronize()
        slots.append(int(ctl[3].item()))
        if call % every == 0:
            want[call] = device_sample(mb, loc, codes, single, order)
    assert slots == [-1, -1, 0, -1, -1, 1, -1, -1, -1]
    assert ctl.cpu().tolist() == [9, cycle0 + 9, 2, -1, 1]  # seen, cycle, rows, slot, dropped
    raw = rows.cpu().numpy()
    assert np.array_equal(raw[capacity * ncomp * n:], before[capacity * ncomp * n:])  # the canary
    got = raw[:capacity * ncomp * n].view(np.float32 if single else np.float64).reshape(capacity, ncomp, n)
    assert same_bits(got[0], want[3]) and same_bits(got[1], want[6]) and not same_bits(want[3], want[6])
    assert np.isnan(got[0][:, loc[:, 0] < 0]).all() and not np.isnan(got[0][:, loc[:, 0] >= 0]).any()
    h = head.cpu().numpy()
    assert np.array_equal(h[:6].view(np.int64)[[0, 3]], [cycle0 + 3, cycle0 + 6])
    assert same_bits(h[[1, 2, 4, 5]], np.array(clock_of(3) + clock_of(6))) and (h[6:] == 0.0).all()


def test_no_points_and_refusals(hiplib):
    """npoints = 0 still ticks and writes the head; what the two entry points refuse leaves every buffer as it was"""
    import torch
    from artemis_amd import capi
    mb, bounds, lo, hi = make_pack("sph3d")
    pts = pack_points("sph3d", bounds, mb.nx, lo, hi)
    loc = ref.locate(pts, bounds, mb.nx, NG, hi)
    n = len(pts)
    ld = torch.from_numpy(loc.reshape(-1).copy()).to(mb.dev)
    ctl = torch.tensor([0, 41, 0, -1, 0], dtype=torch.int64, device=mb.dev)
    head = torch.zeros(6, dtype=torch.float64, device=mb.dev)
    rows = payload_nan(2 * n + CANARY, False, mb.dev)
    before = rows.cpu().numpy().copy()
    assert tick(mb, ctl, head, None, 0.5, 0.25, 1, 2) == 0 and record(mb, 0, ld, None, [0], False, ctl, 2, rows) == 0
    assert record(mb, n, ld, None, [], False, ctl, 2, rows) == 0  # no components
    torch.cuda.synchronize()
    assert ctl.cpu().tolist() == [1, 42, 1, 0, 0] and np.array_equal(rows.cpu().numpy(), before)
    h = head.cpu().numpy()
    assert h[:1].view(np.int64)[0] == 42 and h[1] == 0.5 and h[2] == 0.25
    state = ctl.cpu().tolist()
    for bad in (lambda: tick(mb, ctl, head, None, 0.0, 0.0, 0, 2), lambda: tick(mb, ctl, head, None, 0.0, 0.0, 1, 0),
                lambda: tick(mb, None, head, None, 0.0, 0.0, 1, 2), lambda: tick(mb, ctl, None, None, 0.0, 0.0, 1, 2),
                lambda: record(mb, n, ld, None, [0], False, ctl, 0, rows), lambda: record(mb, n, ld, None, [0], False, None, 2, rows),
                lambda: record(mb, n, ld, None, [0], False, ctl, 2, None), lambda: record(mb, -1, ld, None, [0], False, ctl, 2, rows),
                lambda: record(mb, n, ld, None, [0, 1000], False, ctl, 2, rows), lambda: record(mb, n, ld, None, [0, 8], False, ctl, 2, rows),
                lambda: record(mb, n, ld, None, [0], False, ctl, 2, rows, nsel=33)):
        assert bad() == capi.EINVAL
    torch.cuda.synchronize()
    assert ctl.cpu().tolist() == state and np.array_equal(rows.cpu().numpy(), before)


# ---- the driver, against the stepping loop ------------------------------------------------------------------------------
CYCLES = 9
RUN = BLAST32 + ["parthenon/time/tlim=-1.0", "parthenon/time/nlim=%d" % CYCLES]


def blast32(extra=()):
    from artemis_amd.driver import Simulation
    return lambda: Simulation(DECK("blast", "blast.in"), RUN + list(extra))


def points_of(make):
    sim = make()
    try:
        return rc.probe_points(sim)
    finally:
        sim.close()


@pytest.fixture(scope="module")
def blast_runs(hiplib):
    """the stepping loop of the 32^3 blast (2 x 2 x 2 blocks of 16^3, nine cycles), made once per kind, shared, never modified"""
    pts = points_of(blast32())
    cache = {}

    def get(kind="plain"):
        if kind not in cache:
            names = rc.DERIVED if kind == "derived" else rc.VARS
            cache[kind] = rc.stepping(blast32(), pts, names, CYCLES, single=(kind == "single"))
            assert np.array_equal(cache[kind]["cycle"], np.arange(1, CYCLES + 1))
        return cache[kind]
    return pts, get


def test_one_evolve_equals_the_stepping_loop(blast_runs):
    """nine cycles in one evolve(9): three plain steps, one capture per ping-pong phase, replays.  read() equals the stepping
    loop in every array, and the final state is that of the stepping loop and of a run without a recorder"""
    pts, get = blast_runs
    A = get()
    assert np.isnan(A["values"][:, :, 256:258]).all() and not np.isnan(A["values"][:, :, :256]).any() and not np.isnan(A["values"][:, :, 258]).any()
    assert not same_bits(A["values"][0], A["values"][-1])
    c = blast32()()
    assert c.uses_tuned_kernel and c.nblocks == 8 and c.evolve(CYCLES) == CYCLES
    rc.same_run(c, A, "no recorder")  # first: without any recorder the two loops agree
    c.close()
    b = blast32()()
    rec = b.record(pts, rc.VARS)
    assert rec.rows == 0 and b.evolve(CYCLES) == CYCLES and rec.rows == CYCLES
    rc.same_series(rec.read(), A)
    rc.same_run(b, A, "recorder")
    b.close()


@pytest.mark.parametrize("variant", ["every2_capacity1", "two_calls", "derived", "single", "two_recorders", "sync_loop", "no_graph"])
def test_variants(blast_runs, variant):
    from artemis_amd import capi
    import contextlib
    pts, get = blast_runs
    kind = variant if variant in ("derived", "single") else "plain"
    names, single, A = (rc.DERIVED if kind == "derived" else rc.VARS), kind == "single", get(kind)
    with (capi.option(variant) if variant in ("sync_loop", "no_graph") else contextlib.nullcontext()):
        if variant in ("sync_loop", "no_graph"):  # the option does not change the run's bits
            c = blast32()()
            assert c.evolve(CYCLES) == CYCLES
            rc.same_run(c, A, variant + ", no recorder")
            c.close()
        b = blast32()()
        try:
            if variant == "every2_capacity1":  # every row fills the buffer: drains inside evolve, between replays
                rec = b.record(pts, names, every=2, capacity=1)
                assert b.evolve(CYCLES) == CYCLES
                rc.same_series(rec.read(), A, [1, 3, 5, 7])
            elif variant == "two_calls":
                rec = b.record(pts, names, capacity=4)
                assert b.evolve(4) == 4
                rc.same_series(rec.read(clear=True), A, [0, 1, 2, 3])
                assert rec.rows == 0 and b.evolve(5) == 5 and rec.rows == 5
                rc.same_series(rec.read(), A, [4, 5, 6, 7, 8])
            elif variant == "two_recorders":
                plan = b.sample_plan(pts)
                r1, r3 = b.record(plan, names, every=1, capacity=2), b.record(plan, names, every=3, capacity=2)
                assert b.evolve(CYCLES) == CYCLES
                rc.same_series(r1.read(), A, tag="every 1")
                rc.same_series(r3.read(), A, [2, 5, 8], tag="every 3")
            else:
                rec = b.record(pts, names, single=single, capacity=2 if variant in ("sync_loop", "no_graph") else None)
                assert b.evolve(CYCLES) == CYCLES
                rc.same_series(rec.read(), A, tag=variant)
                if variant == "derived":
                    assert np.any(A["values"][-1][4:, :256] != 0.0)
            rc.same_run(b, A, variant)
        finally:
            b.close()


def test_run_that_ends_by_time(blast_runs):
    """tlim between the 5th and the 6th cycle's time: batches far from tlim, one cycle at a time near it, the last step clamped"""
    pts, get = blast_runs
    free = get()
    tlim = 0.5 * (free["time"][4] + free["time"][5])
    make = blast32(["parthenon/time/tlim=%r" % float(tlim)])
    A = rc.stepping(make, pts, rc.VARS, CYCLES)
    assert len(A["cycle"]) == 6 and A["time"][-1] == tlim and A["time"][-2] < tlim
    c = make()
    assert c.evolve() == 6
    rc.same_run(c, A, "no recorder")
    c.close()
    b = make()
    rec = b.record(pts, rc.VARS)
    assert b.evolve() == 6
    ts = rec.read()
    rc.same_series(ts, A)
    assert ts.time[-1] == tlim
    rc.same_run(b, A)
    b.close()


def test_adaptive_mesh_rows_follow_the_remesh(hiplib):
    """the refined cylindrical blast at 64^2 root zones, a forced split that merges again inside the run: the rows equal the
    stepping loop across the remesh, the NaN pattern included"""
    from artemis_amd.driver import Simulation
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    make = lambda: Simulation(DECK(*c["deck"]), list(c["overrides"]))  # noqa: E731
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.DERIVED, 8, prepare=rc.split_a_coarsest_leaf)
    assert A["remeshes"] >= 1, "the case shows nothing: no remesh within 8 cycles"
    assert np.isnan(A["values"][:, :, 256:258]).all() and not np.isnan(A["values"][:, :, :256]).any()
    b = make()
    try:
        rc.split_a_coarsest_leaf(b)
        r0 = b.remeshes
        rec = b.record(pts, rc.DERIVED, capacity=3)
        assert b.evolve(8) == 8 and b.remeshes - r0 == A["remeshes"]
        rc.same_series(rec.read(), A)
        rc.same_run(b, A)
    finally:
        b.close()


def test_statically_refined_spherical_wedge(hiplib):
    """tests/test_multilevel.py's spherical wedge with a refined region: the fused multilevel step, the loop that keeps the
    clock on the host"""
    from artemis_amd.driver import Simulation
    from test_multilevel import CASES
    make = lambda: Simulation(DECK(*CASES["sph3d"]["deck"]), list(CASES["sph3d"]["ov"]))  # noqa: E731
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.DERIVED, 6)
    assert len(A["cycle"]) == 6 and np.isnan(A["values"][:, :, 256:258]).all() and not np.isnan(A["values"][:, :, :256]).any()
    b = make()
    try:
        assert b.uses_fused_path and len({b.block_level(q) for q in range(b.nblocks)}) == 2
        rec = b.record(pts, rc.DERIVED, every=2, capacity=2)
        assert b.evolve() == 6
        rc.same_series(rec.read(), A, [1, 3, 5])
        rc.same_run(b, A)
    finally:
        b.close()


def test_lifetime(blast_runs):
    """a plan in use cannot be closed; close() then read raises; a recorder attached after five cycles starts seen at 0 and
    its first row is cycle 6; refusals"""
    pts, get = blast_runs
    A = get()
    b, other = blast32()(), blast32()()
    try:
        assert b.evolve(5) == 5
        plan = b.sample_plan(pts)
        rec = b.record(plan, rc.VARS, every=2)
        assert rec.capacity == min(4096, (64 << 20) // (4 * len(pts) * 8))
        b.gather(rc.VARS), plan.values(rc.VARS)  # nothing but evolve records
        assert rec.rows == 0
        every1 = b.record(plan, rc.VARS)
        assert b.evolve(4) == 4
        rc.same_series(every1.read(), A, [5, 6, 7, 8])
        rc.same_series(rec.read(), A, [6, 8])  # seen = 2 and 4: cycles 7 and 9
        assert b.L.artemis_sim_sample_plan_destroy(b.h, plan.id) != 0 and b"in use by a recorder" in b.L.artemis_sim_last_error()
        rec.close(), every1.close()
        for use in (lambda: rec.read(), lambda: rec.rows):
            with pytest.raises(RuntimeError, match="closed"):
                use()
        plan.close()
        for kw in (dict(every=0), dict(capacity=0)):
            with pytest.raises(ValueError):
                b.record(pts, rc.VARS, **kw)
        with pytest.raises(ValueError, match="another simulation"):
            b.record(other.sample_plan(pts), rc.VARS)
        with pytest.raises(RuntimeError, match="unknown variable"):
            b.record(pts, ["gas.prim.density", "dust.prim.density"])
        rc.same_run(b, A)
    finally:
        b.close(), other.close()
