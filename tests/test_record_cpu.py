"""Time series of point samples -- Simulation.record (include/artemis_driver.h "a time series of samples") -- on the CPU test
double: no GPU.  The double defines neither record kernel, so csrc/driver/record.cpp counts the cycles itself and forms a row
with the host loop of plan.values; what is checked here is the driver: where in the time loop a row is taken (the batched
loop with the clock on the "device", the one-by-one loop near tlim, the forced synchronous loop, the adaptive loop after
its remesh check), which cycles are due, that no row is lost, and that the run is not disturbed.  The definition is the
stepping loop of tests/record_cases.py: evolve(1), then ncycle, time, dt and plan.values.  Every comparison is bitwise.  The
GPU cases, the kernels among them, are tests/test_record.py.

A one-rank case runs in a process of its own (`isolated`: this file as a script runs one `check_*` function), like the other
CPU suites; the rank case runs tests/record_worker.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
import record_cases as rc
from fields_sample_ref import same_bits
from test_fields_derived_cpu import blast3d
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CYCLES = 9
RUN = ["parthenon/time/tlim=-1.0", "parthenon/time/nlim=%d" % CYCLES]


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def isolated(check, *args):
    """run check(*args) (a function of this module, JSON-able arguments) in a fresh interpreter"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), check.__name__, json.dumps(args)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode()[-4000:]


def library():
    return C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))


def case_of(deck):
    return blast(nlim=CYCLES) if deck == "blast2d" else blast3d(True, nlim=CYCLES)


def maker(deck, extra=()):
    from artemis_amd.driver import Simulation
    case = case_of(deck)
    return lambda: Simulation(os.path.join(ROOT, "inputs", *case["deck"]), list(case["overrides"]) + RUN + list(extra), lib=library())


def points_of(make):
    sim = make()
    try:
        return rc.probe_points(sim)
    finally:
        sim.close()


def check_one_evolve_equals_the_stepping_loop(deck):
    """nine cycles in one evolve(9) with a recorder against nine evolve(1) + values: every array of read(), and the final state
    with a recorder, without one, and of the stepping loop"""
    make = maker(deck)
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.VARS, CYCLES)
    assert len(A["cycle"]) == CYCLES and np.array_equal(A["cycle"], np.arange(1, CYCLES + 1))
    assert np.isnan(A["values"][:, :, 256:258]).all() and not np.isnan(A["values"][:, :, :256]).any() and not np.isnan(A["values"][:, :, 258]).any()
    assert not same_bits(A["values"][0], A["values"][-1])  # (the series is not constant)
    c = make()
    assert c.evolve(CYCLES) == CYCLES
    rc.same_run(c, A, "no recorder")  # first: the stepping loop and one call agree without any recorder
    c.close()
    b = make()
    rec = b.record(pts, rc.VARS)
    assert rec.rows == 0 and b.evolve(CYCLES) == CYCLES and rec.rows == CYCLES
    rc.same_series(rec.read(), A)
    rc.same_run(b, A, "recorder")
    assert rec.rows == CYCLES  # (read() without clear keeps them)
    f = b.record(pts, rc.VARS, single=True)  # attached at the end of the run: no cycle follows, no row
    assert f.read().values.shape == (0, 4, len(pts)) and f.read().values.dtype == np.float32
    b.close()


def check_variants(deck, variant):
    """variants of the nine-cycle run, each against the rows of the stepping loop"""
    from artemis_amd.driver import Simulation  # noqa: F401
    make = maker(deck)
    pts = points_of(make)
    names = rc.DERIVED if variant == "derived" else rc.VARS
    single = variant == "single"
    A = rc.stepping(make, pts, names, CYCLES, single=single)
    b = make()
    try:
        if variant == "every2_capacity1":  # every row fills the buffer: the loop drains inside evolve
            rec = b.record(pts, names, every=2, capacity=1)
            assert b.evolve(CYCLES) == CYCLES
            rc.same_series(rec.read(), A, [1, 3, 5, 7])
        elif variant == "two_calls":
            rec = b.record(pts, names, capacity=4)
            assert b.evolve(4) == 4
            rc.same_series(rec.read(clear=True), A, [0, 1, 2, 3])
            assert rec.rows == 0 and b.evolve(5) == 5 and rec.rows == 5
            rc.same_series(rec.read(), A, [4, 5, 6, 7, 8])
        elif variant in ("derived", "single"):
            rec = b.record(pts, names, single=single)
            assert b.evolve(CYCLES) == CYCLES
            rc.same_series(rec.read(), A)
            if variant == "derived":
                assert np.any(A["values"][-1][4:, :256] != 0.0)  # (the vorticity is there)
        elif variant == "two_recorders":
            plan = b.sample_plan(pts)
            r1, r3 = b.record(plan, names, every=1, capacity=2), b.record(plan, names, every=3, capacity=2)
            assert b.evolve(CYCLES) == CYCLES
            rc.same_series(r1.read(), A, tag="every 1")
            rc.same_series(r3.read(), A, [2, 5, 8], tag="every 3")
        else:
            raise AssertionError(variant)
        rc.same_run(b, A, variant)
    finally:
        b.close()


def check_forced_paths(deck, option):
    """sync_loop: the loop that keeps the clock on the host; no_graph: the batched loop without captured graphs.  The run
    itself first (the option does not change its bits), then the rows"""
    make = maker(deck)
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.VARS, CYCLES)
    lib = library()
    assert lib.artemis_hip_set_option(option.encode(), 1) == 0
    c = make()
    assert c.evolve(CYCLES) == CYCLES
    rc.same_run(c, A, option + ", no recorder")
    c.close()
    b = make()
    rec = b.record(pts, rc.VARS, capacity=2)
    assert b.evolve(CYCLES) == CYCLES
    rc.same_series(rec.read(), A)
    rc.same_run(b, A, option)
    b.close()


def check_run_that_ends_by_time(deck):
    """tlim between the 5th and the 6th cycle's time: the batched loop far from tlim, then one cycle at a time, the last step
    clamped onto tlim"""
    free = rc.stepping(maker(deck), points_of(maker(deck)), rc.VARS, CYCLES)
    tlim = 0.5 * (free["time"][4] + free["time"][5])
    make = maker(deck, ["parthenon/time/tlim=%r" % float(tlim)])
    pts = points_of(make)
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


def check_lifetime(deck):
    from artemis_amd.driver import Recorder, SamplePlan, TimeSeries
    make = maker(deck)
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.VARS, 4, start=5)
    assert list(A["cycle"]) == [6, 7, 8, 9]
    b, other = make(), make()
    try:
        assert b.evolve(5) == 5
        plan = b.sample_plan(pts)
        rec = b.record(plan, rc.VARS, every=2)  # attached after 5 cycles: seen starts at 0, the first row is cycle 7
        assert isinstance(rec, Recorder) and isinstance(plan, SamplePlan) and rec.capacity == min(4096, (64 << 20) // (4 * len(pts) * 8))
        # nothing but evolve records
        b.gather(rc.VARS), plan.values(rc.VARS)
        assert rec.rows == 0
        empty, bare = b.record(np.empty((0, 3)), rc.VARS), b.record(pts, [])  # no points, no variables: the heads alone
        assert b.evolve(4) == 4
        for r, shape in ((empty, (4, 4, 0)), (bare, (4, 0, len(pts)))):
            got = r.read()
            assert got.values.shape == shape and np.array_equal(got.cycle, A["cycle"]) and same_bits(got.time, A["time"]) and same_bits(got.dt, A["dt"])
        ts = rec.read()
        assert isinstance(ts, TimeSeries)
        rc.same_series(ts, A, [1, 3])
        # a plan in use cannot be closed under the recorder
        assert b.L.artemis_sim_sample_plan_destroy(b.h, plan.id) != 0 and b"in use by a recorder" in b.L.artemis_sim_last_error()
        assert same_bits(plan.values(rc.VARS), A["values"][3])
        rec.close()
        for use in (lambda: rec.read(), lambda: rec.rows):
            with pytest.raises(RuntimeError, match="closed"):
                use()
        rec.close()  # (closing twice is no error)
        plan.close()
        with pytest.raises(RuntimeError, match="closed"):
            b.record(plan, rc.VARS)
        # a recorder that made its plan closes it
        own = b.record(pts, rc.VARS)
        own.close()
        with pytest.raises(RuntimeError, match="closed"):
            own.plan.values(rc.VARS)
        # refusals
        for kw in (dict(every=0), dict(every=-3), dict(capacity=0), dict(capacity=-1)):
            with pytest.raises(ValueError):
                b.record(pts, rc.VARS, **kw)
        foreign = other.sample_plan(pts)
        with pytest.raises(ValueError, match="another simulation"):
            b.record(foreign, rc.VARS)
        with pytest.raises(ValueError):
            b.record(pts.astype(np.float32), rc.VARS)
        with pytest.raises(RuntimeError, match="unknown variable dust.prim.density"):
            b.record(pts, ["gas.prim.density", "dust.prim.density"])
        assert b.L.artemis_sim_record_rows(b.h, 12345) == -1 and b"does not exist" in b.L.artemis_sim_last_error()
    finally:
        b.close(), other.close()


def check_adaptive():
    """the refined cylindrical blast: rows follow the remesh check of their cycle, the plan locates again on the new blocks,
    and the NaN pattern (the two points outside) stays"""
    from artemis_amd.driver import Simulation
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    make = lambda: Simulation(os.path.join(ROOT, "inputs", *c["deck"]), list(c["overrides"]), lib=library())  # noqa: E731
    pts = points_of(make)
    A = rc.stepping(make, pts, rc.DERIVED, 8, prepare=rc.split_a_coarsest_leaf)
    assert A["remeshes"] >= 1, "the case shows nothing: no remesh within 8 cycles"
    assert np.isnan(A["values"][:, :, 256:258]).all() and not np.isnan(A["values"][:, :, :256]).any()
    b = make()
    try:
        rc.split_a_coarsest_leaf(b)
        r0 = b.remeshes
        rec, half = b.record(pts, rc.DERIVED, capacity=3), b.record(pts, rc.VARS, every=4)
        assert b.evolve(8) == 8 and b.remeshes - r0 == A["remeshes"]
        rc.same_series(rec.read(), A)
        got = half.read()
        assert np.array_equal(got.cycle, [4, 8]) and same_bits(got.values, A["values"][[3, 7]][:, :4])
        rc.same_run(b, A)
    finally:
        b.close()


def run_ranks(world, case, points, tmp_path, tag):
    """tests/record_worker.py on `world` ranks; returns what each rank left"""
    out = str(tmp_path / tag)
    np.save(out + ".points.npy", points)
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]) + RUN, cycles=CYCLES, variables=rc.DERIVED, every=2, capacity=2, out=out)
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "record_worker.py"), json.dumps(spec)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        rendezvous = any(p.returncode != 0 and ("Address already in use" in o or "Connection re" in o or "timed out" in o.lower()
                                                or "terminate called without an active exception" in o)
                         for p, o in zip(procs, outs))
        if not (rendezvous and attempt == 0):
            break
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [dict(np.load(out + ".rank%d.npz" % r)) for r in range(world)]


def test_two_ranks_record_their_own_blocks(tmp_path):
    """a gloo world of two ranks: for every row and point exactly one rank has a value, the one-rank run's; cycle, time and dt
    are the same on both ranks"""
    case = blast3d(True, nlim=CYCLES)
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    from artemis_amd import sample as smp
    pts = np.concatenate([smp.lattice((lo[0], lo[1], 0.06), (hi[0], hi[1], 0.06), (16, 16, 1)), np.array([hi, 0.5 * (lo + hi), lo])])
    one = run_ranks(1, case, pts, tmp_path, "one")[0]
    two = run_ranks(2, case, pts, tmp_path, "two")
    assert np.array_equal(one["cycle"], [2, 4, 6, 8]) and not np.isnan(one["values"]).any() and one["values"].shape == (4, 7, len(pts))
    found = np.stack([~np.isnan(r["values"]) for r in two])
    assert (found.sum(axis=0) == 1).all() and found[0].any() and found[1].any()
    union = np.where(found[0], two[0]["values"], two[1]["values"])
    assert same_bits(union, one["values"])
    for r in two:
        assert np.array_equal(r["cycle"], one["cycle"]) and same_bits(r["time"], one["time"]) and same_bits(r["dt"], one["dt"])
        assert (np.isnan(r["values"]).all(axis=1) == np.isnan(r["values"]).any(axis=1)).all()  # a point is a rank's in every component


DECKS = ["blast2d", "blast3d"]


@pytest.mark.parametrize("deck", DECKS)
def test_one_evolve_equals_the_stepping_loop(deck):
    isolated(check_one_evolve_equals_the_stepping_loop, deck)


@pytest.mark.parametrize("variant", ["every2_capacity1", "two_calls", "derived", "single", "two_recorders"])
@pytest.mark.parametrize("deck", DECKS)
def test_variants(deck, variant):
    isolated(check_variants, deck, variant)


@pytest.mark.parametrize("option", ["sync_loop", "no_graph"])
@pytest.mark.parametrize("deck", DECKS)
def test_forced_paths(deck, option):
    isolated(check_forced_paths, deck, option)


@pytest.mark.parametrize("deck", DECKS)
def test_run_that_ends_by_time(deck):
    isolated(check_run_that_ends_by_time, deck)


@pytest.mark.parametrize("deck", DECKS)
def test_lifetime(deck):
    isolated(check_lifetime, deck)


def test_adaptive():
    isolated(check_adaptive)


if __name__ == "__main__":
    globals()[sys.argv[1]](*json.loads(sys.argv[2]))
