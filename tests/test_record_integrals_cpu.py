"""Time series of the history integrals and of the n-body force sums -- Simulation.record_integrals (include/artemis_driver.h
"a time series of the history integrals") -- on the CPU test double: no GPU.  The double defines none of the recorder
kernels, so csrc/driver/record.cpp counts the cycles itself and forms a row on the host: the rank-local host sum behind
history_device() restricted by the windows' index ranges, and the host's force rows plus a download of the accumulators.
What is checked here is the driver: where in the time loop a row is taken, which cycles are due, the index ranges of the
windows, that no row is lost and that the run is not disturbed.  The definition is the stepping loop of
tests/record_integrals_cases.py: evolve(1), then ncycle, time, dt and history_device(); set 0 is compared bitwise.  The GPU
cases, the kernels among them, are tests/test_record_integrals.py.

A one-rank case runs in a process of its own (`isolated`), like the other CPU suites; the rank case runs
tests/record_integrals_worker.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
import record_cases as rc
import record_integrals_cases as ric
from fields_sample_ref import same_bits
from test_fields_derived_cpu import blast3d
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CYCLES = 9
RUN = ["parthenon/time/tlim=-1.0", "parthenon/time/nlim=%d" % CYCLES]
NBODY_DECK = os.path.join(ROOT, "inputs", "disk", "disk_nbody_cyl.in")


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


def windows_of(make):
    sim = make()
    try:
        bounds, nx = ric.sim_blocks(sim)
        return ric.seven_windows(bounds, nx), bounds, nx
    finally:
        sim.close()


def check_one_evolve_equals_the_stepping_loop(deck):
    """nine cycles in one evolve(9) with an integral recorder against nine evolve(1) + history_device(); the window that holds
    every zone has the bits of set 0, the empty one is +0.0; the index ranges are the numpy membership; a sample recorder
    beside it changes neither series"""
    make = maker(deck)
    win, bounds, nx = windows_of(make)
    A = ric.stepping(make, CYCLES)
    assert len(A["cycle"]) == CYCLES and np.array_equal(A["cycle"], np.arange(1, CYCLES + 1))
    assert not same_bits(A["set0"][0], A["set0"][-1]) and A["set0"][0, 0] > 0.0
    c = make()
    assert c.evolve(CYCLES) == CYCLES
    rc.same_run(c, A, "no recorder")
    c.close()
    b = make()
    rec = b.record_integrals(windows=win)
    assert rec.labels[:6] == ["gas_mass_0", "gas_momentum_x1_0", "gas_momentum_x2_0", "gas_momentum_x3_0", "gas_energy_0", "gas_internal_energy_0"]
    table = rec.window_zones()
    assert table.shape == (b.nblocks, 7, 6) and np.array_equal(table, ric.zone_table(bounds, nx, win))
    assert np.array_equal(ric.mask_of_table(table, nx), ric.membership(bounds, nx, win))
    assert rec.rows == 0 and b.evolve(CYCLES) == CYCLES and rec.rows == CYCLES
    ts = rec.read()
    ric.same_series(ts, A)
    assert ts.nbody is None and ts.integrals.shape == (CYCLES, 8, len(rec.labels))
    assert same_bits(ts.integrals[-1, 0], b.history_device())
    assert same_bits(ts.integrals[:, 1], ts.integrals[:, 0])  # (a) every zone
    assert same_bits(ts.integrals[:, 2], np.zeros_like(ts.integrals[:, 2]))  # (b) no zone: +0.0
    # the other windows against a float64 numpy sum of the final state's terms, within the derived bound
    mask = ric.membership(bounds, nx, win)
    w = [(bounds[:, 2 * d + 1] - bounds[:, 2 * d]) / nx[d] for d in range(3)]  # Cartesian decks: the volume is dx1 dx2 dx3
    vol = np.broadcast_to((w[0] * w[1] * w[2])[:, None, None, None], mask[:, 0].shape)
    terms = ric.sim_terms(b, vol)
    for w_ in range(2, 7):
        want, S, n = ric.window_sums(terms, mask[:, w_])
        assert n > 0
        ric.within_bound(ts.integrals[-1, 1 + w_], want, S, n, "window %d" % w_)
    rc.same_run(b, A, "recorder")
    b.close()
    # a sample recorder beside it
    d = make()
    pts = rc.probe_points(d)
    B = rc.stepping(make, pts, rc.VARS, CYCLES)
    samples, integrals = d.record(pts, rc.VARS, capacity=2), d.record_integrals(capacity=3)
    assert d.evolve(CYCLES) == CYCLES
    rc.same_series(samples.read(), B)
    ric.same_series(integrals.read(), A)
    rc.same_run(d, A, "both kinds")
    d.close()


def check_variants(deck, variant):
    make = maker(deck)
    A = ric.stepping(make, CYCLES)
    lib = library()
    if variant in ("sync_loop", "no_graph"):
        assert lib.artemis_hip_set_option(variant.encode(), 1) == 0
    b = make()
    try:
        if variant in ("every2", "every3"):
            every = int(variant[-1])
            rec = b.record_integrals(every=every)
            assert b.evolve(CYCLES) == CYCLES
            ric.same_series(rec.read(), A, list(range(every - 1, CYCLES, every)))
        elif variant == "capacity2":
            rec = b.record_integrals(capacity=2)
            assert b.evolve(CYCLES) == CYCLES
            ric.same_series(rec.read(), A)
        elif variant == "two_calls":
            rec = b.record_integrals(capacity=4)
            assert b.evolve(4) == 4
            ric.same_series(rec.read(clear=True), A, [0, 1, 2, 3])
            assert rec.rows == 0 and b.evolve(5) == 5 and rec.rows == 5
            ric.same_series(rec.read(), A, [4, 5, 6, 7, 8])
        elif variant in ("sync_loop", "no_graph"):
            rec = b.record_integrals(capacity=2)
            assert b.evolve(CYCLES) == CYCLES
            ric.same_series(rec.read(), A, tag=variant)
        else:
            raise AssertionError(variant)
        rc.same_run(b, A, variant)
    finally:
        b.close()


def check_run_that_ends_by_time(deck):
    free = ric.stepping(maker(deck), CYCLES)
    tlim = 0.5 * (free["time"][4] + free["time"][5])
    make = maker(deck, ["parthenon/time/tlim=%r" % float(tlim)])
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


def check_lifetime(deck):
    make = maker(deck)
    win, _, _ = windows_of(make)
    b = make()
    try:
        for kw in (dict(every=0), dict(capacity=0), dict(windows=np.zeros((8, 3, 2))), dict(windows=np.zeros((2, 3)))):
            with pytest.raises(ValueError):
                b.record_integrals(**kw)
        bad = win[:1].copy()
        bad[0, 0] = [0.25, 0.25]  # lo >= hi along x1
        with pytest.raises(RuntimeError, match="lo < hi"):
            b.record_integrals(windows=bad)
        with pytest.raises(RuntimeError, match="without particles"):
            b.record_integrals(nbody=True)
        rec = b.record_integrals(windows=win[:2])
        assert rec.capacity == min(4096, (64 << 20) // (3 * len(rec.labels) * 8))
        b.history_device(), b.gather(rc.VARS)  # nothing but evolve records
        assert rec.rows == 0 and b.evolve(2) == 2 and rec.rows == 2
        assert b.L.artemis_sim_record_read(b.h, rec.id, None, None, None, None, 0) == -1 and b"records integrals" in b.L.artemis_sim_last_error()
        rec.close()
        for use in (lambda: rec.read(), lambda: rec.rows, lambda: rec.window_zones()):
            with pytest.raises(RuntimeError, match="closed"):
                use()
        rec.close()  # (closing twice is no error)
    finally:
        b.close()


def check_adaptive():
    """the refined cylindrical blast: set 0 follows the stepping loop across the remesh, window_zones() has the new block
    count afterwards, and the mass inside a proper window that only sees blocks split or merged moves within the bound
    record_integrals_cases.window_across_remeshes derives (the index ranges compared with numpy on every mesh)"""
    from artemis_amd.driver import Simulation
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    make = lambda: Simulation(os.path.join(ROOT, "inputs", *c["deck"]), list(c["overrides"]), lib=library())  # noqa: E731
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
        assert same_bits(ts.integrals[:, 1], ts.integrals[:, 0])
        assert rec.window_zones().shape == (b.nblocks, 1, 6)
        rc.same_run(b, A)
    finally:
        b.close()
    # a proper window about the leaf that is split: its ranges on every new mesh, its mass across the split and the merge
    w = make()
    try:
        assert ric.window_across_remeshes(w) >= 2
    finally:
        w.close()


def nbody_maker(path=None):
    from artemis_amd.driver import Simulation
    nx = (16, 8, 4)
    ov = ["parthenon/time/nlim=4"] + ["parthenon/mesh/nx%d=%d" % (d + 1, n) for d, n in enumerate(nx)] + \
         ["parthenon/meshblock/nx%d=%d" % (d + 1, n) for d, n in enumerate(nx)]
    for d in ("x1", "x3"):
        ov += ["parthenon/mesh/i%s_bc=ic" % d, "parthenon/mesh/o%s_bc=ic" % d]

    def make():
        s = Simulation(NBODY_DECK, ov, lib=library())
        if path:
            s.set_path(path)
        return s
    return make


def check_nbody(path):
    """row k of one recorded evolve(4) is nbody_force() called once after evolve(k) on a fresh run; recording flushes nothing"""
    make = nbody_maker(path or None)
    want = []
    for k in range(1, 5):
        s = make()
        assert s.evolve(k) == k
        want.append(s.nbody_force())
        s.close()
    plain = make()
    assert plain.evolve(4) == 4
    b = make()
    rec = b.record_integrals(nbody=True)
    assert b.evolve(4) == 4
    ts = rec.read()
    assert ts.nbody.shape == (4, 1, 7) and np.abs(ts.nbody).max() > 0.0
    for k in range(4):
        assert same_bits(ts.nbody[k], want[k]), (k, ts.nbody[k], want[k])
    assert same_bits(b.nbody_force(), plain.nbody_force()) and same_bits(b.nbody_force(), want[3])
    b.close(), plain.close()


def run_ranks(world, case, windows, tmp_path, tag):
    """tests/record_integrals_worker.py on `world` ranks; returns what each rank left"""
    out = str(tmp_path / tag)
    np.save(out + ".windows.npy", windows)
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]) + RUN, cycles=CYCLES, every=2, capacity=2, out=out)
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "record_integrals_worker.py"), json.dumps(spec)],
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


def test_two_ranks_integrate_their_own_blocks(tmp_path):
    """a gloo world of two ranks: every rank's set 0 is finite and positive in mass, and the two ranks' rows, added in rank
    order, are within the derived bound of the one-rank series: the same zones' terms in another order, so 2 gamma_{n-1} S
    with n the zones of the mesh"""
    case = blast3d(True, nlim=CYCLES)
    whole = np.array([[[-1e3, 1e3]] * 3])
    one = run_ranks(1, case, whole, tmp_path, "one")[0]
    two = run_ranks(2, case, whole, tmp_path, "two")
    assert np.array_equal(one["cycle"], [2, 4, 6, 8])
    total = np.zeros_like(one["integrals"])
    for r in two:
        assert np.array_equal(r["cycle"], one["cycle"]) and same_bits(r["time"], one["time"]) and same_bits(r["dt"], one["dt"])
        assert np.isfinite(r["integrals"]).all() and (r["integrals"][:, 0, 0] > 0.0).all()
        assert int(r["zones"]) < int(one["zones"])
        total = total + r["integrals"]
    assert sum(int(r["zones"]) for r in two) == int(one["zones"])
    n = int(one["zones"])
    # S per row from the row itself: mass and the energies have positive terms; for a momentum sum|rho v| vol <=
    # sqrt(sum rho vol * sum rho v^2 vol) <= sqrt(2 M E) (Cauchy-Schwarz)
    S = np.abs(one["integrals"]).copy()
    M, E = one["integrals"][..., 0], one["integrals"][..., 4]
    for d in range(3):
        S[..., 1 + d] = np.sqrt(2.0 * M * E) * (1.0 + 1e-12)
    bound = 2.0 * ric.gamma(n - 1) * S
    err = np.abs(total - one["integrals"])
    print("two ranks: max err / bound", np.max(err / np.where(bound > 0, bound, 1.0)))
    assert one["integrals"].shape[2] == 6 and np.all(err <= bound), (err, bound)


DECKS = ["blast2d", "blast3d"]


@pytest.mark.parametrize("deck", DECKS)
def test_one_evolve_equals_the_stepping_loop(deck):
    isolated(check_one_evolve_equals_the_stepping_loop, deck)


@pytest.mark.parametrize("variant", ["every2", "every3", "capacity2", "two_calls", "sync_loop", "no_graph"])
def test_variants(variant):
    isolated(check_variants, "blast3d", variant)


def test_run_that_ends_by_time():
    isolated(check_run_that_ends_by_time, "blast3d")


def test_lifetime():
    isolated(check_lifetime, "blast2d")


def test_adaptive():
    isolated(check_adaptive)


@pytest.mark.parametrize("path", ["", "unfused"])
def test_nbody(path):
    isolated(check_nbody, path)


if __name__ == "__main__":
    globals()[sys.argv[1]](*json.loads(sys.argv[2]))
