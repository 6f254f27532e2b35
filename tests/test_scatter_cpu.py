"""Simulation.scatter / load_fields and artemis_sim_scatter_fields on the CPU test double: no GPU.  The double does not
define artemis_hip_unpack_fields, so the values go through the driver's host loop over downloaded and uploaded primitives
-- the staging of the state, the sequence behind it (PrimToCons, ConsToPrim, ghost fill, PrimToCons), the fresh dt, the
block matching of load_fields and the Python layer are the code under test here, on one rank and on gloo ranks.  Every
comparison is bitwise.  The GPU cases are tests/test_scatter.py (the kernel) and tests/test_scatter_driver.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRIM = ["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"]


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag):
    """The worker (tests/scatter_worker.py) on `world` ranks; returns (what each rank recorded, prefix of its .npz files)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "scatter_worker.py"), json.dumps(spec)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        rendezvous = any(p.returncode != 0 and ("Address already in use" in o or "Connection re" in o or "timed out" in o.lower()
                                                or "terminate called without an active exception" in o)
                         for p, o in zip(procs, outs))
        if not (rendezvous and attempt == 0):
            break
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [json.load(open(spec["out"] + ".rank%d.json" % r)) for r in range(world)], spec["out"]


def by_bounds(res, prefix, tag, snap, key="gas", cycle=""):
    """{bounds of a block: its interior primitives} over all ranks, so that runs on different rank counts compare"""
    out = {}
    for r, one in enumerate(res):
        a = np.load(prefix + ".%s.rank%d.npz" % (tag, r))[key + str(cycle)]
        rows = one[snap] if isinstance(one[snap], dict) else [q for q in one[snap] if q["ncycle"] == cycle][0]
        assert len(rows["bounds"]) == a.shape[0]
        for b, bounds in enumerate(rows["bounds"]):
            out[(rows["levels"][b],) + tuple(bounds)] = a[b]
    return out


def same(x, y):
    return x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)


def clocks(rows):
    return [(r["ncycle"], r["time"], r["dt"], r["kernel"]) for r in rows]


@pytest.mark.parametrize("world", [1, 2])
def test_scatter_reproduces_a_problem_generator(tmp_path, world):
    """Run A is the blast at cycle 0, run B the same deck with another radius: after B.scatter(A.gather(...)) B has A's dt
    and takes A's five cycles -- clock, kernel and interiors on every one."""
    acts = [["create", "A", []], ["create", "B", ["problem/radius=0.2"]], ["evolve", "A", 0], ["evolve", "B", 0],
            ["snap", "a0", "A"], ["snap", "b0", "B"], ["prims", "A0", "A"], ["prims", "B0", "B"],
            ["gather", "g", "A", PRIM, False], ["scatter", "B", PRIM, "g", None], ["snap", "b1", "B"], ["prims", "B1", "B"],
            ["track", "TA", "A", 5], ["track", "TB", "B", 5]]
    res, pre = run(world, blast(), acts, tmp_path, "pgen")
    assert not same(by_bounds(res, pre, "A0", "a0"), by_bounds(res, pre, "B0", "b0"))  # B's own initial state is another one
    assert same(by_bounds(res, pre, "A0", "a0"), by_bounds(res, pre, "B1", "b1"))
    for r in res:
        assert r["b1"]["dt"] == r["a0"]["dt"] and r["b1"]["time"] == 0.0 and r["b1"]["ncycle"] == 0
        assert clocks(r["TA"]) == clocks(r["TB"]) and [q["ncycle"] for q in r["TA"]] == [1, 2, 3, 4, 5]
    for c in range(1, 6):
        assert same(by_bounds(res, pre, "TA", "TA", cycle=c), by_bounds(res, pre, "TB", "TB", cycle=c)), c


MID = [["create", "A", []], ["create", "B", []], ["create", "C", []], ["create", "D", []],
       ["evolve", "A", 6], ["evolve", "B", 3], ["evolve", "C", 3], ["gather", "g", "B", PRIM, False],
       ["scatter", "C", PRIM, "g", "B"], ["snap", "b", "B"], ["snap", "c", "C"], ["prims", "PB", "B"], ["prims", "PC", "C"],
       ["scatter", "D", PRIM, "g", "B"], ["snap", "d", "D"], ["track", "TC", "C", 3], ["track", "TD", "D", 3], ["snap", "a", "A"]]


@pytest.mark.parametrize("world", [1, 2])
def test_scatter_in_the_middle_of_a_run(tmp_path, world):
    """C scatters, after three cycles, the state it already holds (B's, an identical run): the ghost fill and the flags
    about ghost zones start from a ping-pong buffer other than 0.  C's interiors then equal B's, and its next three cycles
    are those of a fresh run D given the same arrays and time.  C's clock is NOT A's (six cycles without a scatter): the dt
    after a scatter is a fresh estimate, without the "at most doubles" rule that still holds A's dt back at cycle 3 of a
    blast; that is by construction and not asserted."""
    res, pre = run(world, blast(), MID, tmp_path, "mid")
    assert same(by_bounds(res, pre, "PB", "b"), by_bounds(res, pre, "PC", "c"))
    for r in res:
        assert r["c"]["time"] == r["b"]["time"] == r["d"]["time"] and r["c"]["dt"] == r["d"]["dt"]
        assert (r["c"]["ncycle"], r["d"]["ncycle"]) == (3, 0)
        assert [q[1:] for q in clocks(r["TC"])] == [q[1:] for q in clocks(r["TD"])]
    for c in range(1, 4):
        assert same(by_bounds(res, pre, "TC", "TC", cycle=3 + c), by_bounds(res, pre, "TD", "TD", cycle=c)), c


def amr(*extra):
    case = amr_cases.blast_amr(n=64)
    return dict(deck=case["deck"], overrides=case["overrides"] + list(extra))


@pytest.mark.parametrize("world", [1, 2])
def test_refined_mesh_round_trip_through_a_dump(tmp_path, world):
    """blast_amr.in (cylindrical, three levels) at 64 x 64 root zones: write_fields, load_fields into a fresh run of the same
    deck, and both take the same three cycles, dt included; a run whose mesh has other leaves refuses, naming a block."""
    path = str(tmp_path / "amr.fld")
    acts = [["create", "A", []], ["create", "B", []], ["create", "X", ["parthenon/mesh/numlevel=2"]], ["evolve", "A", 0],
            ["write", "A", path, PRIM, False], ["load", "B", path, True], ["snap", "a", "A"], ["snap", "b", "B"],
            ["raises", "x", ["load", "X", path, True]], ["track", "TA", "A", 3], ["track", "TB", "B", 3]]
    res, pre = run(world, amr(), acts, tmp_path, "amr")
    for r in res:
        assert r["loaded"] == [PRIM] and len(set(r["a"]["levels"])) >= 2
        assert (r["a"]["time"], r["a"]["bounds"]) == (0.0, r["b"]["bounds"]) and r["b"]["time"] == 0.0
        assert r["b"]["dt"] == r["TA"][0]["time"]  # (A's first dt exists once it steps: the time its first cycle ends at)
        assert clocks(r["TA"]) == clocks(r["TB"])
        assert r["x"]["type"] == "ValueError" and "holds no block on level" in r["x"]["text"] and "bounds [" in r["x"]["text"]
    for c in range(1, 4):
        assert same(by_bounds(res, pre, "TA", "TA", cycle=c), by_bounds(res, pre, "TB", "TB", cycle=c)), c


def test_a_dump_of_two_ranks_loads_on_one_and_on_three(tmp_path):
    """The blocks of a dump are matched by level and bounds: written on 2 ranks after 3 cycles of a 48 x 32 blast in six
    blocks, loaded (clock included) into fresh runs on 1 and on 3 ranks, which then take the three cycles of a one-rank run
    that scatters its own state at that point."""
    case = blast()
    case = dict(deck=case["deck"], overrides=[o for o in case["overrides"] if "mesh/nx1" not in o] + ["parthenon/mesh/nx1=48"])
    path = str(tmp_path / "two.fld")
    w, _ = run(2, case, [["create", "B", []], ["evolve", "B", 3], ["snap", "b", "B"], ["write", "B", path, PRIM, False]], tmp_path, "w")
    assert [r["b"]["nblocks"] for r in w] == [3, 3]
    ref, rpre = run(1, case, [["create", "C", []], ["evolve", "C", 3], ["gather", "g", "C", PRIM, False],
                              ["scatter", "C", PRIM, "g", None], ["snap", "c", "C"], ["track", "TC", "C", 3]], tmp_path, "ref")
    acts = [["create", "D", []], ["load", "D", path, True], ["snap", "d", "D"], ["track", "TD", "D", 3]]
    for world in (1, 3):
        res, pre = run(world, case, acts, tmp_path, "r%d" % world)
        assert sum(r["d"]["nblocks"] for r in res) == 6
        for r in res:
            assert (r["d"]["time"], r["d"]["dt"], r["d"]["ncycle"]) == (ref[0]["c"]["time"], ref[0]["c"]["dt"], 0)
            assert [q[1:] for q in clocks(r["TD"])] == [q[1:] for q in clocks(ref[0]["TC"])]
        for c in range(1, 4):
            assert same(by_bounds(res, pre, "TD", "TD", cycle=c), by_bounds(ref, rpre, "TC", "TC", cycle=3 + c)), (world, c)


def test_python_layer_refusals(tmp_path):
    """ValueError before any state is touched: an array of the wrong shape, dtype or layout; a dump without a complete form
    (naming the variable) or of a fluid the run lacks.  RuntimeError with the driver's text: a mixed form, an unknown name.
    The run is untouched by all of them."""
    some, dusty = str(tmp_path / "some.fld"), str(tmp_path / "cons.fld")
    acts = [["create", "A", []], ["evolve", "A", 2], ["prims", "P0", "A"], ["snap", "s0", "A"],
            ["write", "A", some, ["gas.prim.density", "gas.prim.velocity"], False],
            ["write", "A", dusty, ["gas.cons.density", "gas.cons.total_energy", "gas.cons.internal_energy"], False]]
    for how in ("shape", "dtype", "strided"):
        acts += [["gather", how, "A", PRIM, False], ["mangle", how, how], ["raises", how, ["scatter", "A", PRIM, how, None]]]
    acts += [["gather", "g", "A", PRIM, False],
             ["raises", "mixed", ["scatter", "A", ["gas.prim.density", "gas.prim.velocity", "gas.cons.total_energy"], "g", None]],
             ["raises", "unknown", ["scatter", "A", ["gas.prim.density", "gas.prim.velocity", "gas.prim.temperature"], "g", None]],
             ["raises", "dust", ["scatter", "A", ["dust.prim.density", "dust.prim.velocity"], "g", None]],
             ["raises", "some", ["load", "A", some, True]], ["raises", "cons", ["load", "A", dusty, True]],
             ["sizes", "z8", "A", PRIM, False], ["sizes", "z4", "A", PRIM, True], ["prims", "P1", "A"], ["snap", "s1", "A"]]
    res, pre = run(1, blast(), acts, tmp_path, "refuse")
    r = res[0]
    assert r["z8"] == [4 * 5 * 256 * 8] * 3 and r["z4"] == [4 * 5 * 256 * 4] * 3  # host_in = NULL: the bytes gather returns
    for how, text in (("shape", "the array is (4, 4, 1, 16, 16)"), ("dtype", "float64 or float32, not int64"), ("strided", "C-contiguous")):
        assert r[how]["type"] == "ValueError" and text in r[how]["text"], r[how]
    assert r["mixed"]["type"] == "RuntimeError" and "mix the primitive and the conserved form" in r["mixed"]["text"]
    assert r["unknown"]["type"] == "RuntimeError" and "unknown variable gas.prim.temperature" in r["unknown"]["text"]
    assert r["dust"]["type"] == "RuntimeError" and "unknown variable dust.prim.density" in r["dust"]["text"]
    assert r["some"]["type"] == "ValueError" and "gas.prim.sie (or gas.prim.pressure) is missing" in r["some"]["text"]
    assert r["cons"]["type"] == "ValueError" and "gas.cons.momentum is missing" in r["cons"]["text"]
    assert r["s0"] == r["s1"] and same(by_bounds(res, pre, "P0", "s0"), by_bounds(res, pre, "P1", "s1"))


def test_blocks_narrower_than_the_ghost_width_are_refused(tmp_path):
    """16 x 2 blocks with nghost = 4: a neighbour's slab reaches into ghost zones of a buffer written stages ago, the state of
    such a run is all three primitive buffers (a checkpoint stores them), and scatter says so instead of setting one."""
    case = blast()
    case = dict(deck=case["deck"], overrides=case["overrides"] + ["parthenon/meshblock/nx2=2", "parthenon/mesh/nghost=4"])
    acts = [["create", "A", []], ["evolve", "A", 2], ["snap", "s0", "A"], ["prims", "P0", "A"], ["gather", "g", "A", PRIM, False],
            ["raises", "narrow", ["scatter", "A", PRIM, "g", None]], ["snap", "s1", "A"], ["prims", "P1", "A"]]
    res, pre = run(1, case, acts, tmp_path, "narrow")
    r = res[0]
    assert r["s0"]["nblocks"] == 32 and r["narrow"]["type"] == "RuntimeError"
    assert "blocks of 2 zones along x2 are narrower than the 4 ghost zones" in r["narrow"]["text"]
    assert r["s0"] == r["s1"] and same(by_bounds(res, pre, "P0", "s0"), by_bounds(res, pre, "P1", "s1"))
