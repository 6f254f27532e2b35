"""Deck-driven outputs of the host driver (artemis_sim_enable_outputs) on the CPU test double: no GPU.  The double does
not define artemis_hip_history_sums, so the rows come from the driver's host sum over all species -- the scheduler, the
file format and the rank reduction are the code under test here.  The GPU cases are tests/test_outputs.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_multirank_cpu import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from artemis_amd.history import HEADER, read_history  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag, cwd=None):
    """The worker (tests/outputs_worker.py) on `world` ranks; returns what each rank recorded."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "outputs_worker.py"), json.dumps(spec)],
                                          env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        rendezvous = any(p.returncode != 0 and ("Address already in use" in o or "Connection re" in o or "timed out" in o.lower()
                                                or "terminate called without an active exception" in o)
                         for p, o in zip(procs, outs))
        if not (rendezvous and attempt == 0):
            break
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [json.load(open(spec["out"] + ".rank%d.json" % r)) for r in range(world)]


def blast(*blocks, nlim=12):
    """The 2-D blast of tests/test_restart_cpu.py (4 blocks of 16 x 16) with output blocks (index, file_type, dt) added"""
    ov = ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16",
          "problem/radius=0.3", "problem/samples=0", "parthenon/time/nlim=%d" % nlim]
    for n, kind, dt in blocks:
        ov += ["parthenon/output%d/file_type=%s" % (n, kind), "parthenon/output%d/dt=%r" % (n, dt)]
    return dict(deck=["blast", "blast.in"], overrides=ov)


def next_multiple(time, dt_out):
    m = int(np.floor(time / dt_out)) + 1
    while m * dt_out <= time:
        m += 1
    while m > 1 and (m - 1) * dt_out > time:
        m -= 1
    return m * dt_out


def due_cycles(clock, dt_out):
    """Cycles after which a block of interval dt_out is written, from (ncycle, time) of every cycle"""
    out, nxt = [], 0.0
    for cycle, time in clock:
        if time >= nxt:
            out.append(cycle)
            nxt = next_multiple(time, dt_out)
    return out


def gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


@pytest.fixture(scope="module")
def clock(tmp_path_factory):
    """(ncycle, time) of every cycle of the 12-cycle blast, from a run without outputs; its directory stays empty"""
    d = tmp_path_factory.mktemp("clock")
    cwd = tmp_path_factory.mktemp("cwd")
    res = run(1, blast((0, "hst", 0.01), (1, "rst", 0.02)), [["create"], ["track", "T"], ["snap", "E"], ["close"]], d, "clock", cwd=str(cwd))[0]
    assert os.listdir(cwd) == []  # the deck carries output blocks; nobody enabled them
    assert all(b["status"] == "inactive: outputs are not enabled" for b in res["E"]["outputs"]["blocks"])
    assert res["E"]["outputs"]["enabled"] is False
    return [(r["ncycle"], r["time"]) for r in res["T"]], res


def test_history_file_round_trip_and_schedule(tmp_path, clock):
    """One `hst` block every 0.01, a `rst` block every 0.02 and an `hdf5` block, run to nlim in one evolve(): the rows sit
    at cycle 0 and at the first cycle that reached each multiple, the last cycle is written once although it is both due
    and the end of the run, every float of the file reads back to the double the driver holds, and next_time is a product
    m * dt."""
    ticks, straight = clock
    out = tmp_path / "out"
    case = blast((0, "hst", 0.01), (1, "rst", 0.02), (2, "hdf5", 0.005))
    res = run(1, case, [["create"], ["snap", "0"], ["enable", str(out)], ["evolve", -1], ["snap", "E"], ["close"]], tmp_path, "a")[0]
    E = res["E"]
    assert (E["time"], E["dt"], E["ncycle"]) == (straight["E"]["time"], straight["E"]["dt"], 12)  # outputs never touch dt
    raw = open(out / "blast_cart.out0.hst").read().split("\n")
    assert raw[0] == HEADER and raw[1].startswith("# [1]=time [2]=dt [3]=cycle [4]=nbtotal [5]=gas_mass_0 [6]=gas_momentum_x1_0 ")
    assert raw[1].endswith(" [9]=gas_energy_0 [10]=gas_internal_energy_0") and raw.count(HEADER) == 1
    h = read_history(out / "blast_cart.out0.hst")
    assert list(h) == ["time", "dt", "cycle", "nbtotal", "gas_mass_0", "gas_momentum_x1_0", "gas_momentum_x2_0",
                       "gas_momentum_x3_0", "gas_energy_0", "gas_internal_energy_0"]
    want = due_cycles(ticks, 0.01)
    assert want[0] == 0 and want[-1] == 12 and 2 < len(want) < 13  # (cycle 12 reaches t >= 0.07: due AND the end of the run)
    assert list(h["cycle"]) == want and list(h["time"]) == [dict(ticks)[c] for c in want]
    assert np.all(h["nbtotal"] == 4)
    # %.16e reads back to the same doubles
    assert h["time"][-1] == E["time"] and h["dt"][-1] == E["dt"]
    assert [h[k][-1] for k in list(h)[4:]] == E["history_device"]
    assert E["history_device"] == E["history"]  # the host sum, generalised: one gas species gives artemis_sim_history's bits
    # next_time by multiplication
    blocks = {b["index"]: b for b in E["outputs"]["blocks"]}
    assert blocks[0]["next_time"] == next_multiple(E["time"], 0.01) and blocks[1]["next_time"] == next_multiple(E["time"], 0.02)
    assert blocks[0]["written"] == len(want) and blocks[0]["last_cycle"] == 12 and blocks[0]["status"] == "active"
    # dumps: numbered from cycle 0, then the final one; the hdf5 block is listed and writes nothing
    dumps = sorted(f for f in os.listdir(out) if f.endswith(".rst"))
    assert dumps == ["blast_cart.out1.%05d.rst" % q for q in range(len(due_cycles(ticks, 0.02)))] + ["blast_cart.out1.final.rst"]
    assert blocks[2]["status"] == "skipped: hdf5 is not built" and blocks[2]["written"] == 0 and blocks[2]["next_time"] is None
    assert sorted(os.listdir(out)) == ["blast_cart.out0.hst"] + dumps
    assert {b["index"]: b["status"] for b in res["0"]["outputs"]["blocks"]}[2] == "skipped: hdf5 is not built"


def test_final_row_only_when_the_run_ends(tmp_path, clock):
    """hst every 0.02: the run ends at t = 0.0749, between two multiples, so the end adds a row of its own; an evolve(5)
    whose budget runs out adds none, and evolve() calls after the end add nothing."""
    ticks, _ = clock
    out = tmp_path / "out"
    case = blast((0, "hst", 0.02))
    acts = [["create"], ["enable", str(out)], ["evolve", 0], ["snap", "c0"], ["evolve", 5], ["snap", "c5"], ["evolve", -1], ["snap", "E"],
            ["evolve", -1], ["evolve", 3], ["snap", "EE"], ["close"]]
    res = run(1, case, acts, tmp_path, "b")[0]
    due = due_cycles(ticks, 0.02)
    assert due[-1] != 12 and 5 not in due and [c for c in due if 0 < c < 5]
    assert res["c0"]["outputs"]["blocks"][0]["written"] == 1 and res["c0"]["ncycle"] == 0  # the cycle-0 row, dt estimated
    assert res["c0"]["dt"] < 1.0
    assert res["c5"]["ncycle"] == 5 and res["c5"]["outputs"]["blocks"][0]["written"] == len([c for c in due if c <= 5])
    assert res["c5"]["outputs"]["blocks"][0]["last_cycle"] == max(c for c in due if c <= 5)
    h = read_history(out / "blast_cart.out0.hst")
    assert list(h["cycle"]) == due + [12]
    assert h["dt"][0] == res["c0"]["dt"] and h["time"][0] == 0.0
    assert res["EE"]["outputs"]["blocks"][0]["written"] == len(due) + 1 == res["E"]["outputs"]["blocks"][0]["written"]


def test_restored_run_appends_a_section_and_writes_no_cycle_zero_row(tmp_path, clock):
    ticks, straight = clock
    out = tmp_path / "out"
    case = blast((0, "hst", 0.01), (1, "rst", 0.02))
    run(1, case, [["create"], ["enable", str(out)], ["evolve", 6], ["close"]], tmp_path, "first")
    dumps = due_cycles(ticks, 0.02)
    k = max(q for q, c in enumerate(dumps) if c <= 6)
    res = run(1, case, [["restore", str(out / ("blast_cart.out1.%05d.rst" % k)), []], ["snap", "R"], ["enable", str(out)], ["snap", "R1"],
                        ["evolve", -1], ["snap", "E"], ["close"]], tmp_path, "second")[0]
    start = dumps[k]
    assert res["R"]["ncycle"] == start > 0
    nxt = {b["index"]: b["next_time"] for b in res["R1"]["outputs"]["blocks"]}
    assert nxt[0] == next_multiple(res["R"]["time"], 0.01) and nxt[1] == next_multiple(res["R"]["time"], 0.02)
    assert (res["E"]["time"], res["E"]["dt"], res["E"]["ncycle"]) == (straight["E"]["time"], straight["E"]["dt"], 12)
    assert open(out / "blast_cart.out0.hst").read().count(HEADER) == 2
    h = read_history(out / "blast_cart.out0.hst")
    assert list(h["cycle"]) == [c for c in due_cycles(ticks, 0.01) if c > start]
    assert "blast_cart.out1.%05d.rst" % (k + 1) in os.listdir(out)  # the numbering goes on where an unbroken run would be


def test_two_ranks_write_one_file_with_the_rows_of_one_rank(tmp_path):
    """Two gloo ranks, each given its own directory: only rank 0's holds a file.  Its rows equal the one-rank rows to the
    round-off of a reordered sum: |two - one| <= 2 gamma_{n-1} S, S = the value for mass and energies, max |M_d / D| * mass
    for a momentum (tests/test_outputs.py)."""
    case = blast((0, "hst", 0.01), nlim=8)
    acts = [["create"], ["enable", str(tmp_path / "w{rank}")], ["track", "T"], ["snap", "E"], ["close"]]
    one = run(1, case, [[a[0], a[1].replace("w{rank}", "one")] if a[0] == "enable" else a for a in acts], tmp_path, "one")
    two = run(2, case, acts, tmp_path, "two")
    assert os.listdir(tmp_path / "w0") == ["blast_cart.out0.hst"] and os.listdir(tmp_path / "w1") == []
    a, b = read_history(tmp_path / "one" / "blast_cart.out0.hst"), read_history(tmp_path / "w0" / "blast_cart.out0.hst")
    assert list(a) == list(b)
    for k in ("time", "dt", "cycle", "nbtotal"):
        assert np.array_equal(a[k], b[k]), k
    assert len(a["cycle"]) >= 4 and a["cycle"][-1] == 8
    n = one[0]["E"]["total_zones"]
    assert n == 32 * 32 == two[0]["E"]["total_zones"]
    labels = list(a)[4:]
    for row, cycle in enumerate(a["cycle"]):
        f = np.maximum(*[np.array(r["T"][int(cycle)]["factors"]) for r in two])
        assert two[0]["T"][int(cycle)]["ncycle"] == cycle
        mass = a["gas_mass_0"][row]
        for q, lab in enumerate(labels):
            S = abs(a[lab][row]) if q in (0, 4, 5) else f[q] * mass
            assert abs(a[lab][row] - b[lab][row]) <= 2.0 * gamma(n - 1) * S, (lab, cycle)


def test_nbtotal_follows_the_remeshes_of_an_adaptive_mesh(tmp_path):
    """linear_wave_amr.in at half resolution (tests/test_adaptive_cpu.py), a row every 0.02 (every cycle or two): the
    nbtotal column is the number of leaves after the remesh of the row's cycle."""
    case = dict(deck=["linwave", "linear_wave_amr.in"],
                overrides=["problem/nperiod=1", "parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx1=8",
                           "parthenon/meshblock/nx2=8", "parthenon/mesh/derefine_count=3", "parthenon/time/nlim=30",
                           "parthenon/output0/file_type=hst", "parthenon/output0/dt=0.02"])
    out = tmp_path / "amr"
    res = run(1, case, [["create"], ["snap", "0"], ["enable", str(out)], ["track", "T"], ["snap", "E"], ["close"]], tmp_path, "amr")[0]
    rows = {r["ncycle"]: r for r in res["T"]}
    h = read_history(out / "linear_wave.out0.hst")
    assert res["E"]["remeshes"] >= res["0"]["remeshes"] + 2 and h["cycle"][0] == 0 and h["cycle"][-1] == 30
    assert len(set(h["nbtotal"])) >= 2
    for c, nb, t in zip(h["cycle"], h["nbtotal"], h["time"]):
        assert rows[int(c)]["nblocks_global"] == nb and rows[int(c)]["time"] == t
    due = due_cycles([(r["ncycle"], r["time"]) for r in res["T"]], 0.02)
    assert list(h["cycle"]) == (due if due[-1] == 30 else due + [30]) and len(due) >= 10


def test_the_reference_reader_parses_the_file(tmp_path):
    """Where the reference tree is present, its own reader (analysis/ahistory.py) loads the file and agrees with
    read_history on the last section; elsewhere this check is skipped."""
    import importlib.util
    from oracle.reference import reference_dir
    path = os.path.join(reference_dir() or "", "analysis", "ahistory.py")
    if not os.path.isfile(path):
        pytest.skip("no reference tree here")
    out = tmp_path / "out"
    case = blast((0, "hst", 0.01), nlim=6)
    run(1, case, [["create"], ["enable", str(out)], ["evolve", 3], ["close"]], tmp_path, "r1")
    run(1, case, [["create"], ["enable", str(out)], ["evolve", -1], ["close"]], tmp_path, "r2")  # a second section behind the first
    spec = importlib.util.spec_from_file_location("reference_ahistory", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    f = str(out / "blast_cart.out0.hst")
    theirs, ours = mod.ahistory(f), read_history(f)
    assert open(f).read().count(HEADER) == 2 and list(theirs.dict) == list(ours)
    assert ours["cycle"][0] == 0 and ours["cycle"][-1] == 6
    for k in ours:
        assert np.array_equal(theirs.Get(k), ours[k]), k
