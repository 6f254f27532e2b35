"""Deck-driven field outputs (file_type = fld), Simulation.gather / write_fields and artemis_amd.fields.read_fields on the CPU
test double: no GPU.  The double does not define artemis_hip_pack_fields, so the values come from the driver's host loop over
the downloaded primitives -- the scheduler, the dump format, the rank layout and the reader are the code under test here.
Every comparison is bitwise.  The GPU cases are tests/test_fields.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_multirank_cpu import free_port
from test_outputs_cpu import blast, due_cycles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from artemis_amd.fields import read_fields  # noqa: E402

SHIPPED = "gas.prim.density, gas.prim.velocity, gas.prim.pressure"  # the `variables` line of the shipped decks (gas-only)
NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"]


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag):
    """The worker (tests/fields_worker.py) on `world` ranks; returns (what each rank recorded, prefix of its .npz files)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fields_worker.py"), json.dumps(spec)],
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


def fld(case, n, **keys):
    """`case` with keys of <parthenon/outputN> added (variables, single_precision_output, ghost_zones)"""
    return dict(deck=case["deck"], overrides=case["overrides"] + ["parthenon/output%d/%s=%s" % (n, k, v) for k, v in keys.items()])


def place(blocks, data, nx):
    """[ncomp, NZ, NY, NX] from per-block arrays and their bounds, the independent form of FieldDump.uniform"""
    lo = [min(b["bounds"][2 * d] for b in blocks) for d in range(3)]
    hi = [max(b["bounds"][2 * d + 1] for b in blocks) for d in range(3)]
    n = [int(round((hi[d] - lo[d]) / (blocks[0]["bounds"][2 * d + 1] - blocks[0]["bounds"][2 * d]))) * nx[d] for d in range(3)]
    out = np.full((data.shape[1], n[2], n[1], n[0]), np.nan, dtype=data.dtype)
    for g, b in enumerate(blocks):
        o = [int(round((b["bounds"][2 * d] - lo[d]) / (hi[d] - lo[d]) * n[d])) for d in range(3)]
        out[:, o[2]:o[2] + nx[2], o[1]:o[1] + nx[1], o[0]:o[0] + nx[0]] = data[g]
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The 12-cycle blast without outputs: its clock per cycle, its final clock and its final primitives (ghosts included)"""
    d = tmp_path_factory.mktemp("plain")
    res, out = run(1, blast(), [["create"], ["evolve", -1], ["snap", "E"], ["state", "S"], ["close"]], d, "plain")
    return res[0]["E"], np.load(out + ".S.rank0.npz")["prim"]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """The same run with a `fld` block every 0.02 (double), one every 0.02 in single precision and an `hdf5` block, stepped
    one cycle at a time with the primitives recorded after every cycle; a gather and a write_fields at the end."""
    d = tmp_path_factory.mktemp("dumped")
    out = d / "out"
    case = fld(fld(blast((0, "fld", 0.02), (1, "hdf5", 0.005), (2, "fld", 0.02)), 0, variables=SHIPPED), 2, variables=SHIPPED,
               single_precision_output="true")
    acts = [["create"], ["snap", "0"], ["enable", str(out)], ["track", "T"], ["snap", "E"], ["gather", "G", NAMES, False],
            ["write", str(d / "direct.fld"), NAMES, False], ["state", "S"], ["close"]]
    res, prefix = run(1, case, acts, d, "dumped")
    return res[0], prefix, out, d


def test_fld_block_writes_the_scheduled_dumps_and_reports_them(dumped):
    res, prefix, out, d = dumped
    ticks = [(r["ncycle"], r["time"]) for r in res["T"]]
    due = due_cycles(ticks, 0.02)
    assert due[0] == 0 and due[-1] != 12 and len(due) >= 3
    want = ["blast_cart.out0.%05d.fld" % q for q in range(len(due))] + ["blast_cart.out0.final.fld"]
    assert sorted(f for f in os.listdir(out) if ".out0." in f) == sorted(want)
    assert [read_fields(out / f).cycle for f in want] == due + [12]
    assert sorted(os.listdir(out)) == sorted(want + [w.replace(".out0.", ".out2.") for w in want])  # the hdf5 block writes nothing
    blocks = {b["index"]: b for b in res["E"]["outputs"]["blocks"]}
    assert blocks[0]["status"] == "active" and blocks[0]["written"] == len(due) + 1 and blocks[0]["file_type"] == "fld"
    assert blocks[0]["variables"] == NAMES and blocks[0]["single_precision"] is False and blocks[2]["single_precision"] is True
    assert blocks[0]["path"] == str(out / "blast_cart.out0.final.fld") and blocks[0]["last_cycle"] == due[-1]
    assert blocks[1]["status"] == "skipped: hdf5 is not built" and blocks[1]["written"] == 0 and "variables" not in blocks[1]
    assert {b["index"]: b["status"] for b in res["0"]["outputs"]["blocks"]} == {
        0: "inactive: outputs are not enabled", 1: "skipped: hdf5 is not built", 2: "inactive: outputs are not enabled"}


def test_every_dump_holds_the_state_of_its_cycle(dumped):
    res, prefix, out, d = dumped
    states = np.load(prefix + ".T.rank0.npz")
    clock = {r["ncycle"]: r for r in res["T"]}
    names = sorted(f for f in os.listdir(out) if ".out0." in f)
    assert len(names) >= 4
    for f in names:
        fd = read_fields(out / f)
        prim = states["c%d" % fd.cycle]  # [4 blocks, 6, 1, 16, 16]: field("gas.prim") materialises the pressure slot
        assert fd.time == clock[fd.cycle]["time"] and fd.dtype == np.float64
        # (the clock of cycle 0 was recorded before the first dt existed; the dump is written once it does)
        assert fd.dt == clock[fd.cycle]["dt"] if fd.cycle else 0.0 < fd.dt < 1.0
        assert fd.variables == {"gas.prim.density": 1, "gas.prim.velocity": 3, "gas.prim.pressure": 1}
        assert [b["gid"] for b in fd.blocks] == [0, 1, 2, 3] and all(b["level"] == 0 and b["nx"] == [16, 16, 1] for b in fd.blocks)
        assert [b["bounds"] for b in fd.blocks] == res["E"]["bounds"]
        assert np.array_equal(fd.get("gas.prim.density"), prim[:, 0:1])
        assert np.array_equal(fd.get("gas.prim.velocity"), prim[:, 1:4])
        assert np.array_equal(fd.get("gas.prim.pressure"), prim[:, 4:5]) and fd.get("gas.prim.pressure").min() > 0.0
        for name in NAMES:
            u = fd.uniform(name)
            assert u.shape == (fd.variables[name], 1, 32, 32) and np.array_equal(u, place(fd.blocks, fd.get(name), [16, 16, 1]))
    assert not np.array_equal(states["c0"], states["c12"])


def test_gather_and_write_fields_agree_with_the_last_dump(dumped):
    res, prefix, out, d = dumped
    last, direct = read_fields(out / "blast_cart.out0.final.fld"), read_fields(d / "direct.fld")
    g = np.load(prefix + ".G.rank0.npz")["a"]
    assert g.shape == (4, 5, 1, 16, 16) and g.dtype == np.float64
    for fd in (last, direct):
        assert np.array_equal(np.concatenate([fd.get(n) for n in NAMES], axis=1), g)
    assert direct.cycle == 12 and sorted(os.listdir(d / "direct.fld")) == ["meta.json", "rank0.bin"]
    assert not os.path.exists(str(d / "direct.fld") + ".tmp")


def test_single_precision_is_the_rounded_double(dumped):
    res, prefix, out, d = dumped
    names = sorted(f for f in os.listdir(out) if ".out0." in f)
    for f in names:
        a, b = read_fields(out / f), read_fields(out / f.replace(".out0.", ".out2."))
        assert b.dtype == np.float32 and json.load(open(out / f.replace(".out0.", ".out2.") / "meta.json"))["dtype"] == "<f4"
        assert os.path.getsize(out / f / "rank0.bin") == 2 * os.path.getsize(out / f.replace(".out0.", ".out2.") / "rank0.bin") == 4 * 5 * 256 * 8
        for name in NAMES:
            assert b.get(name).dtype == np.float32 and np.array_equal(b.get(name), a.get(name).astype(np.float32))


def test_a_run_with_field_dumps_takes_the_same_steps(dumped, plain):
    res, prefix, out, d = dumped
    E, prim = plain
    assert (res["E"]["time"], res["E"]["dt"], res["E"]["ncycle"]) == (E["time"], E["dt"], 12)
    assert np.array_equal(np.load(prefix + ".S.rank0.npz")["prim"], prim)


def test_two_ranks_write_one_dump_that_reads_like_the_one_rank_dump(tmp_path):
    case = fld(blast((0, "fld", 0.02), nlim=4), 0, variables=SHIPPED)
    acts = [["create"], ["enable", "DIR"], ["evolve", -1], ["snap", "E"], ["close"]]
    one, _ = run(1, case, [[a[0], str(tmp_path / "one")] if a[0] == "enable" else a for a in acts], tmp_path, "one")
    two, _ = run(2, case, [[a[0], str(tmp_path / "two")] if a[0] == "enable" else a for a in acts], tmp_path, "two")
    assert sorted(os.listdir(tmp_path / "one")) == sorted(os.listdir(tmp_path / "two")) and len(os.listdir(tmp_path / "two")) >= 2
    assert two[0]["E"]["nblocks"] == 2 == two[1]["E"]["nblocks"]
    for f in os.listdir(tmp_path / "two"):
        assert sorted(os.listdir(tmp_path / "two" / f)) == ["meta.json", "rank0.bin", "rank1.bin"]
        a, b = read_fields(tmp_path / "one" / f), read_fields(tmp_path / "two" / f)
        meta = json.load(open(tmp_path / "two" / f / "meta.json"))
        assert [blk["gid"] for blk in meta["blocks"]] == [0, 1, 2, 3] and meta["nranks"] == 2
        assert sorted(blk["rank"] for blk in meta["blocks"]) == [0, 0, 1, 1]
        for r in (0, 1):  # a rank's blocks by its own local order
            mine = [blk for blk in meta["blocks"] if blk["rank"] == r]
            assert sorted(blk["index"] for blk in mine) == [0, 1]
            assert [blk["bounds"] for blk in sorted(mine, key=lambda q: q["index"])] == two[r]["E"]["bounds"]
        assert (a.time, a.dt, a.cycle) == (b.time, b.dt, b.cycle) and a.blocks == b.blocks
        for name in NAMES:
            assert np.array_equal(a.get(name), b.get(name)) and np.array_equal(a.uniform(name), b.uniform(name))


def test_blocks_that_cannot_be_written_are_listed_and_write_nothing(tmp_path, plain):
    """An unknown name, no `variables`, ghost_zones = true and a dust variable on a gas-only deck: skipped, never an error"""
    case = blast((0, "fld", 0.02), (1, "fld", 0.02), (2, "fld", 0.02), (3, "fld", 0.02))
    case = fld(case, 0, variables="gas.prim.density, gas.prim.temperature")
    case = fld(case, 2, variables=SHIPPED, ghost_zones="true")
    case = fld(case, 3, variables="gas.prim.density, dust.prim.density")
    out = tmp_path / "out"
    res, _ = run(1, case, [["create"], ["snap", "0"], ["enable", str(out)], ["evolve", -1], ["snap", "E"], ["close"]], tmp_path, "skip")
    want = {0: "skipped: unknown variable gas.prim.temperature", 1: "skipped: no variables", 2: "skipped: ghost_zones is not built",
            3: "skipped: unknown variable dust.prim.density"}
    for tag in ("0", "E"):
        assert {b["index"]: b["status"] for b in res[0][tag]["outputs"]["blocks"]} == want
        assert all(b["written"] == 0 and b["next_time"] is None and b["path"] is None for b in res[0][tag]["outputs"]["blocks"])
    assert os.listdir(out) == []
    assert (res[0]["E"]["time"], res[0]["E"]["dt"], res[0]["E"]["ncycle"]) == (plain[0]["time"], plain[0]["dt"], 12)


def test_reader_refuses_a_damaged_dump(dumped, tmp_path):
    import shutil
    res, prefix, out, d = dumped
    src = out / "blast_cart.out0.final.fld"
    for tag in ("missing", "short", "version", "empty"):
        shutil.copytree(src, tmp_path / tag)
    read_fields(tmp_path / "missing")
    os.remove(tmp_path / "missing" / "rank0.bin")
    with pytest.raises(ValueError, match="rank0.bin is missing"):
        read_fields(tmp_path / "missing")
    with open(tmp_path / "short" / "rank0.bin", "r+b") as f:
        f.truncate(os.path.getsize(src / "rank0.bin") - 8)
    with pytest.raises(ValueError, match="truncated"):
        read_fields(tmp_path / "short")
    meta = json.load(open(tmp_path / "version" / "meta.json"))
    meta["version"] = 99
    json.dump(meta, open(tmp_path / "version" / "meta.json", "w"))
    with pytest.raises(ValueError, match="version 99"):
        read_fields(tmp_path / "version")
    os.remove(tmp_path / "empty" / "meta.json")
    with pytest.raises(ValueError, match="no meta.json"):
        read_fields(tmp_path / "empty")
