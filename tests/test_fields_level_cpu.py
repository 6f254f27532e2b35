"""Field outputs at a refinement level (Simulation.gather / write_fields with level=L, a deck's `level = L`, version-2 dumps
and their reader) on the CPU test double: no GPU.  The double defines no artemis_hip_pack_fields_level, so the values come
from the driver's host loop over the downloaded primitives -- the same tree as the kernel's; the definition is emulated in
numpy (tests/fields_level_ref.py) with the volumes of the CPU oracle, and every comparison of values is bitwise.  The GPU
cases are tests/test_fields_level.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
from fields_level_ref import oracle_volumes, place, resample, same_bits
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from artemis_amd.fields import read_fields  # noqa: E402

NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.cons.total_energy"]
NCOMP = 5


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag):
    """The worker (tests/fields_level_worker.py) on `world` ranks; returns (what each rank recorded, prefix of its files)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fields_level_worker.py"), json.dumps(spec)],
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


def amr():
    case = amr_cases.blast_amr(n=64)
    return dict(deck=case["deck"], overrides=case["overrides"])


# (case, zones of a block, ghost zones, coordinates, levels asked for)
CASES = {"blast": (blast, (16, 16, 1), 2, "cartesian", (-1, -2)), "amr": (amr, (8, 8, 1), 2, "cylindrical", (0, 1, 2))}


def expected_blocks(full, snap, nx, ng, coordinates, level, single=False):
    """the numpy tree or replication applied to the full-resolution gather of one rank, block by block"""
    out = []
    for b in range(full.shape[0]):
        bd = snap["bounds"][b]
        vol = oracle_volumes(nx, bd[0::2], bd[1::2], ng, coordinates)
        out.append(resample(full[b], vol, snap["levels"][b] - level, single))
    return out


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_gather_and_dump_at_a_level_equal_the_numpy_tree(tmp_path, name, world):
    """gather(level=L) equals, block by block, the numpy tree or replication of gather() of the same run, in double and in
    float; write_fields(level=L) is a version-2 dump whose meta.json has the level, each block's own nx and its element
    offset in its rank's part, and whose reader returns those blocks, places them by bounds in uniform() and refuses get()
    where they differ in shape.  One rank and two gloo ranks."""
    make, nx, ng, coordinates, levels = CASES[name]
    acts = [["create"], ["evolve", 2], ["snap", "s"], ["gather", "full", NAMES, False, None]]
    for L in levels:
        acts += [["gather", "g%d" % L, NAMES, False, L], ["gather", "f%d" % L, NAMES, True, L],
                 ["write", str(tmp_path / ("L%d.fld" % L)), NAMES, False, L]]
    acts += [["write", str(tmp_path / "plain.fld"), NAMES, False, None], ["snap", "e"], ["close"]]
    res, pre = run(world, make(), acts, tmp_path, "w%d" % world)
    for L in levels:
        by_bounds = {}
        for r in range(world):
            snap = res[r]["s"]
            assert res[r]["e"]["time"] == snap["time"] and res[r]["e"]["dt"] == snap["dt"]  # a gather moves no clock
            full = np.load(pre + ".full.rank%d.npz" % r)["a"]
            assert full.shape == (snap["nblocks"], NCOMP, nx[2], nx[1], nx[0])
            got, got32 = np.load(pre + ".g%d.rank%d.npz" % (L, r)), np.load(pre + ".f%d.rank%d.npz" % (L, r))
            want = expected_blocks(full, snap, nx, ng, coordinates, L)
            for b, w in enumerate(want):
                assert same_bits(got["b%d" % b], w), (L, r, b)
                assert same_bits(got32["b%d" % b], w.astype(np.float32)), (L, r, b)
                by_bounds[tuple(snap["bounds"][b])] = w
        fd = read_fields(tmp_path / ("L%d.fld" % L))
        meta = json.load(open(tmp_path / ("L%d.fld" % L) / "meta.json"))
        assert meta["version"] == 2 and meta["level"] == L == fd.level and meta["nranks"] == world
        for r in range(world):  # the blocks of a rank follow each other in index order, each with its own nx
            at = 0
            for blk in sorted((q for q in meta["blocks"] if q["rank"] == r), key=lambda q: q["index"]):
                s = blk["level"] - L
                assert blk["nx"] == [m if m == 1 else (m >> s if s >= 0 else m << -s) for m in nx] and blk["offset"] == at
                at += NCOMP * blk["nx"][0] * blk["nx"][1] * blk["nx"][2]
            assert os.path.getsize(tmp_path / ("L%d.fld" % L) / ("rank%d.bin" % r)) == 8 * at
        at = 0
        for v, n in (("gas.prim.density", 1), ("gas.prim.velocity", 3), ("gas.cons.total_energy", 1)):
            blocks = fd.get_blocks(v)
            assert len(blocks) == len(fd.blocks) == len(by_bounds)
            for blk, a in zip(fd.blocks, blocks):
                assert same_bits(a, by_bounds[tuple(blk["bounds"])][at:at + n]), (L, v, blk["gid"])
            u = fd.uniform(v)
            assert same_bits(u, place(fd.blocks, blocks)) and not np.isnan(u).any()
            root = 32 if name == "blast" else 64
            assert u.shape == (n, 1, (root << L) if L >= 0 else (root >> -L), (root << L) if L >= 0 else (root >> -L))
            if len({tuple(b["nx"]) for b in fd.blocks}) > 1:
                with pytest.raises(ValueError, match="get_blocks"):
                    fd.get(v)
            else:
                assert same_bits(fd.get(v), np.stack(blocks))
            at += n
    # the dump without a level is version 1, and the reader's get_blocks works on it too
    plain = read_fields(tmp_path / "plain.fld")
    meta = json.load(open(tmp_path / "plain.fld" / "meta.json"))
    assert meta["version"] == 1 and "level" not in meta and plain.level is None and all("offset" not in b for b in meta["blocks"])
    assert same_bits(np.stack(plain.get_blocks("gas.prim.velocity")), plain.get("gas.prim.velocity"))
    if name == "amr":
        assert len({b["level"] for b in plain.blocks}) >= 2
        with pytest.raises(ValueError, match="levels"):
            plain.uniform("gas.prim.density")


def test_deck_block_with_a_level_beside_one_without(tmp_path):
    """A `fld` block with level = -1 beside a plain one: the plain block's dumps are byte-identical to those of the same run
    without the levelled block (version 1 unchanged), the levelled ones are version 2 and hold the numpy tree of the plain
    ones; outputs() reports the level; load_fields refuses a levelled dump before touching the run; a truncated part is
    reported."""
    keys = ["parthenon/output0/variables=" + ", ".join(NAMES), "parthenon/output1/variables=" + ", ".join(NAMES)]
    both = blast((0, "fld", 0.02), (1, "fld", 0.02), nlim=4)
    both = dict(deck=both["deck"], overrides=both["overrides"] + keys + ["parthenon/output1/level=-1"])
    one = blast((0, "fld", 0.02), nlim=4)
    one = dict(deck=one["deck"], overrides=one["overrides"] + keys[:1])
    a, b = tmp_path / "both", tmp_path / "one"
    final = str(a / "blast_cart.out1.final.fld")
    res, _ = run(1, both, [["create"], ["enable", str(a)], ["evolve", -1], ["snap", "s"], ["load", "l", final], ["snap", "e"], ["close"]],
                 tmp_path, "both_run")
    run(1, one, [["create"], ["enable", str(b)], ["evolve", -1], ["close"]], tmp_path, "one_run")
    plain = sorted(f for f in os.listdir(a) if ".out0." in f)
    assert plain == sorted(os.listdir(b)) and len(plain) >= 2
    for f in plain:
        for part in ("meta.json", "rank0.bin"):
            assert open(a / f / part, "rb").read() == open(b / f / part, "rb").read(), (f, part)
        lv, fd = read_fields(a / f.replace(".out0.", ".out1.")), read_fields(a / f)
        assert lv.version == 2 and lv.level == -1 and fd.version == 1 and (lv.time, lv.cycle) == (fd.time, fd.cycle)
        for v in NAMES:
            for blk, got, full in zip(fd.blocks, lv.get_blocks(v), fd.get(v)):
                bd = blk["bounds"]
                assert same_bits(got, resample(full, oracle_volumes((16, 16, 1), bd[0::2], bd[1::2], 2, "cartesian"), 1)), (f, v)
            assert lv.uniform(v).shape[1:] == (1, 16, 16)
    st = {q["index"]: q for q in res[0]["s"]["outputs"]["blocks"]}
    assert st[1]["level"] == -1 and st[1]["status"] == "active" and "level" not in st[0]
    assert "resampled to level -1: not a state" in res[0]["l"]["error"]
    assert (res[0]["e"]["time"], res[0]["e"]["dt"], res[0]["e"]["ncycle"]) == (res[0]["s"]["time"], res[0]["s"]["dt"], res[0]["s"]["ncycle"])
    with open(os.path.join(final, "rank0.bin"), "r+b") as f:
        f.truncate(os.path.getsize(os.path.join(final, "rank0.bin")) - 8)
    with pytest.raises(ValueError, match="truncated"):
        read_fields(final)


def test_levels_a_deck_can_never_serve_are_skipped_and_refused(tmp_path):
    """enable_outputs checks the worst shifts the deck can produce -- its finest possible level and the root grid -- against
    the block extents: such a block is listed as skipped with the reason and writes nothing; gather names the block, its
    level and the rule and returns nothing."""
    case = blast((0, "fld", 0.02), (1, "fld", 0.02), (2, "fld", 0.02), nlim=2)
    v = ", ".join(NAMES)
    case = dict(deck=case["deck"], overrides=case["overrides"] + ["parthenon/output%d/variables=%s" % (n, v) for n in range(3)] +
                ["parthenon/output0/level=4", "parthenon/output1/level=-4", "parthenon/output2/level=-3"])
    out = tmp_path / "out"
    res, _ = run(1, case, [["create"], ["enable", str(out)], ["evolve", -1], ["snap", "s"], ["gather", "g", NAMES, False, -4],
                           ["close"]], tmp_path, "skip")
    st = {q["index"]: q["status"] for q in res[0]["s"]["outputs"]["blocks"]}
    assert st == {0: "skipped: level 4: a block on level 0 would need shift -4, |shift| <= 3 is built",
                  1: "skipped: level -4: a block on level 0 would need shift 4, |shift| <= 3 is built", 2: "active"}
    assert all(".out2." in f for f in os.listdir(out)) and len(os.listdir(out)) >= 2
    assert read_fields(out / "blast_cart.out2.final.fld").uniform("gas.prim.density").shape == (1, 1, 4, 4)
    err = res[0]["g"]["error"]
    assert "local block 0" in err and "on level 0" in err and "shift 4" in err
    # numlevel = 3: level -2 would restrict the finest blocks the mesh can ever hold four times; level -1 three times (8 % 8 == 0)
    deep = amr()
    deep = dict(deck=deep["deck"], overrides=deep["overrides"] + [
        "parthenon/output5/file_type=fld", "parthenon/output5/dt=0.1", "parthenon/output5/variables=" + v, "parthenon/output5/level=-2",
        "parthenon/output6/file_type=fld", "parthenon/output6/dt=0.1", "parthenon/output6/variables=" + v, "parthenon/output6/level=-1"])
    res, _ = run(1, deep, [["create"], ["snap", "s"], ["close"]], tmp_path, "deep")
    st = {q["index"]: q["status"] for q in res[0]["s"]["outputs"]["blocks"] if q["index"] >= 5}
    assert st == {5: "skipped: level -2: a block on level 2 would need shift 4, |shift| <= 3 is built",
                  6: "inactive: outputs are not enabled"}
    # blocks of 15 x 16 zones cannot be halved along x1
    odd = blast((0, "fld", 0.02), nlim=2)
    odd = dict(deck=odd["deck"], overrides=[o for o in odd["overrides"] if not o.endswith("nx1=32") and not o.endswith("nx1=16")] +
               ["parthenon/mesh/nx1=30", "parthenon/meshblock/nx1=15", "parthenon/output0/variables=" + v, "parthenon/output0/level=-1"])
    res, _ = run(1, odd, [["create"], ["snap", "s"], ["gather", "g", NAMES, False, -1], ["close"]], tmp_path, "odd")
    assert res[0]["s"]["outputs"]["blocks"][0]["status"] == \
        "skipped: level -1: a block on level 0 would need shift 1, and its nx1 = 15 is not divisible by 2"
    assert "nx1 = 15 is not divisible by 2" in res[0]["g"]["error"]
