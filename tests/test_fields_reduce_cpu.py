"""Reduced field outputs (Simulation.gather / write_fields with reduce=..., a deck's `reduce = x2,x3`, version-3 dumps and
their reader) on the CPU test double: no GPU.  The double defines no artemis_hip_reduce_fields, so the values come from the
driver's host loop over the downloaded primitives -- the same sums in the same order as the kernel's; the definition is
emulated in numpy (tests/fields_reduce_ref.py) with the volumes of the CPU oracle, and every comparison of values is
bitwise.  The GPU cases are tests/test_fields_reduce.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fields_reduce_ref import assemble, names_of, oracle_volumes, out_shape, reduce_block, same_bits, subsets
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
    """The worker (tests/fields_reduce_worker.py) on `world` ranks; returns (what each rank recorded, prefix of its files)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fields_reduce_worker.py"), json.dumps(spec)],
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


def wide():
    """the 2-D blast in two blocks of 72 x 16: a chunk of 64 and a tail of 8 along x1"""
    case = blast()
    ov = [o for o in case["overrides"] if "nx1=" not in o and "nx2=" not in o]
    return dict(deck=case["deck"], overrides=ov + ["parthenon/mesh/nx1=144", "parthenon/mesh/nx2=16", "parthenon/meshblock/nx1=72",
                                                   "parthenon/meshblock/nx2=16"])


def disk():
    """the cylindrical disk deck at 16 x 8 x 6 in four blocks of 8 x 8 x 3 (the block of tests/test_outputs.py, split)"""
    return dict(deck=["disk", "disk_cyl.in"],
                overrides=["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=8", "parthenon/mesh/nx3=6", "parthenon/meshblock/nx1=8",
                           "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=3", "parthenon/mesh/x1min=0.8",
                           "parthenon/mesh/x1max=4.3", "parthenon/mesh/x3min=-1.0", "parthenon/mesh/x3max=1.0", "parthenon/time/nlim=3"])


# (case, zones of a block, ghost zones, coordinates)
CASES = {"blast": (blast, (16, 16, 1), 2, "cartesian"), "wide": (wide, (72, 16, 1), 2, "cartesian"),
         "disk": (disk, (8, 8, 3), 2, "cylindrical")}


@pytest.mark.parametrize("name", list(CASES))
def test_gather_and_dump_reduced_equal_the_emulation_on_one_rank_and_on_two(tmp_path, name):
    """For every subset of the active directions: gather(reduce=...) equals, block by block, the emulation applied to gather()
    of the same run, in double and in float, and moves no clock; write_fields(reduce=...) is a version-3 dump whose meta.json
    names the directions, lists `volume` last and gives every block its reduced nx and its element offset; get_blocks
    returns the per-block integrals and reduced() the independent assembly; and reduced() of the dump written on two gloo
    ranks has the bits of the one written on one."""
    make, nx, ng, coordinates = CASES[name]
    all_axes = subsets(nx)
    acts = [["create"], ["evolve", 2], ["snap", "s"], ["gather", "full", NAMES, False, None, None]]
    for axes in all_axes:
        red = list(names_of(axes))
        acts += [["gather", "g%d" % axes, NAMES, False, red, None], ["gather", "f%d" % axes, NAMES, True, ",".join(red), None]]
    acts += [["snap", "e"], ["close"]]
    assembled = {}
    for world in (1, 2):
        wacts = acts[:-2] + [["write", str(tmp_path / ("w%d_R%d.fld" % (world, axes))), NAMES, False, list(names_of(axes))]
                             for axes in all_axes] + acts[-2:]
        res, pre = run(world, make(), wacts, tmp_path, "w%d" % world)
        for axes in all_axes:
            by_bounds = {}
            for r in range(world):
                snap = res[r]["s"]
                assert (res[r]["e"]["time"], res[r]["e"]["dt"], res[r]["e"]["ncycle"]) == (snap["time"], snap["dt"], snap["ncycle"])
                full = np.load(pre + ".full.rank%d.npz" % r)["a"]
                assert full.shape == (snap["nblocks"], NCOMP, nx[2], nx[1], nx[0])
                got, got32 = np.load(pre + ".g%d.rank%d.npz" % (axes, r))["a"], np.load(pre + ".f%d.rank%d.npz" % (axes, r))["a"]
                assert got.shape == (snap["nblocks"], NCOMP + 1) + out_shape(nx, axes) and got32.dtype == np.float32
                for b in range(snap["nblocks"]):
                    bd = snap["bounds"][b]
                    w = reduce_block(full[b], oracle_volumes(nx, bd[0::2], bd[1::2], ng, coordinates), axes)
                    assert same_bits(got[b], w), (axes, r, b)
                    assert same_bits(got32[b], w.astype(np.float32)), (axes, r, b)
                    by_bounds[tuple(bd)] = w
            path = tmp_path / ("w%d_R%d.fld" % (world, axes))
            fd, meta = read_fields(path), json.load(open(path / "meta.json"))
            assert meta["version"] == 3 == fd.version and meta["reduce"] == list(names_of(axes)) == fd.reduce and fd.level is None
            assert meta["nranks"] == world and "level" not in meta
            assert meta["variables"][-1] == dict(name="volume", ncomp=1, components=["volume"]) and len(meta["variables"]) == len(NAMES) + 1
            per = (NCOMP + 1) * int(np.prod(out_shape(nx, axes)))
            for r in range(world):
                mine = sorted((q for q in meta["blocks"] if q["rank"] == r), key=lambda q: q["index"])
                assert all(q["nx"] == list(out_shape(nx, axes))[::-1] and q["offset"] == n * per for n, q in enumerate(mine))
                assert os.path.getsize(path / ("rank%d.bin" % r)) == 8 * per * len(mine)
            assert [q["gid"] for q in fd.blocks] == sorted(q["gid"] for q in fd.blocks) and len(fd.blocks) == len(by_bounds)
            want = [by_bounds[tuple(q["bounds"])] for q in fd.blocks]  # gid order
            N, W = assemble(fd.blocks, [w[:-1] for w in want], [w[-1:] for w in want], axes, nx)
            assert not np.isnan(N).any() and not np.isnan(W).any()
            at = 0
            for v, n in (("gas.prim.density", 1), ("gas.prim.velocity", 3), ("gas.cons.total_energy", 1), ("volume", 1)):
                for blk, w in zip(fd.get_blocks(v), want):
                    assert same_bits(blk, w[at:at + n]), (axes, v)
                if v != "volume":
                    integral, mean = fd.reduced(v, "integral"), fd.reduced(v)
                    assert same_bits(integral, N[at:at + n]) and same_bits(mean, N[at:at + n] / W), (axes, v)
                    assembled[(world, axes, v)] = (integral, mean)
                else:
                    assert same_bits(fd.reduced(v), W)
                at += n
    for (world, axes, v), (integral, mean) in assembled.items():
        if world == 2:
            assert same_bits(integral, assembled[(1, axes, v)][0]) and same_bits(mean, assembled[(1, axes, v)][1]), (axes, v)


def test_deck_blocks_with_reduce_the_skipped_ones_and_the_refusals(tmp_path):
    """A `fld` block with reduce = x1,x2 beside a plain one: the plain block's dumps are byte-identical to those of the same
    run without the reduced block (version 1 unchanged) and the clock is the same; the reduced ones are version 3 and hold
    the emulation of the plain ones; outputs() reports the directions; a block that names an inactive or unknown direction,
    none at all, or that also sets `level`, is listed as skipped with the reason and writes nothing; load_fields refuses a
    reduced dump before touching the run; gather with reduce and level raises ValueError, with an inactive direction
    RuntimeError."""
    v = ", ".join(NAMES)
    both = blast(*[(n, "fld", 0.02) for n in range(6)], nlim=4)
    both = dict(deck=both["deck"], overrides=both["overrides"] + ["parthenon/output%d/variables=%s" % (n, v) for n in range(6)] +
                ["parthenon/output1/reduce=x1, x2", "parthenon/output2/reduce=x3", "parthenon/output3/reduce=x2",
                 "parthenon/output3/level=0", "parthenon/output4/reduce=x2,y", "parthenon/output5/reduce=,"])
    one = blast((0, "fld", 0.02), nlim=4)
    one = dict(deck=one["deck"], overrides=one["overrides"] + ["parthenon/output0/variables=" + v])
    a, b = tmp_path / "both", tmp_path / "one"
    final = str(a / "blast_cart.out1.final.fld")
    res, _ = run(1, both, [["create"], ["enable", str(a)], ["evolve", -1], ["snap", "s"], ["load", "l", final], ["snap", "e"],
                           ["gather", "lv", NAMES, False, ["x1"], 0], ["gather", "x3", NAMES, False, ["x3"], None],
                           ["gather", "x4", NAMES, False, ["x4"], None], ["close"]], tmp_path, "both_run")
    rone, _ = run(1, one, [["create"], ["enable", str(b)], ["evolve", -1], ["snap", "s"], ["close"]], tmp_path, "one_run")
    assert (res[0]["s"]["time"], res[0]["s"]["dt"], res[0]["s"]["ncycle"]) == (rone[0]["s"]["time"], rone[0]["s"]["dt"], rone[0]["s"]["ncycle"])
    st = {q["index"]: q for q in res[0]["s"]["outputs"]["blocks"]}
    assert st[1]["status"] == "active" and st[1]["reduce"] == ["x1", "x2"] and "reduce" not in st[0]
    assert st[2]["status"] == "skipped: reduce: x3 has one zone and is not a direction to reduce"
    assert st[3]["status"] == "skipped: reduce: a block that also sets level is not built"
    assert st[4]["status"] == "skipped: reduce: unknown direction y (x1, x2, x3)"
    assert st[5]["status"] == "skipped: reduce: no direction"
    assert not [f for f in os.listdir(a) if ".out0." not in f and ".out1." not in f]
    plain = sorted(f for f in os.listdir(a) if ".out0." in f)
    assert plain == sorted(os.listdir(b)) and len(plain) >= 2
    for f in plain:
        for part in ("meta.json", "rank0.bin"):
            assert open(a / f / part, "rb").read() == open(b / f / part, "rb").read(), (f, part)
        rd, fd = read_fields(a / f.replace(".out0.", ".out1.")), read_fields(a / f)
        assert rd.version == 3 and rd.reduce == ["x1", "x2"] and fd.version == 1 and fd.reduce is None and (rd.time, rd.cycle) == (fd.time, fd.cycle)
        full = np.concatenate([fd.get(n) for n in NAMES], axis=1)
        got = np.concatenate([np.stack(rd.get_blocks(n)) for n in NAMES + ["volume"]], axis=1)
        for g, blk in enumerate(fd.blocks):
            bd = blk["bounds"]
            assert same_bits(got[g], reduce_block(full[g], oracle_volumes((16, 16, 1), bd[0::2], bd[1::2], 2, "cartesian"), 3)), (f, g)
        assert rd.reduced("gas.prim.density").shape == (1, 1, 1, 1)
        with pytest.raises(ValueError, match="not a reduced dump"):
            fd.reduced("gas.prim.density")
        with pytest.raises(ValueError, match="has no mean"):
            rd.reduced("volume", "mean")
        assert same_bits(rd.reduced("volume"), rd.reduced("volume", "integral"))
    assert "was reduced along x1, x2: not a state" in res[0]["l"]["error"]
    assert (res[0]["e"]["time"], res[0]["e"]["dt"], res[0]["e"]["ncycle"]) == (res[0]["s"]["time"], res[0]["s"]["dt"], res[0]["s"]["ncycle"])
    assert res[0]["lv"]["error"].startswith("ValueError: reduce together with level")
    assert res[0]["x3"]["error"].startswith("RuntimeError") and "x3 has one zone" in res[0]["x3"]["error"]
    assert res[0]["x4"]["error"].startswith("ValueError: reduce takes x1, x2 and/or x3")


def test_the_resource_listing_names_every_instantiation_without_scratch():
    """profiles/fields_reduce_resource_usage.txt is the compiler's kernel-resource-usage listing of kernels_reduce.hip: the
    twelve reduce_fields_kernel<CURV, OUT, DIR> and the two reduce_axis_kernel<OUT> instantiations, each with 0 bytes of
    scratch and 0 bytes of LDS (DESIGN.md 6b cites it)."""
    text = open(os.path.join(ROOT, "profiles", "fields_reduce_resource_usage.txt")).read().split("\n")
    names = [l.split("Function Name: ")[1].strip() for l in text if "Function Name: " in l]
    assert len(names) == len(set(names)) == 14
    assert sum("reduce_fields_kernel" in n for n in names) == 12 and sum("reduce_axis_kernel" in n for n in names) == 2
    assert [l.split(":")[-1].strip() for l in text if "ScratchSize" in l] == ["0"] * 14
    assert [l.split(":")[-1].strip() for l in text if "LDS Size" in l] == ["0"] * 14
    assert all(0 < int(l.split(":")[-1]) <= 256 for l in text if " VGPRs:" in l and "Spill" not in l)
