"""Reduced field outputs on a chosen level (Simulation.gather / write_fields with reduce=... and reduce_level=L, a deck's
`reduce_level = L`, version-4 dumps and their reader) on the CPU test double: no GPU.  The double defines no
artemis_hip_reduce_fields_level, so the values come from the driver's host loop over the downloaded primitives -- the same
operations in the same order as the kernels'; the definition is emulated in numpy (tests/fields_reduce_level_ref.py on top of
tests/fields_reduce_ref.py) with the volumes of the CPU oracle, and every comparison of values is bitwise.  The GPU cases are
tests/test_fields_reduce_level.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
import test_multilevel
from fields_reduce_level_ref import allowed_levels, out_shape_level, place_sum, reduce_block_level
from fields_reduce_ref import names_of, oracle_volumes, same_bits, subsets
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from artemis_amd.fields import read_fields  # noqa: E402

NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.cons.total_energy"]
PARTS = (("gas.prim.density", 1), ("gas.prim.velocity", 3), ("gas.cons.total_energy", 1), ("volume", 1))
NCOMP = 5


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag):
    """The worker (tests/fields_reduce_level_worker.py) on `world` ranks; returns (what each rank recorded, prefix of its files)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fields_reduce_level_worker.py"), json.dumps(spec)],
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


def multilevel(name):
    c = test_multilevel.CASES[name]
    return dict(deck=list(c["deck"]), overrides=list(c["ov"]))


def amr():
    case = amr_cases.blast_amr(n=64)
    return dict(deck=list(case["deck"]), overrides=list(case["overrides"]))


# (case, zones of a block, ghost zones, coordinates, the levels of its blocks after two cycles)
CASES = {"visc3d": (lambda: multilevel("visc3d"), (8, 8, 8), 2, "cartesian", (0, 1)),
         "sph3d": (lambda: multilevel("sph3d"), (8, 8, 8), 2, "spherical", (0, 1)),
         "amr": (amr, (8, 8, 1), 2, "cylindrical", (0, 1, 2))}


def proper(nx):
    """every non-empty mask of active directions that keeps at least one of them"""
    active = sum(1 << d for d in range(3) if nx[d] > 1)
    return [a for a in subsets(nx) if a != active]


def clock(snap):
    return snap["time"], snap["dt"], snap["ncycle"]


@pytest.mark.parametrize("name", list(CASES))
def test_gather_and_dump_on_a_level_equal_the_emulation_on_one_rank_and_on_two(tmp_path, name):
    """For every proper subset of the active directions and every reduce_level the mesh allows (|shift| <= 3 for all its
    levels): gather(reduce=..., reduce_level=L) equals, block by block, the emulation applied to gather() of the same run, in
    double and in float, and moves no clock; write_fields is a version-4 dump whose meta.json names the directions and the
    level, lists `volume` last and gives every block the nx it was brought to and its element offset; get_blocks returns the
    per-block arrays and reduced() an independent placement of the emulated blocks; and reduced() of the dump written on two
    gloo ranks has the bits of the one written on one.  A version-3 dump of the same refined mesh with a kept direction is
    still refused by reduced()."""
    make, nx, ng, coordinates, levels = CASES[name]
    combos = [(axes, L) for axes in proper(nx) for L in allowed_levels(levels, nx, axes)]
    assert {l - L for _, L in combos for l in levels} >= set(range(-3, 4)) and len(combos) >= 10
    acts = [["create"], ["evolve", 2], ["snap", "s"], ["gather", "full", NAMES, False, None, None, None]]
    for axes, L in combos:
        red = list(names_of(axes))
        acts += [["gather", "g%d_%d" % (axes, L), NAMES, False, red, None, L], ["gather", "f%d_%d" % (axes, L), NAMES, True, ",".join(red), None, L]]
    v3 = proper(nx)[0]
    assembled = {}
    for world in (1, 2):
        wacts = (acts if world == 1 else acts[:3]) + [
            ["write", "w", str(tmp_path / ("w%d_R%d_L%d.fld" % (world, axes, L))), NAMES, False, list(names_of(axes)), None, L]
            for axes, L in combos] + [["write", "w3", str(tmp_path / ("w%d_v3.fld" % world)), NAMES, False, list(names_of(v3)), None, None],
                                      ["snap", "e"], ["close"]]
        res, pre = run(world, make(), wacts, tmp_path, "w%d" % world)
        assert all(r["w"]["error"] is None and r["w3"]["error"] is None and clock(r["e"]) == clock(r["s"]) for r in res)
        if world == 1:
            snap = res[0]["s"]
            assert set(snap["levels"]) == set(levels)
            full = np.load(pre + ".full.rank0.npz")["a"]
            assert full.shape == (snap["nblocks"], NCOMP, nx[2], nx[1], nx[0])
            vols = [oracle_volumes(nx, bd[0::2], bd[1::2], ng, coordinates) for bd in snap["bounds"]]
            want = {}
            for axes, L in combos:
                got, got32 = np.load(pre + ".g%d_%d.rank0.npz" % (axes, L)), np.load(pre + ".f%d_%d.rank0.npz" % (axes, L))
                assert len(got.files) == len(got32.files) == snap["nblocks"]
                for b in range(snap["nblocks"]):
                    s = snap["levels"][b] - L
                    w = reduce_block_level(full[b], vols[b], axes, s)
                    assert w.shape == (NCOMP + 1,) + out_shape_level(nx, axes, s)
                    assert same_bits(got["b%d" % b], w), (axes, L, b, s)
                    assert same_bits(got32["b%d" % b], w.astype(np.float32)), (axes, L, b, s)
                    want[(axes, L, tuple(snap["bounds"][b]))] = w
        for axes, L in combos:
            path = tmp_path / ("w%d_R%d_L%d.fld" % (world, axes, L))
            fd, meta = read_fields(path), json.load(open(path / "meta.json"))
            assert meta["version"] == 4 == fd.version and meta["reduce"] == list(names_of(axes)) == fd.reduce
            assert meta["reduce_level"] == L == fd.reduce_level and fd.level is None and "level" not in meta and meta["nranks"] == world
            assert meta["variables"][-1] == dict(name="volume", ncomp=1, components=["volume"]) and len(meta["variables"]) == len(NAMES) + 1
            for r in range(world):  # the blocks of a rank follow each other in index order, each with its own nx
                at = 0
                for q in sorted((q for q in meta["blocks"] if q["rank"] == r), key=lambda q: q["index"]):
                    assert q["nx"] == list(out_shape_level(nx, axes, q["level"] - L))[::-1] and q["offset"] == at
                    at += (NCOMP + 1) * q["nx"][0] * q["nx"][1] * q["nx"][2]
                assert os.path.getsize(path / ("rank%d.bin" % r)) == 8 * at
            assert [q["gid"] for q in fd.blocks] == sorted(q["gid"] for q in fd.blocks)
            blocks = [want[(axes, L, tuple(q["bounds"]))] for q in fd.blocks]  # gid order
            N, W, cover = place_sum(fd.blocks, [w[:-1] for w in blocks], [w[-1:] for w in blocks], axes, nx)
            assert cover.min() >= 1 and cover.max() > 1  # (blocks stacked along a reduced direction meet the same cells)
            at = 0
            for v, n in PARTS:
                for blk, w in zip(fd.get_blocks(v), blocks):
                    assert same_bits(blk, w[at:at + n]), (axes, L, v)
                if v != "volume":
                    integral, mean = fd.reduced(v, "integral"), fd.reduced(v)
                    assert same_bits(integral, N[at:at + n]) and same_bits(mean, N[at:at + n] / W), (axes, L, v)
                    assembled[(world, axes, L, v)] = (integral, mean)
                else:
                    assert same_bits(fd.reduced(v), W)
                at += n
        old = read_fields(tmp_path / ("w%d_v3.fld" % world))
        assert old.version == 3 and old.reduce == list(names_of(v3)) and old.reduce_level is None
        with pytest.raises(ValueError, match="do not share a zone size"):
            old.reduced("gas.prim.density")
    for (world, axes, L, v), (integral, mean) in assembled.items():
        if world == 2:
            assert same_bits(integral, assembled[(1, axes, L, v)][0]) and same_bits(mean, assembled[(1, axes, L, v)][1]), (axes, L, v)


def test_deck_blocks_with_reduce_level_the_skipped_ones_and_the_refusals(tmp_path):
    """On the refined 3-D Cartesian case, a `fld` block with reduce = x3 and reduce_level = 1 beside a plain one: both dump on
    the same schedule, the plain block's dumps and the final state are byte-identical to those of the same run without the
    reduced block, and the version-4 dumps hold the emulation of the plain ones; outputs() reports the level.  A block whose
    reduce_level the deck can never serve, that sets it without reduce, or together with level, is listed as skipped with the
    reason and writes nothing -- and a block with reduce and level is skipped as before.  load_fields refuses a version-4
    dump before touching the run; gather refuses reduce_level without reduce or with level (ValueError), reduce with level
    as before, and an impossible reduce_level with block, level and rule (RuntimeError), as write_fields does."""
    v = ", ".join(NAMES)
    base = multilevel("visc3d")

    def fld(n, **keys):
        return ["parthenon/output%d/file_type=fld" % n, "parthenon/output%d/dt=0.004" % n, "parthenon/output%d/variables=%s" % (n, v)] + \
               ["parthenon/output%d/%s=%s" % (n, k, val) for k, val in keys.items()]
    both = dict(deck=base["deck"], overrides=base["overrides"] + fld(0) + fld(1, reduce="x3", reduce_level=1) + fld(2, reduce="x3", reduce_level=4) +
                fld(3, reduce_level=0) + fld(4, level=0, reduce_level=0) + fld(5, reduce="x3", level=0, reduce_level=0) +
                fld(6, reduce="x3", reduce_level=-3) + fld(7, reduce="x1", level=0))
    one = dict(deck=base["deck"], overrides=base["overrides"] + fld(0))
    a, b = tmp_path / "both", tmp_path / "one"
    final = str(a / "blast_cart.out1.final.fld")
    res, pa = run(1, both, [["create"], ["enable", str(a)], ["evolve", -1], ["snap", "s"], ["load", "l", final], ["snap", "e"], ["state", "st"],
                            ["gather", "no_reduce", NAMES, False, None, None, 1], ["gather", "with_level", NAMES, False, ["x3"], 0, 0],
                            ["gather", "old", NAMES, False, ["x3"], 0, None], ["gather", "far", NAMES, False, ["x3"], None, 4],
                            ["gather", "deep", NAMES, False, ["x3"], None, -3],
                            ["write", "wfar", str(tmp_path / "far.fld"), NAMES, False, ["x3"], None, 4],
                            ["write", "wno", str(tmp_path / "no.fld"), NAMES, False, None, None, 0], ["close"]], tmp_path, "both_run")
    rone, pb = run(1, one, [["create"], ["enable", str(b)], ["evolve", -1], ["snap", "s"], ["state", "st"], ["close"]], tmp_path, "one_run")
    assert clock(res[0]["s"]) == clock(rone[0]["s"]) == clock(res[0]["e"])
    sa, sb = np.load(pa + ".st.rank0.npz")["prim"], np.load(pb + ".st.rank0.npz")["prim"]
    assert sa.tobytes() == sb.tobytes()
    st = {q["index"]: q for q in res[0]["s"]["outputs"]["blocks"]}
    assert st[1]["status"] == "active" and st[1]["reduce"] == ["x3"] and st[1]["reduce_level"] == 1 and "reduce_level" not in st[0]
    assert st[2]["status"] == "skipped: reduce_level 4: a block on level 0 would need shift -4, |shift| <= 3 is built"
    assert st[3]["status"] == "skipped: reduce_level: only valid beside reduce"
    assert st[4]["status"] == "skipped: reduce_level: a block that also sets level is not built"
    assert st[5]["status"] == "skipped: reduce: a block that also sets level is not built"
    assert st[6]["status"] == "skipped: reduce_level -3: a block on level 1 would need shift 4, |shift| <= 3 is built"
    assert st[7]["status"] == "skipped: reduce: a block that also sets level is not built"
    files = os.listdir(a)
    assert not [f for f in files if ".out0." not in f and ".out1." not in f]
    plain = sorted(f for f in files if ".out0." in f)
    assert plain == sorted(os.listdir(b)) and len(plain) >= 3
    assert sorted(f.replace(".out1.", ".out0.") for f in files if ".out1." in f) == plain  # on the same schedule
    for f in plain:
        for part in ("meta.json", "rank0.bin"):
            assert open(a / f / part, "rb").read() == open(b / f / part, "rb").read(), (f, part)
        rd, fd = read_fields(a / f.replace(".out0.", ".out1.")), read_fields(a / f)
        assert rd.version == 4 and rd.reduce == ["x3"] and rd.reduce_level == 1 and fd.version == 1 and fd.reduce is None
        assert fd.reduce_level is None and (rd.time, rd.cycle) == (fd.time, fd.cycle)
        full = np.concatenate([np.stack(fd.get_blocks(n)) for n in NAMES], axis=1)
        for g, blk in enumerate(fd.blocks):
            bd = blk["bounds"]
            w = reduce_block_level(full[g], oracle_volumes((8, 8, 8), bd[0::2], bd[1::2], 2, "cartesian"), 4, blk["level"] - 1)
            got = np.concatenate([rd.get_blocks(n)[g] for n in NAMES + ["volume"]], axis=0)
            assert same_bits(got, w), (f, g)
        assert rd.reduced("gas.prim.density").shape == (1, 1, 32, 64)
        with pytest.raises(ValueError, match="has no mean"):
            rd.reduced("volume", "mean")
    assert "was reduced along x3: not a state" in res[0]["l"]["error"]
    assert res[0]["no_reduce"]["error"] == "ValueError: reduce_level is only valid beside reduce"
    assert res[0]["wno"]["error"] == "ValueError: reduce_level is only valid beside reduce"
    assert res[0]["with_level"]["error"].startswith("ValueError: reduce_level together with level")
    assert res[0]["old"]["error"].startswith("ValueError: reduce together with level")
    for tag, shift in (("far", -4), ("deep", 4), ("wfar", -4)):
        err = res[0][tag]["error"]
        assert err.startswith("RuntimeError") and "local block" in err and "on level" in err and "shift %d, |shift| <= 3 is built" % shift in err
    assert not os.path.exists(tmp_path / "far.fld") and not os.path.exists(tmp_path / "no.fld")


def test_only_the_kept_extents_must_be_divisible(tmp_path):
    """One-level 2-D blast in blocks of 12 x 16: with x1 reduced, reduce_level = -3 adds pairs three times along x2 (16 = 2 * 8)
    although 8 does not divide 12; with x2 reduced the same level is refused, gather naming block, shift and extent and the
    deck block listed as skipped; reduce_level = 0 returns the blocks of gather(reduce=...) bit for bit."""
    case = blast((0, "fld", 0.02), (1, "fld", 0.02), nlim=2)
    v = ", ".join(NAMES)
    ov = [o for o in case["overrides"] if not o.endswith("nx1=32") and not o.endswith("nx1=16")]
    case = dict(deck=case["deck"], overrides=ov + ["parthenon/mesh/nx1=24", "parthenon/meshblock/nx1=12"] +
                ["parthenon/output%d/variables=%s" % (n, v) for n in range(2)] +
                ["parthenon/output0/reduce=x1", "parthenon/output0/reduce_level=-3", "parthenon/output1/reduce=x2", "parthenon/output1/reduce_level=-3"])
    res, pre = run(1, case, [["create"], ["evolve", 2], ["snap", "s"], ["gather", "full", NAMES, False, None, None, None],
                             ["gather", "x1", NAMES, False, ["x1"], None, -3], ["gather", "x2", NAMES, False, ["x2"], None, -3],
                             ["gather", "r0", NAMES, False, ["x2"], None, 0], ["gather", "r", NAMES, False, ["x2"], None, None], ["close"]],
                   tmp_path, "odd")
    snap, full, got = res[0]["s"], np.load(pre + ".full.rank0.npz")["a"], np.load(pre + ".x1.rank0.npz")
    for b in range(snap["nblocks"]):
        bd = snap["bounds"][b]
        w = reduce_block_level(full[b], oracle_volumes((12, 16, 1), bd[0::2], bd[1::2], 2, "cartesian"), 1, 3)
        assert w.shape == (NCOMP + 1, 1, 2, 1) and same_bits(got["b%d" % b], w)
    err = res[0]["x2"]["error"]
    assert err.startswith("RuntimeError") and "local block 0" in err and "shift 3, and its nx1 = 12 is not divisible by 8" in err
    st = {q["index"]: q["status"] for q in snap["outputs"]["blocks"]}
    assert st == {0: "inactive: outputs are not enabled",
                  1: "skipped: reduce_level -3: a block on level 0 would need shift 3, and its nx1 = 12 is not divisible by 8"}
    r0, r = np.load(pre + ".r0.rank0.npz"), np.load(pre + ".r.rank0.npz")["a"]
    assert same_bits(np.stack([r0["b%d" % b] for b in range(snap["nblocks"])]), r)


def test_the_resource_listing_names_both_instantiations_without_scratch():
    """profiles/fields_reduce_level_resource_usage.txt is the compiler's kernel-resource-usage listing of the kernels this
    output adds to kernels_reduce.hip: resample_reduced_kernel<float> and <double>, each with 0 bytes of scratch and 0 bytes
    of LDS (DESIGN.md 6b cites it)."""
    text = open(os.path.join(ROOT, "profiles", "fields_reduce_level_resource_usage.txt")).read().split("\n")
    names = [l.split("Function Name: ")[1].strip() for l in text if "Function Name: " in l]
    assert len(names) == len(set(names)) == 2 and all("resample_reduced_kernel" in n for n in names)
    assert [l.split(":")[-1].strip() for l in text if "ScratchSize" in l] == ["0"] * 2
    assert [l.split(":")[-1].strip() for l in text if "LDS Size" in l] == ["0"] * 2
    assert all(0 < int(l.split(":")[-1]) <= 64 for l in text if " VGPRs:" in l and "Spill" not in l)
