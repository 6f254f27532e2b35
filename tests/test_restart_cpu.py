"""Checkpoint and restart of the host driver (artemis_sim_save / artemis_sim_restore) on the CPU test double: no GPU.

The pattern of every case: run A does evolve(n1); evolve(n2).  Run B does evolve(n1); save; close; restore; evolve(n2).
Directly after the restore every zone of every field of every block equals the saved simulation's (the whole arrays are
stored: ghost zones too); after n2 the clock, the kernel family and the interior of every field equal A's, bit for bit.
The GPU cases are tests/test_restart.py."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_multirank_cpu import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def run(world, case, actions, tmp_path, tag):
    """The worker (tests/restart_worker.py) on `world` ranks; returns per rank (meta, arrays)."""
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), actions=actions, out=str(tmp_path / tag))
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                       OMP_NUM_THREADS=case.get("threads", threads))
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "restart_worker.py"), json.dumps(spec)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        rendezvous = any(p.returncode != 0 and ("Address already in use" in o or "Connection re" in o or "timed out" in o.lower()
                                                or "terminate called without an active exception" in o)
                         for p, o in zip(procs, outs))
        if not (rendezvous and attempt == 0):
            break
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    res = []
    for r in range(world):
        z = np.load(spec["out"] + ".rank%d.npz" % r)
        res.append((json.loads(str(z["meta"])), z))
    return res


def blocks(res, tag, field, interior=False):
    """{(level, bounds): array} of one field over the blocks of all ranks."""
    out = {}
    for meta, z in res:
        m = meta[tag]
        ks, ke, js, je, is_, ie = m["interior"]
        for b in range(m["nblocks"]):
            a = z["%s.%s.%d" % (tag, field, b)]
            key = (m["levels"][b],) + tuple(np.round(z["%s.bounds.%d" % (tag, b)], 12))
            assert key not in out
            out[key] = a[:, ks:ke + 1, js:je + 1, is_:ie + 1] if interior else a
    return out


def same_blocks(x, y, what):
    assert x.keys() == y.keys(), what
    for key in x:
        assert np.array_equal(x[key], y[key]), (what, key)


def pattern_actions(ck, n1, n2, extra=()):
    first = [["evolve", n1]] if n1 > 0 else []  # (n1 = 0: saved before anything has stepped or estimated a dt)
    return ([["create"], ["dump", "I"]] + first + [["evolve", n2], ["dump", "A"], ["close"], ["create"]] + first +
            [["dump", "S", False], ["save", ck], ["close"],
             ["restore", ck, list(extra)], ["dump", "R", False], ["evolve", n2], ["dump", "B"], ["close"]])


def check_pattern(straight, saved, restored, tags=("A", "S", "R", "B"), same_ranks=True):
    """saved -> restored: every zone; straight vs continued: clock, kernel family, tree and the interior of every field.
    The error norms are sums over blocks reduced over the ranks: exact at equal rank count, and equal to the round-off of
    a reordered sum of a few hundred terms (1e-12 relative) when the rank count differs."""
    A, S, R, B = tags
    ms, mr, ma, mb = saved[0][0][S], restored[0][0][R], straight[0][0][A], restored[0][0][B]
    for k in ("time", "dt", "ncycle", "remeshes", "nblocks_global"):
        assert ms[k] == mr[k], k
    for f in ms["fields"]:
        same_blocks(blocks(saved, S, f), blocks(restored, R, f), "after restore: " + f)
    for k in ("time", "dt", "ncycle", "stage_kernel", "remeshes", "nblocks_global") + (("errors",) if same_ranks else ()):
        assert ma[k] == mb[k], (k, ma[k], mb[k])
    assert np.allclose(ma["errors"], mb["errors"], rtol=1e-12, atol=0.0)
    for f in ma["fields"]:
        same_blocks(blocks(straight, A, f, True), blocks(restored, B, f, True), "after n2: " + f)


LINWAVE_1D = dict(deck=["linwave", "linear_wave.in"], threads="1", overrides=[
    "parthenon/mesh/nx1=256", "parthenon/mesh/nx2=1", "parthenon/mesh/nx3=1", "parthenon/meshblock/nx1=256",
    "parthenon/meshblock/nx2=1", "parthenon/meshblock/nx3=1", "problem/along_x1=true", "problem/amp=1.0e-6",
    "problem/wave_flag=0", "problem/vflow=0.0", "parthenon/time/nlim=100000"])  # tests/test_config0_linwave1d.py
BLAST_2D = dict(deck=["blast", "blast.in"], overrides=[
    "parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16",
    "problem/radius=0.3", "problem/samples=0"])
# linear_wave_amr.in at half resolution (tests/test_adaptive_cpu.py); derefine_count 3 so that blocks merge as well as
# split inside each half of the run
LINWAVE_AMR = dict(deck=["linwave", "linear_wave_amr.in"], overrides=[
    "problem/nperiod=1", "parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx1=8",
    "parthenon/meshblock/nx2=8", "parthenon/mesh/derefine_count=3"])


@pytest.mark.parametrize("name,case,n1,n2", [("linwave1d", LINWAVE_1D, 37, -1), ("blast2d", BLAST_2D, 5, 6),
                                            ("linwave_amr", LINWAVE_AMR, 22, 23)])
def test_restored_run_continues_bit_for_bit(tmp_path, name, case, n1, n2):
    res = run(1, case, pattern_actions(str(tmp_path / "ck"), n1, n2), tmp_path, name)
    check_pattern(res, res, res)
    m = res[0][0]
    assert m["S"]["ncycle"] == n1 and m["B"]["ncycle"] > n1
    if name == "linwave1d":  # ran to the deck's time limit: the tlim clamp of the last step is part of the check
        assert m["B"]["errors"][0] > 0.0 and m["B"]["time"] >= 3.0
    if name == "linwave_amr":  # at least two remeshes in each half, or the derefinement counters would not matter
        assert m["S"]["remeshes"] >= m["I"]["remeshes"] + 2 and m["B"]["remeshes"] >= m["S"]["remeshes"] + 2
        assert set(m["B"]["levels"]) == {0, 1}


def test_save_at_cycle_zero_and_unfused_path(tmp_path):
    """A checkpoint written before the first step holds dt = DBL_MAX: the restored run derives its first dt like a fresh
    one.  The per-task chain (set_path is a runtime setting: re-applied after the restore) continues bit for bit too."""
    ck = str(tmp_path / "ck0")
    res = run(1, BLAST_2D, pattern_actions(ck, 0, 4), tmp_path, "zero")
    check_pattern(res, res, res)
    assert res[0][0]["S"]["ncycle"] == 0 and res[0][0]["S"]["dt"] > 1e300 and res[0][0]["B"]["ncycle"] == 4
    cku = str(tmp_path / "cku")
    acts = [["create"], ["path", "unfused"], ["evolve", 3], ["evolve", 3], ["dump", "A"], ["close"],
            ["create"], ["path", "unfused"], ["evolve", 3], ["dump", "S"], ["save", cku], ["close"],
            ["restore", cku, []], ["path", "unfused"], ["dump", "R"], ["evolve", 3], ["dump", "B"], ["close"]]
    res = run(1, BLAST_2D, acts, tmp_path, "unfused")
    check_pattern(res, res, res)
    assert res[0][0]["B"]["stage_kernel"] == "per-task chain"


def test_any_rank_count_reads_any_checkpoint(tmp_path):
    """Saved by 2 ranks under gloo, restored by 1 and by 3 (the Z-order split of the adaptive mesh deals the blocks of
    the file anew): fields, time and dt equal the straight one-rank run bit for bit."""
    ck = str(tmp_path / "ck2")
    n1, n2 = 22, 10
    straight = run(1, LINWAVE_AMR, [["create"], ["evolve", n1], ["evolve", n2], ["dump", "A"], ["close"]], tmp_path, "one")
    saved = run(2, LINWAVE_AMR, [["create"], ["evolve", n1], ["dump", "S"], ["save", ck], ["close"]], tmp_path, "two")
    assert sorted(os.listdir(ck)) == ["part-00000.bin", "part-00001.bin"] and not os.path.exists(ck + ".tmp")
    for world in (1, 3):
        cont = run(world, LINWAVE_AMR, [["restore", ck, []], ["dump", "R"], ["evolve", n2], ["dump", "B"], ["close"]],
                   tmp_path, "w%d" % world)
        assert sum(m["R"]["nblocks"] for m, _ in cont) == saved[0][0]["S"]["nblocks_global"]
        check_pattern(straight, saved, cont, same_ranks=False)
        for m, _ in cont:
            assert m["B"]["time"] == straight[0][0]["A"]["time"] and m["B"]["dt"] == straight[0][0]["A"]["dt"]


def test_nbody_sums_across_rank_counts(tmp_path):
    """The disk + planet + dust deck of tests/amr_cases.py: the accumulated particle_force rows are exact when the rank
    count stays (1 -> 1), and agree to 1e-11 of their magnitude when the parts of 2 ranks are summed into 1 or dealt to 3
    (the tolerance tests/test_adaptive.py uses for these sums: the order of the additions changes)."""
    import amr_cases
    c = amr_cases.disk_planet_dust_amr()
    case = dict(deck=list(c["deck"]), overrides=c["overrides"])
    n1, n2 = 3, 3
    ck1, ck2 = str(tmp_path / "n1"), str(tmp_path / "n2")
    one = run(1, case, pattern_actions(ck1, n1, n2), tmp_path, "nb1")
    check_pattern(one, one, one)
    fa = np.array(one[0][0]["A"]["nbody"])
    assert np.abs(fa).max() > 0.0 and np.array_equal(fa, np.array(one[0][0]["B"]["nbody"]))
    saved = run(2, case, [["create"], ["evolve", n1], ["dump", "S", False], ["save", ck2], ["close"]], tmp_path, "nb2")
    for world in (1, 3):
        cont = run(world, case, [["restore", ck2, []], ["dump", "R", False], ["evolve", n2], ["dump", "B"], ["close"]], tmp_path, "nbw%d" % world)
        check_pattern(one, saved, cont, same_ranks=False)
        for m, _ in cont:  # (the read is an all-reduce: every rank holds the same sums)
            assert np.all(np.abs(np.array(m["B"]["nbody"]) - fa) <= 1e-11 * np.abs(fa).max()), world


def test_malformed_checkpoints_are_refused_by_name_and_the_process_goes_on(tmp_path):
    """Each malformed input raises RuntimeError naming the cause; the same process then restores the intact checkpoint."""
    ck = str(tmp_path / "good")
    run(1, LINWAVE_1D, [["create"], ["evolve", 5], ["save", ck], ["close"]], tmp_path, "mk")
    part = os.path.join(ck, "part-00000.bin")
    raw = open(part, "rb").read()
    d = run(1, LINWAVE_1D, [["describe", "D", ck]], tmp_path, "d")[0][0]["D"]
    payload = 6 * d["block_zones"][0] * 8
    assert len(raw) > payload

    def variant(name, data=None):
        p = str(tmp_path / name)
        shutil.copytree(ck, p)
        if data is None:
            os.remove(os.path.join(p, "part-00000.bin"))
        else:
            open(os.path.join(p, "part-00000.bin"), "wb").write(data)
        return p

    flipped = bytearray(raw)
    flipped[len(raw) - payload // 2] ^= 0x10
    head = bytearray(raw)
    head[100] ^= 0x01
    cases = [("truncated", variant("truncated", raw[:len(raw) - 100]), [], "truncated"),
             ("flipped", variant("flipped", bytes(flipped)), [], "checksum mismatch in the payload"),
             ("header", variant("header", bytes(head)), [], "checksum mismatch in the header"),
             ("magic", variant("magic", b"NOTACKPT" + raw[8:]), [], "wrong magic"),
             ("deleted", variant("deleted"), [], "missing part"),
             ("nx1", ck, ["parthenon/meshblock/nx1=128"], "parthenon/meshblock/nx1"),
             ("nowhere", str(tmp_path / "nowhere"), [], "no checkpoint directory")]
    acts = [["refuse", n, p, ov] for n, p, ov, _ in cases]
    acts += [["restore", ck, ["parthenon/time/nlim=8"]], ["evolve", -1], ["dump", "B"], ["close"]]
    m = run(1, LINWAVE_1D, acts, tmp_path, "refuse")[0][0]
    for n, _, _, cause in cases:
        assert m[n] is not None and cause in m[n], (n, m[n])
    assert m["B"]["ncycle"] == 8  # (an accepted override, applied after the stored ones; and the process went on)


def test_describe_checkpoint_and_size_bound(tmp_path):
    """describe_checkpoint returns the header without a device or a communicator; the checkpoint is no larger than the
    format allows: payload + deck text + 64 B per block + 4 KB."""
    ck = str(tmp_path / "ck")
    run(1, BLAST_2D, [["create"], ["evolve", 3], ["save", ck], ["close"]], tmp_path, "mk")
    d = run(1, BLAST_2D, [["describe", "D", ck]], tmp_path, "d")[0][0]["D"]
    assert d["ncycle"] == 3 and d["nblocks"] == 4 and d["nranks"] == 1 and d["block_shape"] == [16, 16, 1]
    assert d["nghost"] == 2 and d["ns_gas"] == 1 and d["ns_dust"] == 0 and d["ndim"] == 2 and d["integrator"] == "rk2"
    assert d["overrides"] == BLAST_2D["overrides"] and d["time"] > 0.0 and d["dt"] > 0.0 and not d["adaptive"]
    assert d["deck"] == open(os.path.join(ROOT, "inputs", "blast", "blast.in")).read()
    size = sum(os.path.getsize(os.path.join(ck, f)) for f in os.listdir(ck))
    assert d["bytes"] == size
    assert size <= 4 * 6 * 20 * 20 * 1 * 8 + len(d["deck"]) + 64 * 4 + 4096


def test_reader_survives_damaged_checkpoints_under_host_sanitizers(tmp_path):
    """tests/restart_reader: a stand-alone program (driver sources + CPU double, -fsanitize=address,undefined) saves a
    16-zone 1-D run and restores from copies truncated at every 97th byte and from copies with one byte changed at 500
    positions over header and directory.  Every restore succeeds or fails cleanly; a sanitizer report aborts it."""
    d = os.path.join(ROOT, "tests", "restart_reader")
    subprocess.check_call(["make", "-C", d, "-s", "-j4"])
    p = subprocess.run([os.path.join(ROOT, "tests", "_build", "restart_reader"), os.path.join(ROOT, "inputs", "linwave", "linear_wave.in"),
                        str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-3000:]
    assert "restart_reader: ok" in out
