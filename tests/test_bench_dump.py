"""bench.py --dump-outputs (dump_outputs()): the final state of the timed path as float64 .npy files -- every interior zone
when they fit, else the same seeded sample of them on every run, within DUMP_FIELD_BYTES.  A stand-in for Simulation
whose primitive values encode (block, zone, variable) runs it without a GPU, in a child process (importing bench sets
OpenMP variables that must not reach this one)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench


class Sim:
    """nb blocks of n^3 interior zones, ng ghost zones; value = 1000 * (global interior zone index) + variable (ghost
    zones -1)."""
    def __init__(self, nb, n, ng, ns_dust):
        self.nblocks, self.ns_gas, self.ns_dust = nb, 1, ns_dust
        self.ni = self.nj = self.nk = n + 2 * ng
        self.is_ = self.js = self.ks = ng
        self.ie = self.je = self.ke = ng + n - 1
        self.n, self.ng, self.dt, self.time = n, ng, 1.0e-3, 0.25

    def field(self, name, block):
        nv = 6 if name == "gas.prim" else 4 * self.ns_dust
        a = -np.ones((nv, self.nk, self.nj, self.ni))
        z = np.arange(self.n ** 3).reshape(self.n, self.n, self.n) + block * self.n ** 3
        g = self.ng
        for v in range(nv):
            a[v, g:g + self.n, g:g + self.n, g:g + self.n] = 1000.0 * z + v
        return a

    def history(self):
        return np.arange(10.0)


nb, n, ns_dust, budget = (int(x) for x in sys.argv[3:7])
bench.DUMP_FIELD_BYTES = budget
bench.dump_outputs(Sim(nb, n, 2, ns_dust), sys.argv[2], 0, 1)
'''


def dump(tmp_path, name, nb, n, ns_dust, budget):
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    out = tmp_path / name
    subprocess.check_call([sys.executable, str(child), ROOT, str(out)] + [str(x) for x in (nb, n, ns_dust, budget)])
    return {f[:-4]: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}


def test_dump_outputs_every_zone_when_they_fit(tmp_path):
    d = dump(tmp_path, "all", 3, 4, 1, 48 << 20)
    assert sorted(d) == ["dt", "dust_prim", "gas_prim", "history", "time"]
    assert all(a.dtype == np.float64 for a in d.values())
    zones = np.arange(3 * 4 ** 3)
    assert np.array_equal(d["gas_prim"], 1000.0 * zones[None, :] + np.arange(6)[:, None])  # block order, no ghost zone
    assert np.array_equal(d["dust_prim"], 1000.0 * zones[None, :] + np.arange(4)[:, None])
    assert d["dt"].tolist() == [1.0e-3] and d["time"].tolist() == [0.25] and d["history"].shape == (10,)


def test_dump_outputs_a_fixed_sample_within_the_bound(tmp_path):
    budget = 8 * 10 * 500  # 500 zones of 6 gas + 4 dust variables
    a = dump(tmp_path, "a", 5, 8, 1, budget)
    b = dump(tmp_path, "b", 5, 8, 1, budget)
    for k in a:
        assert np.array_equal(a[k], b[k]), k  # the same zones on every run
    g = a["gas_prim"]
    assert g.shape == (6, 500) and a["dust_prim"].shape == (4, 500)
    assert g.nbytes + a["dust_prim"].nbytes <= budget
    z = g[0] / 1000.0
    assert np.array_equal(z, np.round(z)) and np.all(np.diff(z) > 0) and 0 <= z[0] and z[-1] < 5 * 8 ** 3
    assert np.array_equal(g, 1000.0 * z[None, :] + np.arange(6)[:, None])  # every variable of one zone in one column
    assert len(set((z // 8 ** 3).astype(int))) == 5  # drawn from every block
