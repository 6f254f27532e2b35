"""Reader of the field dumps the host driver writes (<problem_id>.outN.<counter>.fld, Simulation.write_fields;
include/artemis_driver.h "field output"): a directory with meta.json -- clock, variables, and one entry per mesh block of
the global mesh in gid order -- and one raw little-endian part rank<r>.bin per writing rank, [block][component][nz][ny][nx]
over interior zones.  Needs numpy only and no device."""
import json
import os

import numpy as np

FORMAT, VERSIONS = "artemis_fld", (1,)


class FieldDump:
    """time, dt, cycle, coordinates, ndim, gamma, dtype; variables: {name: number of components}; components: {name: their
    names}; blocks: [{gid, level, bounds, nx}] in gid order."""

    def __init__(self, path, meta):
        self.path, self.meta = path, meta
        for k in ("time", "dt", "cycle", "coordinates", "ndim", "gamma"):
            setattr(self, k, meta[k])
        self.dtype = np.dtype(meta["dtype"])
        self.variables = {v["name"]: v["ncomp"] for v in meta["variables"]}
        self.components = {v["name"]: list(v["components"]) for v in meta["variables"]}
        self.blocks = [dict(gid=b["gid"], level=b["level"], bounds=list(b["bounds"]), nx=list(b["nx"])) for b in meta["blocks"]]
        self.ncomp = sum(self.variables.values())
        self.nx = list(meta["nx"])
        self._parts = {}

    def _part(self, rank):
        """[blocks of that rank, ncomp, nz, ny, nx] as a read-only memory map"""
        if rank not in self._parts:
            name = os.path.join(self.path, "rank%d.bin" % rank)
            nblk = sum(1 for b in self.meta["blocks"] if b["rank"] == rank)
            shape = (nblk, self.ncomp, self.nx[2], self.nx[1], self.nx[0])
            want = int(np.prod(shape)) * self.dtype.itemsize
            if not os.path.isfile(name):
                raise ValueError("%s: part %s is missing" % (self.path, os.path.basename(name)))
            have = os.path.getsize(name)
            if have != want:
                raise ValueError("%s: part %s holds %d bytes, meta.json describes %d (truncated or not of this dump)"
                                 % (self.path, os.path.basename(name), have, want))
            self._parts[rank] = np.memmap(name, dtype=self.dtype, mode="r", shape=shape) if want else np.empty(shape, self.dtype)
        return self._parts[rank]

    def get(self, name):
        """[nblocks_global, ncomp of the variable, nz, ny, nx] in gid order"""
        if name not in self.variables:
            raise KeyError("%s holds %s, not %s" % (self.path, ", ".join(self.variables), name))
        at = 0
        for v in self.meta["variables"]:
            if v["name"] == name:
                break
            at += v["ncomp"]
        n = self.variables[name]
        out = np.empty((len(self.meta["blocks"]), n, self.nx[2], self.nx[1], self.nx[0]), dtype=self.dtype)
        for g, b in enumerate(self.meta["blocks"]):
            out[g] = self._part(b["rank"])[b["index"], at:at + n]
        return out

    def uniform(self, name):
        """One [ncomp, NZ, NY, NX] array of the whole mesh, every block placed by its bounds.  Only where every block is on
        one refinement level (ValueError otherwise)."""
        levels = {b["level"] for b in self.blocks}
        if len(levels) != 1:
            raise ValueError("%s: blocks on levels %s do not form one uniform array" % (self.path, sorted(levels)))
        data = self.get(name)
        lo = [min(b["bounds"][2 * d] for b in self.blocks) for d in range(3)]
        hi = [max(b["bounds"][2 * d + 1] for b in self.blocks) for d in range(3)]
        w = [self.blocks[0]["bounds"][2 * d + 1] - self.blocks[0]["bounds"][2 * d] for d in range(3)]
        nblk = [int(round((hi[d] - lo[d]) / w[d])) for d in range(3)]
        out = np.empty((data.shape[1], nblk[2] * self.nx[2], nblk[1] * self.nx[1], nblk[0] * self.nx[0]), dtype=self.dtype)
        seen = set()
        for g, b in enumerate(self.blocks):
            at = tuple(int(round((b["bounds"][2 * d] - lo[d]) / w[d])) for d in range(3))
            seen.add(at)
            o = [at[d] * self.nx[d] for d in range(3)]
            out[:, o[2]:o[2] + self.nx[2], o[1]:o[1] + self.nx[1], o[0]:o[0] + self.nx[0]] = data[g]
        if len(seen) != nblk[0] * nblk[1] * nblk[2]:
            raise ValueError("%s: the blocks do not tile their bounding box" % self.path)
        return out


def read_fields(path):
    """The dump at `path` as a FieldDump.  ValueError for a directory without meta.json (a dump is renamed into place only
    when it is complete), a format or version this reader does not know, and a missing or truncated part."""
    path = os.fspath(path)
    name = os.path.join(path, "meta.json")
    if not os.path.isfile(name):
        raise ValueError("%s is not a field dump: no meta.json" % path)
    with open(name) as f:
        meta = json.load(f)
    if meta.get("format") != FORMAT or meta.get("version") not in VERSIONS:
        raise ValueError("%s: format %r version %r is not one this reader knows (%s %s)"
                         % (path, meta.get("format"), meta.get("version"), FORMAT, VERSIONS))
    dump = FieldDump(path, meta)
    for rank in sorted({b["rank"] for b in meta["blocks"]}):
        dump._part(rank)  # (a missing or truncated part is reported now, not at the first get)
    return dump
