"""Reader of the field dumps the host driver writes (<problem_id>.outN.<counter>.fld, Simulation.write_fields;
include/artemis_driver.h "field output"): a directory with meta.json -- clock, variables, and one entry per mesh block of
the global mesh in gid order -- and one raw little-endian part rank<r>.bin per writing rank, [block][component][nz][ny][nx]
over interior zones.  Version 1: every block has the zones of a mesh block.  Version 2 (write_fields(level=L), a deck's
`level = L`): every block was resampled to the zone size of refinement level L on the device, so the blocks differ in shape
-- each entry carries its own nx and the element offset of its first value in its rank's part -- and share one zone size.
Version 3 (write_fields(reduce=("x2", "x3")), a deck's `reduce = x2,x3`): every block was integrated over those directions
on the device -- per component N = sum of V q, and W = sum of V as the last variable, "volume" -- in an order of additions
that depends on the block alone (include/artemis_hip.h, artemis_hip_reduce_fields); the reduced extents of every nx are 1.
FieldDump.reduced() adds the blocks and forms the means.  Version 4 (write_fields(reduce=..., reduce_level=L), a deck's
`reduce_level = L` beside `reduce`): a version-3 dump whose blocks were also brought to the zone size of refinement level L
along the directions they keep (include/artemis_hip.h, artemis_hip_reduce_fields_level) -- each entry carries its own nx and
offset -- so reduced() assembles it on any mesh.  Needs numpy only and no device."""
import json
import os

import numpy as np

FORMAT, VERSIONS = "artemis_fld", (1, 2, 3, 4)


class FieldDump:
    """time, dt, cycle, coordinates, ndim, gamma, dtype; variables: {name: number of components}; components: {name: their
    names}; blocks: [{gid, level, bounds, nx}] in gid order; level: None, or the level a version-2 dump was resampled to;
    reduce: None, or the directions (["x2", "x3"]) a version-3 or version-4 dump was integrated over; reduce_level: None, or
    the level the kept directions of a version-4 dump were brought to."""

    def __init__(self, path, meta):
        self.path, self.meta = path, meta
        for k in ("time", "dt", "cycle", "coordinates", "ndim", "gamma"):
            setattr(self, k, meta[k])
        self.version = meta["version"]
        self.level = meta["level"] if self.version == 2 else None
        self.reduce = list(meta["reduce"]) if self.version in (3, 4) else None
        self.reduce_level = meta["reduce_level"] if self.version == 4 else None
        self.dtype = np.dtype(meta["dtype"])
        self.variables = {v["name"]: v["ncomp"] for v in meta["variables"]}
        self.components = {v["name"]: list(v["components"]) for v in meta["variables"]}
        self.blocks = [dict(gid=b["gid"], level=b["level"], bounds=list(b["bounds"]), nx=list(b["nx"])) for b in meta["blocks"]]
        self.ncomp = sum(self.variables.values())
        self.nx = list(meta["nx"])
        self._parts = {}

    def _elements(self, b):
        return self.ncomp * b["nx"][0] * b["nx"][1] * b["nx"][2]

    def _offset(self, b):
        """element offset of a block of meta["blocks"] in its rank's part"""
        return b["offset"] if self.version >= 2 else b["index"] * self._elements(b)

    def _part(self, rank):
        """the part of that rank as a flat read-only memory map"""
        if rank not in self._parts:
            name = os.path.join(self.path, "rank%d.bin" % rank)
            mine = [b for b in self.meta["blocks"] if b["rank"] == rank]
            count = sum(self._elements(b) for b in mine)
            want = count * self.dtype.itemsize
            if not os.path.isfile(name):
                raise ValueError("%s: part %s is missing" % (self.path, os.path.basename(name)))
            have = os.path.getsize(name)
            if have != want or any(self._offset(b) + self._elements(b) > count for b in mine):
                raise ValueError("%s: part %s holds %d bytes, meta.json describes %d (truncated or not of this dump)"
                                 % (self.path, os.path.basename(name), have, want))
            self._parts[rank] = np.memmap(name, dtype=self.dtype, mode="r", shape=(count,)) if want else np.empty((0,), self.dtype)
        return self._parts[rank]

    def _at(self, name):
        if name not in self.variables:
            raise KeyError("%s holds %s, not %s" % (self.path, ", ".join(self.variables), name))
        at = 0
        for v in self.meta["variables"]:
            if v["name"] == name:
                break
            at += v["ncomp"]
        return at, self.variables[name]

    def get_blocks(self, name):
        """The variable block by block, in gid order: a list of [ncomp of the variable, nz_b, ny_b, nx_b] arrays (views of
        the parts).  Works on every dump."""
        at, n = self._at(name)
        out = []
        for b in self.meta["blocks"]:
            nx, o = b["nx"], self._offset(b)
            out.append(self._part(b["rank"])[o:o + self._elements(b)].reshape(self.ncomp, nx[2], nx[1], nx[0])[at:at + n])
        return out

    def get(self, name):
        """[nblocks_global, ncomp of the variable, nz, ny, nx] in gid order; ValueError where the blocks differ in shape
        (a dump at a level of a refined mesh): get_blocks gives them one by one."""
        at, n = self._at(name)
        shapes = {tuple(b["nx"]) for b in self.blocks}
        if len(shapes) > 1:
            raise ValueError("%s: its blocks differ in shape (%s) and do not form one array: use get_blocks(%r)"
                             % (self.path, ", ".join(str(list(s)) for s in sorted(shapes)), name))
        nx = self.blocks[0]["nx"] if self.blocks else self.nx
        out = np.empty((len(self.meta["blocks"]), n, nx[2], nx[1], nx[0]), dtype=self.dtype)
        for g, blk in enumerate(self.get_blocks(name)):
            out[g] = blk
        return out

    def uniform(self, name):
        """One [ncomp, NZ, NY, NX] array of the whole mesh, every block placed by its bounds with its own nx.  Every
        version-2 dump forms one (all its blocks share one zone size); a version-1 dump only where every block is on one
        refinement level (ValueError otherwise)."""
        levels = {b["level"] for b in self.blocks}
        if self.version < 2 and len(levels) != 1:
            raise ValueError("%s: blocks on levels %s do not form one uniform array" % (self.path, sorted(levels)))
        data = self.get_blocks(name)
        lo = [min(b["bounds"][2 * d] for b in self.blocks) for d in range(3)]
        hi = [max(b["bounds"][2 * d + 1] for b in self.blocks) for d in range(3)]
        # the zone size, from the first block; every block then starts a whole number of zones from the mesh's corner
        b0 = self.blocks[0]
        dz = [(b0["bounds"][2 * d + 1] - b0["bounds"][2 * d]) / b0["nx"][d] for d in range(3)]
        n = [int(round((hi[d] - lo[d]) / dz[d])) for d in range(3)]
        out = np.empty((data[0].shape[0], n[2], n[1], n[0]), dtype=self.dtype)
        filled = 0
        for b, blk in zip(self.blocks, data):
            o = [int(round((b["bounds"][2 * d] - lo[d]) / dz[d])) for d in range(3)]
            m = b["nx"]
            if any(int(round((b["bounds"][2 * d + 1] - b["bounds"][2 * d]) / dz[d])) != m[d] for d in range(3)):
                raise ValueError("%s: block %d is not on the zone size of block 0" % (self.path, b["gid"]))
            out[:, o[2]:o[2] + m[2], o[1]:o[1] + m[1], o[0]:o[0] + m[0]] = blk
            filled += m[0] * m[1] * m[2]
        if filled != n[0] * n[1] * n[2]:
            raise ValueError("%s: the blocks do not tile their bounding box" % self.path)
        return out

    def reduced(self, name, op=None):
        """A version-3 or version-4 dump assembled into one [ncomp, NZ, NY, NX] float64 array of the whole mesh, the reduced extents 1:
        every block is placed by its bounds in the kept directions, and blocks that meet the same output cell are added as
        float64 in gid order -- the first one assigned, each later one added -- both the integrals N and the volumes W.
        op = "integral": N; op = "mean": N / W, one division per cell.  gid order is global, so the bits do not depend on
        the number of ranks that wrote the dump.  On a mesh with several refinement levels the kept directions have no
        common zone size in a version-3 dump: only one with every active direction reduced (scalars) is assembled, any other
        is refused.  A version-4 dump (reduce_level) of any mesh is assembled: its blocks share the zone size of that level.
        There each of the 2^(|s| m) cells under a block |s| levels coarser (m kept directions) received an EQUAL share of
        that zone's N and W -- even in index space, not geometric.  op="mean" is exact on every mesh, each such cell holding
        the coarse zone's own mean where no other block adds to it.  op="integral" of a single cell under a coarser block
        is its even share: on a curvilinear mesh the sub-volumes of a coarse zone along a kept direction are not equal, so
        only sums over the cells of whole coarse zones are exact there; on Cartesian meshes every cell is.
        name = "volume" returns W itself, [1, NZ, NY, NX]; it has no mean, so `op` must be "integral" or left at its default
        (ValueError for an explicit op="mean")."""
        if self.reduce is None:
            raise ValueError("%s is not a reduced dump (version %d)" % (self.path, self.version))
        if name == "volume" and op == "mean":
            raise ValueError("reduced: the volume is an integral and has no mean")
        op = "mean" if op is None else op
        if op not in ("mean", "integral"):
            raise ValueError("reduced: op is 'mean' or 'integral', not %r" % (op,))
        axes = {int(a[1]) - 1 for a in self.reduce}
        kept = [d for d in range(3) if d not in axes and self.nx[d] > 1]
        levels = sorted({b["level"] for b in self.blocks})
        if len(levels) != 1 and kept and self.reduce_level is None:
            raise ValueError("%s: blocks on levels %s kept along %s do not share a zone size: only a dump with every active "
                             "direction reduced is assembled on a refined mesh"
                             % (self.path, levels, ", ".join("x%d" % (d + 1) for d in kept)))
        lo = [min(b["bounds"][2 * d] for b in self.blocks) for d in range(3)]
        hi = [max(b["bounds"][2 * d + 1] for b in self.blocks) for d in range(3)]
        b0 = self.blocks[0]
        dz = [(b0["bounds"][2 * d + 1] - b0["bounds"][2 * d]) / b0["nx"][d] for d in range(3)]
        n = [int(round((hi[d] - lo[d]) / dz[d])) if d in kept else 1 for d in range(3)]
        num, den = self.get_blocks(name), self.get_blocks("volume")
        N = np.zeros((num[0].shape[0], n[2], n[1], n[0]), dtype=np.float64)
        W = np.zeros((1, n[2], n[1], n[0]), dtype=np.float64)
        seen = np.zeros((n[2], n[1], n[0]), dtype=bool)
        for b, bn, bw in zip(self.blocks, num, den):
            o = [int(round((b["bounds"][2 * d] - lo[d]) / dz[d])) if d in kept else 0 for d in range(3)]
            m = b["nx"]
            at = (slice(o[2], o[2] + m[2]), slice(o[1], o[1] + m[1]), slice(o[0], o[0] + m[0]))
            if seen[at].shape != tuple(m[::-1]):
                raise ValueError("%s: block %d does not lie inside the mesh" % (self.path, b["gid"]))
            old = seen[at]
            N[(slice(None),) + at] = np.where(old, N[(slice(None),) + at] + bn.astype(np.float64), bn.astype(np.float64))
            W[(slice(None),) + at] = np.where(old, W[(slice(None),) + at] + bw.astype(np.float64), bw.astype(np.float64))
            seen[at] = True
        if not seen.all():
            raise ValueError("%s: the blocks do not cover their bounding box" % self.path)
        if name == "volume":
            return W
        return N / W if op == "mean" else N


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
