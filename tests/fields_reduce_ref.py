"""The definition of a reduced field output (include/artemis_hip.h, artemis_hip_reduce_fields), emulated in numpy for
tests/test_fields_reduce.py and tests/test_fields_reduce_cpu.py.  Not a test module.

Per zone and component the leaf is N = V q and W = V.  Both are reduced one direction at a time, x1 first, then x2, then x3,
the directions not asked for skipped:
    x1        the row is cut into chunks of 64 from its first zone, the last chunk padded with +0.0; six times
              x[..., 0::2] + x[..., 1::2] gives a chunk's sum (the butterfly x'[l] = x[l] + x[l ^ (1 << m)], m = 0..5, leaves
              exactly that tree in every lane); the chunks are added in increasing order, acc = chunk[0]; acc = acc + chunk[1]
    x2, x3    acc = x[0]; acc = acc + x[1]; ... in increasing index, from the first element and not from 0.0
numpy adds float64 arrays element by element with IEEE additions, so these are the bits the device must give; np.sum, which
sums pairwise, is never used."""
import numpy as np

from fields_level_ref import oracle_volumes, same_bits  # noqa: F401  (shared with the tests)

AXES = {"x1": 1, "x2": 2, "x3": 4}


def mask(names):
    return sum(AXES[n] for n in names)


def names_of(axes):
    return tuple(n for n, bit in AXES.items() if axes & bit)


def reduce_x1(x):
    """[..., nx] -> [..., 1]"""
    nx = x.shape[-1]
    pad = (-nx) % 64
    if pad:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), dtype=np.float64)], axis=-1)  # the literal +0.0
    acc = None
    for c0 in range(0, x.shape[-1], 64):
        chunk = x[..., c0:c0 + 64]
        for _ in range(6):
            chunk = chunk[..., 0::2] + chunk[..., 1::2]
        acc = chunk if acc is None else acc + chunk
    return acc


def reduce_seq(x, axis):
    """sequential along `axis`, which is kept with extent 1"""
    x = np.moveaxis(x, axis, 0)
    acc = x[0].copy()
    for t in range(1, x.shape[0]):
        acc = acc + x[t]
    return np.moveaxis(acc[None], 0, axis)


def reduce_block(q, vol, axes, single=False):
    """q [ncomp, nz, ny, nx] float64 at full resolution, vol [nz, ny, nx] -> [ncomp + 1, nz', ny', nx'], the volume last"""
    q = np.asarray(q, dtype=np.float64)
    vol = np.asarray(vol, dtype=np.float64)
    x = np.concatenate([vol[None] * q, vol[None]], axis=0)
    if axes & 1:
        x = reduce_x1(x)
    if axes & 2:
        x = reduce_seq(x, 2)
    if axes & 4:
        x = reduce_seq(x, 1)
    return x.astype(np.float32) if single else x


def out_shape(nx, axes):
    """(nz', ny', nx') of a block of nx = (nx1, nx2, nx3)"""
    return tuple(1 if (axes >> d) & 1 else nx[d] for d in range(3))[::-1]


def subsets(nx):
    """every non-empty mask of the active directions of nx = (nx1, nx2, nx3)"""
    active = sum(1 << d for d in range(3) if nx[d] > 1)
    return [a for a in range(1, 8) if a & ~active == 0]


def assemble(blocks, num, den, axes, nx):
    """The independent form of FieldDump.reduced on a one-level mesh: (N, W) with the blocks (dicts with "bounds", gid
    order) placed by bounds along the kept directions; the first block at a cell is assigned, each later one added."""
    kept = [d for d in range(3) if not (axes >> d) & 1 and nx[d] > 1]
    lo = [min(b["bounds"][2 * d] for b in blocks) for d in range(3)]
    hi = [max(b["bounds"][2 * d + 1] for b in blocks) for d in range(3)]
    w = [blocks[0]["bounds"][2 * d + 1] - blocks[0]["bounds"][2 * d] for d in range(3)]
    n = [int(round((hi[d] - lo[d]) / w[d])) * nx[d] if d in kept else 1 for d in range(3)]
    N, W = {}, {}
    shape = None
    for b, bn, bw in zip(blocks, num, den):
        o = [int(round((b["bounds"][2 * d] - lo[d]) / w[d])) * nx[d] if d in kept else 0 for d in range(3)]
        bn, bw = np.asarray(bn, dtype=np.float64), np.asarray(bw, dtype=np.float64)
        shape = bn.shape[0]
        for k in range(bn.shape[1]):
            for j in range(bn.shape[2]):
                for i in range(bn.shape[3]):
                    at = (o[2] + k, o[1] + j, o[0] + i)
                    N[at] = bn[:, k, j, i] if at not in N else N[at] + bn[:, k, j, i]
                    W[at] = bw[:, k, j, i] if at not in W else W[at] + bw[:, k, j, i]
    outN, outW = np.full((shape, n[2], n[1], n[0]), np.nan), np.full((1, n[2], n[1], n[0]), np.nan)
    for at in N:
        outN[(slice(None),) + at], outW[(slice(None),) + at] = N[at], W[at]
    return outN, outW
