"""The definition of a field output at a refinement level (include/artemis_hip.h, artemis_hip_pack_fields_level), emulated in
numpy for tests/test_fields_level.py and tests/test_fields_level_cpu.py.  Not a test module.

A block on level l asked for level L has shift s = l - L.  s >= 1: per zone N = V q and V, both s times up the reference's
tree ((c000 + c010) + (c001 + c011)) + ((c100 + c110) + (c101 + c111)) -- the offset-1 children of an inactive direction
(one zone) are the literal 0.0 -- and the output is N / V.  s <= -1: every zone repeated 2^|s| times along the active
directions.  numpy adds float64 arrays element by element with IEEE additions, so these are the bits the device must give."""
import numpy as np


def tree(x, active):
    """one level of the tree over the last three axes [nz, ny, nx]; active = (x1, x2, x3 have more than one zone)"""
    ax, ay, az = active

    def c(ok, oj, oi):
        if (ok and not az) or (oj and not ay) or (oi and not ax):
            return np.zeros_like(c(0, 0, 0))
        return x[..., (slice(ok, None, 2) if az else slice(None)), (slice(oj, None, 2) if ay else slice(None)),
                 (slice(oi, None, 2) if ax else slice(None))]
    return ((c(0, 0, 0) + c(0, 1, 0)) + (c(0, 0, 1) + c(0, 1, 1))) + ((c(1, 0, 0) + c(1, 1, 0)) + (c(1, 0, 1) + c(1, 1, 1)))


def resample(q, vol, shift, single=False):
    """q [ncomp, nz, ny, nx] float64 at full resolution, vol [nz, ny, nx] -> the block at `shift`"""
    q = np.asarray(q, dtype=np.float64)
    active = tuple(q.shape[-1 - d] > 1 for d in range(3))
    if shift > 0:
        num, den = vol * q, np.array(vol, dtype=np.float64)
        for _ in range(shift):
            num, den = tree(num, active), tree(den, active)
        out = num / den
    else:
        out = q
        for d in range(3):
            if active[d] and shift < 0:
                out = np.repeat(out, 1 << -shift, axis=q.ndim - 1 - d)
    return out.astype(np.float32) if single else out


def same_bits(a, b):
    """equal shape, dtype and bit patterns (so -0.0 differs from +0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def oracle_volumes(nx, xmin, xmax, ng, coordinates):
    """Coords::Volume of the interior zones of a block with these bounds, [nz, ny, nx], from the CPU oracle"""
    from oracle.oracle import Oracle
    o = Oracle(tuple(nx), tuple(xmin), tuple(xmax), ng=ng, coordinates=coordinates)
    return np.ascontiguousarray(o.face_areas(0)[o.ks:o.ke + 1, o.js:o.je + 1, o.is_:o.ie + 1])


def place(blocks, data):
    """[ncomp, NZ, NY, NX] from per-block arrays of one zone size and the blocks' bounds: the independent form of
    FieldDump.uniform on a version-2 dump"""
    lo = [min(b["bounds"][2 * d] for b in blocks) for d in range(3)]
    hi = [max(b["bounds"][2 * d + 1] for b in blocks) for d in range(3)]
    shape0 = data[0].shape[:0:-1]  # (nx, ny, nz) of block 0
    dz = [(blocks[0]["bounds"][2 * d + 1] - blocks[0]["bounds"][2 * d]) / shape0[d] for d in range(3)]
    n = [int(round((hi[d] - lo[d]) / dz[d])) for d in range(3)]
    out = np.full((data[0].shape[0], n[2], n[1], n[0]), np.nan, dtype=data[0].dtype)
    for b, a in zip(blocks, data):
        o = [int(round((b["bounds"][2 * d] - lo[d]) / (hi[d] - lo[d]) * n[d])) for d in range(3)]
        out[:, o[2]:o[2] + a.shape[1], o[1]:o[1] + a.shape[2], o[0]:o[0] + a.shape[3]] = a
    return out
