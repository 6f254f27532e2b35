"""The definition of a reduced field output on a chosen level (include/artemis_hip.h, artemis_hip_reduce_fields_level),
emulated in numpy for tests/test_fields_reduce_level.py and tests/test_fields_reduce_level_cpu.py.  Not a test module.

Step 1 is reduce_block of tests/fields_reduce_ref.py: the block reduced at its own resolution, N_c and W as doubles.  A block
with shift s = its level - the level asked for is then brought there along the KEPT directions -- the active ones (more than
one zone) outside `axes`, m of them -- and along no other:
    s == 0    nothing more
    s >= 1    for each kept direction in the order x1, x2, x3:  x = x[0::2] + x[1::2] along it, s times
    s <= -1   x times the double 2^(-|s| m), then every element repeated 2^|s| times along each kept direction; m == 0: nothing
and only then narrowed to float.  numpy adds and multiplies float64 arrays element by element with IEEE operations, so these
are the bits the device must give."""
import numpy as np

from fields_reduce_ref import reduce_block


def kept_directions(axes, active):
    return [d for d in range(3) if active[d] and not (axes >> d) & 1]


def resample_reduced(block, s, axes, active):
    """block [ncomp + 1, nz', ny', nx'] float64, what reduce_block leaves; active = (x1, x2, x3 have more than one zone in the
    mesh block) -> the block at shift s, float64"""
    x = np.asarray(block, dtype=np.float64)
    assert x.dtype == np.float64 and abs(s) <= 3
    kept = kept_directions(axes, active)
    for d in kept if s > 0 else ():
        ax = x.ndim - 1 - d
        for _ in range(s):
            assert x.shape[ax] % 2 == 0
            even, odd = [slice(None)] * x.ndim, [slice(None)] * x.ndim
            even[ax], odd[ax] = slice(0, None, 2), slice(1, None, 2)
            x = x[tuple(even)] + x[tuple(odd)]
    if s < 0 and kept:
        x = x * np.float64(2.0) ** (s * len(kept))
        for d in kept:
            x = np.repeat(x, 1 << -s, axis=x.ndim - 1 - d)
    return np.ascontiguousarray(x)


def reduce_block_level(q, vol, axes, s, single=False):
    """q [ncomp, nz, ny, nx] float64 at full resolution, vol [nz, ny, nx] -> [ncomp + 1, nz', ny', nx'] at shift s, W last"""
    active = tuple(np.asarray(q).shape[-1 - d] > 1 for d in range(3))
    x = resample_reduced(reduce_block(q, vol, axes), s, axes, active)
    return x.astype(np.float32) if single else x


def out_shape_level(nx, axes, s):
    """(nz', ny', nx') of a block of nx = (nx1, nx2, nx3) at shift s"""
    return tuple(1 if (axes >> d) & 1 or nx[d] == 1 else (nx[d] >> s if s >= 0 else nx[d] << -s) for d in range(3))[::-1]


def allowed_levels(levels, nx, axes):
    """every reduce_level that keeps |shift| <= 3 for all `levels` of a mesh whose kept extents the shifts divide"""
    out = []
    for L in range(min(levels) - 3, max(levels) + 4):
        shifts = [l - L for l in levels]
        if all(abs(s) <= 3 for s in shifts) and all(nx[d] % (1 << s) == 0 for s in shifts if s > 0 for d in range(3)
                                                  if nx[d] > 1 and not (axes >> d) & 1):
            out.append(L)
    return out


def place_sum(blocks, num, den, axes, nx):
    """The independent form of FieldDump.reduced on a version-4 dump: (N, W, cover) with the blocks (dicts with "bounds", gid
    order; num / den their [ncomp, nz_b, ny_b, nx_b] / [1, ...] arrays on ONE zone size) placed by the fraction of the mesh
    their lower bounds mark; the first block at a cell assigned, each later one added.  cover: how many blocks met a cell."""
    kept = kept_directions(axes, tuple(n > 1 for n in nx))
    lo = [min(b["bounds"][2 * d] for b in blocks) for d in range(3)]
    hi = [max(b["bounds"][2 * d + 1] for b in blocks) for d in range(3)]
    first = num[0].shape[:0:-1]
    n = [int(round((hi[d] - lo[d]) / (blocks[0]["bounds"][2 * d + 1] - blocks[0]["bounds"][2 * d]) * first[d])) if d in kept else 1
         for d in range(3)]
    N = np.full((num[0].shape[0], n[2], n[1], n[0]), np.nan)
    W = np.full((1, n[2], n[1], n[0]), np.nan)
    cover = np.zeros((n[2], n[1], n[0]), dtype=int)
    for b, bn, bw in zip(blocks, num, den):
        o = [int(round((b["bounds"][2 * d] - lo[d]) / (hi[d] - lo[d]) * n[d])) if d in kept else 0 for d in range(3)]
        at = tuple(slice(o[d], o[d] + bn.shape[3 - d]) for d in (2, 1, 0))
        assert cover[at].shape == bn.shape[1:]
        new = cover[at] == 0
        for out, x in ((N, bn), (W, bw)):
            x = np.asarray(x, dtype=np.float64)
            with np.errstate(invalid="ignore"):
                out[(slice(None),) + at] = np.where(new, x, out[(slice(None),) + at] + x)
        cover[at] += 1
    return N, W, cover
