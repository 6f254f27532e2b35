"""GPU parity of Gas / Dust CalculateFluxes against the REFERENCE'S OWN HEADERS, bit for bit, not through the oracle.

Every case uploads random primitives, runs artemis_hip_calculate_fluxes and compares the fluxes, the face pressure and
the face velocity with oracle/_ref/libartemis_ref.so (oracle/ref/ref_leaves.cpp): the reference's unmodified
Reconstruction<>::apply and RiemannSolver<>::solve over scratch rows with the index bounds of fluid_fluxes.hpp:105-206,
and ScaleMomentumFlux as one IEEE multiply by the scale factors of the reference's Coords.  The Oracle objects below
only hold the inputs (the primitives and the block's logical coordinates); Oracle.CalculateFluxes is never called.
The library is built by `make -C oracle` where the reference's source tree is present and travels with the tree; here
it is required, and a missing library fails.
"""
import numpy as np
import pytest

from oracle import reference as ref
from test_parity_geometry import GEOMS
from test_parity_geometry import make_pair as make_curvilinear_pair
from test_parity_ops import face_slices, make_pair, push
from test_reference_leaves import mirror_state

pytestmark = pytest.mark.gpu
GAS, DUST = 0, 1


@pytest.fixture(autouse=True)
def _library():
    ref.need()


def same_bits(got_gpu, want, what):
    g = got_gpu.cpu().numpy()
    assert np.isfinite(want).all(), f"{what}: the reference sweep left faces of the range unwritten"
    if not np.array_equal(g.view(np.int64), np.ascontiguousarray(want).view(np.int64)):
        bad = np.argwhere(g.view(np.int64) != np.ascontiguousarray(want).view(np.int64))
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ in bits from the reference, first at "
                             f"{first}: reference {want[first]!r}, kernel {g[first]!r}")


def check(mb, b, o, fluid=GAS, pcm=False):
    """Block b of the pack against ref_sweep of the same primitives."""
    s = ref.sweep_of(o, fluid, pcm)
    for d in range(o.ndim):
        sl = face_slices(o, d)
        if fluid == GAS:
            same_bits(mb.gas_flux[d][b][sl], s.scaled_flux(d)[sl], f"block {b} gas flux x{d + 1}")
            same_bits(mb.gas_pflux[d][b][sl], s.pflux[d][sl], f"block {b} face pressure x{d + 1}")
            same_bits(mb.gas_vface[d][b][sl], s.vface[d][sl], f"block {b} face velocity x{d + 1}")
        else:
            same_bits(mb.dust_flux[d][b][sl], s.scaled_flux(d)[sl], f"block {b} dust flux x{d + 1}")


# ---- the one-thread-per-zone kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
@pytest.mark.parametrize("nx,ng,recon", [((5, 3, 2), 2, "plm"), ((24, 12, 10), 2, "plm"), ((20, 8, 6), 4, "ppm")])
def test_per_task_kernel(hiplib, nx, ng, recon, riem):
    (o,), mb = make_pair(nx, ng=ng, recon=recon, riem=riem, seed=41)
    mb.CalculateFluxes(GAS, False)
    check(mb, 0, o)


# ---- the LDS-staged tile march (one gas species, PCM / PLM, blocks at least a 32 x 8 tile wide) ---------------------
@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
@pytest.mark.parametrize("nx", [(40, 17, 21), (67, 9, 5), (64, 16, 1)])
def test_tile_march(hiplib, nx, riem):
    (o,), mb = make_pair(nx, recon="plm", riem=riem, seed=42)
    mb.CalculateFluxes(GAS, False)
    check(mb, 0, o)


@pytest.mark.parametrize("nx,ng,riem", [((67, 9, 5), 2, "hllc"), ((33, 8, 1), 4, "llf")])
def test_tile_march_pcm(hiplib, nx, ng, riem):
    (o,), mb = make_pair(nx, ng=ng, recon="pcm", riem=riem, seed=43)
    mb.CalculateFluxes(GAS, False)
    check(mb, 0, o)


@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
def test_tile_march_three_blocks(hiplib, riem):
    oracles, mb = make_pair((48, 20, 19), recon="plm", riem=riem, seed=44, nb=3)
    mb.CalculateFluxes(GAS, False)
    for b, o in enumerate(oracles):
        check(mb, b, o)


@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
def test_tile_march_vanishing_velocities(hiplib, riem):
    """The upwind (lower x1) half of the block moves at 1e-250: the march's shared reciprocals would lose such
    quotients, so it redoes those planes and columns with IEEE divisions; the result must still be the reference's."""
    (o,), mb = make_pair((48, 20, 19), recon="plm", riem=riem, seed=45)
    w = o.gprim
    w[1:4, :, :, : o.ni // 2] = np.abs(w[1:4, :, :, : o.ni // 2]) * 1.0e-250 + 1.0e-250
    w[1:4, :, :, o.ni // 2:] = np.abs(w[1:4, :, :, o.ni // 2:])  # (the flow leaves the slow half: it is upwind)
    o.PrimToCons()
    push([o], mb)
    mb.CalculateFluxes(GAS, False)
    check(mb, 0, o)


@pytest.mark.parametrize("nx", [(24, 12, 10), (40, 18, 20)])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_mirror_plane(hiplib, nx, d):
    """HLLC's contact speed is exactly 0 on the central faces of a block that is its own mirror image (am >= 0 falls
    on the equality, hllc.hpp:157), with random velocities on both sides; per-task kernel and tile march."""
    (o,), mb = make_pair(nx, recon="plm", riem="hllc", seed=48)
    mirror_state(o, d)
    push([o], mb)
    mb.CalculateFluxes(GAS, False)
    check(mb, 0, o)


# ---- dust ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driem", ["hlle", "llf"])
@pytest.mark.parametrize("drecon,ng", [("plm", 2), ("ppm", 4)])
def test_dust_two_species(hiplib, drecon, ng, driem):
    (o,), mb = make_pair((24, 12, 10), ng=ng, ns_gas=1, ns_dust=2, recon="plm", riem="hlle", drecon=drecon,
                         driem=driem, seed=46)
    mb.CalculateFluxes(DUST, False)
    check(mb, 0, o, DUST)


# ---- curvilinear: the first block of each system in test_parity_geometry.GEOMS -----------------------------------------
def first_blocks():
    seen, out = set(), []
    for name, nx, lo, hi in GEOMS:
        system = ref.coord_select(name, sum(n > 1 for n in nx))
        if system not in seen:
            seen.add(system)
            out.append(pytest.param(name, nx, lo, hi, id=f"{name}-{'x'.join(map(str, nx))}"))
    return out


@pytest.mark.parametrize("recon,riem", [("plm", "hlle"), ("ppm", "llf")])
@pytest.mark.parametrize("coordinates,nx,lo,hi", first_blocks())
def test_curvilinear(hiplib, coordinates, nx, lo, hi, recon, riem):
    """PLM_G with the metric tables of artemis_hip_metric_fill against PLM_G fed by the reference's Coords, and the
    scaled momentum fluxes against the reference's face-centre scale factors; gas and one dust species."""
    o, mb = make_curvilinear_pair(coordinates, nx, lo, hi, ng=3 if recon == "ppm" else 2, ns_gas=1, ns_dust=1,
                                  recon=recon, riem=riem, seed=47)
    for fluid in (GAS, DUST):
        mb.CalculateFluxes(fluid, False)
        check(mb, 0, o, fluid)
