#!/usr/bin/env python3
"""A/B of the Cartesian dust / shearing-box tile march (kernels_curv.hip) against the kernels the same packs ran
before it (NO_CART_DUST_MARCH: the cell-centred stage, one launch per fluid + drag finish + timestep launches), in ONE
process, the two paths alternating, HIP events around every artemis_hip_stage_general call of the host driver
(Simulation.set_kernel_timing / kernel_ms):

  * advection: inputs/advection/advection.in at 256 x 128 x 128 in one block (gas + two dust species);
  * strat3d:   inputs/ssheet/ssheet.in in 3-D at 256 x 256 x 64 with one dust species and simple_dust drag.

    python scripts/cart_dust_ab.py [--decks advection,strat3d,disk_cart] [--cycles 50] [--warmup 5] [--reps 3]
                                   [--lib other/libartemis_hip.so] [--out profiles/cart_dust_march_ab.txt]

Prints, per deck and path, the stage time per cycle of every repetition, their mean and spread (max - min), and the
ratio of the means; a path counts as faster only when the means differ by more than both spreads.  --lib runs the
same measurement through another build of the library (e.g. the parent commit's, where the switch does not exist and
both legs take that build's only path): what NO_CART_DUST_MARCH stands for can be confirmed against it.  disk_cart
(inputs/disk/disk_cart.in as shipped: Cartesian gas on the march before and after) takes the same two legs; the switch
does not touch it, so its two columns measure the spread alone; the driver places no events around the stages of a refined
mesh, so that deck reports the wall time of a whole cycle instead."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_block(nx):
    ov = []
    for d, n in enumerate(nx, 1):
        ov += ["parthenon/mesh/nx%d=%d" % (d, n), "parthenon/meshblock/nx%d=%d" % (d, n)]
    return ov


DECKS = {
    "advection": (("advection", "advection.in"), one_block((256, 128, 128))),
    "strat3d": (("ssheet", "ssheet.in"),
                one_block((256, 256, 64)) + ["parthenon/mesh/x3min=-0.2", "parthenon/mesh/x3max=0.2", "parthenon/mesh/ix3_bc=extrap",
                                             "parthenon/mesh/ox3_bc=extrap", "physics/dust=true", "physics/drag=true",
                                             "dust/nspecies=1", "dust/cfl=0.3", "dust/reconstruct=plm", "dust/riemann=hlle",
                                             "dust/dfloor=1.0e-10", "dust/stopping_time/type=constant",
                                             "dust/stopping_time/tau=0.01", "drag/type=simple_dust", "gravity/point/mass=1.0e-3"]),
    "disk_cart": (("disk", "disk_cart.in"), []),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decks", default="advection,strat3d")
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    if args.lib:  # another build of the same C ABI, loaded in place of the tree's
        L = C.CDLL(os.path.abspath(args.lib), mode=C.RTLD_GLOBAL)
        L.artemis_hip_source_sha.restype = C.c_char_p
        L.artemis_hip_get_option.argtypes = [C.c_char_p]
        L.artemis_hip_set_option.argtypes = [C.c_char_p, C.c_int]
    else:
        L = capi.load()
    has_switch = L.artemis_hip_get_option(b"NO_CART_DUST_MARCH") >= 0
    lines = ["# scripts/cart_dust_ab.py --cycles %d --warmup %d --reps %d%s" % (args.cycles, args.warmup, args.reps,
                                                                              " --lib (another build)" if args.lib else ""),
             "# library source sha %s%s" % (L.artemis_hip_source_sha().decode(),
                                            "" if has_switch else "  (no NO_CART_DUST_MARCH in this build: both legs run its only path)"),
             "# stage time = HIP events around every artemis_hip_stage_general call, summed over a cycle's stages, ms"]
    for name in args.decks.split(","):
        deck, ov = DECKS[name]
        ms = {0: [], 1: []}
        kern = {}
        for rep in range(args.reps):
            for off in (0, 1):  # alternating: march, previous kernels, march, ...
                if has_switch:
                    L.artemis_hip_set_option(b"NO_CART_DUST_MARCH", off)
                s = Simulation(os.path.join(ROOT, "inputs", *deck), ov + ["parthenon/time/nlim=%d" % (args.warmup + args.cycles)],
                               lib=L if args.lib else None)
                s.evolve(args.warmup)
                s.set_kernel_timing(True)
                n = s.evolve(args.cycles)
                per_launch, launches = s.kernel_ms()
                if launches:
                    ms[off].append(per_launch * launches / max(n, 1))
                    kern[off] = "%s, %d blocks, %d timed calls in %d cycles" % (s.stage_kernel, s.nblocks, launches, n)
                else:  # (refined meshes: the driver places no events around their stages -- the whole cycle's wall time)
                    ms[off].append(1.0e3 * s.last_wall_seconds / max(n, 1))
                    kern[off] = "%s, %d blocks, WALL time of %d cycles (no stage events on a refined mesh)" % (s.stage_kernel, s.nblocks, n)
                s.close()
        if has_switch:
            L.artemis_hip_set_option(b"NO_CART_DUST_MARCH", 0)
        lines.append("%s" % name)
        mean, spread = {}, {}
        for off in (0, 1):
            mean[off], spread[off] = sum(ms[off]) / len(ms[off]), max(ms[off]) - min(ms[off])
            lines.append("  %-22s %s" % ("NO_CART_DUST_MARCH=%d" % off if has_switch else "leg %d" % off, kern[off]))
            lines.append("    ms per cycle: %s   mean %.4f   spread %.4f" % (" ".join("%.4f" % v for v in ms[off]), mean[off], spread[off]))
        gap = mean[1] - mean[0]
        verdict = "faster" if gap > max(spread.values()) else ("slower" if -gap > max(spread.values()) else "equal within the spread")
        lines.append("    leg 0 / leg 1 = %.3f  (leg 0 is %s)" % (mean[0] / mean[1], verdict))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
