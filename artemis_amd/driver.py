"""Simulation: Python handle on the C++ host driver (include/artemis_driver.h).

Usage mirrors `artemis -i <deck> block/key=value ...` (tst/scripts/utils/artemis.py:122-156):

    sim = Simulation("inputs/blast/blast.in", ["parthenon/mesh/nx3=256", ...])
    sim.evolve()

One process per GPU: the mesh-block grid is split over the ranks and ghost slabs travel through an
artemis_comm_t -- RcclComm = the native C++ RCCL transport (GPU runs), TorchComm = callbacks into
torch.distributed ("gloo" in the CPU tests of the host logic).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import capi


class Msg(C.Structure):
    _fields_ = [("peer", C.c_int), ("tag", C.c_int), ("send", C.c_void_p), ("recv", C.c_void_p),
                ("count", C.c_long)]


EXCH_START = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(Msg), C.c_void_p)
EXCH_FINISH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
ALLRED_MIN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))
ALLRED_SUM = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
ALLRED_MIN_DEV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)


class Comm(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int), ("nranks", C.c_int),
                ("exchange_start", EXCH_START), ("exchange_finish", EXCH_FINISH),
                ("allreduce_min", ALLRED_MIN), ("allreduce_min_dev", ALLRED_MIN_DEV),
                ("allreduce_sum", ALLRED_SUM)]


class _DevView:
    """Zero-copy torch view of a raw device (or host) buffer of doubles."""

    def __init__(self, ptr, count, cuda):
        self.ptr, self.count, self.cuda = ptr, count, cuda
        if cuda:
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8",
                                             "data": (ptr, False), "version": 2}


def _tensor_of(ptr, count, device, cache):
    key = (ptr, count)
    t = cache.get(key)
    if t is None:
        if device.type == "cuda":
            t = torch.as_tensor(_DevView(ptr, count, True), device=device)
        else:
            buf = (C.c_double * count).from_address(ptr)
            t = torch.frombuffer(buf, dtype=torch.float64)
        cache[key] = t
    return t


class TorchComm:
    """artemis_comm_t bound to torch.distributed (nccl/RCCL on GPUs, gloo on CPUs)."""

    def __init__(self, device, group=None):
        import torch.distributed as dist
        self.dist, self.group, self.device = dist, group, torch.device(device)
        self.rank, self.nranks = dist.get_rank(group), dist.get_world_size(group)
        self._cache, self._works, self._opcache = {}, [], {}
        self._cbs = (EXCH_START(self._start), EXCH_FINISH(self._finish),
                     ALLRED_MIN(self._min), ALLRED_MIN_DEV(self._min_dev), ALLRED_SUM(self._sum))
        self.struct = Comm(None, self.rank, self.nranks, *self._cbs)

    def _stream_ctx(self, stream_ptr):
        if self.device.type != "cuda":
            import contextlib
            return contextlib.nullcontext()
        return torch.cuda.stream(torch.cuda.ExternalStream(stream_ptr, device=self.device))

    def _start(self, ctx, nmsg, msgs, stream):
        try:
            dist = self.dist
            # the same message set comes back every stage: build the P2POp list once
            key = tuple((m.peer, m.tag, m.send, m.recv, m.count) for m in (msgs[i] for i in range(nmsg)))
            ops = self._opcache.get(key)
            if ops is None:
                ops = []
                # deterministic global order (RCCL matches sends and receives by posting order,
                # not by tag): sort by tag, receives and sends alike
                items = sorted((msgs[i] for i in range(nmsg)), key=lambda m: (m.tag, m.send is None))
                for m in items:
                    if m.send:
                        ops.append(dist.P2POp(dist.isend, _tensor_of(m.send, m.count, self.device, self._cache),
                                              m.peer, group=self.group, tag=m.tag))
                    if m.recv:
                        ops.append(dist.P2POp(dist.irecv, _tensor_of(m.recv, m.count, self.device, self._cache),
                                              m.peer, group=self.group, tag=m.tag))
                self._opcache[key] = ops
            with self._stream_ctx(stream):
                self._works = dist.batch_isend_irecv(ops) if ops else []
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            print("TorchComm.exchange_start failed:", repr(e), flush=True)
            return 1

    def _finish(self, ctx, stream):
        try:
            with self._stream_ctx(stream):
                for w in self._works:
                    w.wait()
            self._works = []
            return 0
        except Exception as e:
            print("TorchComm.exchange_finish failed:", repr(e), flush=True)
            return 1

    def _min(self, ctx, value):
        try:
            t = torch.tensor([value[0]], dtype=torch.float64, device=self.device)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN, group=self.group)
            value[0] = float(t.item())
            return 0
        except Exception as e:
            print("TorchComm.allreduce_min failed:", repr(e), flush=True)
            return 1

    def _min_dev(self, ctx, dev_value, stream):
        try:
            t = _tensor_of(dev_value, 1, self.device, self._cache)
            with self._stream_ctx(stream):
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN, group=self.group)
            return 0
        except Exception as e:
            print("TorchComm.allreduce_min_dev failed:", repr(e), flush=True)
            return 1

    def _sum(self, ctx, values, n):
        try:
            t = torch.tensor([values[i] for i in range(n)], dtype=torch.float64, device=self.device)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
            for i, v in enumerate(t.tolist()):
                values[i] = v
            return 0
        except Exception as e:
            print("TorchComm.allreduce_sum failed:", repr(e), flush=True)
            return 1


class RcclComm:
    """The native C++ transport (artemis_comm_rccl_*, csrc/driver/comm_rccl.cpp): RCCL called directly from
    the driver's streams, no Python in the loop.  `share(obj) -> obj` broadcasts rank 0's unique id to every
    rank over any out-of-band channel (bench.py: a gloo broadcast); a single rank needs none."""

    def __init__(self, rank=0, nranks=1, share=None, lib=None):
        self.L = lib if lib is not None else capi.load()
        L = self.L
        L.artemis_comm_rccl_unique_id.argtypes = [C.c_char_p, C.c_int]
        L.artemis_comm_rccl_create.restype = C.c_void_p
        L.artemis_comm_rccl_create.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.artemis_comm_rccl_destroy.argtypes = [C.c_void_p]
        L.artemis_comm_rccl_count.argtypes = [C.c_void_p]
        L.artemis_comm_rccl_barrier.argtypes = [C.c_void_p]
        L.artemis_comm_rccl_last_error.restype = C.c_char_p
        nbytes = L.artemis_comm_rccl_unique_id_bytes()
        uid = None
        if rank == 0:
            buf = C.create_string_buffer(nbytes)
            if L.artemis_comm_rccl_unique_id(buf, nbytes):
                raise RuntimeError("ncclGetUniqueId: " + L.artemis_comm_rccl_last_error().decode())
            uid = buf.raw
        if nranks > 1:
            if share is None:
                raise ValueError("RcclComm with nranks > 1 needs a `share` callable to distribute the unique id")
            uid = share(uid)
        self.h = L.artemis_comm_rccl_create(uid, rank, nranks)
        if not self.h:
            raise RuntimeError("artemis_comm_rccl_create: " + L.artemis_comm_rccl_last_error().decode())
        self.struct = Comm.from_address(self.h)
        self.rank, self.nranks = rank, nranks

    @property
    def count(self):
        return self.L.artemis_comm_rccl_count(self.h)

    def barrier(self):
        if self.L.artemis_comm_rccl_barrier(self.h):
            raise RuntimeError("RCCL barrier: " + self.L.artemis_comm_rccl_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.artemis_comm_rccl_destroy(self.h)
            self.h = None


def _declare(L):
    if getattr(L, "_sim_declared", False):
        return
    vp, d, i, l = C.c_void_p, C.c_double, C.c_int, C.c_long
    L.artemis_sim_create.restype = vp
    L.artemis_sim_create.argtypes = [C.c_char_p, i, C.POINTER(C.c_char_p), C.POINTER(Comm)]
    L.artemis_sim_destroy.argtypes = [vp]
    L.artemis_sim_last_error.restype = C.c_char_p
    L.artemis_sim_evolve.restype = l
    L.artemis_sim_evolve.argtypes = [vp, l]
    for n in ("time", "dt", "tlim", "last_wall_seconds"):
        f = getattr(L, "artemis_sim_" + n)
        f.restype, f.argtypes = d, [vp]
    for n in ("ncycle", "local_zones", "total_zones"):
        f = getattr(L, "artemis_sim_" + n)
        f.restype, f.argtypes = l, [vp]
    L.artemis_sim_uses_fused_path.argtypes = [vp]
    L.artemis_sim_uses_tuned_kernel.argtypes = [vp]
    L.artemis_sim_remeshes.argtypes = [vp]
    L.artemis_sim_remeshes.restype = C.c_long
    L.artemis_sim_force_refine.argtypes = [vp, C.c_long]
    L.artemis_sim_force_refine.restype = C.c_int
    L.artemis_sim_inject_refine_tags.argtypes = [vp, C.POINTER(C.c_long), C.c_int]
    L.artemis_sim_inject_refine_tags.restype = C.c_int
    L.artemis_sim_load_balance.argtypes = [vp]
    L.artemis_sim_load_balance.restype = C.c_double
    L.artemis_sim_remesh_seconds.argtypes = [vp, C.POINTER(C.c_double)]
    L.artemis_sim_remesh_seconds.restype = C.c_long
    L.artemis_sim_last_remesh.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_double)]
    L.artemis_sim_last_remesh.restype = None
    L.artemis_rt_device_bytes.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int]
    L.artemis_rt_device_bytes.restype = None
    L.artemis_rt_pool_bytes.restype = C.c_size_t
    L.artemis_rt_pool_bytes.argtypes = []
    L.artemis_sim_stage_kernel.argtypes = [vp]
    L.artemis_sim_stage_kernel.restype = C.c_char_p
    L.artemis_sim_set_path.argtypes = [vp, C.c_char_p]
    L.artemis_sim_set_overlap.argtypes = [vp, i]
    L.artemis_sim_overlap.argtypes = [vp]
    L.artemis_sim_set_dropin.argtypes = [vp, i]
    L.artemis_sim_species.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.artemis_sim_set_kernel_timing.argtypes = [vp, i]
    L.artemis_sim_nbody_force.argtypes = [vp, C.POINTER(d), i]
    L.artemis_sim_block_level.argtypes = [vp, i]
    L.artemis_sim_nblocks_global.restype = l
    L.artemis_sim_nblocks_global.argtypes = [vp]
    L.artemis_sim_dims.argtypes = [vp, C.POINTER(i)]
    L.artemis_sim_get_field.argtypes = [vp, C.c_char_p, i, vp]
    L.artemis_sim_block_bounds.argtypes = [vp, i, C.POINTER(d)]
    L.artemis_sim_history.argtypes = [vp, C.POINTER(d)]
    L.artemis_sim_errors.argtypes = [vp, C.POINTER(d)]
    L.artemis_sim_kernel_ms.restype = d
    L.artemis_sim_kernel_ms.argtypes = [vp, C.POINTER(l)]
    L.artemis_sim_save.argtypes = [vp, C.c_char_p]
    L.artemis_sim_restore.restype = vp
    L.artemis_sim_restore.argtypes = [C.c_char_p, i, C.POINTER(C.c_char_p), C.POINTER(Comm)]
    L.artemis_sim_checkpoint_describe.argtypes = [C.c_char_p, C.c_char_p, l]
    L.artemis_sim_checkpoint_seconds.argtypes = [C.POINTER(d)]
    L.artemis_sim_checkpoint_seconds.restype = None
    L.artemis_sim_enable_outputs.argtypes = [vp, C.c_char_p]
    L.artemis_sim_history_device.argtypes = [vp, C.POINTER(d)]
    L.artemis_sim_outputs_describe.argtypes = [vp, C.c_char_p, l]
    L.artemis_sim_gather_fields.restype = l
    L.artemis_sim_gather_fields.argtypes = [vp, i, C.POINTER(C.c_char_p), i, vp]
    L.artemis_sim_write_fields.argtypes = [vp, C.c_char_p, i, C.POINTER(C.c_char_p), i]
    L.artemis_sim_gather_fields_level.restype = l
    L.artemis_sim_gather_fields_level.argtypes = [vp, i, C.POINTER(C.c_char_p), i, i, vp, C.POINTER(l)]
    L.artemis_sim_write_fields_level.argtypes = [vp, C.c_char_p, i, C.POINTER(C.c_char_p), i, i]
    L.artemis_sim_gather_fields_reduced.restype = l
    L.artemis_sim_gather_fields_reduced.argtypes = [vp, i, C.POINTER(C.c_char_p), i, i, vp]
    L.artemis_sim_write_fields_reduced.argtypes = [vp, C.c_char_p, i, C.POINTER(C.c_char_p), i, i]
    L.artemis_sim_gather_fields_reduced_level.restype = l
    L.artemis_sim_gather_fields_reduced_level.argtypes = [vp, i, C.POINTER(C.c_char_p), i, i, i, vp, C.POINTER(l)]
    L.artemis_sim_write_fields_reduced_level.argtypes = [vp, C.c_char_p, i, C.POINTER(C.c_char_p), i, i, i]
    L.artemis_sim_scatter_fields.restype = l
    L.artemis_sim_scatter_fields.argtypes = [vp, i, C.POINTER(C.c_char_p), i, vp, d]
    L.artemis_sim_sample_plan_create.restype = l
    L.artemis_sim_sample_plan_create.argtypes = [vp, l, vp]
    L.artemis_sim_sample_plan_locations.argtypes = [vp, l, vp]
    L.artemis_sim_sample_plan_values.restype = l
    L.artemis_sim_sample_plan_values.argtypes = [vp, l, i, C.POINTER(C.c_char_p), i, vp]
    L.artemis_sim_sample_plan_destroy.argtypes = [vp, l]
    L.artemis_sim_record_create.restype = l
    L.artemis_sim_record_create.argtypes = [vp, l, i, C.POINTER(C.c_char_p), l, l, i]
    L.artemis_sim_record_rows.restype = l
    L.artemis_sim_record_rows.argtypes = [vp, l]
    L.artemis_sim_record_read.restype = l
    L.artemis_sim_record_read.argtypes = [vp, l, vp, vp, vp, vp, i]
    L.artemis_sim_record_destroy.argtypes = [vp, l]
    L.artemis_sim_record_integrals_create.restype = l
    L.artemis_sim_record_integrals_create.argtypes = [vp, l, l, i, vp, i]
    L.artemis_sim_record_integrals_read.restype = l
    L.artemis_sim_record_integrals_read.argtypes = [vp, l, vp, vp, vp, vp, vp, i]
    L.artemis_sim_record_integrals_window_zones.restype = l
    L.artemis_sim_record_integrals_window_zones.argtypes = [vp, l, vp]
    L._sim_declared = True


class SamplePlan:
    """A list of points of a Simulation, located in this rank's blocks on the device (Simulation.sample_plan makes one; it
    belongs to the simulation and is freed with it, or by close()).  After a remesh -- evolve() on an adaptive mesh,
    force_refine() -- the next use locates the points again by itself."""

    def __init__(self, sim, points):
        if not isinstance(points, np.ndarray) or points.dtype != np.dtype(np.float64):
            raise ValueError("sample points are a numpy array of float64, not %s"
                             % (points.dtype if isinstance(points, np.ndarray) else type(points).__name__))
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("sample points are [npoints, 3] (x1, x2, x3), not %s" % (tuple(points.shape),))
        if not points.flags["C_CONTIGUOUS"]:
            raise ValueError("sample points are a C-contiguous array")
        self.sim, self.npoints = sim, int(points.shape[0])
        self.id = sim.L.artemis_sim_sample_plan_create(sim.h, self.npoints, points.ctypes.data)
        if self.id < 0:
            self.id = None
            raise RuntimeError(sim.L.artemis_sim_last_error().decode())

    def _live(self):
        if self.id is None or not getattr(self.sim, "h", None):
            raise RuntimeError("the sample plan is closed")

    def _locations(self):
        self._live()
        loc = np.empty((self.npoints, 4), dtype=np.int32)
        if self.sim.L.artemis_sim_sample_plan_locations(self.sim.h, self.id, loc.ctypes.data):
            raise RuntimeError(self.sim.L.artemis_sim_last_error().decode())
        return loc

    @property
    def block(self):
        """[npoints] int32: the local block that holds each point, -1 for a point that is not found (outside the mesh, not
        finite, or in a block of another rank)"""
        return np.ascontiguousarray(self._locations()[:, 0])

    @property
    def zone(self):
        """[npoints, 3] int32: the zone of that block as k, j, i, interior-relative (gather's array indices); -1 where not found"""
        return np.ascontiguousarray(self._locations()[:, 1:4])

    def values(self, variables, single=False):
        """The named variables (as gather names and orders them, the derived ones included) at the points: [ncomp, npoints]
        float64 (float32 with single=True) in the order of the points, each value the one gather returns for the zone that
        holds the point, bit for bit -- nothing is interpolated -- and NaN where the point is not found.  Formed from the
        primitives on the device; the run is not disturbed.  RuntimeError for what the driver refuses (an unknown variable,
        one of a fluid the run lacks, a closed plan)."""
        self._live()
        names, n = Simulation._names(variables)
        L, h = self.sim.L, self.sim.h
        nbytes = L.artemis_sim_sample_plan_values(h, self.id, n, names, int(single), None)
        if nbytes < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        count = nbytes // (4 if single else 8)
        out = np.empty(max(count, 1), dtype=np.float32 if single else np.float64)  # (never empty: NULL asks for the size)
        ncomp = L.artemis_sim_sample_plan_values(h, self.id, n, names, int(single), out.ctypes.data)
        if ncomp < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        return out[:count].reshape(ncomp, self.npoints)

    def close(self):
        """Free the plan (its device arrays); every later use raises RuntimeError."""
        if self.id is not None and getattr(self.sim, "h", None):
            self.sim.L.artemis_sim_sample_plan_destroy(self.sim.h, self.id)
        self.id = None


class TimeSeries:
    """What Recorder.read returns: cycle [n] int64, time [n], dt [n] float64, values [n, ncomp, npoints]"""

    def __init__(self, cycle, time, dt, values):
        self.cycle, self.time, self.dt, self.values = cycle, time, dt, values


# Rows a recorder's device buffers hold when the caller names no capacity: at most 4096 rows and at most 64 MiB.  A design
# constant, not a measurement: large enough that a run drains rarely, small enough not to compete with the state for memory.
RECORD_DEFAULT_ROWS, RECORD_DEFAULT_BYTES = 4096, 64 << 20


class Recorder:
    """A time series of a SamplePlan's values, recorded on the device inside evolve() (Simulation.record makes one; it
    belongs to the simulation and is freed with it, or by close()).  After every `every`-th cycle completed since it was
    made one row is appended: the cycle number, the time the values hold at, the next step's dt, and what
    plan.values(variables, single) would return at that moment, bit for bit.  Rank-local like a plan, not part of a
    checkpoint, nothing interpolated in space or time."""

    def __init__(self, sim, plan, variables, every, capacity, single, owns_plan):
        self.sim, self.plan, self.single, self._owns_plan, self.id = sim, plan, bool(single), owns_plan, None
        self.variables = [variables] if isinstance(variables, str) else list(variables)
        names, n = Simulation._names(self.variables)
        L, h = sim.L, sim.h
        if capacity is None:
            row = L.artemis_sim_sample_plan_values(h, plan.id, n, names, int(self.single), None)  # bytes of [ncomp][npoints]
            if row < 0:
                raise RuntimeError(L.artemis_sim_last_error().decode())
            capacity = max(1, min(RECORD_DEFAULT_ROWS, RECORD_DEFAULT_BYTES // max(row, 1)))
        self.every, self.capacity = int(every), int(capacity)
        rid = L.artemis_sim_record_create(h, plan.id, n, names, self.every, self.capacity, int(self.single))
        if rid < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        self.id = rid
        self.ncomp = L.artemis_sim_record_read(h, rid, None, None, None, None, 0)  # (no buffer: the size query)

    def _live(self):
        if self.id is None or not getattr(self.sim, "h", None):
            raise RuntimeError("the recorder is closed")

    @property
    def rows(self):
        """rows recorded so far and not cleared by read(clear=True); waits for the device and empties its buffers first"""
        self._live()
        n = self.sim.L.artemis_sim_record_rows(self.sim.h, self.id)
        if n < 0:
            raise RuntimeError(self.sim.L.artemis_sim_last_error().decode())
        return n

    def read(self, clear=False):
        """A TimeSeries of the rows so far, oldest first; clear=True forgets them afterwards (the counters go on)."""
        n = self.rows
        L, h, ncomp = self.sim.L, self.sim.h, self.ncomp
        cycle, time, dt = np.empty(n, dtype=np.int64), np.empty(n), np.empty(n)
        count = n * ncomp * self.plan.npoints
        values = np.empty(max(count, 1), dtype=np.float32 if self.single else np.float64)  # (never empty: NULL is "no buffer")
        if L.artemis_sim_record_read(h, self.id, cycle.ctypes.data if n else None, time.ctypes.data if n else None,
                                     dt.ctypes.data if n else None, values.ctypes.data, int(bool(clear))) < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        return TimeSeries(cycle, time, dt, values[:count].reshape(n, ncomp, self.plan.npoints))

    def close(self):
        """Free the recorder (and the plan it made for itself); every later use raises RuntimeError."""
        if self.id is not None and getattr(self.sim, "h", None):
            self.sim.L.artemis_sim_record_destroy(self.sim.h, self.id)
            if self._owns_plan:
                self.plan.close()
        self.id = None


class IntegralSeries:
    """What IntegralRecorder.read returns: cycle [n] int64, time [n], dt [n], integrals [n, 1 + nwin, nq] float64 and nbody
    [n, npart, 7] (None for a recorder without n-body rows)"""

    def __init__(self, cycle, time, dt, integrals, nbody):
        self.cycle, self.time, self.dt, self.integrals, self.nbody = cycle, time, dt, integrals, nbody


_HST_GAS = ("gas_mass", "gas_momentum_x1", "gas_momentum_x2", "gas_momentum_x3", "gas_energy", "gas_internal_energy")
_HST_DUST = ("dust_mass", "dust_momentum_x1", "dust_momentum_x2", "dust_momentum_x3")


class IntegralRecorder:
    """A time series of the history integrals -- of this rank's mesh (set 0) and of up to seven windows (set 1 + w) -- and,
    with nbody=True, of the n-body force sums, recorded on the device inside evolve() (Simulation.record_integrals makes
    one).  Set 0 of a row is, on one rank, what history_device() would return had evolve returned after that cycle, bit for
    bit; the n-body rows what nbody_force() would return if called for the first time there.  Rank-local, not part of a
    checkpoint; recording flushes nothing and does not disturb the run.  labels[i] names entry i of a set as an hst file
    names that column; the order is the history_device layout (species outermost), not the file's column order."""

    def __init__(self, sim, every, capacity, windows, nbody):
        self.sim, self.id, self.nbody = sim, None, bool(nbody)
        self.windows = np.ascontiguousarray(np.zeros((0, 3, 2)) if windows is None else windows, dtype=np.float64)
        if self.windows.ndim != 3 or self.windows.shape[1:] != (3, 2):
            raise ValueError("windows: an [nwin, 3, 2] array of [lo, hi) per direction, not %r" % (self.windows.shape,))
        self.nwin = len(self.windows)
        if self.nwin > 7:
            raise ValueError("%d windows: at most 7" % self.nwin)
        L, h = sim.L, sim.h
        self.nq = 6 * sim.ns_gas + 4 * sim.ns_dust
        self.npart = L.artemis_sim_nbody_force(h, None, 0) if self.nbody else 0
        if capacity is None:
            row = 8 * ((1 + self.nwin) * self.nq + 7 * self.npart)
            capacity = max(1, min(RECORD_DEFAULT_ROWS, RECORD_DEFAULT_BYTES // max(row, 1)))
        self.every, self.capacity = int(every), int(capacity)
        rid = L.artemis_sim_record_integrals_create(h, self.every, self.capacity, self.nwin, self.windows.ctypes.data if self.nwin else None,
                                                    int(self.nbody))
        if rid < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        self.id = rid
        if L.artemis_sim_record_integrals_read(h, rid, None, None, None, None, None, 0) != self.nq:  # (no buffer: the size query)
            self.close()
            raise RuntimeError("the driver's integrals per set are not 6 ns_gas + 4 ns_dust")
        # labels[i]: the hst column label of entry i (the strings artemis_amd.history.read_history yields), in the order of the
        # history_device layout -- species outermost -- not in the file's column order, which is quantity outermost
        self.labels = ["%s_%d" % (name, n) for n in range(sim.ns_gas) for name in _HST_GAS] + \
                      ["%s_%d" % (name, n) for n in range(sim.ns_dust) for name in _HST_DUST]

    def _live(self):
        if self.id is None or not getattr(self.sim, "h", None):
            raise RuntimeError("the recorder is closed")

    @property
    def rows(self):
        """rows recorded so far and not cleared by read(clear=True); waits for the device and empties its buffers first"""
        self._live()
        n = self.sim.L.artemis_sim_record_rows(self.sim.h, self.id)
        if n < 0:
            raise RuntimeError(self.sim.L.artemis_sim_last_error().decode())
        return n

    def read(self, clear=False):
        """An IntegralSeries of the rows so far, oldest first; clear=True forgets them afterwards (the counters go on)."""
        n = self.rows
        L, h = self.sim.L, self.sim.h
        cycle, time, dt = np.empty(n, dtype=np.int64), np.empty(n), np.empty(n)
        ni, nb = n * (1 + self.nwin) * self.nq, n * self.npart * 7
        integrals, nbody = np.empty(max(ni, 1)), np.empty(max(nb, 1))  # (never empty: NULL is "no buffer")
        if L.artemis_sim_record_integrals_read(h, self.id, cycle.ctypes.data if n else None, time.ctypes.data if n else None,
                                               dt.ctypes.data if n else None, integrals.ctypes.data, nbody.ctypes.data, int(bool(clear))) < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        return IntegralSeries(cycle, time, dt, integrals[:ni].reshape(n, 1 + self.nwin, self.nq),
                              nbody[:nb].reshape(n, self.npart, 7) if self.nbody else None)

    def window_zones(self):
        """[nblocks, nwin, 6] int32: the zones {i0, i1, j0, j1, k0, k1} of every window on every local block of the current
        mesh, half-open and relative to the block's first interior zone; an empty range has i0 == i1"""
        self._live()
        L, h = self.sim.L, self.sim.h
        nb = L.artemis_sim_record_integrals_window_zones(h, self.id, None)
        if nb < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        out = np.zeros((nb, self.nwin, 6), dtype=np.int32)
        if out.size and L.artemis_sim_record_integrals_window_zones(h, self.id, out.ctypes.data) != nb:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        return out

    def close(self):
        """Free the recorder; every later use raises RuntimeError."""
        if self.id is not None and getattr(self.sim, "h", None):
            self.sim.L.artemis_sim_record_destroy(self.sim.h, self.id)
        self.id = None


class Simulation:
    def __init__(self, deck, overrides=(), comm=None, lib=None):
        """deck: path to an input deck or its text; overrides: 'block/key=value' strings;
        comm: a TorchComm (or any object with a .struct artemis_comm_t) for multi-rank runs;
        lib: an alternative shared library exporting the same C ABI (tests only)."""
        self.L = lib if lib is not None else capi.load()
        _declare(self.L)
        text = open(deck).read() if os.path.exists(deck) else deck
        ov = (C.c_char_p * max(len(overrides), 1))(*[o.encode() for o in overrides])
        self.comm = comm
        cptr = C.byref(comm.struct) if comm is not None else None
        self.h = self.L.artemis_sim_create(text.encode(), len(overrides), ov, cptr)
        if not self.h:
            raise RuntimeError("artemis_sim_create: " + self.L.artemis_sim_last_error().decode())
        self._attach()

    def _attach(self):
        self._refresh_dims()
        ng_, nd_ = C.c_int(0), C.c_int(0)
        self.L.artemis_sim_species(self.h, C.byref(ng_), C.byref(nd_))
        self.ns_gas, self.ns_dust = ng_.value, nd_.value

    def save(self, path):
        """Write a checkpoint directory at `path` (collective over the ranks of the run; replaces an existing one).
        Call it between evolve() calls."""
        if self.L.artemis_sim_save(self.h, os.fspath(path).encode()):
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    @classmethod
    def restore(cls, path, overrides=(), comm=None, lib=None):
        """The run a checkpoint holds, on this process' ranks (any count): continues bit for bit like the saved one.
        overrides are applied after the stored ones ('parthenon/time/nlim=10'); runtime settings (set_path,
        set_overlap, set_dropin) are not part of a checkpoint."""
        self = cls.__new__(cls)
        self.L = lib if lib is not None else capi.load()
        _declare(self.L)
        ov = (C.c_char_p * max(len(overrides), 1))(*[o.encode() for o in overrides])
        self.comm = comm
        cptr = C.byref(comm.struct) if comm is not None else None
        self.h = self.L.artemis_sim_restore(os.fspath(path).encode(), len(overrides), ov, cptr)
        if not self.h:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        self._attach()
        return self

    def checkpoint_seconds(self):
        """The last save() or restore() of this thread: (total, device copies, checksums, file writes or reads) in seconds"""
        out = (C.c_double * 4)()
        self.L.artemis_sim_checkpoint_seconds(out)
        return tuple(out)

    @staticmethod
    def describe_checkpoint(path, lib=None):
        """Header fields of a checkpoint as a dict (no device, no communicator)."""
        import json
        L = lib if lib is not None else capi.load()
        _declare(L)
        p = os.fspath(path).encode()
        n = L.artemis_sim_checkpoint_describe(p, None, 0)
        if n < 0:
            raise RuntimeError(L.artemis_sim_last_error().decode())
        buf = C.create_string_buffer(n + 1)
        if L.artemis_sim_checkpoint_describe(p, buf, n + 1) != n:
            raise RuntimeError("the checkpoint changed while it was read")
        return json.loads(buf.value.decode())

    def _refresh_dims(self):
        """Block layout of this rank (an adaptive mesh changes it between cycles)."""
        d = (C.c_int * 11)()
        self.L.artemis_sim_dims(self.h, d)
        (self.nblocks, self.ni, self.nj, self.nk, self.is_, self.ie, self.js, self.je, self.ks,
         self.ke, self.ng) = list(d)

    def close(self):
        if getattr(self, "h", None):
            self.L.artemis_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evolve(self, max_cycles=-1):
        n = self.L.artemis_sim_evolve(self.h, max_cycles)
        if n < 0:
            raise RuntimeError("artemis_sim_evolve: " + self.L.artemis_sim_last_error().decode())
        self._refresh_dims()
        return n

    time = property(lambda s: s.L.artemis_sim_time(s.h))
    dt = property(lambda s: s.L.artemis_sim_dt(s.h))
    tlim = property(lambda s: s.L.artemis_sim_tlim(s.h))
    ncycle = property(lambda s: s.L.artemis_sim_ncycle(s.h))
    local_zones = property(lambda s: s.L.artemis_sim_local_zones(s.h))
    total_zones = property(lambda s: s.L.artemis_sim_total_zones(s.h))
    uses_fused_path = property(lambda s: bool(s.L.artemis_sim_uses_fused_path(s.h)))
    uses_tuned_kernel = property(lambda s: bool(s.L.artemis_sim_uses_tuned_kernel(s.h)))
    stage_kernel = property(lambda s: s.L.artemis_sim_stage_kernel(s.h).decode())
    remeshes = property(lambda s: s.L.artemis_sim_remeshes(s.h))  # adaptive meshes: tree changes so far

    def force_refine(self, gid):
        """Split leaf `gid` (global Z-order index) through the ordinary remesh machinery; True if the mesh changed."""
        rc = self.L.artemis_sim_force_refine(self.h, gid)
        if rc < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        self._refresh_dims()
        return bool(rc)

    def inject_refine_tags(self, gids):
        """Tag the listed leaves +1 next to the criterion's own tags and run one remesh check; True if the mesh changed."""
        arr = (C.c_long * len(gids))(*gids)
        rc = self.L.artemis_sim_inject_refine_tags(self.h, arr, len(gids))
        if rc < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        self._refresh_dims()
        return bool(rc)

    def remesh_seconds(self):
        """(number of remeshes during the run, total seconds, build seconds, hand-over seconds, tagging seconds)"""
        out = (C.c_double * 4)()
        n = self.L.artemis_sim_remesh_seconds(self.h, out)
        return (n,) + tuple(out)

    def last_remesh(self):
        """The most recent remesh: (leaves before, after, created, destroyed), (seconds total, build, hand-over)"""
        lv, sec = (C.c_long * 4)(), (C.c_double * 3)()
        self.L.artemis_sim_last_remesh(self.h, lv, sec)
        return tuple(lv), tuple(sec)

    def device_bytes(self, reset_peak=False):
        """(current, peak) bytes of device memory held through the library's runtime shim"""
        cur, peak = C.c_size_t(0), C.c_size_t(0)
        self.L.artemis_rt_device_bytes(C.byref(cur), C.byref(peak), int(reset_peak))
        return cur.value, peak.value

    def cached_bytes(self):
        """bytes of device_bytes()[0] that sit free in the library's buffer cache (artemis_rt_pool_trim(0) returns them)"""
        return self.L.artemis_rt_pool_bytes()
    last_wall_seconds = property(lambda s: s.L.artemis_sim_last_wall_seconds(s.h))

    @property
    def load_balance(self):
        """max over ranks / mean of the cost of the Z-order rank split of a refined mesh (1 = even)."""
        return self.L.artemis_sim_load_balance(self.h)

    def set_path(self, which):
        if self.L.artemis_sim_set_path(self.h, which.encode()):
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    def set_overlap(self, mode):
        """False/0 off, True/2 one launch with in-kernel shell signalling, 1 shell + bulk launches."""
        mode = 2 if mode is True else int(mode)
        if self.L.artemis_sim_set_overlap(self.h, mode):
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    overlap = property(lambda s: s.L.artemis_sim_overlap(s.h))

    def set_dropin(self, on):
        """Tuned path only: also write cons on the last stage and run the whole-block PrimToCons per stage."""
        if self.L.artemis_sim_set_dropin(self.h, int(on)):  # 0 off, 1 whole-block PrimToCons, 2 ghost-zone PrimToCons
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    def set_kernel_timing(self, on):
        self.L.artemis_sim_set_kernel_timing(self.h, int(on))

    def kernel_ms(self):
        n = C.c_long(0)
        ms = self.L.artemis_sim_kernel_ms(self.h, C.byref(n))
        return ms, n.value

    def field(self, name, block=0):
        nvar = {"gas.prim": 6 * self.ns_gas, "gas.cons": 6 * self.ns_gas, "dust.prim": 4 * self.ns_dust,
                "dust.cons": 4 * self.ns_dust}[name]
        buf = np.empty((max(nvar, 1), self.nk, self.nj, self.ni))  # sized from the sim's species counts
        nv = self.L.artemis_sim_get_field(self.h, name.encode(), block, buf.ctypes.data)
        if nv < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        return buf.reshape(-1)[: nv * self.nk * self.nj * self.ni].reshape(nv, self.nk, self.nj, self.ni).copy()

    def interior(self, a):
        return a[..., self.ks:self.ke + 1, self.js:self.je + 1, self.is_:self.ie + 1]

    def nbody_force(self, reset=False):
        """[npart, 7] accumulated back-reaction rows of the n-body particles (summed over ranks)."""
        buf = (C.c_double * max(7 * self.L.artemis_sim_nbody_force(self.h, None, 0), 1))()  # sized by the size query
        n = self.L.artemis_sim_nbody_force(self.h, buf, int(reset))
        if n < 0:
            raise RuntimeError("artemis_sim_nbody_force failed")
        return np.array(buf[: 7 * n]).reshape(n, 7)

    def block_level(self, block=0):
        return self.L.artemis_sim_block_level(self.h, block)

    nblocks_global = property(lambda s: s.L.artemis_sim_nblocks_global(s.h))

    def block_bounds(self, block=0):
        o = (C.c_double * 6)()
        self.L.artemis_sim_block_bounds(self.h, block, o)
        return list(o)

    def history(self):
        o = (C.c_double * (6 + 4 * self.ns_dust))()
        n = self.L.artemis_sim_history(self.h, o)
        if n < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        return np.array(o[:n])

    def history_device(self):
        """The history integrals of every species, summed on the device from the primitives and reduced over the ranks:
        [mass, mom1..3, energy, internal energy] per gas species, then [mass, mom1..3] per dust species."""
        o = (C.c_double * max(6 * self.ns_gas + 4 * self.ns_dust, 1))()
        n = self.L.artemis_sim_history_device(self.h, o)
        if n < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        return np.array(o[:n])

    def enable_outputs(self, directory):
        """Act on the deck's <parthenon/outputN> blocks from now on: `hst` blocks append rows to
        <directory>/<problem_id>.outN.hst (artemis_amd.history.read_history reads them), `rst` blocks save checkpoints to
        <directory>/<problem_id>.outN.<counter>.rst (Simulation.restore reads them), `fld` blocks write their `variables` to
        <directory>/<problem_id>.outN.<counter>.fld (artemis_amd.fields.read_fields reads them).  Output times never change dt."""
        if self.L.artemis_sim_enable_outputs(self.h, os.fspath(directory).encode()):
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    def outputs(self):
        """The deck's output blocks and their state (status, next_time, rows or dumps written) as a dict."""
        import json
        n = self.L.artemis_sim_outputs_describe(self.h, None, 0)
        if n < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        buf = C.create_string_buffer(n + 1)
        if self.L.artemis_sim_outputs_describe(self.h, buf, n + 1) != n:
            raise RuntimeError("the output state changed while it was read")
        return json.loads(buf.value.decode())

    @staticmethod
    def _names(variables):
        variables = [variables] if isinstance(variables, str) else list(variables)
        return (C.c_char_p * max(len(variables), 1))(*[v.encode() for v in variables]), len(variables)

    @staticmethod
    def _axes(reduce, level):
        """the mask of a `reduce` argument ("x2", ("x2", "x3"), "x2,x3"): 1 = x1, 2 = x2, 4 = x3"""
        if level is not None:
            raise ValueError("reduce together with level is not built: splitting a coarse zone's integral across finer "
                             "output cells needs a rule")
        names = reduce.split(",") if isinstance(reduce, str) else list(reduce)
        axes = 0
        for name in names:
            name = name.strip()
            if name not in ("x1", "x2", "x3"):
                raise ValueError("reduce takes x1, x2 and/or x3, not %r" % (name,))
            axes |= 1 << (int(name[1]) - 1)
        if not axes:
            raise ValueError("reduce names no direction")
        return axes

    @staticmethod
    def _reduce_level(reduce, level, reduce_level):
        """reduce_level as an int, or None; it is only valid beside reduce and never with level"""
        if reduce_level is None:
            return None
        if reduce is None:
            raise ValueError("reduce_level is only valid beside reduce")
        if level is not None:
            raise ValueError("reduce_level together with level is not built: level resamples means, reduce_level integrals")
        return int(reduce_level)

    @classmethod
    def _field_mode(cls, level, reduce, reduce_level):
        """The two choices of gather / write_fields resolved: (suffix of the C entry point's name, its arguments after
        `single`, the mask of reduce or 0, the level the blocks are brought to or None)"""
        rl = cls._reduce_level(reduce, level, reduce_level)
        axes = 0 if reduce is None else cls._axes(reduce, level)
        lv = rl if axes else (None if level is None else int(level))
        return (("_reduced" if axes else "") + ("" if lv is None else "_level"), ([axes] if axes else []) + ([] if lv is None else [lv]),
                axes, lv)

    def gather(self, variables, single=False, level=None, reduce=None, reduce_level=None):
        """The named variables ('gas.prim.density', 'gas.prim.velocity', 'gas.prim.pressure', ...: include/artemis_driver.h
        "field output") of this rank's blocks, interior zones only, as [nblocks_local, ncomp, nz, ny, nx] float64 (float32
        with single=True).  Formed from the primitives on the device; nothing is materialised and the run is not disturbed.
        'gas.derived.divergence' (one component per species), 'gas.derived.vorticity' (three) and their 'dust.derived.*' forms
        are the velocity divergence and curl, formed on the device from a zone and its face neighbours, ghost zones included:
        right across block, rank and coarse-fine edges, and a component like any other in the modes below.
        level = an int: every block resampled on the device to the zone size of refinement level `level` (0 the root grid,
        negative coarser) -- finer blocks by the volume-weighted mean of the reference's restriction, coarser ones by
        replication -- and returned as a list, in local block order, of [ncomp, nz_b, ny_b, nx_b] views of one buffer.  Each
        requested component is averaged as formed (a velocity as a velocity): ask for gas.cons.* for the conservative answer.
        reduce = ("x2", "x3") (any of x1, x2, x3 that have more than one zone): every block integrated over those directions
        on the device -- per component the sum of V q, and the sum of the volumes V as one more, last, component -- and
        returned as [nblocks_local, ncomp + 1, nz', ny', nx'] with the reduced extents 1.  The order of the additions is
        fixed (include/artemis_hip.h, artemis_hip_reduce_fields), so the bits depend on the block alone; a mean is N / W
        after the blocks that share an output cell have been added.  reduce with level raises ValueError.
        reduce_level = an int (beside reduce): every reduced block also brought, on the device, to the zone size of refinement
        level `reduce_level` along the directions it keeps -- finer blocks by adding pairs, coarser ones by an equal share of
        N and W for each output cell under a coarse zone (include/artemis_hip.h, artemis_hip_reduce_fields_level) -- and
        returned as a list, in local block order, of [ncomp + 1, nz_b, ny_b, nx_b] views of one buffer, the volume last.
        All blocks then share a zone size, so those of a refined mesh add cell by cell.  reduce_level without reduce, or
        with level, raises ValueError."""
        names, n = self._names(variables)
        suffix, args, axes, lv = self._field_mode(level, reduce, reduce_level)
        fn = getattr(self.L, "artemis_sim_gather_fields" + suffix)
        self._refresh_dims()
        off = (C.c_long * (self.nblocks + 1))()
        tail = [] if lv is None else [off]
        nbytes = fn(self.h, n, names, int(single), *args, None, *tail)
        if nbytes < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        out = np.empty(nbytes // (4 if single else 8), dtype=np.float32 if single else np.float64)
        ncomp = fn(self.h, n, names, int(single), *args, out.ctypes.data, *tail)
        if ncomp < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        nx = [self.ie - self.is_ + 1, self.je - self.js + 1, self.ke - self.ks + 1]

        def shape(s):  # of a block at shift s: the rows (the volume last where axes are set), then nz', ny', nx'
            e = [1 if (axes >> q) & 1 or m == 1 else (m >> s if s >= 0 else m << -s) for q, m in enumerate(nx)]
            return (ncomp + (1 if axes else 0), e[2], e[1], e[0])
        if lv is None:
            return out.reshape((self.nblocks,) + shape(0))
        return [out[off[b]:off[b + 1]].reshape(shape(self.block_level(b) - lv)) for b in range(self.nblocks)]

    def write_fields(self, path, variables, single=False, level=None, reduce=None, reduce_level=None):
        """One dump of the named variables as a directory at `path` (collective over the ranks of the run; replaces an
        existing one).  artemis_amd.fields.read_fields reads it.  level = an int: every block resampled to refinement level
        `level` as in gather (a version-2 dump; FieldDump.uniform() then works on any mesh).  reduce = ("x2", "x3"): every
        block integrated over those directions as in gather (a version-3 dump; FieldDump.reduced() assembles it).
        reduce_level = an int beside reduce: the reduced blocks brought to that level along their kept directions as in gather
        (a version-4 dump, which FieldDump.reduced() assembles on any mesh)."""
        names, n = self._names(variables)
        suffix, args, _, _ = self._field_mode(level, reduce, reduce_level)
        fn = getattr(self.L, "artemis_sim_write_fields" + suffix)
        if fn(self.h, os.fspath(path).encode(), n, names, int(single), *args):
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    def scatter(self, variables, array, time=None):
        """The inverse of gather: the run takes its state from `array`, [nblocks_local, ncomp, nz, ny, nx] float64 or float32,
        C-contiguous, laid out as gather(variables) returns it.  For each fluid the variables give one complete form or
        nothing: gas.prim.density + .velocity + one of .sie / .pressure, or gas.cons.density + .momentum + .total_energy
        (+ .internal_energy); dust.prim.density + .velocity, or dust.cons.density + .momentum.  The ghost zones are filled
        and the conserved state formed as after a problem generator, `time` becomes the clock (None keeps it) and dt a fresh
        estimate; ncycle, the mesh and the output schedule stay.  Collective over the ranks of the run.  ValueError for an
        array of the wrong shape, dtype or layout, RuntimeError for what the driver refuses."""
        names, n = self._names(variables)
        if not isinstance(array, np.ndarray) or array.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("scatter takes a numpy array of float64 or float32, not %s"
                             % (array.dtype if isinstance(array, np.ndarray) else type(array).__name__))
        if not array.flags["C_CONTIGUOUS"]:
            raise ValueError("scatter takes a C-contiguous array")
        single = array.dtype == np.float32
        listed = [variables] if isinstance(variables, str) else list(variables)
        species = {"gas": self.ns_gas, "dust": self.ns_dust}
        # (a name outside the list, or of a fluid the run lacks, is the driver's to refuse)
        if all(v in capi.FIELD_VAR and species[v.split(".")[0]] > 0 for v in listed):
            self._refresh_dims()
            ncomp = sum((3 if v.endswith(("velocity", "momentum")) else 1) * (self.ns_dust if v.startswith("dust.") else self.ns_gas)
                        for v in listed)
            want = (self.nblocks, ncomp, self.ke - self.ks + 1, self.je - self.js + 1, self.ie - self.is_ + 1)
            if tuple(array.shape) != want:
                raise ValueError("scatter: the array is %s, these variables on this rank's blocks are %s" % (tuple(array.shape), want))
        t = float("nan") if time is None else float(time)
        if self.L.artemis_sim_scatter_fields(self.h, n, names, int(single), array.ctypes.data, t) < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())

    def sample_plan(self, points):
        """A SamplePlan of `points`, [npoints, 3] float64, C-contiguous, in the mesh's own coordinates (x1, x2, x3): each point
        is found on the device in this rank's blocks -- leaves are half-open, the mesh's upper edge is closed, coordinates
        along a direction with one zone are ignored, nothing wraps periodically -- and plan.values(variables) returns the
        zone's values as gather forms them.  The cost follows the points, not the mesh: the midplane of a 256^3 block is a
        256^2 plan (artemis_amd.sample.lattice), a zoom at the finest level of a refined mesh a lattice of that zone size,
        an image of a disk artemis_amd.sample.from_cartesian of its pixels.  Not collective: a rank answers for its own blocks
        (plan.block is -1 and the values NaN for the rest), and an in-domain point is found on exactly one rank.  ValueError
        for an array of another dtype, shape or layout."""
        return SamplePlan(self, points)

    def sample(self, variables, points, single=False):
        """(values [ncomp, npoints], block [npoints]) of a plan made, used once and closed: sample_plan(points).values(...)"""
        plan = self.sample_plan(points)
        try:
            return plan.values(variables, single), plan.block
        finally:
            plan.close()

    def record(self, points_or_plan, variables, every=1, capacity=None, single=False):
        """A Recorder: after every `every`-th cycle that evolve() completes from now on, one row {cycle, time, dt, values
        [ncomp, npoints]} is taken ON THE DEVICE, inside the time loop and its captured graphs -- the cycle number, time and
        next dt that ncycle / time / dt would show had evolve returned there, and what plan.values(variables, single) would
        return at that moment, bit for bit.  points_or_plan: a SamplePlan of this simulation, or an [npoints, 3] float64 array
        (a plan is made; the recorder owns and closes it).  capacity: rows the device buffers hold before evolve() copies
        them to the host at a batch boundary (no row is lost); None: max(1, min(4096, 64 MiB // bytes of a row)).  The run is
        not disturbed: the same bits with and without recorders.  Only evolve() records; scatter, load_fields, force_refine,
        gather and values do not.  ValueError: every < 1, capacity < 1, a plan of another simulation; RuntimeError: what the
        driver refuses (an unknown variable, a closed plan)."""
        if int(every) < 1:
            raise ValueError("every = %r: at least 1" % (every,))
        if capacity is not None and int(capacity) < 1:
            raise ValueError("capacity = %r: at least 1 row" % (capacity,))
        if isinstance(points_or_plan, SamplePlan):
            if points_or_plan.sim is not self:
                raise ValueError("the sample plan belongs to another simulation")
            points_or_plan._live()
            return Recorder(self, points_or_plan, variables, every, capacity, single, False)
        plan = self.sample_plan(points_or_plan)
        try:
            return Recorder(self, plan, variables, every, capacity, single, True)
        except Exception:
            plan.close()
            raise

    def record_integrals(self, every=1, capacity=None, windows=None, nbody=False):
        """An IntegralRecorder: after every `every`-th cycle that evolve() completes from now on, one row {cycle, time, dt,
        integrals [1 + nwin, nq], nbody [npart, 7]} is taken ON THE DEVICE through the same tick as record().  Set 0 is the
        history integrals of this rank's mesh -- what history_device() would return there, bit for bit on one rank -- and set
        1 + w those of window w: windows is an [nwin, 3, 2] array (at most 7) of boxes [lo, hi) in the mesh's own coordinates,
        an annular sector on a cylindrical mesh; a zone belongs to a window when the midpoint of its faces lies in it along
        every direction with more than one zone (rec.window_zones() shows the index ranges).  nbody=True adds the n-body
        force sums, what nbody_force() would return if first called there; nothing is flushed.  capacity: as for record().
        ValueError: every < 1, capacity < 1, a windows array of another shape or with more than 7 windows; RuntimeError: what
        the driver refuses (a window with lo >= hi, nbody=True on a deck without particles)."""
        if int(every) < 1:
            raise ValueError("every = %r: at least 1" % (every,))
        if capacity is not None and int(capacity) < 1:
            raise ValueError("capacity = %r: at least 1 row" % (capacity,))
        return IntegralRecorder(self, every, capacity, windows, nbody)

    # the complete forms a dump may hold, in the order load_fields prefers them
    _GAS_FORMS = (("gas.prim.density", "gas.prim.velocity", "gas.prim.sie"),
                  ("gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"),
                  ("gas.cons.density", "gas.cons.momentum", "gas.cons.total_energy"))
    _DUST_FORMS = (("dust.prim.density", "dust.prim.velocity"), ("dust.cons.density", "dust.cons.momentum"))

    def _agree(self, problem):
        """Raise on every rank if any rank has a problem (a rank that raised alone would leave the others in a collective)."""
        if self.comm is not None and self.comm.struct.nranks > 1:
            v = C.c_double(0.0 if problem else 1.0)
            if self.comm.struct.allreduce_min(self.comm.struct.ctx, C.byref(v)):
                raise RuntimeError("allreduce failed")
            if problem is None and v.value == 0.0:
                problem = "load_fields: another rank could not take its blocks from the dump"
        if problem:
            raise ValueError(problem)

    def load_fields(self, path, clock=True):
        """Start from a `fld` dump (write_fields, or a deck's fld block): its blocks are matched to this rank's by level and
        bounds, so a dump written on any number of ranks loads on any other, and scatter() takes whichever complete form
        the dump holds of each fluid -- primitives with sie first, then primitives with the pressure, then the conserved
        variables.  clock=True also takes the dump's time.  ValueError names the first block of this rank the dump lacks,
        or the first variable missing for a complete form.  Collective.  Returns the variables taken."""
        from .fields import read_fields
        fd = read_fields(path)
        if fd.level is not None:
            raise ValueError("%s was resampled to level %d: not a state" % (path, fd.level))
        if fd.reduce is not None:
            raise ValueError("%s was reduced along %s: not a state" % (path, ", ".join(fd.reduce)))
        have = set(fd.variables)
        names = []
        for fluid, ns, forms in (("gas", self.ns_gas, self._GAS_FORMS), ("dust", self.ns_dust, self._DUST_FORMS)):
            mine = sorted(v for v in have if v.startswith(fluid + "."))
            if not mine:
                continue
            if ns == 0:
                raise ValueError("%s holds %s, and this run has no %s" % (path, mine[0], fluid))
            form = next((f for f in forms if have.issuperset(f)), None)
            if form is None:  # the form the dump is closest to, and what it lacks first
                near = max(forms, key=lambda f: sum(v in have for v in f))
                lacking = next(v for v in near if v not in have)
                if lacking in ("gas.prim.sie", "gas.prim.pressure"):
                    lacking = "gas.prim.sie (or gas.prim.pressure)"
                raise ValueError("%s holds %s: %s is missing for a complete form" % (path, ", ".join(mine), lacking))
            names += list(form)
            if form[0] == "gas.cons.density" and "gas.cons.internal_energy" in have:
                names.append("gas.cons.internal_energy")
            for v in form:
                if fd.variables[v] != (3 if v.endswith(("velocity", "momentum")) else 1) * ns:
                    raise ValueError("%s: %s has %d components, this run %d species" % (path, v, fd.variables[v], ns))
        if not names:
            raise ValueError("%s holds no variable of this run's fluids" % path)
        self._refresh_dims()
        nx = [self.ie - self.is_ + 1, self.je - self.js + 1, self.ke - self.ks + 1]
        problem, gids = None, []
        if list(fd.nx) != nx:
            problem = "%s: its blocks are %s zones, this run's %s" % (path, list(fd.nx), nx)
        where = {(b["level"], tuple(b["bounds"])): g for g, b in enumerate(fd.blocks)}
        for b in range(self.nblocks if problem is None else 0):
            key = (self.block_level(b), tuple(self.block_bounds(b)))
            if key not in where:
                problem = "%s holds no block on level %d with the bounds %s (local block %d of this run)" % (path, key[0], list(key[1]), b)
                break
            gids.append(where[key])
        self._agree(problem)
        array = np.concatenate([fd.get(v)[gids] for v in names], axis=1) if gids else \
            np.empty((0, sum(fd.variables[v] for v in names), nx[2], nx[1], nx[0]), dtype=fd.dtype)
        self.scatter(names, np.ascontiguousarray(array), time=fd.time if clock else None)
        return names

    def errors(self):
        o = (C.c_double * 16)()
        n = self.L.artemis_sim_errors(self.h, o)
        if n < 0:
            raise RuntimeError(self.L.artemis_sim_last_error().decode())
        return np.array(o[:n])
