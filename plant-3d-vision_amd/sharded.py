"""Multi-GPU space carving: one process per GPU, the grid sharded by X-planes.

The reference is single-device (one module-global OpenCL queue, ``plant3dvision/cl.py:29-30``);
this module is the MI355X-native addition.  Voxels are independent
(``kernels/backprojection.c:64-84``: one owner per voxel), so:

* rank r owns a set of x-planes of the C-order ``[nx][ny][nz]`` grid, computed from GLOBAL
  indices, hence bit-identical to the single-GPU result.  Two partitions:
  ``"cyclic"`` (default): planes ``r, r+W, r+2W, ...`` (``sc_create_cyclic``).  The object sits
  in the middle of the grid, so contiguous slabs give the middle ranks all the surviving voxels
  (measured at 1024^3 / 8 ranks: 6.3 ms on ranks 3-4 against 0.34 ms on the others); dealing the
  planes round-robin gives every rank the same mix.
  ``"slab"``: ``i in [nx*r//W, nx*(r+1)//W)`` (``sc_create_slab``), a contiguous block of the
  output, for consumers that want one;
* every rank applies every view to its slab: the data path needs NO collective;
* assembling the full grid is a separate, optional step: ``gather_to_host`` (what a
  ``Voxels`` run needs: the volume in host memory of one process), ``all_gather`` (RCCL
  all-gather over xGMI, every GPU ends with the full grid) or ``all_reduce`` (the
  zero-padded sum the north star words; ring-bound).

``torch.distributed`` is plumbing only (process group, RCCL/gloo collectives); the carve runs
in the HIP engine.  ``engine_factory`` exists so the host logic can be exercised on CPU with
gloo in tests; the default is the HIP engine and there is no CPU fallback.
"""
import numpy as np

from . import _native as nat


def rank_planes(nx, world_size, rank, partition="cyclic"):
    """The global x indices rank ``rank`` owns, as a ``range``."""
    if partition == "cyclic":
        if not 0 <= rank < world_size:
            raise ValueError("rank out of range")
        if world_size > nx:
            raise ValueError(f"cannot shard {nx} planes over {world_size} ranks")
        return range(rank, nx, world_size)
    if partition == "slab":
        i0, i1 = slab_bounds(nx, world_size, rank)
        return range(i0, i1)
    raise ValueError("partition must be 'cyclic' or 'slab'")


def slab_bounds(nx, world_size, rank):
    """X range ``[i0, i1)`` of ``rank``; slabs differ by at most one plane."""
    if not 0 <= rank < world_size:
        raise ValueError("rank out of range")
    if world_size > nx:
        raise ValueError(f"cannot shard {nx} planes over {world_size} ranks")
    return nx * rank // world_size, nx * (rank + 1) // world_size


class _DeviceBuffer:
    """Exposes an engine-owned device allocation to torch (zero copy)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2}


class PackedGrid:
    """The assembled grid as the all-gather left it: every rank's planes at ``bits`` per label, rank-major, on this
    rank's device.  ``vol2pcd`` reads it as it is (``proc3d.vol2pcd(packed_grid, ...)``: the occupancy ``label == 1``
    is what the reference binarises to, proc3d.py:515); ``unpack()`` makes the int8 / int32 grid in global order for
    consumers that want one -- 1 GiB of writes per GPU at 1024^3 that a ``vol2pcd`` run never needs."""

    def __init__(self, recv, rank_bytes, world, partition, shape, bits, device):
        self.recv, self.rank_bytes, self.world = recv, int(rank_bytes), int(world)
        self.partition, self.shape, self.bits, self.device = partition, [int(s) for s in shape], int(bits), int(device)

    def unpack(self, widen=False, out=None):
        import torch
        n = int(np.prod(self.shape))
        dt = torch.int32 if widen else torch.int8
        if out is None or out.dtype != dt or out.numel() < n:
            out = torch.empty(n, dtype=dt, device=self.recv.device)
        nat.unpack_labels(self.device, torch.cuda.current_stream(self.recv.device).cuda_stream, self.recv.data_ptr(),
                          self.rank_bytes, self.world, self.partition, self.shape, self.bits, out.data_ptr(), 4 if widen else 1)
        return out[:n].view(self.shape)


class SparseOverflow(RuntimeError):
    """A rank had more mixed bricks than the capacity every rank sent with: gather again with ``needed`` slots."""

    def __init__(self, needed, cap):
        super().__init__(f"{needed} mixed bricks on some rank for a capacity of {cap}")
        self.needed, self.cap = int(needed), int(cap)


class DevMem:
    """Device memory of the engine's device without torch (``sc_dev_alloc``): the receive buffers of the library's own
    collectives."""

    def __init__(self, engine, nbytes):
        self._engine, self.nbytes = engine, int(nbytes)
        self.ptr = engine.dev_alloc(max(16, self.nbytes))

    def data_ptr(self):
        return self.ptr

    def free(self):
        if self.ptr:
            self._engine.dev_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if self.ptr and getattr(self._engine, "_h", 0):
                self.free()
        except Exception:  # noqa: BLE001
            pass


class SparseGrid:
    """The assembled grid in the BRICK-SPARSE form (``include/spacecarve.h``): every rank's header, one code per
    16 x 64-voxel brick and the 2-bit labels of its mixed bricks only, rank-major -- 131 KB + 260 bytes per mixed brick
    and rank where the dense 2-bit form is 32 MiB.  ``recv`` is a CUDA / host torch tensor or a :class:`DevMem`;
    ``stream`` the HIP stream the collective ran on (0: torch's current / none).  ``verify()`` waits for the
    collective and checks that no rank ran out of slots; ``unpack()`` writes the int8 / int32 grid in global order;
    ``occupancy_device()`` the uint8 ``label == 1`` volume ``proc3d.vol2pcd`` reads (proc3d.py:515);
    ``to_host()`` the int32 array of cl.py:229-232 (widened by the library's host pool)."""

    def __init__(self, recv, rank_bytes, world, shape, device, cap, stream=0, on_gpu=True, engine=None, done_event=0,
                 headers_host=0):
        self.recv, self.rank_bytes, self.world = recv, int(rank_bytes), int(world)
        self.shape, self.device, self.cap = [int(s) for s in shape], int(device), int(cap)
        self.stream, self.on_gpu, self._engine = int(stream or 0), bool(on_gpu), engine
        #: the event the library recorded behind this grid's collective: ``verify`` waits for it and not for whatever the
        #: collectives' stream has been given since (the next batch's collective, which waits for the next batch's carve)
        self.done_event = int(done_event or 0)
        #: ... and the page-locked copy of the ranks' headers the library made behind that collective
        self.headers_host = int(headers_host or 0)
        self.nmixed = None

    def _ptr(self):
        return int(self.recv.data_ptr())

    def _host_bytes(self):
        if self.on_gpu:
            if hasattr(self.recv, "cpu"):
                return self.recv.cpu().numpy()
            out = np.empty(self.rank_bytes * self.world, dtype=np.uint8)
            self._engine.dev_download(out, self.recv.ptr)
            return out
        return self.recv.numpy() if hasattr(self.recv, "numpy") else np.asarray(self.recv)

    def verify(self):
        """Waits for the collective; raises :class:`SparseOverflow` if some rank had more mixed bricks than slots."""
        if self.nmixed is None:
            if self.on_gpu:
                stream = self.stream
                if not stream and hasattr(self.recv, "is_cuda"):
                    import torch
                    stream = torch.cuda.current_stream(self.recv.device).cuda_stream
                if self.done_event and self.headers_host:
                    nm, cp = nat.sparse_wait_headers(self.done_event, self.headers_host, self.rank_bytes, self.world)
                else:
                    nm, cp = nat.sparse_headers(self.device, stream, self._ptr(), self.rank_bytes, self.world,
                                                done_event=self.done_event)
                self.done_event = self.headers_host = 0  # (the engine uses them again two gathers later)
            else:
                buf = self._host_bytes().reshape(self.world, self.rank_bytes)
                hdr = np.ascontiguousarray(buf[:, :64]).view(np.uint32)
                if not (hdr[:, 0] == 0x50534353).all():
                    raise ValueError("not a sparse label buffer")
                nm, cp = hdr[:, 5].copy(), hdr[:, 4].copy()
            self.nmixed, self.caps = nm, cp
        worst = int(max(int(n) for n in self.nmixed))
        if any(int(n) > int(c) for n, c in zip(self.nmixed, self.caps)):
            raise SparseOverflow(worst, self.cap)
        return self

    def unpack(self, widen=False, out=None, kind=None):
        """The grid in global order on the device: int8 labels, ``widen``: int32; ``kind=0``: uint8 occupancy."""
        self.verify()
        kind = (4 if widen else 1) if kind is None else int(kind)
        n = int(np.prod(self.shape))
        if not self.on_gpu:
            raise RuntimeError("host tensors: use to_host()")
        if hasattr(self.recv, "is_cuda"):
            import torch
            dt = {4: torch.int32, 1: torch.int8, 0: torch.uint8}[kind]
            if out is None or out.dtype != dt or out.numel() < n:
                out = torch.empty(n, dtype=dt, device=self.recv.device)
            stream = self.stream or torch.cuda.current_stream(self.recv.device).cuda_stream
            nat.unpack_sparse(self.device, stream, self._ptr(), self.rank_bytes, self.world, self.shape, out.data_ptr(), kind)
            return out[:n].view(self.shape)
        if out is None:
            out = DevMem(self._engine, n * (4 if kind == 4 else 1))
        nat.unpack_sparse(self.device, self.stream, self._ptr(), self.rank_bytes, self.world, self.shape, out.data_ptr(), kind)
        return out

    def occupancy_device(self):
        """(device pointer, keep-alive object) of the uint8 occupancy ``label == 1`` in global order; the kernel has
        completed when this returns."""
        occ = self.unpack(kind=0)
        if hasattr(occ, "is_cuda"):
            import torch
            torch.cuda.current_stream(occ.device).synchronize()
            return int(occ.data_ptr()), occ
        nat.sparse_headers(self.device, self.stream, self._ptr(), self.rank_bytes, self.world)  # (waits for the stream)
        return int(occ.ptr), occ

    def to_host(self, out=None):
        self.verify()
        return nat.widen_sparse_ranks(self._host_bytes(), self.rank_bytes, self.world, self.shape, out=out)


def exchange_unique_id(rank, world_size, addr=None, port=None, timeout=300.0):
    """The 128-byte RCCL id from rank 0 to every rank over a TCP socket of the standard library (no torch): rank 0
    listens on (``addr``, ``port``) -- ``SC_COMM_ADDR`` / ``SC_COMM_PORT``, else ``MASTER_ADDR`` / ``MASTER_PORT`` + 1 --
    and serves the id to the world_size - 1 others, who retry their connection until it is there."""
    import os
    import socket
    import time
    addr = addr or os.environ.get("SC_COMM_ADDR") or os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(port or os.environ.get("SC_COMM_PORT") or int(os.environ.get("MASTER_PORT", "29511")) + 1)
    if rank == 0:
        uid = nat.Comm.unique_id()
        if world_size > 1:
            with socket.socket() as srv:
                srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                srv.bind((addr, port))
                srv.listen(world_size)
                srv.settimeout(timeout)
                for _ in range(world_size - 1):
                    conn, _ = srv.accept()
                    with conn:
                        conn.sendall(uid)
        return uid
    deadline = time.time() + timeout
    while True:
        try:
            with socket.create_connection((addr, port), timeout=5.0) as so:
                buf = b""
                while len(buf) < nat.Comm.ID_BYTES:
                    chunk = so.recv(nat.Comm.ID_BYTES - len(buf))
                    if not chunk:
                        break
                    buf += chunk
            if len(buf) == nat.Comm.ID_BYTES:
                return buf
        except OSError:
            pass
        if time.time() > deadline:
            raise TimeoutError(f"no RCCL id from rank 0 at {addr}:{port}")
        time.sleep(0.05)


class ShardedBackprojection:
    """Slab-sharded ``Backprojection``: same per-view interface, one slab per rank."""

    def __init__(self, shape, origin, voxel_size, type="carving", default_value=0, rank=None,
                 world_size=None, device=None, engine_factory=None, views_per_launch=0,
                 partition="cyclic", log=False, unpack_fn=None):
        if rank is None or world_size is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_initialized() else 0
            world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.rank, self.world_size = int(rank), int(world_size)
        #: rehearsal switch: with a process group of ONE rank, still go through the collectives (RCCL on a
        #: one-GPU box exercises the same calls, buffers and stream ordering as on eight)
        self.force_collective = False
        self.shape = [int(s) for s in shape]
        self.origin = origin
        self.voxel_size = voxel_size
        self.default_value = default_value
        self.log = log
        self._lut = None
        if type == "carving":
            self.dtype, self._mode = np.int32, nat.SC_MODE_CARVE
        elif type == "averaging":
            self.dtype, self._mode = np.float32, nat.SC_MODE_AVERAGE
        else:
            raise ValueError(f"Unknown kernel type {type}, valid values are 'averaging' or 'carving'!")
        self.partition = partition
        self.planes = rank_planes(self.shape[0], self.world_size, self.rank, partition)
        self.device = self.rank if device is None else int(device)
        factory = engine_factory or nat.Engine
        if partition == "cyclic":
            self._engine = factory(self.shape, origin, voxel_size, self._mode,
                                   default_value=float(default_value), device=self.device,
                                   cyclic=(self.rank, self.world_size))
        else:
            self._engine = factory(self.shape, origin, voxel_size, self._mode,
                                   default_value=float(default_value), device=self.device,
                                   slab=(self.planes.start, self.planes.stop))
        if views_per_launch:
            self._engine.set_option(nat.SC_OPT_VIEWS_PER_LAUNCH, int(views_per_launch))
        self._on_gpu = engine_factory is None
        #: ``all_gather(overlap=True)``: the stream whose collective still reads the engine's packed labels; the
        #: engine waits for it right before it packs again (``_settle``), not right behind the collective, so the
        #: collective of batch k runs beside the carve of batch k + 1
        self._lazy_wait = None
        #: host tensors only (CPU tests of the host logic over gloo): what stands in for ``sc_unpack_labels``
        self._unpack_fn = unpack_fn
        #: the library's own RCCL communicator (``init_comm``): collectives without torch
        self.comm = None
        #: payload slots (bricks) every rank sends with in the sparse form; grows when a rank runs out (every rank sees
        #: the same headers, so all ranks change it alike)
        self._sparse_cap = max(1024, self._bricks_max() // 8)
        self._sparse_recv = [None, None]
        self._sparse_turn = 0
        self._streams = None
        self._comm_shared = False
        self._ctor = dict(type=type, default_value=default_value, engine_factory=engine_factory,
                          views_per_launch=views_per_launch, partition=partition, log=log, unpack_fn=unpack_fn)

    def twin(self):
        """A second engine on the SAME planes of the same rank and device, sharing this one's communicator: two
        engines taking turns are the double buffering of a pipeline of scans -- while the labels of scan k are packed
        and gathered (``all_gather(..., overlap=True)``), the twin carves scan k + 1 on its own stream and label volume,
        and nobody's carve waits for a pack.  Every rank must alternate alike (the collectives pair up in call order).
        Close the twin before (or with) its parent; the communicator stays the parent's."""
        other = ShardedBackprojection(self.shape, self.origin, self.voxel_size, rank=self.rank, world_size=self.world_size,
                                      device=self.device, **self._ctor)
        other.force_collective = self.force_collective
        other.comm = self.comm
        other._comm_shared = True
        other._sparse_cap = self._sparse_cap
        return other

    def _bricks_max(self):
        ny, nz = self.shape[1], self.shape[2]
        return self._planes_max() * ((ny + 15) // 16) * ((nz + 63) // 64)

    def init_comm(self, unique_id=None):
        """The library's RCCL communicator for this rank (collective: every rank calls it).  The 128-byte id comes from
        rank 0 -- ``unique_id`` if the caller has moved it, else over ``torch.distributed`` when a process group
        exists, else over a TCP socket (``exchange_unique_id``: no torch anywhere on a carve rank)."""
        if self.comm is not None:
            return self.comm
        if not self._on_gpu:
            raise RuntimeError("the library's collectives need the HIP engine")
        if unique_id is None:
            dist = None
            try:
                import sys
                if "torch" in sys.modules:
                    import torch.distributed as dist
                    if not dist.is_initialized():
                        dist = None
            except ImportError:
                dist = None
            if dist is not None:
                box = [None]
                if self.rank == 0:
                    try:
                        box = [nat.Comm.unique_id()]
                    except Exception as ex:  # noqa: BLE001 -- the others are waiting in the broadcast: tell them
                        box = [ex]
                dist.broadcast_object_list(box, src=0)
                if isinstance(box[0], Exception):
                    raise RuntimeError(f"rank 0 could not make the RCCL id: {box[0]!r}")
                unique_id = box[0]
            else:
                unique_id = exchange_unique_id(self.rank, self.world_size)
        self.comm = nat.Comm(unique_id, self.world_size, self.rank, self.device)
        return self.comm

    @property
    def engine(self):
        return self._engine

    @property
    def slab_shape(self):
        return (len(self.planes), self.shape[1], self.shape[2])

    def process_view(self, intrinsics, rot, tvec, mask, mask_dtype=None):
        """``Backprojection.process_view`` on this rank's planes: the same host conversions
        (cl.py:205-215: ``img_as_float32``, the ``log`` step, the dtype casts, uint8 + table for
        averaging).  ``mask_dtype`` hands an already converted mask straight to the engine."""
        if mask_dtype is not None:
            self._engine.process_view(intrinsics, rot, tvec, np.ascontiguousarray(mask), mask_dtype)
            return
        from .cl import submit_view
        self._lut = submit_view(self._engine, self.dtype, self.log, self._lut, intrinsics, rot, tvec,
                                mask, invert=False)

    def clear(self):
        self._engine.clear()

    def flush(self):
        self._engine.flush()

    def _settle(self):
        """The engine's stream waits for a collective that ``all_gather(overlap=True)`` left reading the packed
        labels (device-side order; the host does not wait).  Called before anything packs or reads back again."""
        if self._lazy_wait is not None:
            self._engine.order_after(self._lazy_wait)
            self._lazy_wait = None

    def synchronize(self):
        self._settle()
        self._engine.synchronize()

    def get_local(self):
        """This rank's planes as a host array ``[len(planes), ny, nz]`` (in ``self.planes`` order)."""
        self._settle()
        return self._engine.get_values()

    # -- assembling the grid ----------------------------------------------------------------
    def _slab_tensor(self, on_device=True):
        import torch
        if self._on_gpu and on_device:
            ptr = self._engine.values_device_ptr()
            self._engine.synchronize()
            typestr = "<i4" if self.dtype == np.int32 else "<f4"
            buf = _DeviceBuffer(ptr, self._engine.num_voxels(), typestr)
            return torch.as_tensor(buf, device=f"cuda:{self.device}")
        return torch.from_numpy(np.ascontiguousarray(self.get_local()).reshape(-1))

    def _planes_max(self):
        return max(len(rank_planes(self.shape[0], self.world_size, r, self.partition))
                   for r in range(self.world_size))

    def _is_even(self):
        return self.shape[0] % self.world_size == 0

    @property
    def _alone(self):
        """A group of one that does not rehearse the collectives: this rank's buffer is the whole grid."""
        return self.world_size == 1 and not self.force_collective

    def _three_state(self, wire):
        """Carve labels that a default value of -1, 0 or 1 keeps in three states, on an engine with the host method
        ``wire`` (``"get_values_packed"`` / ``"get_values_sparse"``): what the 2-bit and sparse wires carry."""
        return self.dtype == np.int32 and float(self.default_value) in (-1.0, 0.0, 1.0) and hasattr(self._engine, wire)

    def _wire_bytes(self, bits=None, cap=None, on_device=True):
        """This rank's labels packed for the wire -- ``bits`` per label, or the sparse form with ``cap`` payload slots --
        as a uint8 tensor, and torch's stream the engine was ordered before (None: host bytes)."""
        import torch
        if self._on_gpu and on_device:
            # the batch's kernels first, THEN the wait for the previous collective, then the pack
            self._engine.flush()
            self._settle()
            ptr, nbytes = self._engine.values_packed(bits) if cap is None else self._engine.values_sparse(cap)
            # packed on the engine's stream; the collective and the unpack run on torch's: ordered on the device,
            # nothing waits on the host
            tstream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
            self._engine.order_before(tstream)
            return torch.as_tensor(_DeviceBuffer(ptr, nbytes, "|u1"), device=f"cuda:{self.device}"), tstream
        host = self._engine.get_values_packed(bits) if cap is None else self._engine.get_values_sparse(cap)
        return torch.from_numpy(np.ascontiguousarray(host).view(np.uint8)), None

    @staticmethod
    def _pad(local, n):
        """``local`` as the ``n`` elements every rank sends (the rank with the most planes sets ``n``): zeros after a
        rank with one plane fewer; a packed tail longer than the stride is cut."""
        if local.numel() == n:
            return local
        import torch
        send = torch.zeros(n, dtype=local.dtype, device=local.device)
        send[: min(local.numel(), n)] = local[:n]
        return send

    def _all_gather_into(self, send, recv=None):
        """Every rank's ``send`` rank-major in ``recv`` (a new buffer unless ``recv`` has the dtype, the device and
        the size), or ``send`` itself when ``_alone``.  gloo takes device tensors through the host."""
        import torch
        import torch.distributed as dist
        if self._alone:
            return send
        n = send.numel() * self.world_size
        if recv is None or getattr(recv, "dtype", None) != send.dtype or recv.numel() < n or recv.device != send.device:
            recv = torch.empty(n, dtype=send.dtype, device=send.device)
        recv = recv[:n]
        staged = dist.get_backend() == "gloo" and recv.is_cuda  # rehearsal on one box: through the host
        if staged and self.world_size == 1:  # (gloo takes 50 ms to gather a group of one: a poll that waits for nobody)
            return recv.copy_(send.cpu())
        into = torch.empty(recv.shape, dtype=recv.dtype) if staged else recv
        dist.all_gather_into_tensor(into, send.cpu() if staged else send)
        if staged:
            recv.copy_(into)
        return recv

    def _gather_to(self, send, dst):
        """Every rank's ``send`` rank-major in a new buffer on rank ``dst``; None on the other ranks."""
        import torch
        import torch.distributed as dist
        recv = None
        if self.rank == dst:
            recv = torch.empty(send.numel() * self.world_size, dtype=send.dtype, device=send.device)
        dist.gather(send, list(recv.view(self.world_size, -1).unbind(0)) if recv is not None else None, dst=dst)
        return recv

    def _hand_back(self, tstream, overlap=False):
        """The engine's next pack must not overwrite what the collective on torch's stream ``tstream`` still reads: it
        waits for it from now on, or (``overlap``) only right before that pack (``_settle``)."""
        if tstream is None:
            return
        if overlap:
            self._lazy_wait = tstream
        else:
            self._engine.order_after(tstream)

    def _land(self, recv, out=None):
        """Global-order grid from the all-gather's receive buffer ``[W][P][ny*nz]`` (P = the
        largest plane count of a rank; shorter ranks are padded at the end).

        slab, nx % W == 0 : the receive buffer IS the grid -- nothing moves;
        cyclic            : ONE strided copy (a device kernel) interleaves the planes,
                            ``full[p*W + r] = recv[r][p]``, into a buffer of P*W planes whose
                            first nx planes are returned (a contiguous view);
        slab, uneven      : one block copy per rank.
        """
        import torch
        W, P = self.world_size, self._planes_max()
        nx, ny, nz = self.shape
        plane = ny * nz
        recv = recv.view(W, P, plane)
        if self.partition == "slab" and self._is_even():
            return recv.view(nx, ny, nz)
        if out is None:
            out = torch.empty(P * W * plane, dtype=recv.dtype, device=recv.device)
        if self.partition == "cyclic":
            out.view(P, W, plane).copy_(recv.transpose(0, 1))
            return out[: nx * plane].view(nx, ny, nz)
        full = out[: nx * plane].view(nx, plane)
        for r in range(W):
            pl = rank_planes(nx, W, r, "slab")
            full[pl.start:pl.stop] = recv[r, : len(pl)]
        return full.view(nx, ny, nz)

    def packed_rank_bytes(self, bits):
        """Bytes one rank contributes to a packed all-gather (its planes padded to the largest plane count)."""
        return nat.packed_bytes(self._planes_max() * self.shape[1] * self.shape[2], bits)

    def _all_gather_packed(self, bits, widen, recv, out, unpack=True, overlap=False):
        """Labels at 2 bits each (or 1: the occupancy ``label == 1`` the consumer binarises to, proc3d.py:515)
        over the wire -- 1/16 (1/32) of the int32 planes: 32 MiB per rank at 1024^3 / 8 -- and ONE kernel
        (``sc_unpack_labels``) that unpacks and puts the planes in global order, as int8 or, ``widen``, int32.
        ``overlap`` (``unpack=False`` only): the engine's stream is NOT made to wait behind the collective -- it
        waits right before its next pack instead (``_settle``), so the carve of the next batch runs beside this
        batch's collective.  The caller hands alternating ``recv`` buffers if it still reads the previous grid."""
        import torch
        if self.dtype != np.int32:
            raise ValueError("packed labels are carve labels")
        W = self.world_size
        local, tstream = self._wire_bytes(bits=bits)
        rank_bytes = int(local.numel()) if self._alone else self.packed_rank_bytes(bits)
        recv = self._all_gather_into(self._pad(local, rank_bytes), recv)
        if not unpack:
            # the packed planes as they are (a PackedGrid): vol2pcd reads them directly.  A single rank's buffer is
            # the engine's own and is overwritten by its next pack: copied, it is 1/16 of the grid
            if self._alone and recv.is_cuda:
                recv = recv.clone()
            self._hand_back(tstream, overlap)
            return PackedGrid(recv, rank_bytes, W, self.partition, self.shape, bits, self.device)
        n_out = int(np.prod(self.shape))
        out_dtype = torch.int32 if widen else torch.int8
        if out is None or out.dtype != out_dtype or out.numel() < n_out:
            out = torch.empty(n_out, dtype=out_dtype, device=local.device)
        if recv.is_cuda:
            nat.unpack_labels(self.device, torch.cuda.current_stream(recv.device).cuda_stream, recv.data_ptr(), rank_bytes, W,
                              self.partition, self.shape, bits, out.data_ptr(), 4 if widen else 1)
            self._hand_back(tstream)
        else:
            if self._unpack_fn is None:
                raise RuntimeError("host tensors: no HIP unpack (the product path keeps the labels on the device)")
            out[:n_out] = torch.from_numpy(self._unpack_fn(recv.numpy(), rank_bytes, W, self.partition, self.shape, bits,
                                                            np.int32 if widen else np.int8).reshape(-1))
        return out[:n_out].view(self.shape)

    def sparse_rank_bytes(self, cap=None):
        """Bytes every rank contributes to a sparse all-gather with ``cap`` payload slots (the rank with the most planes)."""
        return nat.sparse_rank_bytes(self._bricks_max(), self._sparse_cap if cap is None else cap)

    def _all_gather_sparse(self, widen, recv, out, unpack=True, overlap=False, check=True):
        """Labels in the brick-sparse form over the wire (``include/spacecarve.h``): codes for all bricks, 2-bit labels
        of the mixed ones only, packed from the batch's own verdict bytes and live list.  Through the library's RCCL
        communicator when ``init_comm`` was called (no torch: ``recv`` is then a :class:`DevMem`, kept and reused),
        else through ``torch.distributed`` (gloo rehearsals, CPU tests).  ``check``: wait for the headers and gather
        again with more slots if a rank ran out (every rank takes the same decision from the same headers);
        ``check=False`` (pipelines): the :class:`SparseGrid` comes back unverified -- ``verify()`` it later."""
        if self.dtype != np.int32:
            raise ValueError("packed labels are carve labels")
        W = self.world_size
        while True:
            cap = self._sparse_cap
            stride = self.sparse_rank_bytes(cap)
            if self.comm is not None:
                if recv is None or not isinstance(recv, DevMem) or recv.nbytes < stride * W:
                    turn = self._sparse_turn
                    self._sparse_turn ^= 1
                    buf = self._sparse_recv[turn]
                    if buf is None or buf.nbytes < stride * W:
                        if buf is not None:
                            self.comm.synchronize()
                            self._engine.synchronize()
                            buf.free()
                        buf = self._sparse_recv[turn] = DevMem(self._engine, stride * W)
                    rbuf = buf
                else:
                    rbuf = recv
                ev, hh = self._engine.all_gather_sparse(self.comm, cap, rbuf.ptr, stride, overlap=overlap)
                if self._streams is None:
                    self._streams = (self.comm.stream(), self._engine.stream())
                grid = SparseGrid(rbuf, stride, W, self.shape, self.device, cap,
                                  stream=self._streams[0 if overlap else 1], engine=self._engine, done_event=ev, headers_host=hh)
            else:
                grid = self._all_gather_sparse_torch(cap, stride, recv, overlap)
            if not check:
                return grid if not unpack else grid.unpack(widen=widen, out=out)
            try:
                grid.verify()
            except SparseOverflow as ex:
                # (the engine's labels are as they were: gather again, every rank with the same larger capacity)
                self._sparse_cap = min(self._bricks_max(), (ex.needed + ex.needed // 8 + 15) & ~15)
                recv = None
                continue
            # far fewer mixed bricks than slots: the next gathers travel lighter (every rank reads the same headers and
            # changes its capacity alike); a later batch that needs more is gathered again, as above
            worst = int(max(int(n) for n in grid.nmixed))
            if 2 * worst < cap and cap > 1024:
                self._sparse_cap = max(1024, (worst + worst // 2 + 15) & ~15)
            return grid.unpack(widen=widen, out=out) if unpack else grid

    def _all_gather_sparse_torch(self, cap, stride, recv, overlap):
        local, tstream = self._wire_bytes(cap=cap)
        recv = self._all_gather_into(self._pad(local, stride), recv)
        if self._alone and recv.is_cuda:
            recv = recv.clone()  # (the engine's own buffer, overwritten by its next pack)
        # two send buffers alternate inside the engine: the next pack does not touch the one this collective reads,
        # the one after it does -- the engine waits then (lazily), or now
        self._hand_back(tstream, overlap)
        return SparseGrid(recv, stride, self.world_size, self.shape, self.device, cap, on_gpu=bool(recv.is_cuda),
                          engine=self._engine)

    def all_gather(self, compress=False, widen=True, recv=None, out=None, unpack=True, overlap=False, check=True):
        """Full grid on every rank (torch tensor on the slab's device), by all-gather.

        compress=True sends carve labels as int8 (labels are in {-1, 0, 1} when default_value
        is): 4x less xGMI traffic; ``widen`` turns the assembled grid back into int32 (the
        reference's dtype, cl.py:145-147) -- a device consumer that takes 1-byte volumes
        (``vol2pcd``) passes ``widen=False`` and spares the 4 bytes per voxel.
        compress="2bit" sends them at 2 bits each, "1bit" the occupancy ``label == 1`` alone (what
        ``vol2pcd`` binarises to): 16x / 32x less traffic, packed by the engine and unpacked into global
        order by one kernel (``_all_gather_packed``).
        compress="sparse" (round 6): one code per 16 x 64-voxel brick + the 2-bit labels of the mixed bricks only,
        packed from the batch's verdict bytes and live list (``_all_gather_sparse``): 2 MB per rank on a plant where
        "2bit" is 32 MiB; ``unpack=False`` returns a :class:`SparseGrid`.
        recv / out: reusable buffers (``W * P * ny * nz`` elements of the wire dtype; packed: recv
        ``W * packed_rank_bytes(bits)`` bytes, out ``nx * ny * nz`` int8 / int32).
        unpack=False (packed forms only): no grid is written at all -- the result is a ``PackedGrid`` (the ranks'
        packed planes on this device), which ``proc3d.vol2pcd`` consumes as it is and ``.unpack()`` turns into the
        grid on demand.
        overlap=True (with unpack=False): a pipeline of batches -- the collective of this batch runs beside the
        carve of the next one; the engine waits for it only before it packs again.
        """
        if overlap and (unpack or compress not in ("2bit", "1bit", "sparse")):
            raise ValueError("overlap=True is for the packed forms left packed (compress='2bit' / '1bit' / 'sparse', unpack=False)")
        if compress == "sparse":
            if unpack and not self._on_gpu:
                import torch
                grid = self._all_gather_sparse(widen, recv, None, unpack=False, overlap=False, check=True)
                return torch.from_numpy(grid.to_host().astype(np.int32 if widen else np.int8))
            return self._all_gather_sparse(widen, recv, out, unpack, overlap, check and not overlap)
        if compress in ("2bit", "1bit"):
            if not unpack and not self._on_gpu:
                # (a PackedGrid is a device object -- unpack() and vol2pcd read it with HIP kernels)
                raise ValueError("unpack=False needs the HIP engine: a PackedGrid lives on the device")
            return self._all_gather_packed(2 if compress == "2bit" else 1, widen, recv, out, unpack, overlap)
        if not unpack:
            raise ValueError("unpack=False is for the packed forms (compress='2bit' / '1bit')")
        return self._all_gather_dense(compress, widen, recv, out)

    def _all_gather_dense(self, compress, widen, recv, out):
        """The planes in the engine's dtype over the wire, or carve labels as int8 (``compress``)."""
        import torch
        self._settle()
        local = self._slab_tensor()
        if compress:
            if self.dtype != np.int32:
                raise ValueError("compression is for carve labels only")
            if not -128 <= int(self.default_value) <= 127:
                raise ValueError("default_value does not fit int8")
            local = local.to(torch.int8)
        if self._alone:
            full = local.reshape(self.shape)
        else:
            send = self._pad(local, self._planes_max() * self.shape[1] * self.shape[2])
            full = self._land(self._all_gather_into(send, recv), out)
        return full.to(torch.int32) if compress and widen else full

    def all_reduce(self):
        """Full grid on every rank by summing zero-padded full-size buffers (the north
        star's wording).  Exact: every voxel is non-zero on exactly one rank."""
        import torch
        import torch.distributed as dist
        self._settle()
        local = self._slab_tensor()
        full = torch.zeros((self.shape[0], self.shape[1], self.shape[2]), dtype=local.dtype,
                           device=local.device)
        pl = self.planes
        full[pl.start:pl.stop:pl.step] = local.reshape(len(pl), *self.shape[1:])
        if not self._alone:
            if dist.get_backend() == "gloo" and full.is_cuda:
                h = full.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM)
                full.copy_(h)
            else:
                dist.all_reduce(full, op=dist.ReduceOp.SUM)
        return full

    def gather_to_host(self, dst=0, compress=None, out=None):
        """Full grid as a NumPy array of the reference's dtype on rank ``dst`` (None elsewhere) --
        what ``get_values`` (cl.py:229-232) hands a ``Voxels`` run.

        Carve labels of a default value of -1 / 0 / 1 take the sparse wire of ``all_gather`` by default when there are
        collectives to run: every rank ends with every rank's (small) buffer, ``dst`` copies it over PCIe once and the
        host pool widens it and puts it in global order.  compress="2bit": the 2-bit wire (``_gather_to_host_2bit``).
        Otherwise the planes travel as int8 unless ``compress=False`` (``_gather_to_host_dense``).
        ``out``: an int32 array of the grid's size to widen into on ``dst`` -- one whose pages have been touched
        takes 512^3 labels in ~4 ms, a fresh ``np.empty`` ~30 (first-touch page faults, not the transfer)."""
        if compress is None and not self._alone and self._three_state("get_values_sparse"):
            compress = "sparse"  # (round 6: the default wire of a sharded run's labels)
        if compress == "sparse":
            if not self._three_state("get_values_sparse"):
                raise ValueError("the sparse wire carries carve labels of a default_value of -1, 0 or 1")
            self._settle()
            grid = self._all_gather_sparse(True, None, None, unpack=False, overlap=False, check=True)
            return grid.to_host(out=out) if self.rank == dst else None
        self._settle()
        two_bit = compress in (None, "2bit") and self._three_state("get_values_packed")
        if compress == "2bit" and not two_bit:
            raise ValueError("the 2-bit wire carries carve labels of a default_value of -1, 0 or 1")
        if self._alone:
            if two_bit and self._on_gpu and int(np.prod(self.shape)) >= (1 << 24):
                if out is None or out.dtype != np.int32 or out.size != int(np.prod(self.shape)) or not out.flags["C_CONTIGUOUS"]:
                    out = np.empty(self.shape, dtype=np.int32)
                self._engine.get_values_wire2(out.reshape(-1))
                return out.reshape(self.shape)
            return np.ascontiguousarray(self.get_local()).reshape(self.shape)
        if two_bit:
            return self._gather_to_host_2bit(dst, out)
        return self._gather_to_host_dense(dst, compress)

    def _gather_to_host_dense(self, dst, compress):
        """The planes to ``dst``'s GPU (RCCL: tensors over xGMI; gloo: through the hosts), as int8 when ``compress`` (by
        default for carve labels that fit), put in global order there by the strided copy of ``all_gather``, and one
        PCIe copy."""
        import torch
        import torch.distributed as dist
        if compress is None:
            compress = self.dtype == np.int32 and -128 <= int(self.default_value) <= 127
        local = self._slab_tensor(on_device=dist.get_backend() != "gloo")
        if compress:
            local = local.to(torch.int8)
        recv = self._gather_to(self._pad(local, self._planes_max() * self.shape[1] * self.shape[2]), dst)
        if recv is None:
            return None
        full = self._land(recv).cpu().numpy()
        return full.astype(self.dtype) if full.dtype != self.dtype else full

    def _gather_to_host_2bit(self, dst, out=None):
        """Three-state labels to ``dst``'s host memory over the 2-bit wire: every rank's planes packed on its device
        (``sc_values_packed``), gathered to ``dst``'s GPU (RCCL; gloo: through the hosts), ONE PCIe copy of 1/16 of
        the grid's bytes, and the host pool widens and interleaves the planes into the int32 grid of cl.py:229-232
        (``sc_widen_labels2_ranks``)."""
        import torch.distributed as dist
        rank_bytes = self.packed_rank_bytes(2)
        local, tstream = self._wire_bytes(bits=2, on_device=dist.get_backend() != "gloo")
        recv = self._gather_to(self._pad(local, rank_bytes), dst)
        self._hand_back(tstream)  # the engine's next pack waits for the collective's read
        if recv is None:
            return None
        if out is not None and (out.dtype != np.int32 or out.size != int(np.prod(self.shape)) or not out.flags["C_CONTIGUOUS"]):
            out = None
        return nat.widen_labels2_ranks(recv.cpu().numpy(), rank_bytes, self.world_size, self.partition, self.shape, out=out)

    def close(self):
        if self._engine is not None:
            self._settle()
            if self.comm is not None and getattr(self.comm, "_h", 0):  # (a twin outliving its parent: the communicator is gone)
                self.comm.synchronize()
            self._engine.synchronize()
            for buf in self._sparse_recv:
                if buf is not None:
                    buf.free()
            self._sparse_recv = [None, None]
            if self.comm is not None:
                if not self._comm_shared:
                    self.comm.close()
                self.comm = None
            self._engine.close()
            self._engine = None
