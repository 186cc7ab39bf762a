"""multigrid_amd -- MI355X-native matrix-free geometric multigrid for the Laplace operator.

Host-side mirror (Python, for tests and bench.py) of the reference's operator / solver interface
for the poisson_cube path on top of the C ABI in include/mgx.h:

    LaplaceOperator  <-> multigrid::LaplaceOperator   common/laplace_operator.h:56-164
    MultigridSolver  <-> multigrid::MultigridSolver   common/multigrid_solver.h:96-782
    DGLaplaceOperator <-> multigrid::LaplaceOperatorCompactCombine + JacobiTransformed
                                                       common/laplace_operator_dg.h:350-2256
    Cube             <-> the deal.II mesh / DoFHandler / MatrixFree data of poisson_cube/program.cc

All numerical work runs in hand-written HIP kernels inside libmgx.so; nothing here computes.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import F32, F64, INVALID_INDEX, MgxError, check

__all__ = ["Context", "DeviceVector", "Cube", "LaplaceOperator", "Chebyshev", "Transfer", "MultigridSolver",
           "Communicator", "process_grid", "F32", "F64", "INVALID_INDEX", "MgxError", "DGLaplaceOperator", "dg_cheby_mesh",
           "dg_box_neighbours", "dg_box_partition", "dg_partition", "DG_HERMITE", "DG_GAUSS_LOBATTO", "DG_GAUSS", "DGMultigridSolver",
           "DGConjugateGradient", "DG_PCG_MERGED", "DG_PCG_SEPARATE", "spawn_ranks"]


def spawn_ranks(script, argv, n, one_gpu=False, grace=30.0):
    """Start n ranks of `script` (fresh child processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*; the
    calling process never touches the GPU) and wait for them.  Once a rank has failed the others get `grace`
    seconds -- they may sit in a collective the failed rank never joins -- and are then ended (exactly the
    processes started here).  Returns the exit codes."""
    import os
    import socket
    import subprocess
    import sys
    import time
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0" if one_gpu else str(r), WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(script)] + list(argv), env=env))
    failed_at = None
    while any(p.poll() is None for p in procs):
        time.sleep(0.5)
        if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
            failed_at = time.time()
        if failed_at is not None and time.time() - failed_at > grace:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10.0)
                except subprocess.TimeoutExpired:
                    p.kill()
    return [p.wait() for p in procs]


def process_grid(size):
    """1 / 2x1x1 / 2x2x1 / 2x2x2; generally the most cubic power-of-two grid"""
    procs = [1, 1, 1]
    d = 0
    while size > 1:
        if size % 2:
            raise ValueError("number of ranks must be a power of two")
        procs[d] *= 2
        size //= 2
        d = (d + 1) % 3
    return tuple(procs)


class Communicator:
    """Transport of the interface exchange and of the scalar reductions (mgx_comm_desc) on top of
    torch.distributed: backend "nccl" (= RCCL over xGMI, one process per GPU) or "gloo" (CPU
    processes; used by the tests, also with several processes sharing one GPU).

    exchange(plan): the library has packed its send buffers (device memory); they are delivered
    with one batch of point-to-point operations (at most 7 neighbours in a 2x2x2 process grid,
    each a direct xGMI peer)."""

    def __init__(self, ctx, dist, device_transport=None, native=None):
        """native: also create an RCCL communicator inside the library (mgx_context_set_rccl; the
        unique id travels over `dist`).  It stays switched off until verify_and_enable_native() has
        compared one exchange and one reduction with the callback transport on every rank.
        Default: on for the nccl backend unless MGX_NATIVE_RCCL=0."""
        self.ctx, self.dist = ctx, dist
        self.rank, self.size = dist.get_rank(), dist.get_world_size()
        self.device_transport = (dist.get_backend() == "nccl") if device_transport is None else device_transport
        self.native_ready = False
        self.native_enabled = False
        self._native_wanted = (self.device_transport and os.environ.get("MGX_NATIVE_RCCL", "1") != "0") \
            if native is None else native
        self._tensors = {}   # device pointer -> torch CUDA tensor backing an exchange buffer
        self._p2p = {}       # plan_id -> cached P2POp list
        self._ex = _lib.EXCHANGE_FN(self._exchange)
        self._ar = _lib.ALLREDUCE_FN(self._allreduce)
        self._al = _lib.ALLOC_FN(self._alloc) if self.device_transport else _lib.ALLOC_FN()
        self.desc = _lib.CommDesc(self.rank, self.size, None, self._ex, self._ar, self._al)
        check(ctx.lib.mgx_context_set_comm(ctx.h, C.byref(self.desc)))
        ctx._comm = self  # keep the callbacks alive
        if self._native_wanted:
            self._setup_native()

    def _setup_native(self):
        """collective: every rank must arrive here; a failure on any rank disables it on all"""
        import sys
        import torch
        lib, h = self.ctx.lib, self.ctx.h
        buf = (C.c_uint8 * 128)()
        ok = 1
        if self.rank == 0 and lib.mgx_rccl_unique_id(buf) != 0:
            ok = 0
        dev = "cuda" if self.dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor(list(buf) + [ok], dtype=torch.uint8, device=dev)
        self.dist.broadcast(t, 0)
        vals = t.cpu().tolist()
        if vals[128] == 0:
            print("mgx Communicator: librccl unavailable, callback transport stays", file=sys.stderr, flush=True)
            return
        idb = (C.c_uint8 * 128)(*vals[:128])
        rc = lib.mgx_context_set_rccl(h, self.rank, self.size, idb)
        if rc == 0:
            rc = lib.mgx_context_use_rccl(h, 0)  # off until verified
        flag = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device=dev)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN)
        self.native_ready = int(flag.item()) == 1
        if not self.native_ready:
            print("mgx Communicator: RCCL communicator not created on every rank (%s), callback transport stays"
                  % lib.mgx_last_error().decode(), file=sys.stderr, flush=True)

    def verify_and_enable_native(self, op, n_dofs, number=F64):
        """One interface exchange and one dot product of a test vector through both transports;
        the native one is switched on only if every rank finds them bitwise identical."""
        if not self.native_ready:
            return False
        import sys
        import torch
        lib, h = self.ctx.lib, self.ctx.h
        rng = np.random.default_rng(1234 + self.rank)
        v = rng.uniform(-1, 1, n_dofs).astype(_DT[number])
        a, b = self.ctx.vector(n_dofs, number, v), self.ctx.vector(n_dofs, number, v)
        good = True
        try:
            check(lib.mgx_exchange_add(op.h, a.ptr))        # callbacks
            da = self.ctx.dot(a, a)
            check(lib.mgx_context_use_rccl(h, 1))
            check(lib.mgx_exchange_add(op.h, b.ptr))        # native
            db = self.ctx.dot(b, b)
            good = np.array_equal(a.download(), b.download()) and abs(da - db) <= 1e-12 * abs(da)
        except Exception as e:  # noqa: BLE001
            print("mgx Communicator: native RCCL check failed:", repr(e), file=sys.stderr, flush=True)
            good = False
        lib.mgx_context_use_rccl(h, 0)
        dev = "cuda" if self.dist.get_backend() == "nccl" else "cpu"
        flag = torch.tensor([1 if good else 0], dtype=torch.int32, device=dev)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN)
        self.native_enabled = int(flag.item()) == 1
        if self.native_enabled:
            check(lib.mgx_context_use_rccl(h, 1))
        elif self.rank == 0:
            print("mgx Communicator: native RCCL transport disagrees with the callback transport, not used",
                  file=sys.stderr, flush=True)
        return self.native_enabled

    def _alloc(self, user, nbytes):
        """exchange buffers as torch CUDA tensors: RCCL sends from / receives into them directly"""
        try:
            import torch
            t = torch.zeros(max(int(nbytes), 8), dtype=torch.uint8, device="cuda")
            self._tensors[t.data_ptr()] = t
            return t.data_ptr()
        except Exception as e:
            import sys
            print("mgx Communicator.alloc failed:", repr(e), file=sys.stderr, flush=True)
            return None

    def _device_tensor(self, ptr, nbytes):
        """torch view of `nbytes` of device memory at `ptr`: the tensor the alloc callback handed out, or -- for
        buffers the library owns (the DG ghost exchange sends from hipMalloc'd pack buffers and receives straight
        into the ghost part of the vector it was given, mgx_dg_api.cpp) -- a zero-copy wrapper of the raw pointer"""
        import torch
        t = self._tensors.get(ptr)
        if t is not None:
            return t[:nbytes]

        class _Raw:  # __cuda_array_interface__ v2: torch wraps the memory, it does not own it
            pass
        raw = _Raw()
        raw.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(raw, device="cuda")

    def _exchange(self, user, plan_id, number, n_neighbors, ranks, counts, send, recv):
        try:
            import torch
            dt = torch.float64 if number == F64 else torch.float32
            es = 8 if number == F64 else 4
            if self.device_transport:
                # the operations are cached per plan AND buffer set: one plan serves many vectors when the
                # library receives in place (DG ghosts), each with its own receive pointers
                key = (plan_id, tuple(send[k] for k in range(n_neighbors)), tuple(recv[k] for k in range(n_neighbors)))
                ops = self._p2p.get(key)
                if ops is None:
                    ops = []
                    for k in range(n_neighbors):
                        cnt = counts[k]
                        st = self._device_tensor(send[k], cnt * es).view(dt)
                        rt = self._device_tensor(recv[k], cnt * es).view(dt)
                        ops.append(self.dist.P2POp(self.dist.isend, st, ranks[k]))
                        ops.append(self.dist.P2POp(self.dist.irecv, rt, ranks[k]))
                    if len(self._p2p) > 256:
                        self._p2p.clear()
                    self._p2p[key] = ops
                if ops:
                    for req in self.dist.batch_isend_irecv(ops):
                        req.wait()
                    torch.cuda.synchronize()
                return 0
            lib, h = self.ctx.lib, self.ctx.h
            ops, bufs = [], []
            for k in range(n_neighbors):
                rk, cnt = ranks[k], counts[k]
                st = torch.empty(cnt, dtype=dt)
                rt = torch.empty(cnt, dtype=dt)
                check(lib.mgx_download(h, C.c_void_p(st.data_ptr()), C.c_void_p(send[k]), cnt * es))
                bufs.append((rt, recv[k], cnt))
                ops.append(self.dist.P2POp(self.dist.isend, st, rk))
                ops.append(self.dist.P2POp(self.dist.irecv, rt, rk))
            if ops:
                for req in self.dist.batch_isend_irecv(ops):
                    req.wait()
            for (rt, rbuf, cnt) in bufs:
                check(lib.mgx_upload(h, C.c_void_p(rbuf), C.c_void_p(rt.data_ptr()), cnt * es))
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            import sys
            print("mgx Communicator.exchange failed:", repr(e), file=sys.stderr, flush=True)
            return 1

    def _allreduce(self, user, values, count):
        try:
            import torch
            a = np.ctypeslib.as_array(values, shape=(count,))
            t = torch.from_numpy(a.copy())
            if self.device_transport:
                t = t.cuda()
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
            a[:] = t.cpu().numpy()
            return 0
        except Exception as e:
            import sys
            print("mgx Communicator.allreduce failed:", repr(e), file=sys.stderr, flush=True)
            return 1

    def allreduce(self, values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        if self._allreduce(None, a.ctypes.data_as(_lib.f64p), a.size) != 0:
            raise RuntimeError("allreduce failed")
        return a

_DT = {F32: np.float32, F64: np.float64}


class Context:
    """HIP device + stream (mgx_context_t)."""

    def __init__(self, device=0, options=None):
        """options: {name: value} for mgx_context_set_option (code-path selectors and thresholds; include/mgx.h)"""
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.mgx_context_create(C.byref(h), device))
        self.h = h
        self.device = device
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name, value):
        check(self.lib.mgx_context_set_option(self.h, name.encode(), float(value)))

    def sync(self):
        check(self.lib.mgx_sync(self.h))

    @property
    def stream(self):
        return self.lib.mgx_context_stream(self.h)

    def profile_enable(self, on=True):
        check(self.lib.mgx_profile_enable(self.h, int(on)))

    def range(self, name):
        """context manager: a profiler range (roctx) with one of the reference's LIKWID region names --
        "fmg_solver", "cg_solver", "matvec", "matvec_sp" (poisson_cube/program.cc:282-375); no-op unless the
        context option "roctx" is set"""
        ctx = self

        class _Range:
            def __enter__(self):
                check(ctx.lib.mgx_range_push(ctx.h, name.encode()))

            def __exit__(self, *exc):
                check(ctx.lib.mgx_range_pop(ctx.h))
                return False
        return _Range()

    def profile_read(self, form):
        """(kernel launches, summed duration in ms) of one form of the profiled cell loop:
        0 plain vmult, 1 residual, 2 fused Chebyshev iteration, 3 first step, 4 zero x_old; resets"""
        n, ms = C.c_uint64(), C.c_double()
        check(self.lib.mgx_profile_read(self.h, form, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.mgx_context_destroy(self.h)
            self.h = None

    def vector(self, n, number=F64, data=None):
        return DeviceVector(self, n, number, data)

    def dot(self, x, y):
        r = C.c_double()
        check(self.lib.mgx_dot(self.h, x.number, x.ptr, y.ptr, x.n, C.byref(r)))
        return r.value

    def l2_norm(self, x):
        r = C.c_double()
        check(self.lib.mgx_l2_norm(self.h, x.number, x.ptr, x.n, C.byref(r)))
        return r.value


class DeviceVector:
    """Device storage of one level vector (LinearAlgebra::distributed::Vector<number>)."""

    def __init__(self, ctx, n, number=F64, data=None, ptr=None):
        self.ctx, self.n, self.number = ctx, int(n), number
        self.owned = ptr is None
        if ptr is None:
            p = C.c_void_p()
            check(ctx.lib.mgx_malloc(ctx.h, C.byref(p), self.nbytes))
            self.ptr = p
            if data is None:
                self.zero()
        else:
            self.ptr = C.c_void_p(ptr) if not isinstance(ptr, C.c_void_p) else ptr
        if data is not None:
            self.upload(data)

    @property
    def nbytes(self):
        return self.n * (8 if self.number == F64 else 4)

    def zero(self):
        check(self.ctx.lib.mgx_memset_zero(self.ctx.h, self.ptr, self.nbytes))

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=_DT[self.number])
        assert a.size == self.n
        check(self.ctx.lib.mgx_upload(self.ctx.h, self.ptr, a.ctypes.data_as(C.c_void_p), self.nbytes))

    def download(self):
        a = np.empty(self.n, dtype=_DT[self.number])
        check(self.ctx.lib.mgx_download(self.ctx.h, a.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes))
        return a

    def free(self):
        if self.owned and self.ptr:
            self.ctx.lib.mgx_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Mesh:
    """What Cube and Square share: the handle `h` and the accessors whose C names differ in the prefix only
    (mgx_cube_* / mgx_square_*)."""

    _prefix, _dim = None, 0

    def _c(self, name):
        return getattr(self.lib, self._prefix + name)

    def close(self):
        if getattr(self, "h", None):
            self._c("destroy")(self.h)
            self.h = None

    def n_cells(self, l):
        return self._c("n_cells")(self.h, l)

    def n_dofs(self, l):
        return self._c("n_dofs")(self.h, l)

    def n_constrained(self, l):
        return self._c("n_constrained")(self.h, l)

    def cell_size(self, l):
        return self._c("cell_size")(self.h, l)

    def _arr(self, name, shape, *args):
        f = self._c(name)
        p = f(self.h, *args)
        n = int(np.prod(shape))
        if n == 0:
            return np.zeros(shape, dtype=np.dtype(f.restype._type_))
        return np.ctypeslib.as_array(p, shape=(n,)).reshape(shape).copy()

    def _filled(self, name, shape, l):
        out = np.empty(shape)
        check(self._c(name)(self.h, l, out.ctypes.data_as(_lib.f64p)))
        return out

    def constrained(self, l):
        return self._arr("constrained", (self.n_constrained(l),), l)

    def cell_coords(self, l):
        return self._arr("cell_coords", (self.n_cells(l), self._dim), l)

    def dof_grid(self, l):
        return self._arr("dof_grid", (self.n_dofs(l),), l)

    def shape_values(self):
        n = self.degree + 1
        return self._arr("shape_values", (n, n))

    def colloc_grad(self):
        n = self.degree + 1
        return self._arr("colloc_grad", (n, n))

    def qweights(self):
        return self._arr("qweights", (self.degree + 1,))

    def qpoints(self):
        return self._arr("qpoints", (self.degree + 1,))

    def gll(self):
        return self._arr("gll", (self.degree + 1,))

    def prolong_1d(self):
        n = self.degree + 1
        return self._arr("prolong_1d", (2 * n - 1, n))

    def operator_desc(self, l, number=F64):
        d = _lib.OperatorDesc()
        check(self._c("operator_desc")(self.h, l, number, C.byref(d)))
        return d

    def seeded_vector(self, l, seed=42):
        out = np.empty(self.n_dofs(l))
        check(self._c("seeded_vector")(self.h, l, seed, out.ctypes.data_as(_lib.f64p)))
        return out


class Cube(_Mesh):
    """Host-side discretisation of poisson_cube (include/mgx_cube.h): what deal.II supplies."""

    _prefix, _dim = "mgx_cube_", 3

    NUMBERING = {"brick": 0, "cell": 1}
    GEOMETRY = {"cartesian": 0, "sheared": 1, "shell_sector": 2}
    PROBLEM = {"cube": 0, "shell": 1}

    def __init__(self, degree, n_subdiv=1, n_refine=3, box=None, procs=(1, 1, 1), rank=0, numbering="brick",
                 origin=-1.0, h0=1.9, geometry="cartesian", problem="cube", shell=None):
        """box=None: the square mesh [-0.9,1]^3 with n_subdiv coarse cells per direction.
        box=(sx,sy,sz): a box of sx x sy x sz cubic coarse cells of size h0 from (origin,)*3,
        optionally distributed over the process grid `procs`; this rank owns box[d]/procs[d] coarse
        cells per direction on every level.  The defaults (size 1.9 from -1) are the reference's
        doubling-mesh family (program.cc:509-529: one coarse cube per rank = weak scaling);
        box=(n,n,n), origin=-0.9, h0=1.9/n is the square mesh of poisson_cube with n_subdiv = n,
        block-split over the ranks (strong scaling of one problem).
        geometry / problem (box form only): mapped meshes and the variable coefficient of
        poisson_shell, MGX_CUBE_GEOMETRY_* / MGX_CUBE_PROBLEM_* in mgx_cube.h.
        numbering: "brick" (default, grouped for the device cell loop) or "cell" (the
        plain first-touch order), MGX_CUBE_NUMBERING_* in mgx_cube.h.
        shell=6 | 12: the mesh of poisson_shell instead, GridGenerator::hyper_shell(0, 0.5, 1.0, shell) refined
        n_refine times (mgx_cube_create_shell); problem "shell" (default there) or "cube"; procs=(n,1,1), rank=r:
        the coarse cells distributed over n <= `shell` ranks (contiguous shares, one cell more on some ranks where n
        does not divide them: 12 cells on 8 ranks)."""
        self.lib = _lib.load()
        h = C.c_void_p()
        num = self.NUMBERING[numbering]
        self.shell = shell
        if shell is not None:
            self.box_desc = None
            self.shell_desc = dict(shell=int(shell), problem=problem)
            n_ranks = int(procs[0]) * int(procs[1]) * int(procs[2])
            check(self.lib.mgx_cube_create_shell_ranks(degree, int(shell), n_refine, self.PROBLEM[problem], n_ranks, rank,
                                                       C.byref(h)))
            self.h = h
            self.rank, self.size = rank, n_ranks
            self.degree = degree
            self.n_levels = self.lib.mgx_cube_n_levels(h)
            self.max_level = self.n_levels - 1
            # level i of this object is level i + level_offset of the whole mesh (1 where the cells of level 1 are
            # dealt out to the ranks: 8 ranks hold 6 of 48 / 12 of 96 cells each)
            self.level_offset = self.lib.mgx_cube_level_offset(h)
            return
        self.level_offset = 0
        self.box_desc = None if box is None else dict(box=tuple(box), origin=origin, h0=h0, geometry=geometry,
                                                        problem=problem, numbering=numbering)
        if box is None:
            check(self.lib.mgx_cube_create_numbered(degree, n_subdiv, n_refine, num, C.byref(h)))
        else:
            d = _lib.CubeBoxDesc(degree, n_refine, (C.c_int * 3)(*box), origin, h0, (C.c_int * 3)(*procs), rank, num,
                                 self.GEOMETRY[geometry], self.PROBLEM[problem])
            check(self.lib.mgx_cube_create_box(C.byref(d), C.byref(h)))
        self.h = h
        self.rank, self.size = self.lib.mgx_cube_rank(h), self.lib.mgx_cube_size(h)
        self.degree = degree
        self.n_levels = self.lib.mgx_cube_n_levels(h)
        self.max_level = self.n_levels - 1

    def cells_per_dim(self, l):
        return self.lib.mgx_cube_cells_per_dim(self.h, l)

    def idx27(self, l):
        return self._arr("idx27", (self.n_cells(l), 27), l)

    def idx27_plain(self, l):
        return self._arr("idx27_plain", (self.n_cells(l), 27), l)

    def coef_q(self, l):
        """[n_cells, 6, (p+1)^3] merged coefficient of a mapped level (None on the Cartesian cube)"""
        ptr = self.lib.mgx_cube_coef_q(self.h, l)
        if not ptr:
            return None
        return np.ctypeslib.as_array(ptr, shape=(self.n_cells(l), 6, (self.degree + 1) ** 3)).copy()

    def jxw_q(self, l):
        """[n_cells, (p+1)^3] JxW at the quadrature points of a mapped level (None on the Cartesian cube)"""
        ptr = self.lib.mgx_cube_jxw_q(self.h, l)
        if not ptr:
            return None
        return np.ctypeslib.as_array(ptr, shape=(self.n_cells(l), (self.degree + 1) ** 3)).copy()

    def children(self, l):
        return self._arr("children", (self.n_cells(l - 1), 8), l)

    def cell_nodes(self, l):
        """physical Gauss-Lobatto points of every cell, [n_cells, 3, (p+1)^3] (x fastest)"""
        return self._filled("cell_nodes", (self.n_cells(l), 3, (self.degree + 1) ** 3), l)

    def entity_multiplicity(self, l):
        """multi-block meshes: cells around each of the 27 entities of every cell, [n_cells, 27]"""
        ptr = self.lib.mgx_cube_entity_multiplicity(self.h, l)
        if not ptr:
            return None
        return np.ctypeslib.as_array(ptr, shape=(self.n_cells(l) * 27,)).reshape(-1, 27).copy()

    def rhs(self, l):
        return self._arr("rhs", (self.n_dofs(l),), l)

    def rhs_quadrature(self, l):
        """f(x_q) JxW_q, [n_cells, (p+1)^3]: the integrand of the right-hand side (input of compute_residual)"""
        return self._filled("rhs_quadrature", (self.n_cells(l), (self.degree + 1) ** 3), l)

    def bc(self, l):
        n = self.lib.mgx_cube_bc_count(self.h, l)
        return self._arr("bc_index", (n,), l), self._arr("bc_value", (n,), l)

    def neighbors(self, l):
        """[(rank, index array)] of the interface exchange on level l (ascending rank)"""
        out = []
        for k in range(self.lib.mgx_cube_n_neighbors(self.h, l)):
            n = self.lib.mgx_cube_neighbor_count(self.h, l, k)
            out.append((self.lib.mgx_cube_neighbor_rank(self.h, l, k),
                        self._arr("neighbor_index", (n,), l, k)))
        return out

    def shared(self, l):
        return self._arr("shared", (self.lib.mgx_cube_n_shared(self.h, l),), l)

    def not_owned(self, l):
        return self._arr("not_owned", (self.lib.mgx_cube_n_not_owned(self.h, l),), l)

    def cells_per_dim3(self, l):
        a, b = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
        self.lib.mgx_cube_cells_per_dim3(self.h, l, C.byref(a), C.byref(b))
        return tuple(a), tuple(b)

    def l2_error_parts(self, l, solution):
        s = np.ascontiguousarray(solution, dtype=np.float64)
        e, v = C.c_double(), C.c_double()
        self.lib.mgx_cube_l2_error_parts(self.h, l, s.ctypes.data_as(_lib.f64p), C.byref(e), C.byref(v))
        return e.value, v.value

    def l2_error(self, l, solution):
        s = np.ascontiguousarray(solution, dtype=np.float64)
        assert s.size == self.n_dofs(l)
        return self.lib.mgx_cube_l2_error(self.h, l, s.ctypes.data_as(_lib.f64p))

    # ---- affine geometry of the Cartesian cube / box for the general branch (mgx_cube_solver_create_general) ----
    def affine_metric(self, l, jacobian=None):
        """(M = J^-1 J^-T as [xx,yy,zz,xy,xz,yz], det J) of the cells of level l, J = h_l A with the constant 3 x 3 matrix
        A = jacobian (None: identity) of an affine map of the whole box"""
        m, det = np.zeros(6), C.c_double()
        a = None if jacobian is None else np.ascontiguousarray(jacobian, dtype=np.float64).ravel()
        check(self.lib.mgx_cube_affine_metric(self.h, l, None if a is None else a.ctypes.data_as(_lib.f64p),
                                              m.ctypes.data_as(_lib.f64p), C.byref(det)))
        return m, det.value

    def unit_law_coefficient(self, l, jacobian=None):
        """[n_cells, 6, (p+1)^3] merged coefficient JxW_q M of the unit law (LAW_UNIT): what puts a level of the
        Cartesian mesh into the general branch of the operator"""
        m, det = self.affine_metric(l, jacobian)
        w = self.qweights()
        jxw = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel() * det
        return np.ascontiguousarray(np.broadcast_to(m[None, :, None] * jxw[None, None, :],
                                                    (self.n_cells(l), 6, jxw.size)))

    def dof_coordinates(self, l, jacobian=None):
        """[n_dofs, 3] physical coordinates of the Gauss-Lobatto node of every DoF of level l (Cartesian cube / box;
        jacobian: the affine map x = x0 + A X of the box about its lower corner x0).  Mapped cubes (sheared and
        shell_sector boxes, hyper_shell): the cell nodes, through the unconstrained index table."""
        assert self.size == 1
        if self.shell is not None or (self.box_desc is not None and self.box_desc["geometry"] != "cartesian"):
            assert jacobian is None
            dofs = _cell_dofs(self.idx27_plain(l), self.degree)
            X = np.empty((self.n_dofs(l), 3))
            X[dofs.ravel()] = self.cell_nodes(l).transpose(0, 2, 1).reshape(-1, 3)
            return X
        p, g = self.degree, self.dof_grid(l).astype(np.int64)
        n = np.array(self.cells_per_dim3(l)[1], dtype=np.int64)
        G = n * p + 1
        ijk = np.stack([g % G[0], (g // G[0]) % G[1], g // (G[0] * G[1])], axis=1)
        cell = np.minimum(ijk // p, n[None, :] - 1)
        X = (cell + self.gll()[ijk - cell * p]) * self.cell_size(l)
        if jacobian is not None:
            X = X @ np.asarray(jacobian, dtype=np.float64).T
        return (-0.9 if self.box_desc is None else self.box_desc["origin"]) + X


class SquareProblem:
    """A linear problem -div(a grad u) = f with Dirichlet values on a Square (mgx_square_problem): kind "cube" --
    u = sin(3 pi x) sin(3 pi y), a = 1, the box's own problem -- or "shell" -- u = sin(2 pi (x+y)), a = 1 + contrast
    prod_e cos^2(2 pi x_e + 0.1 e) (poisson_shell/program.cc with dim = 2; its contrast is 1e6)."""

    KINDS = {"cube": 0, "shell": 1}  # MGX_SQUARE_PROBLEM_*

    def __init__(self, kind="shell", contrast=1e6):
        self.kind, self.contrast = kind, float(contrast)
        # (an unknown kind goes to the provider as it is, if it is a number: the provider refuses it)
        self.c = _lib.SquareProblem(self.KINDS[kind] if kind in self.KINDS else int(kind), self.contrast)

    def __repr__(self):
        return "SquareProblem(%r, contrast=%g)" % (self.kind, self.contrast)


class Square(_Mesh):
    """Host-side discretisation of poisson_cube with dimension = 2 (include/mgx_square.h): what deal.II supplies for
    LaplaceOperator<2,p,number> and MultigridSolver<2,p,...>.  One rank.  Method names are Cube's where they apply."""

    _prefix, _dim = "mgx_square_", 2
    size, rank, shell, box_desc, level_offset = 1, 0, None, None, 0

    MAPPED = {"annulus_sector": 1, "ball": 2}  # MGX_SQUARE_GEOMETRY_*

    def __init__(self, degree, n_subdiv=1, n_refine=3, box=None, origin=-0.9, h0=None, jacobian=None, mapped=None):
        """box=None: the square [-0.9,1]^2 with n_subdiv coarse cells per direction.  box=(sx,sy): a box of sx x sy
        square coarse cells of size h0 from (origin, origin).  jacobian: constant 2 x 2 matrix of an affine map of the
        whole box (a sheared or anisotropic box: the operator's one tensor [xx,yy,xy], the full-tensor form).
        mapped="annulus_sector": curved cells on every level (mgx_square_create_mapped): the box as the quarter annulus
        0.5 <= r <= 1; the operator's coefficient is the per-point unit-law tensor, there is no Poisson problem.
        mapped="ball": the unit disc in five blocks (mgx_square_create_ball: degree and n_refine only), everything of a
        mapped square; it has no lattice of cells and no grid of DoFs: cells_per_dim2, cell_coords, dof_grid and
        weight_shift raise the provider's error."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if box is None:
            box, h0 = (n_subdiv, n_subdiv), 1.9 / n_subdiv
        self._jac = None if jacobian is None else np.ascontiguousarray(jacobian, dtype=np.float64).reshape(2, 2)
        d = _lib.SquareBoxDesc(degree, n_refine, (C.c_int * 2)(*box), origin, 1.9 if h0 is None else h0,
                               None if self._jac is None else self._jac.ctypes.data_as(_lib.f64p))
        self.mapped = mapped
        self.origin = origin
        if mapped == "ball":
            if box != (n_subdiv, n_subdiv) or n_subdiv != 1 or jacobian is not None:
                raise ValueError("Square(mapped=\"ball\"): degree and n_refine only (no box, n_subdiv, jacobian)")
            check(self.lib.mgx_square_create_ball(degree, n_refine, C.byref(h)))
        elif mapped is None:
            check(self.lib.mgx_square_create_box(C.byref(d), C.byref(h)))
        else:
            check(self.lib.mgx_square_create_mapped(C.byref(d), self.MAPPED[mapped], C.byref(h)))
        self.h = h
        self.degree = degree
        self.n_levels = self.lib.mgx_square_n_levels(h)
        self.max_level = self.n_levels - 1

    def _grid(self, name):
        """the disc has no grid: the provider's refusal (the C accessor itself returns NULL or zeros)"""
        if self.mapped == "ball":
            a = (C.c_uint32 * 2)()
            self.lib.mgx_square_cells_per_dim2(self.h, 0, C.byref(a))  # (leaves the reason in mgx_last_error)
            raise _lib.MgxError(-4, "%s: %s" % (name, self.lib.mgx_last_error().decode()))

    def cells_per_dim2(self, l):
        self._grid("cells_per_dim2")
        a = (C.c_uint32 * 2)()
        self.lib.mgx_square_cells_per_dim2(self.h, l, C.byref(a))
        return tuple(a)

    def cell_coords(self, l):
        self._grid("cell_coords")
        return super().cell_coords(l)

    def dof_grid(self, l):
        self._grid("dof_grid")
        return super().dof_grid(l)

    def idx9(self, l):
        return self._arr("idx9", (self.n_cells(l), 9), l)

    def idx9_plain(self, l):
        return self._arr("idx9_plain", (self.n_cells(l), 9), l)

    def children(self, l):
        return self._arr("children", (self.n_cells(l - 1), 4), l)

    def weight_shift(self, l):
        self._grid("weight_shift")
        return self._arr("weight_shift", (self.n_cells(l - 1), 9), l)

    def _poisson_problem(self):
        if self.mapped is not None:
            raise ValueError("a mapped Square has no Poisson problem (rhs, bc, l2_error)")

    def rhs(self, l):
        self._poisson_problem()
        return self._arr("rhs", (self.n_dofs(l),), l)

    def bc(self, l):
        self._poisson_problem()
        n = self.lib.mgx_square_bc_count(self.h, l)
        return self._arr("bc_index", (n,), l), self._arr("bc_value", (n,), l)

    def l2_error(self, l, solution):
        self._poisson_problem()
        s = np.ascontiguousarray(solution, dtype=np.float64)
        assert s.size == self.n_dofs(l)
        return self.lib.mgx_square_l2_error(self.h, l, s.ctypes.data_as(_lib.f64p))

    def coef_q(self, l):
        """[n_cells, 3, (p+1)^2] the per-(cell, q) tensor equivalent to the one tensor of operator_desc (weight folded in)"""
        return self._filled("coef_q", (self.n_cells(l), 3, (self.degree + 1) ** 2), l)

    # ---- geometry for the solution-dependent coefficients (mgx_square_solver_create_general) ----
    def affine_metric(self, l):
        """(M = J^-1 J^-T as [xx,yy,xy], det J) of the cells of level l of a box, J = h_l A with the box's jacobian A"""
        m, det = np.zeros(3), C.c_double()
        check(self.lib.mgx_square_affine_metric(self.h, l, m.ctypes.data_as(_lib.f64p), C.byref(det)))
        return m, det.value

    def unit_law_coefficient(self, l):
        """[n_cells, 3, (p+1)^2] merged coefficient of the unit law (LAW_UNIT): JxW_q M on a box, the per-point tensor of
        a mapped square"""
        return self.coef_q(l)

    def dof_coordinates(self, l):
        """[n_dofs, 2] physical coordinates of the Gauss-Lobatto node of every DoF of level l"""
        return self._filled("dof_coordinates", (self.n_dofs(l), 2), l)

    def cell_nodes(self, l):
        """[n_cells, (p+1)^2, 2] the nodes of every cell, x fastest"""
        return self._filled("cell_nodes", (self.n_cells(l), (self.degree + 1) ** 2, 2), l)

    def unit_q(self, l):
        """[n_cells, 3, (p+1)^2] JxW_q J^-1 J^-T of the isoparametric cells as [xx,yy,xy]"""
        return self._filled("unit_q", (self.n_cells(l), 3, (self.degree + 1) ** 2), l)

    def jxw_q(self, l):
        """[n_cells, (p+1)^2] JxW_q of the isoparametric cells"""
        return self._filled("jxw_q", (self.n_cells(l), (self.degree + 1) ** 2), l)

    # ---- a linear problem on any square, curved ones included (SquareProblem; mgx_square_problem_*) ----
    def _problem(self, name, shape, l, problem):
        out = np.empty(shape)
        check(self._c("problem_" + name)(self.h, l, C.byref(problem.c) if problem is not None else None,
                                         out.ctypes.data_as(_lib.f64p)))
        return out

    def problem_coef_q(self, l, problem):
        """[n_cells, 3, (p+1)^2] a(x_q) JxW_q J^-1 J^-T: the operator's tensor for the problem"""
        return self._problem("coef_q", (self.n_cells(l), 3, (self.degree + 1) ** 2), l, problem)

    def problem_rhs_quadrature(self, l, problem):
        """[n_cells, (p+1)^2] f(x_q) JxW_q (rhs_q of LaplaceOperator.compute_residual)"""
        return self._problem("rhs_quadrature", (self.n_cells(l), (self.degree + 1) ** 2), l, problem)

    def problem_solution_q(self, l, problem):
        """[n_cells, (p+1)^2] u(x_q) (u_q of LaplaceOperator.compute_l2_error)"""
        return self._problem("solution_q", (self.n_cells(l), (self.degree + 1) ** 2), l, problem)

    def problem_bc_value(self, l, problem):
        """[n_constrained] u at the node of every constrained DoF, in the order of constrained(l)"""
        return self._problem("bc_value", (self.n_constrained(l),), l, problem)


def _cell_dofs(idx27, p):
    """[n_cells, (p+1)^3] DoF of every node of every cell (x fastest) from a compressed index table without constrained
    entries (the addressing of read_dof_values_compressed, vector_access_reduced.h:153-229)"""
    n = p + 1
    idx27 = np.asarray(idx27, dtype=np.int64).reshape(-1, 27)
    out = np.empty((idx27.shape[0], n, n, n), dtype=np.int64)
    code = [0 if a == 0 else (2 if a == p else 1) for a in range(n)]
    for k in range(n):
        for j in range(n):
            oz, oy = (k - 1 if code[k] == 1 else 0), (j - 1 if code[j] == 1 else 0)
            off = (p - 1 if code[j] == 1 else 1) * oz + oy
            for i in range(n):
                base = idx27[:, 9 * code[k] + 3 * code[j] + code[i]]
                out[:, k, j, i] = base + (off * (p - 1) + i - 1 if code[i] == 1 else off)
    return out.reshape(idx27.shape[0], n ** 3)


class LaplaceOperator:
    """multigrid::LaplaceOperator<3,p,number> of one level (laplace_operator.h:56-164)."""

    def __init__(self, ctx, desc=None, handle=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.owned = handle is None
        if handle is None:
            h = C.c_void_p()
            check(self.lib.mgx_operator_create(ctx.h, C.byref(desc), C.byref(h)))
            self.h = h
        else:
            self.h = C.c_void_p(handle)
        self.number = self.lib.mgx_operator_number(self.h)

    @classmethod
    def from_cube(cls, ctx, cube, level, number=F64, coef_q=None):
        """coef_q: [n_cells, 6, (p+1)^3] merged coefficient of the general branch instead of the cube's own
        (e.g. cube.unit_law_coefficient(level))"""
        d = cube.operator_desc(level, number)
        if coef_q is not None:
            coef_q = np.ascontiguousarray(coef_q, dtype=np.float64)
            if isinstance(cube, Square):
                assert coef_q.size == cube.n_cells(level) * 3 * (cube.degree + 1) ** 2
            else:
                assert coef_q.size == cube.n_cells(level) * 6 * (cube.degree + 1) ** 3
            d.coef_q = coef_q.ctypes.data_as(_lib.f64p)  # (copied by mgx_operator_create)
        return cls(ctx, d)

    def m(self):
        return self.lib.mgx_operator_n_dofs(self.h)

    def set_profiled(self, on=True):
        check(self.lib.mgx_operator_set_profiled(self.h, int(on)))

    def initialize_dof_vector(self):
        return DeviceVector(self.ctx, self.m(), self.number)

    def vmult(self, dst, src):
        check(self.lib.mgx_vmult(self.h, dst.ptr, src.ptr))

    def vmult_with_cg_update(self, alpha, beta, r, q, p, x):
        """laplace_operator.h:638-719; returns the four sums {q.p, r.r, q.r, q.q}"""
        sums = np.zeros(4)
        check(self.lib.mgx_vmult_with_cg_update(self.h, alpha, beta, r.ptr, q.ptr, p.ptr, x.ptr, None,
                                                sums.ctypes.data_as(_lib.f64p)))
        return sums

    def vmult_residual(self, rhs, lhs, residual):
        check(self.lib.mgx_vmult_residual(self.h, rhs.ptr, lhs.ptr, residual.ptr))

    def compute_residual(self, dst, src=None, rhs_q=None):
        """LaplaceOperator::compute_residual (laplace_operator.h:804-845) on the device: dst = int f phi - A u_bc with the
        boundary values in the constrained entries of src and rhs_q = f JxW at the quadrature points (device vectors);
        on a two-dimensional operator mgx_compute_residual_2d"""
        fn = self._by_dimension("mgx_compute_residual", self.lib.mgx_operator_dim(self.h))
        check(fn(self.h, dst.ptr, src.ptr if src is not None else None, rhs_q.ptr if rhs_q is not None else None))

    def compute_l2_error(self, vec, u_q, jxw_q, sums=False):
        """MultigridSolver::compute_l2_error (multigrid_solver.h:298-343) on the device, two-dimensional operators only
        (mgx_compute_l2_error_2d): vec with its boundary values in place, u_q = u(x_q) and jxw_q = JxW_q at the quadrature
        points, device vectors of the operator's number type.  Returns sqrt(sum (u_h - u)^2 JxW / sum JxW), or with
        sums=True the two sums"""
        out = np.zeros(2)
        check(self.lib.mgx_compute_l2_error_2d(self.h, vec.ptr, u_q.ptr, jxw_q.ptr, out.ctypes.data_as(_lib.f64p)))
        return out if sums else float(np.sqrt(out[0] / out[1]))

    def compute_diagonal(self):
        check(self.lib.mgx_compute_diagonal(self.h))

    # ---- MinimalSurfaceOperator (minimal_surface/program.cc:103-200) ----
    def _by_dimension(self, name, dim):
        """the C entry point of a call that exists once per dimension: `name` in three dimensions, `name`_2d in two"""
        return getattr(self.lib, name + ("_2d" if dim == 2 else ""))

    def enable_coefficient_update(self, metric, det_jacobian):
        """affine geometry of the level: M = J^-1 J^-T as [xx,yy,zz,xy,xz,yz] and det J (Cube.affine_metric)"""
        m = np.ascontiguousarray(metric, dtype=np.float64)
        assert m.size in (3, 6)  # 3: a 2D operator, [xx,yy,xy] (Square.affine_metric)
        fn = self._by_dimension("mgx_operator_enable_coefficient_update", 2 if m.size == 3 else 3)
        check(fn(self.h, m.ctypes.data_as(_lib.f64p), float(det_jacobian)))

    def enable_coefficient_update_q(self, unit_q, jxw_q):
        """per-point geometry of a level with curved cells: unit_q [n_cells, 6, (p+1)^3] = JxW_q J^-1 J^-T and jxw_q
        [n_cells, (p+1)^3] = JxW_q (Cube.coef_q, Cube.jxw_q of a mapped cube with problem "cube")"""
        u = np.ascontiguousarray(unit_q, dtype=np.float64)
        w = np.ascontiguousarray(jxw_q, dtype=np.float64)
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.mgx_operator_get_coefficient(self.h, C.byref(p), C.byref(n)))  # (refuses an operator without coef_q)
        dim = 2 if 3 * w.size == n.value else 3  # 2: three tensor entries per point (Square.unit_q, Square.jxw_q)
        assert u.size == n.value and (3, 6)[dim - 2] * w.size == n.value
        fn = self._by_dimension("mgx_operator_enable_coefficient_update_q", dim)
        check(fn(self.h, u.ctypes.data_as(_lib.f64p), w.ctypes.data_as(_lib.f64p)))

    def evaluate_coefficient(self, law, state):
        """evaluate_coefficient(first_time, solution) :120-165: coef_q from the state (operator's number type, boundary
        values in place); law = LAW_UNIT (first_time) | LAW_MINIMAL_SURFACE"""
        check(self.lib.mgx_evaluate_coefficient(self.h, int(law), state.ptr))

    def compute_nonlinear_residual(self, law, dst, state):
        """compute_residual(dst, src, first_time) :169-197"""
        check(self.lib.mgx_compute_nonlinear_residual(self.h, int(law), dst.ptr, state.ptr))

    def get_coefficient(self):
        """the operator's merged coefficient on the device, [n_cells * 6 * (p+1)^3] entries of its number type
        ([n_cells * 3 * (p+1)^2] in two dimensions)"""
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.mgx_operator_get_coefficient(self.h, C.byref(p), C.byref(n)))
        return DeviceVector(self.ctx, n.value, self.number, ptr=p)

    def l2_norm(self, x):
        r = C.c_double()
        check(self.lib.mgx_operator_l2_norm(self.h, x.ptr, C.byref(r)))
        return r.value

    def get_matrix_diagonal_inverse(self):
        p = C.c_void_p()
        check(self.lib.mgx_get_inverse_diagonal(self.h, C.byref(p)))
        return DeviceVector(self.ctx, self.m(), self.number, ptr=p)

    def clear(self):
        if self.owned and self.h:
            self.lib.mgx_operator_destroy(self.h)
            self.h = None


class Chebyshev:
    """dealii::PreconditionChebyshev<LaplaceOperator, Vector> (multigrid_solver.h:269-289)."""

    POLYNOMIAL = {"first_kind": 0, "fourth_kind": 1}

    def __init__(self, op, smoothing_range=20., degree=3, eig_cg_n_iterations=15, handle=None, polynomial=None):
        self.op, self.lib = op, op.lib
        self.owned = handle is None
        if handle is None:
            h = C.c_void_p()
            check(self.lib.mgx_smoother_create(op.h, smoothing_range, degree, eig_cg_n_iterations, C.byref(h)))
            self.h = h
        else:
            self.h = C.c_void_p(handle)
        if polynomial is not None:
            self.set_polynomial_type(polynomial)

    def set_polynomial_type(self, polynomial):
        """AdditionalData::polynomial_type: "first_kind" or "fourth_kind" (multigrid_solver.h:277, 951)"""
        check(self.lib.mgx_smoother_set_polynomial_type(self.h, self.POLYNOMIAL[polynomial]))

    def info(self):
        i = _lib.SmootherInfo()
        check(self.lib.mgx_smoother_get_info(self.h, C.byref(i)))
        return dict(lambda_min=i.lambda_min, lambda_max=i.lambda_max, theta=i.theta, delta=i.delta,
                    degree=i.degree, cg_its=i.cg_iterations)

    def vmult(self, x, b):
        check(self.lib.mgx_smoother_vmult(self.h, x.ptr, b.ptr))

    def step(self, x, b):
        check(self.lib.mgx_smoother_step(self.h, x.ptr, b.ptr))

    def clear(self):
        if self.owned and self.h:
            self.lib.mgx_smoother_destroy(self.h)
            self.h = None


class Transfer:
    """One level pair of dealii::MGTransferMatrixFree (multigrid_solver.h:209-222)."""

    def __init__(self, coarse, fine, children, prolong_1d, handle=None):
        if handle is not None:  # a transfer of a solver, not owned
            self.lib, self.h, self.owned = coarse.lib, C.c_void_p(handle), False
            return
        self.lib, self.owned = coarse.lib, True
        self._children = np.ascontiguousarray(children, dtype=np.uint32)
        self._p1 = np.ascontiguousarray(prolong_1d, dtype=np.float64)
        d = _lib.TransferDesc(self._children.ctypes.data_as(_lib.u32p), self._p1.ctypes.data_as(_lib.f64p))
        h = C.c_void_p()
        check(self.lib.mgx_transfer_create(coarse.h, fine.h, C.byref(d), C.byref(h)))
        self.h = h

    def prolongate(self, fine, coarse, with_constraints=False):
        check(self.lib.mgx_prolongate(self.h, fine.ptr, coarse.ptr, 0, int(with_constraints)))

    def prolongate_and_add(self, fine, coarse, with_constraints=True):
        check(self.lib.mgx_prolongate(self.h, fine.ptr, coarse.ptr, 1, int(with_constraints)))

    def restrict_and_add(self, coarse, fine, with_constraints=True):
        check(self.lib.mgx_restrict_and_add(self.h, coarse.ptr, fine.ptr, int(with_constraints)))

    def interpolate_to_coarse(self, coarse, fine):
        """the state on the next coarser level (minimal_surface/program.cc:425-457): nodal interpolation, boundary DoFs
        included"""
        check(self.lib.mgx_interpolate_to_coarse(self.h, coarse.ptr, fine.ptr))

    def clear(self):
        if self.h and self.owned:
            self.lib.mgx_transfer_destroy(self.h)
            self.h = None


class MultigridSolver:
    """multigrid::MultigridSolver<3,p,Number,double> for poisson_cube (multigrid_solver.h:96-782).

    ctor arguments follow the reference: (dof_handler -> cube, degree_pre, degree_post, n_cycles);
    `vcycle_number` is the template parameter Number (program.cc:76: float; BASELINE: double)."""

    def __init__(self, ctx, cube, degree_pre=3, degree_post=3, n_cycles=1, vcycle_number=F64, comm=None,
                 polynomial="first_kind", agglomerate=True, device_rhs=False, general=False, jacobian=None, coef_q=None,
                 per_point=False, problem=None):
        """problem: a SquareProblem on a Square, curved ones included (mgx_square_solver_create_problem): per-point
        operators with the problem's tensor, its boundary values, right-hand sides assembled on the device
        (mgx_solver_compute_rhs_2d); compute_l2_error then runs on the device as well.  Not with general.
        device_rhs: the right-hand sides are assembled on the GPU (mgx_solver_compute_rhs) instead of on the host.
        general: the hierarchy in the general branch of the operator for solution-dependent coefficients
        (mgx_cube_solver_create_general: one rank; zero right-hand sides, homogeneous boundary values), on a Cartesian
        cube / box with the constant matrix `jacobian` of an affine map of the box (None: identity), or on a mapped cube
        with problem "cube" (sheared, shell_sector, shell=6|12; per-point geometry, jacobian None); per level, the
        merged coefficient coef_q[l] ([n_cells, 6, (p+1)^3]; None: the unit-law tensor).  On a Square
        (mgx_square_solver_create_general): the geometry is the square's own jacobian or map, coef_q[l] is
        [n_cells, 3, (p+1)^2].
        polynomial: Chebyshev polynomial type of the level smoothers: "first_kind" is what
        MultigridSolver<dim,p,Number,Number2> sets (multigrid_solver.h:277-278), "fourth_kind" what
        the Number == Number2 specialisation sets (:951-952)"""
        assert degree_pre == degree_post  # multigrid_solver.h:126
        self.ctx, self.cube, self.lib = ctx, cube, ctx.lib
        self.vnumber = vcycle_number
        self.comm = comm
        self.s = _lib.CubeSolver()
        self.coarse = None
        square = isinstance(cube, Square)
        # MultigridSolver<2,p,...>: one rank, right-hand sides from the host; per_point: the operators in the
        # per-(cell, q) form with the tensor of Square.coef_q
        # general: mgx_square_solver_create_general (the geometry is the square's own: its jacobian or its map)
        if square and (comm is not None or agglomerate is not True or device_rhs or jacobian is not None or
                       (coef_q is not None and not general)):
            raise ValueError("MultigridSolver on a Square: one rank, host right-hand sides "
                             "(comm, agglomerate, device_rhs, jacobian are not accepted; coef_q with general only)")
        if problem is not None and (not square or general):
            raise ValueError("MultigridSolver(problem=...): a SquareProblem on a Square, not with general")
        self.problem = problem
        self._error_operands = {}
        if cube.size > 1 and comm is None:
            raise ValueError("a decomposed cube needs a Communicator")
        self.jacobian = None if jacobian is None else np.ascontiguousarray(jacobian, dtype=np.float64).reshape(3, 3)
        common = (ctx.h, cube.h, vcycle_number, degree_pre, n_cycles)
        if general:
            keep, cq = self._pointer_array(coef_q)  # noqa: F841 (keep: the arrays live until the call returns)
            if square:
                check(self.lib.mgx_square_solver_create_general(*common, cq, C.byref(self.s)))
            else:
                jac = None if self.jacobian is None else self.jacobian.ctypes.data_as(_lib.f64p)
                check(self.lib.mgx_cube_solver_create_general(*common, jac, cq, C.byref(self.s)))
        elif problem is not None:
            check(self.lib.mgx_square_solver_create_problem(*common, C.byref(problem.c), C.byref(self.s)))
        elif square:
            check(self.lib.mgx_square_solver_create(*common, int(bool(per_point)), C.byref(self.s)))
        else:
            check(self.lib.mgx_cube_solver_create_opt(*common, int(bool(device_rhs)), C.byref(self.s)))
        self.n_levels = self.s.n_levels
        self.max_level = self.n_levels - 1
        self.h = C.c_void_p(self.s.solver)
        if cube.size > 1 and (cube.box_desc is not None or cube.shell is not None) and \
                ((agglomerate and os.environ.get("MGX_AGGLOMERATE", "1") != "0") or cube.level_offset > 0):
            # the set-up is local; whether to use it is decided by all ranks together (a rank that
            # could not build its copy must not leave the others waiting in the allreduce)
            prepared = None
            try:
                prepared = self._agglomerate(degree_pre, n_cycles, vcycle_number)
            except Exception as e:  # noqa: BLE001
                import sys
                print("mgx MultigridSolver: coarse levels stay decomposed (%r)" % (e,), file=sys.stderr, flush=True)
            everyone = prepared is not None
            if comm is not None and hasattr(comm, "allreduce"):
                everyone = comm.allreduce([1.0 if prepared is not None else 0.0])[0] == cube.size
            if prepared is not None and everyone:
                coarse, level, mine, owned = prepared
                check(self.lib.mgx_solver_set_agglomeration(self.h, level, coarse.h, mine.ctypes.data_as(_lib.u32p),
                                                            owned.ctypes.data_as(C.POINTER(C.c_uint8)), mine.size))
                self.coarse, self.coarse_level = coarse, level
            elif prepared is not None:
                prepared[0].close()
        if polynomial != "first_kind":
            check(self.lib.mgx_solver_set_polynomial_type(self.h, Chebyshev.POLYNOMIAL[polynomial]))

    @staticmethod
    def _pointer_array(coef_q):
        """the per-level tensors as the C argument `const double *const *` (None: none, an entry None: a null pointer),
        with the contiguous fp64 arrays the pointers refer to"""
        if coef_q is None:
            return None, None
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in coef_q]
        return keep, (_lib.f64p * len(keep))(*[None if a is None else a.ctypes.data_as(_lib.f64p) for a in keep])

    def _agglomerate(self, degree, n_cycles, vnumber):
        """Coarse levels of a decomposed hierarchy on every rank as a whole (mgx_solver_set_agglomeration):
        the levels whose global size is at most MGX_AGGLOMERATE_MAX_DOFS (default 3 000 000) -- there a level's
        work is microseconds and every exchange a latency.  (Up to 600 000 DoFs the copy is replayed as one HIP graph;
        the 2.1 M-DoF level of the 128^3 problem on top of it costs every rank 0.24 ms and a 17 MB allreduce instead
        of 0.45 ms of latency-bound exchanges: emulated rank at N = 8 2.71 -> 2.50 ms.)"""
        # (with the callback transport the allreduce is staged through the host: the seam stays where the vector is small)
        native = bool(getattr(self.comm, "native_ready", False)) or not hasattr(self.comm, "native_ready")
        cube, limit = self.cube, int(os.environ.get("MGX_AGGLOMERATE_MAX_DOFS", "3000000" if native else "600000"))
        level = -1
        # level i of a shell whose level-1 cells are dealt out to the ranks is level i + off of the whole mesh: the
        # coarse cells exist on the undecomposed copy only, which is therefore not optional there
        off = cube.level_offset
        for l in range(self.max_level):
            if cube.shell is not None:   # (cells x p^3 + the DoFs of two spherical boundary layers: an upper bound will do)
                size = cube.shell_desc["shell"] * 8 ** (l + off) * (cube.degree + 1) ** 3
            else:
                size = int((np.array(cube.cells_per_dim3(l)[1], dtype=np.int64) * cube.degree + 1).prod())
            if size <= limit:
                level = l
        if level < 0 and off > 0:
            level = 0   # (a mesh refined once: the rank's hierarchy is its finest level alone, the seam is that level)
        if level < 0:
            return None
        if cube.shell is not None:
            whole = Cube(cube.degree, n_refine=level + off, shell=cube.shell_desc["shell"], problem=cube.shell_desc["problem"])
        else:
            d = cube.box_desc
            whole = Cube(cube.degree, n_refine=level, box=d["box"], procs=(1, 1, 1), rank=0, numbering=d["numbering"],
                         origin=d["origin"], h0=d["h0"], geometry=d["geometry"], problem=d["problem"])
        ctx2 = Context(self.ctx.device)
        coarse = MultigridSolver(ctx2, whole, degree, degree, n_cycles, vnumber, device_rhs=True)  # its rhs is never used
        # local DoF -> DoF of the whole level through the run-independent id of a DoF
        gg = whole.dof_grid(level + off)
        order = np.argsort(gg)
        at = np.searchsorted(gg[order], cube.dof_grid(level))
        assert np.array_equal(gg[order][at], cube.dof_grid(level))
        mine = np.ascontiguousarray(order[at].astype(np.uint32))
        owned = np.ones(mine.size, dtype=np.uint8)
        owned[cube.not_owned(level)] = 0
        return coarse, level, mine, owned

    def matrix_dp(self, level):
        return LaplaceOperator(self.ctx, handle=self.s.matrix_dp[level])

    def matrix(self, level):
        return LaplaceOperator(self.ctx, handle=self.s.matrix[level])

    def smoother(self, level):
        p = C.c_void_p()
        check(self.lib.mgx_solver_get_smoother(self.h, level, C.byref(p)))
        return Chebyshev(self.matrix(level), handle=p.value)

    def solve(self, do_analyze=False, level_errors=False):
        """returns (reduction_rate, trace[n_levels,2] = residual norm start/end per level); with
        level_errors also errors[n_levels,2] = the L2 error of every level before / after its
        cycles, evaluated at the points of the solve where the reference prints them
        (multigrid_solver.h:420-424, 468-472)"""
        rate = C.c_double(1.0)
        trace = np.zeros(2 * self.n_levels)
        if not (do_analyze and level_errors):
            check(self.lib.mgx_solver_solve(self.h, int(do_analyze), C.byref(rate), trace.ctypes.data_as(_lib.f64p)))
            return rate.value, trace.reshape(-1, 2)
        errors = np.zeros((self.n_levels, 2))

        def hook(user, level, stage):
            errors[level, stage] = self.compute_l2_error(level)

        cb = _lib.LEVEL_HOOK_FN(hook)
        check(self.lib.mgx_solver_solve_hooked(self.h, 1, C.byref(rate), trace.ctypes.data_as(_lib.f64p), cb, None))
        return rate.value, trace.reshape(-1, 2), errors

    def solve_cg(self, control=None):
        """control: (max_iterations, abs_tol, reduction) of the ReductionControl (mgx_solver_solve_cg_control) instead of
        the reference's (1000, 1e-16, 1e-9) of MultigridSolver::solve_cg"""
        its = C.c_uint()
        red = C.c_double()
        if control is None:
            check(self.lib.mgx_solver_solve_cg(self.h, C.byref(its), C.byref(red)))
        else:
            check(self.lib.mgx_solver_solve_cg_control(self.h, int(control[0]), float(control[1]), float(control[2]),
                                                       C.byref(its), C.byref(red)))
        return its.value, red.value

    def update_coefficient(self, law, state):
        """LaplaceProblem::solve, minimal_surface/program.cc:425-488: the fp64 state of the finest level down the hierarchy,
        coefficient, diagonal and smoother of every level from it"""
        check(self.lib.mgx_solver_update_coefficient(self.h, int(law), state.ptr))

    def transfer_dp(self, level):
        return Transfer(self.matrix_dp(level - 1), None, None, None, handle=self.s.transfer_dp[level])

    def transfer(self, level):
        return Transfer(self.matrix(level - 1), None, None, None, handle=self.s.transfer[level])

    def cg_history(self):
        """residual norms of the last solve_cg / solve_cg_fused: [0] at the start, [k] after iteration k"""
        out = np.zeros(1001)
        n = C.c_int()
        check(self.lib.mgx_solver_cg_history(self.h, out.ctypes.data_as(_lib.f64p), out.size, C.byref(n)))
        return out[:n.value].copy()

    def vmult(self, dst, src):
        check(self.lib.mgx_solver_vmult(self.h, dst.ptr, src.ptr))

    def vmult_with_residual_update(self, residual, update, factor):
        """multigrid_solver.h:516-619; returns {z.residual, z.(factor update)}"""
        out = np.zeros(2)
        check(self.lib.mgx_solver_vmult_with_residual_update(self.h, residual.ptr, update.ptr, factor,
                                                             out.ctypes.data_as(_lib.f64p)))
        return out

    def solve_cg_fused(self):
        its = C.c_uint()
        red = C.c_double()
        check(self.lib.mgx_solver_solve_cg_fused(self.h, C.byref(its), C.byref(red)))
        return its.value, red.value

    def do_matvec(self):
        check(self.lib.mgx_solver_do_matvec(self.h))

    def do_matvec_smoother(self):
        check(self.lib.mgx_solver_do_matvec_smoother(self.h))

    def get_solution(self, level=None, insert_bc=True):
        level = self.max_level if level is None else level
        p = C.c_void_p()
        check(self.lib.mgx_solver_get_solution(self.h, level, int(insert_bc), C.byref(p)))
        return DeviceVector(self.ctx, self.cube.n_dofs(level), F64, ptr=p)

    def get_vector(self, level, which):
        ids = dict(rhs=0, residual=1, defect=2, t=3, solution_update=4)
        p = C.c_void_p()
        check(self.lib.mgx_solver_get_vector(self.h, level, ids[which], C.byref(p)))
        number = F64 if ids[which] < 2 else self.vnumber
        return DeviceVector(self.ctx, self.cube.n_dofs(level), number, ptr=p)

    def compute_l2_error(self, level=None):
        level = self.max_level if level is None else level
        if self.problem is not None:  # on the device, against u(x_q) of the problem (kept per level)
            if level not in self._error_operands:
                self._error_operands[level] = tuple(
                    self.ctx.vector(a.size, F64, data=a.ravel())
                    for a in (self.cube.problem_solution_q(level, self.problem), self.cube.jxw_q(level)))
            u_q, jxw_q = self._error_operands[level]
            return self.matrix_dp(level).compute_l2_error(self.get_solution(level, True), u_q, jxw_q)
        sol = self.get_solution(level, True).download()
        if self.cube.size == 1:
            return self.cube.l2_error(level, sol)
        e, v = self.comm.allreduce(self.cube.l2_error_parts(level, sol))
        return float(np.sqrt(e / v))

    def enable_timings(self, on=True):
        check(self.lib.mgx_solver_enable_timings(self.h, int(on)))

    def wall_times(self):
        t = np.zeros(6 * self.n_levels)
        check(self.lib.mgx_solver_get_timings(self.h, t.ctypes.data_as(_lib.f64p)))
        return t.reshape(-1, 6)

    def close(self):
        for vectors in getattr(self, "_error_operands", {}).values():
            for v in vectors:
                v.free()
        self._error_operands = {}
        if getattr(self, "h", None):
            self.lib.mgx_cube_solver_destroy(C.byref(self.s))
            self.h = None
        if getattr(self, "coarse", None) is not None:
            c = self.coarse
            self.coarse = None
            c.close()
            c.cube.close()
            c.ctx.close()


# ---------------------------------------------------------------------------------------------
# minimal_surface: solution-dependent coefficient, Newton iteration
LAW_UNIT, LAW_MINIMAL_SURFACE = 0, 1


class MinimalSurfaceProblem:
    """LaplaceProblem<dim> of minimal_surface/program.cc in 3D on the Cartesian cube / box or a mapped cube (curved cells,
    boundary function at the mapped node coordinates), or in 2D on a Square (box, sheared box or mapped; boundary
    function of [n, 2] coordinates): -div(grad u / sqrt(1 + |grad u|^2))
    = 0 with Dirichlet values, Newton's method with a V-cycle-preconditioned CG per step and the reference's
    step-halving line search.  Vectors, norms and updates stay on the device; scalars cross to the host.

    boundary: function of the node coordinates [n, 3] -> values [n] (the reference's Solution, :97-99)."""

    def __init__(self, ctx, cube, boundary, vcycle_number=F32, smoother_degree=2, jacobian=None):
        # (:470-476: Chebyshev degree 2, range 20, 15 CG iterations above the coarsest level)
        self.ctx, self.cube, self.lib = ctx, cube, ctx.lib
        self.solver = MultigridSolver(ctx, cube, smoother_degree, smoother_degree, 1, vcycle_number, general=True,
                                      jacobian=jacobian)
        l = self.level = cube.max_level
        self.op = self.solver.matrix_dp(l)
        n = self.n = cube.n_dofs(l)
        # interpolate_boundary_values(): zero in the interior, the boundary function on the Dirichlet DoFs
        u = np.zeros(n)
        c = cube.constrained(l)
        if isinstance(cube, Square):  # dimension = 2 (:73): coordinates [n, 2]; the geometry is the square's own
            if jacobian is not None:
                raise ValueError("MinimalSurfaceProblem on a Square: the jacobian belongs to the Square")
            u[c] = boundary(cube.dof_coordinates(l)[c])
        else:
            u[c] = boundary(cube.dof_coordinates(l, jacobian)[c])
        self.solution = ctx.vector(n, F64, u)
        self.tentative = ctx.vector(n, F64)
        self.system_rhs = self.solver.get_vector(l, "rhs")
        self.n_residual = self.linear_iterations = 0
        self.time_solve = self.time_residual = self.time_coefficient = 0.0
        self.history = []  # per step: (initial residual norm, halvings, final residual norm, CG iterations)

    def _residual(self, law, state):
        self.op.compute_nonlinear_residual(law, self.system_rhs, state)
        self.n_residual += 1
        return self.op.l2_norm(self.system_rhs)

    def solve(self, first_time, log=None):
        """LaplaceProblem::solve(first_time) :414-573; returns (initial, final) residual norm"""
        import time
        law = LAW_UNIT if first_time else LAW_MINIMAL_SURFACE
        t0 = time.perf_counter()
        self.solver.update_coefficient(law, self.solution)  # :425-488
        self.ctx.sync()
        self.time_coefficient += time.perf_counter() - t0
        t0 = time.perf_counter()
        initial = self._residual(law, self.solution)  # :519-523
        self.time_residual += time.perf_counter() - t0
        t0 = time.perf_counter()
        its = 0
        if initial > 0.0:
            its, _ = self.solver.solve_cg(control=(self.n, 1e-13, 1e-4))  # :514, 537-541
        direction = self.solver.get_solution(self.level, insert_bc=False)  # zero in the Dirichlet rows (:548)
        self.ctx.sync()
        self.time_solve += time.perf_counter() - t0
        self.linear_iterations += its
        t0 = time.perf_counter()
        final, alpha, n_steps, nbytes = initial, 1.0, 0, 8 * self.n
        while n_steps < 100:  # :552-568
            check(self.lib.mgx_copy_device(self.ctx.h, self.tentative.ptr, self.solution.ptr, nbytes))
            check(self.lib.mgx_sadd(self.ctx.h, F64, self.tentative.ptr, 1.0, alpha, direction.ptr, self.n))
            final = self._residual(LAW_MINIMAL_SURFACE, self.tentative)
            if final < initial:
                break
            alpha /= 2.0
            n_steps += 1
        self.time_residual += time.perf_counter() - t0
        if log is not None:
            log("Time solve (%d iterations)" % its)
            log("Residual norm: %.6g in %d steps to %.6g" % (initial, n_steps, final))
        check(self.lib.mgx_copy_device(self.ctx.h, self.solution.ptr, self.tentative.ptr, nbytes))
        self.history.append((initial, n_steps, final, its))
        return initial, final

    def run(self, n_inner_iterations=100, tolerance=1e-12, log=None):
        """the inner loop of run() :656-662; returns the number of Newton steps taken"""
        for it in range(n_inner_iterations):
            _, final = self.solve(it == 0, log)
            if final < tolerance:
                break
        return len(self.history)

    def close(self):
        for v in (self.solution, self.tentative):
            v.free()
        self.solver.close()


# ---------------------------------------------------------------------------------------------
# DG path (include/mgx_dg.h)
DG_HERMITE, DG_GAUSS_LOBATTO, DG_GAUSS = 0, 1, 2
DG_BOUNDARY, DG_NEUMANN = -1, -2   # neighbour entries of a Dirichlet / a Neumann boundary face


def dg_cheby_mesh(n_cell_steps):
    """cells per direction and cell Jacobian of matvec_dg_cheby/program.cc:55-77"""
    cells, jac = (C.c_int * 3)(), (C.c_double * 9)()
    check(_lib.load().mgx_dg_cheby_mesh(n_cell_steps, C.byref(cells), C.byref(jac)))
    return tuple(cells), np.array(jac).reshape(3, 3)


def dg_box_set_sides(cells, cell_pos, neighbours, neumann_sides):
    """marks the sides `neumann_sides` (face numbers 2d+s) of the box as Neumann faces, the others as Dirichlet faces,
    in a neighbour table made with the positions cell_pos (mgx_dg_box_set_sides); returns the table"""
    dim = len(cells)
    sides = set(int(f) for f in neumann_sides)
    assert sides <= set(range(2 * dim)), "sides are face numbers 2d+s"
    kind = (C.c_int * (2 * dim))(*[DG_NEUMANN if f in sides else DG_BOUNDARY for f in range(2 * dim)])
    nb = np.ascontiguousarray(neighbours, dtype=np.int32)
    pos = np.ascontiguousarray(cell_pos, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    check(_lib.load().mgx_dg_box_set_sides(dim, (C.c_int * dim)(*cells), pos.shape[0], pos.ctypes.data_as(i32p), kind,
                                           nb.ctypes.data_as(i32p)))
    return nb


def dg_box_neighbours(cells, ordering="z", neumann_sides=()):
    """(neighbour table [n, 6], cell positions [n, 3]) of a box of cells; the outer faces are Dirichlet faces but for
    the sides in neumann_sides (face numbers 2d+s), which are Neumann faces; a 2-tuple of
    cells gives the tables of a box of quadrilaterals, [n, 4] and [n, 2]"""
    dim = len(cells)
    neumann_sides = tuple(neumann_sides)
    c = (C.c_int * dim)(*cells)
    n = int(np.prod(cells))
    nb = np.empty((n, 2 * dim), dtype=np.int32)
    ijk = np.empty((n, dim), dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    fn = _lib.load().mgx_dg_box_neighbours_2d if dim == 2 else _lib.load().mgx_dg_box_neighbours
    check(fn(C.byref(c), 1 if ordering == "z" else 0, nb.ctypes.data_as(i32p), ijk.ctypes.data_as(i32p)))
    if neumann_sides:
        nb = dg_box_set_sides(cells, ijk, nb, neumann_sides)
    return nb, ijk


def dg_box_children(coarse_cells, coarse_ordering="z", fine_ordering="z"):
    """child table [n_coarse, 8] between a box of cells and its global refinement, both numbered as
    dg_box_neighbours numbers them: entry kx + 2 ky + 4 kz is the fine cell at 2 ijk + (kx, ky, kz); a 2-tuple of
    cells gives [n_coarse, 4], entry kx + 2 ky"""
    dim = len(coarse_cells)
    c = (C.c_int * dim)(*coarse_cells)
    ch = np.empty((int(np.prod(coarse_cells)), 1 << dim), dtype=np.uint32)
    fn = _lib.load().mgx_dg_box_children_2d if dim == 2 else _lib.load().mgx_dg_box_children
    check(fn(C.byref(c), 1 if coarse_ordering == "z" else 0, 1 if fine_ordering == "z" else 0, ch.ctypes.data_as(_lib.u32p)))
    return ch


def dg_degree_embedding(pf, pc, basis):
    """E[i, j]: coefficient i, in the basis of degree pf, of the function j of the basis of degree pc < pf on the same
    cell (mgx_dg_degree_embedding; host only)"""
    E = np.empty((max(pf, 0) + 1, max(pc, 0) + 1))
    check(_lib.load().mgx_dg_degree_embedding(pf, pc, basis, E.ctypes.data_as(_lib.f64p)))
    return E


def dg_partition(ijk, cells, procs, rank):
    """Ghost cells and exchange lists of a block decomposition, for the owned cells `ijk` ([n, 3] global
    positions, in the local cell order) of the rank whose block of the process grid they fill.
    Returns a dict: neighbours [n_owned, 6] (entries >= n_owned: ghost cells, -1: boundary), ijk,
    n_ghost, and exchange = [(rank, send_cells, recv_first, count)] in ascending rank order; the ghosts
    of one rank and the cells sent to it are in ascending global lexicographic order on both sides."""
    cells, procs = np.asarray(cells, dtype=np.int64), np.asarray(procs, dtype=np.int64)
    assert (cells % procs == 0).all(), "the process grid must divide the cells"
    blk = cells // procs
    ijk = np.asarray(ijk, dtype=np.int64)
    n_owned = len(ijk)
    gid = lambda p: p[..., 0] + cells[0] * (p[..., 1] + cells[1] * p[..., 2])   # noqa: E731
    owner = lambda p: (p[..., 0] // blk[0]) + procs[0] * ((p[..., 1] // blk[1]) + procs[1] * (p[..., 2] // blk[2]))  # noqa: E731
    assert (owner(ijk) == rank).all(), "cells outside the rank's block"
    pos = np.full(int(cells.prod()), -1, dtype=np.int64)   # global cell -> local index (owned, then ghosts)
    pos[gid(ijk)] = np.arange(n_owned)
    faces = []
    ghosts, sends = {}, {}
    for d in range(3):
        for s in (-1, 1):
            q = ijk.copy()
            q[:, d] += s
            ok = (q[:, d] >= 0) & (q[:, d] < cells[d])
            g = np.where(ok, gid(np.where(ok[:, None], q, ijk)), -1)
            own = np.where(ok, owner(np.where(ok[:, None], q, ijk)), rank)
            faces.append((ok, g))
            for rk in np.unique(own[ok & (own != rank)]):
                m = ok & (own == rk)
                ghosts.setdefault(int(rk), []).append(g[m])
                sends.setdefault(int(rk), []).append(gid(ijk[m]))
    exchange, first = [], n_owned
    for rk in sorted(ghosts):
        gl, sl = np.unique(np.concatenate(ghosts[rk])), np.unique(np.concatenate(sends[rk]))
        assert len(gl) == len(sl)
        pos[gl] = first + np.arange(len(gl))
        exchange.append((rk, pos[sl].astype(np.uint32), first, len(gl)))
        first += len(gl)
    nb = np.full((n_owned, 6), -1, dtype=np.int32)
    for f, (ok, g) in enumerate(faces):
        nb[ok, f] = pos[g[ok]]
    assert (nb[nb >= 0] < first).all()
    return dict(neighbours=nb, ijk=ijk.astype(np.int32), n_ghost=first - n_owned, exchange=exchange)


def dg_box_partition(cells, procs, rank, ordering="z"):
    """Block decomposition of a box of cells over a process grid (the DG counterpart of the Cube
    provider's decomposition; stands in for the p4est partition of the reference): the rank's block
    in z-order (or lexicographic order), then dg_partition()."""
    cells, procs = np.asarray(cells), np.asarray(procs)
    assert (cells % procs == 0).all(), "the process grid must divide the cells"
    blk = cells // procs
    r3 = np.array([rank % procs[0], (rank // procs[0]) % procs[1], rank // (procs[0] * procs[1])])
    loc = np.stack(np.meshgrid(np.arange(blk[0]), np.arange(blk[1]), np.arange(blk[2]), indexing="ij"), -1).reshape(-1, 3)
    if ordering == "z":
        def spread(v):
            out = np.zeros_like(v, dtype=np.int64)
            for bit in range(21):
                out |= ((v >> bit) & 1) << (3 * bit)
            return out
        key = spread(loc[:, 0]) | (spread(loc[:, 1]) << 1) | (spread(loc[:, 2]) << 2)
    else:
        key = loc[:, 0] + blk[0] * (loc[:, 1] + blk[1] * loc[:, 2])
    loc = loc[np.argsort(key, kind="stable")]
    # cells with a face on another rank last: the library then runs the leading (interior) cells
    # under the ghost exchange without an index list
    at_rank_face = np.zeros(len(loc), dtype=bool)
    for d in range(3):
        if r3[d] > 0:
            at_rank_face |= loc[:, d] == 0
        if r3[d] + 1 < procs[d]:
            at_rank_face |= loc[:, d] == blk[d] - 1
    loc = np.concatenate([loc[~at_rank_face], loc[at_rank_face]])
    return dg_partition(loc + r3 * blk, cells, procs, rank)


class DGFunction:
    """A function for DGLaplaceOperator.compute_rhs / compute_l2_error (mgx_dg_function, include/mgx_dg.h)."""

    def __init__(self, desc, keep=()):
        self.desc, self._keep = desc, keep   # the device vectors of a sampled function live as long as it does

    @classmethod
    def sine_product(cls, amplitude, wave, phase):
        """amplitude prod_d sin(wave[d] x_d + phase[d]), evaluated on the device in fp64; len(wave) is the dimension"""
        wave, phase = np.asarray(wave, dtype=float).ravel(), np.asarray(phase, dtype=float).ravel()
        assert wave.size == phase.size and wave.size in (2, 3)
        d = _lib.DGFunctionDesc()
        d.kind, d.dim, d.amplitude = 1, wave.size, float(amplitude)
        d.wave[:wave.size], d.phase[:wave.size] = wave.tolist(), phase.tolist()
        return cls(d)

    @classmethod
    def sampled(cls, cell_values, face_values=None):
        """fp64 device vectors: cell_values [n_cells, (p+1)^dim] in the Gauss points (x fastest; read where the function
        is f or u, may be None otherwise), face_values [n_cells, 2 dim, (p+1)^(dim-1)] in the Gauss points of face 2d+s
        (read on Dirichlet faces where the function is g)"""
        for v in (cell_values, face_values):
            assert v is None or v.number == F64, "sampled values are fp64 device vectors"
        d = _lib.DGFunctionDesc()
        d.kind = 2
        d.cell_values = cell_values.ptr if cell_values is not None else None
        d.face_values = face_values.ptr if face_values is not None else None
        return cls(d, (cell_values, face_values))


class DGLaplaceOperator:
    """multigrid::LaplaceOperatorCompactCombine<3,p,Number,type> with its JacobiTransformed
    preconditioner (common/laplace_operator_dg.h:350-2256) on an affine mesh; dim=2: <2,p,Number,type> on
    quadrilaterals (one rank)."""

    def __init__(self, ctx, degree, basis, neighbours, jacobian, number=F32, n_ghost=0, exchange=None, plan_id=77, dim=3):
        """n_ghost / exchange: decomposed mesh as dg_box_partition() describes it (the context then
        needs a Communicator); dim: neighbours is [n, 2 dim], jacobian dim x dim"""
        self.ctx, self.lib = ctx, ctx.lib
        self.degree, self.basis, self.number, self.dim = degree, basis, number, dim
        nb = np.ascontiguousarray(neighbours, dtype=np.int32).reshape(-1, 2 * dim)
        d = _lib.DGOperatorDesc()
        d.degree, d.basis, d.number, d.n_cells = degree, basis, number, nb.shape[0]
        d.neighbours = nb.ctypes.data_as(C.POINTER(C.c_int32))
        jac = np.zeros(9)
        jac[:dim * dim] = np.asarray(jacobian, dtype=float).reshape(dim, dim).ravel()
        d.jacobian = (C.c_double * 9)(*jac)
        d.dim = 0 if dim == 3 else dim
        d.n_ghost_cells = n_ghost
        if n_ghost:
            k = len(exchange)
            ranks = (C.c_int * k)(*[e[0] for e in exchange])
            counts = (C.c_uint32 * k)(*[e[3] for e in exchange])
            first = (C.c_uint32 * k)(*[e[2] for e in exchange])
            lists = [np.ascontiguousarray(e[1], dtype=np.uint32) for e in exchange]
            ptrs = (_lib.u32p * k)(*[a.ctypes.data_as(_lib.u32p) for a in lists])
            ex = _lib.DGExchangeDesc(plan_id, k, C.cast(ranks, C.POINTER(C.c_int)), C.cast(counts, _lib.u32p),
                                     C.cast(ptrs, C.POINTER(_lib.u32p)), C.cast(first, _lib.u32p))
            d.exchange = C.pointer(ex)
        h = C.c_void_p()
        check(self.lib.mgx_dg_operator_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    def m(self):
        """owned DoFs of this rank"""
        return int(self.lib.mgx_dg_operator_n_dofs(self.h))

    def vector_size(self):
        """entries of a vector: owned cells, then ghost cells"""
        return int(self.lib.mgx_dg_operator_vector_size(self.h))

    def initialize_dof_vector(self, data=None):
        """data: values of the owned DoFs"""
        v = self.ctx.vector(self.vector_size(), self.number)
        if data is not None:
            a = np.zeros(self.vector_size(), dtype=_DT[self.number])
            a[:self.m()] = np.asarray(data).ravel()
            v.upload(a)
        return v

    def update_ghost_values(self, v):
        check(self.lib.mgx_dg_update_ghost_values(self.h, v.ptr))

    def vmult(self, dst, src):
        check(self.lib.mgx_dg_vmult(self.h, dst.ptr, src.ptr))

    def vmult_residual(self, dst, rhs, src):
        check(self.lib.mgx_dg_vmult_residual(self.h, dst.ptr, rhs.ptr, src.ptr))

    def jacobi_vmult(self, dst, src):
        check(self.lib.mgx_dg_jacobi_vmult(self.h, dst.ptr, src.ptr))

    def vmult_with_chebyshev_update(self, rhs, iteration_index, factor1, factor2, solution, solution_old):
        """as the reference (laplace_operator_dg.h:910-955): on return `solution` holds the new
        iterate and `solution_old` the previous one (the two vectors trade their storage)"""
        check(self.lib.mgx_dg_vmult_with_chebyshev_update(self.h, rhs.ptr, iteration_index, factor1, factor2,
                                                          solution.ptr, solution_old.ptr))
        if iteration_index > 0:
            solution.ptr, solution_old.ptr = solution_old.ptr, solution.ptr
            solution.owned, solution_old.owned = solution_old.owned, solution.owned

    def vmult_with_cg_update(self, alpha, beta, r, q, p, x):
        """one merged CG iteration (laplace_operator_dg.h:863-908): x += alpha p, p = beta p + q (alpha == 0: p = q),
        q = A p; returns (q.p, r.r, q.r, q.q) summed over the ranks"""
        sums = np.empty(4)
        check(self.lib.mgx_dg_vmult_with_cg_update(self.h, alpha, beta, r.ptr, q.ptr, p.ptr, x.ptr,
                                                   sums.ctypes.data_as(_lib.f64p)))
        return sums

    def lumped_mass_inverse(self):
        """inverse of the lumped mass matrix of a cell (solver_dg/program.cc:134-148), (p+1)^dim entries, x fastest, fp64"""
        t = np.empty((self.degree + 1) ** self.dim)
        check(self.lib.mgx_dg_operator_lumped_mass_inverse(self.h, t.ctypes.data_as(_lib.f64p)))
        return t

    def vmult_with_pcg_sums(self, r, q, p):
        """q = A p; returns (q.p, r.(m r), q.(m r), q.(m q)) with m = lumped_mass_inverse() at every entry's local index,
        summed over the ranks: the operator's part of one merged iteration of the lumped-mass PCG"""
        sums = np.empty(4)
        check(self.lib.mgx_dg_vmult_with_pcg_sums(self.h, r.ptr, q.ptr, p.ptr, sums.ctypes.data_as(_lib.f64p)))
        return sums

    def set_cell_positions(self, origin, cell_pos):
        """integer position of every owned cell ([n, dim], as dg_box_neighbours gives it): x = origin + J (pos + xi)"""
        o = np.zeros(3)
        o[:self.dim] = np.asarray(origin, dtype=float).ravel()
        pos = np.ascontiguousarray(cell_pos, dtype=np.int32).reshape(-1, self.dim)
        check(self.lib.mgx_dg_operator_set_cell_positions(self.h, o.ctypes.data_as(_lib.f64p),
                                                          pos.ctypes.data_as(C.POINTER(C.c_int32))))

    def compute_rhs(self, dst, f=None, g=None, h=None):
        """dst_i = int f phi_i + sum over the Dirichlet faces of int g (sigma_F phi_i - d_n phi_i), f and g DGFunctions
        (None: zero; g=None is the reference's volume-only vector); dst in the operator's number type.  h: the flux on
        the Neumann faces, + sum over them of int h phi_i -- sampled: the outward normal derivative in face_values; a
        sine product: the potential u of h = n . grad u (mgx_dg_compute_rhs_mixed); None: zero flux"""
        byref = lambda fn: C.byref(fn.desc) if fn is not None else None
        if h is None:
            check(self.lib.mgx_dg_compute_rhs(self.h, byref(f), byref(g), dst.ptr if dst is not None else None))
        else:
            check(self.lib.mgx_dg_compute_rhs_mixed(self.h, byref(f), byref(g), byref(h), dst.ptr if dst is not None else None))

    def compute_l2_error(self, vec, u):
        """(sum (u_h - u)^2 JxW, sum JxW) over this rank's owned cells; the L2 error is sqrt of their ratio, each summed
        over the ranks first"""
        sums = np.empty(2)
        check(self.lib.mgx_dg_compute_l2_error(self.h, vec.ptr, C.byref(u.desc) if u is not None else None,
                                               sums.ctypes.data_as(_lib.f64p)))
        return sums

    def basis_1d(self):
        """(shape values [q, i] in the Gauss points, Gauss points, Gauss weights) on [0, 1]"""
        n = self.degree + 1
        S, x, w = np.empty((n, n)), np.empty(n), np.empty(n)
        check(self.lib.mgx_dg_operator_basis(self.h, S.ctypes.data_as(_lib.f64p), x.ctypes.data_as(_lib.f64p),
                                             w.ctypes.data_as(_lib.f64p)))
        return S, x, w

    def info(self):
        hd = C.c_double()
        pen = (C.c_double * 3)()
        ev = (C.c_double * 10)()
        check(self.lib.mgx_dg_operator_info(self.h, C.byref(hd), pen, ev))
        return dict(hermite_derivative_on_face=hd.value, penalty=np.array(pen)[:self.dim],
                    eigenvalues_1d=np.array(ev)[:self.degree + 1])

    def clear(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_operator_destroy(self.h)
            self.h = None


DG_PCG_MERGED, DG_PCG_SEPARATE = 0, 1


class DGConjugateGradient:
    """Conjugate gradients on a DGLaplaceOperator alone, preconditioned by the inverse lumped mass matrix: the solver of
    solver_dg/program.cc (:134-148 preconditioner, :177-178 control, :222-263 the two loops).  form DG_PCG_MERGED keeps the
    whole iteration on the device (three launches, no host round trip); DG_PCG_SEPARATE is textbook PCG from separate
    kernels with the scalars on the host, the yardstick.  Vectors are in the operator's number type; one rank."""

    def __init__(self, op, form=DG_PCG_MERGED, max_iterations=100, tolerance=0.0, check_every=1):
        self.op, self.lib, self.h = op, op.lib, None
        d = _lib.DGPcgSolverDesc(op.h, form, max_iterations, tolerance, check_every)
        h = C.c_void_p()
        check(self.lib.mgx_dg_pcg_solver_create(op.ctx.h, C.byref(d), C.byref(h)))
        self.h, self.max_iterations = h, max_iterations

    def solve(self, rhs, solution):
        """zero start, `solution` is overwritten; returns (iterations, reduction rate per iteration)"""
        its, red = C.c_uint(), C.c_double()
        check(self.lib.mgx_dg_pcg_solver_solve(self.h, rhs.ptr, solution.ptr, C.byref(its), C.byref(red)))
        return its.value, red.value

    def history(self):
        """rho_k = r_k . M^-1 r_k of the last solve: [0] at the start, [k] after iteration k"""
        rho, n = np.zeros(self.max_iterations + 1), C.c_uint()
        check(self.lib.mgx_dg_pcg_solver_history(self.h, rho.ctypes.data_as(_lib.f64p), C.byref(n)))
        return rho[:n.value].copy()

    def close(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_pcg_solver_destroy(self.h)
            self.h = None


class DGMultigridSolver:
    """multigrid::MultigridSolverDG<3,p,Number,double> (common/multigrid_solver_dg.h:55-747) on the
    Cartesian meshes of the Cube provider: a DG level (operator, block-Jacobi Chebyshev smoother) on
    top of the FE_Q(p) hierarchy of the same mesh, V-cycle in `vcycle_number`, outer CG in fp64.
    The DG cells are the cells of the cube's finest level in the provider's order.
    A Square in place of the cube gives MultigridSolverDG<2,...> (poisson_dg/program.cc with dimension = 2) on one rank:
    cell_ijk then has two columns."""

    def __init__(self, ctx, cube, basis=DG_HERMITE, degree_pre=3, vcycle_number=F32, comm=None):
        """comm: Communicator of a decomposed cube (box form): the DG cells get ghost cells, the FE_Q
        hierarchy is the decomposed one (not agglomerated: its smoothers are re-configured)"""
        self.ctx, self.cube, self.lib = ctx, cube, ctx.lib
        self.h = self.cfe = self.matrix_dg = self.matrix_dg_dp = None
        if isinstance(cube, Square):
            self._init_square(ctx, cube, basis, degree_pre, vcycle_number, comm)
            return
        l = cube.max_level
        local, whole = (np.array(v, dtype=np.int64) for v in cube.cells_per_dim3(l))
        procs = whole // local
        r3 = np.array([cube.rank % procs[0], (cube.rank // procs[0]) % procs[1], cube.rank // (procs[0] * procs[1])])
        ijk = cube.cell_coords(l).astype(np.int64) + r3 * local      # global positions, provider's cell order
        part = dg_partition(ijk, whole, procs, cube.rank)
        self.neighbours, self.cell_ijk = part["neighbours"], part["ijk"]
        gid = (ijk[:, 0] + whole[0] * (ijk[:, 1] + whole[1] * ijk[:, 2])).astype(np.uint32)
        jac = np.eye(3) * cube.cell_size(l)
        self.cfe = MultigridSolver(ctx, cube, degree_pre, degree_pre, 1, vcycle_number, comm=comm, agglomerate=False)
        ng, ex = part["n_ghost"], part["exchange"]
        self.matrix_dg = DGLaplaceOperator(ctx, cube.degree, basis, part["neighbours"], jac, vcycle_number, ng, ex, plan_id=1001)
        self.matrix_dg_dp = DGLaplaceOperator(ctx, cube.degree, basis, part["neighbours"], jac, F64, ng, ex, plan_id=1002)
        # coordinates for compute_rhs / compute_l2_error: the square mesh starts at -0.9, a box at its origin
        self.matrix_dg_dp.set_cell_positions((cube.box_desc["origin"] if cube.box_desc else -0.9,) * 3, self.cell_ijk)
        d = _lib.DGSolverDesc(self.matrix_dg.h, self.matrix_dg_dp.h, self.cfe.h, degree_pre, gid.ctypes.data_as(_lib.u32p))
        h = C.c_void_p()
        check(self.lib.mgx_dg_solver_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        self.vnumber = vcycle_number
        self.cell_gid = gid

    def _init_square(self, ctx, sq, basis, degree_pre, vcycle_number, comm):
        """the Cartesian box of a Square, one rank: neighbours and global cell ids (i + nx j, the layout the start vector
        of the eigenvalue estimate is defined in) from the provider's cell positions"""
        if comm is not None:
            raise ValueError("DGMultigridSolver on a Square: one rank (comm is not accepted)")
        if sq.mapped is not None or sq._jac is not None:
            raise ValueError("DGMultigridSolver on a Square: the Cartesian box only (no jacobian, not mapped)")
        l = sq.max_level
        nx, ny = sq.cells_per_dim2(l)
        ij = sq.cell_coords(l).astype(np.int64)
        pos = np.empty((ny, nx), dtype=np.int64)
        pos[ij[:, 1], ij[:, 0]] = np.arange(len(ij))
        nb = np.full((len(ij), 4), DG_BOUNDARY, dtype=np.int32)
        for f, (d, s) in enumerate(((0, -1), (0, 1), (1, -1), (1, 1))):   # face 2d+s
            q = ij.copy()
            q[:, d] += s
            ok = (q[:, d] >= 0) & (q[:, d] < (nx, ny)[d])
            nb[ok, f] = pos[q[ok, 1], q[ok, 0]]
        self.neighbours, self.cell_ijk = nb, ij.astype(np.int32)
        gid = (ij[:, 0] + nx * ij[:, 1]).astype(np.uint32)
        jac = np.eye(2) * sq.cell_size(l)
        try:
            self.cfe = MultigridSolver(ctx, sq, degree_pre, degree_pre, 1, vcycle_number)
            self.matrix_dg = DGLaplaceOperator(ctx, sq.degree, basis, nb, jac, vcycle_number, dim=2)
            self.matrix_dg_dp = DGLaplaceOperator(ctx, sq.degree, basis, nb, jac, F64, dim=2)
            self.matrix_dg_dp.set_cell_positions((sq.origin, sq.origin), self.cell_ijk)
            d = _lib.DGSolverDesc(self.matrix_dg.h, self.matrix_dg_dp.h, self.cfe.h, degree_pre, gid.ctypes.data_as(_lib.u32p))
            h = C.c_void_p()
            check(self.lib.mgx_dg_solver_create(ctx.h, C.byref(d), C.byref(h)))
        except Exception:
            self.close()
            raise
        self.h = h
        self.vnumber = vcycle_number
        self.cell_gid = gid

    def initialize_dof_vector(self, data=None):
        """fp64 vector of the solver interface (owned DoFs, then the ghost cells of a decomposed mesh)"""
        return self.matrix_dg_dp.initialize_dof_vector(data)

    def m(self):
        return self.matrix_dg.m()

    def smoother_info(self):
        i = _lib.SmootherInfo()
        check(self.lib.mgx_dg_solver_smoother_info(self.h, C.byref(i)))
        return dict(lambda_min=i.lambda_min, lambda_max=i.lambda_max, theta=i.theta, delta=i.delta,
                    degree=i.degree, cg_its=i.cg_iterations)

    def vmult(self, dst, src):
        """one DG V-cycle (multigrid_solver_dg.h:429-440); fp64 vectors"""
        check(self.lib.mgx_dg_solver_vmult(self.h, dst.ptr, src.ptr))

    def solve_cg(self, rhs, solution, tolerance=1e-9):
        """(iterations, reduction rate per iteration) of the V-cycle-preconditioned CG (:410-424)"""
        its, red = C.c_uint(), C.c_double()
        check(self.lib.mgx_dg_solver_solve_cg(self.h, tolerance, rhs.ptr, solution.ptr, C.byref(its), C.byref(red)))
        return its.value, red.value

    def restrict_to_cg(self, cg_dst, dg_src):
        check(self.lib.mgx_dg_restrict_to_cg(self.h, cg_dst.ptr, dg_src.ptr))

    def prolongate_add_cg_to_dg(self, dg_dst, cg_src):
        check(self.lib.mgx_dg_prolongate_add_cg_to_dg(self.h, dg_dst.ptr, cg_src.ptr))

    def vmult_residual_and_restrict_to_cg(self, cg_dst, rhs, lhs):
        """cg = P^T (rhs - A lhs) in one kernel (laplace_operator_dg.h:852-861), V-cycle number type"""
        check(self.lib.mgx_dg_vmult_residual_and_restrict_to_cg(self.h, cg_dst.ptr, rhs.ptr, lhs.ptr))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_solver_destroy(self.h)
            self.h = None
        for part in ("matrix_dg", "matrix_dg_dp", "cfe"):   # (a constructor that failed half-way leaves some of them)
            obj = getattr(self, part, None)
            if obj is not None:
                obj.clear() if part != "cfe" else obj.close()
                setattr(self, part, None)


class DGLevelTransfer:
    """MGTransferMatrixFree between two DG levels of the same degree and basis (include/mgx_dg.h): a cell and
    its eight children, `children` [n_coarse, 8] as dg_box_children() gives it; [n_coarse, 4]: a quadrilateral and its
    four children."""

    def __init__(self, ctx, degree, basis, children, number=F32):
        self.ctx, self.lib = ctx, ctx.lib
        self.degree, self.basis, self.number = degree, basis, number
        ch = np.asarray(children)
        self.dim = 2 if ch.ndim == 2 and ch.shape[1] == 4 else 3
        ch = np.ascontiguousarray(ch, dtype=np.uint32).reshape(-1, 1 << self.dim)
        d = _lib.DGTransferDesc(degree, basis, number, ch.shape[0], ch.ctypes.data_as(_lib.u32p), 0 if self.dim == 3 else self.dim)
        h = C.c_void_p()
        check(self.lib.mgx_dg_transfer_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    def prolongate_and_add(self, fine, coarse):
        check(self.lib.mgx_dg_transfer_prolongate_and_add(self.h, fine.ptr, coarse.ptr))

    def restrict_and_add(self, coarse, fine):
        check(self.lib.mgx_dg_transfer_restrict_and_add(self.h, coarse.ptr, fine.ptr))

    def matrix(self):
        """P[h, i, j]: coefficient i, in the child's basis, of the parent's function j on the half h of [0, 1]"""
        n = self.degree + 1
        P = np.empty((2, n, n))
        check(self.lib.mgx_dg_transfer_matrix(self.h, P.ctypes.data_as(_lib.f64p)))
        return P

    def clear(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_transfer_destroy(self.h)
            self.h = None


class DGDegreeTransfer:
    """Transfer between two DG levels of degrees coarse_degree < fine_degree and the same basis on the same n_cells cells
    in the same order (include/mgx_dg.h, mgx_dg_degree_transfer_*): p-coarsening.  dim 3 or 2."""

    def __init__(self, ctx, fine_degree, coarse_degree, basis, n_cells, number=F32, dim=3):
        self.ctx, self.lib, self.h = ctx, ctx.lib, None
        self.fine_degree, self.coarse_degree, self.basis, self.number, self.dim = fine_degree, coarse_degree, basis, number, dim
        d = _lib.DGDegreeTransferDesc(fine_degree, coarse_degree, basis, number, n_cells, dim)
        h = C.c_void_p()
        check(self.lib.mgx_dg_degree_transfer_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    def prolongate_and_add(self, fine, coarse):
        check(self.lib.mgx_dg_degree_transfer_prolongate_and_add(self.h, fine.ptr if fine is not None else None,
                                                                 coarse.ptr if coarse is not None else None))

    def restrict_and_add(self, coarse, fine):
        check(self.lib.mgx_dg_degree_transfer_restrict_and_add(self.h, coarse.ptr if coarse is not None else None,
                                                               fine.ptr if fine is not None else None))

    def matrix(self):
        """E[i, j] as dg_degree_embedding gives it"""
        E = np.empty((self.fine_degree + 1, self.coarse_degree + 1))
        check(self.lib.mgx_dg_degree_transfer_matrix(self.h, E.ctypes.data_as(_lib.f64p)))
        return E

    def clear(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_degree_transfer_destroy(self.h)
            self.h = None


class DGPlainMultigridSolver:
    """multigrid::MultigridSolverDGPlain<3,p,Number,double> (common/multigrid_solver_dg_plain.h:55-595) on a box of
    coarse_cells refined n_levels - 1 times: the DG-SIP operator on every level (cells 2^l per coarse cell and
    direction, Jacobian jacobian0 / 2^l), Chebyshev smoothers with the JacobiTransformed preconditioner, DG-to-DG
    transfers, level 0 solved by its Chebyshev iteration; V-cycle in `vcycle_number`, outer CG in fp64.  A 2-tuple of
    coarse_cells (and a 2 x 2 jacobian0) gives <2,p,Number,double>, the dimension poisson_dg_plain/program.cc:65 runs."""

    def __init__(self, ctx, degree, basis, coarse_cells, jacobian0, n_levels, degree_pre=3, vcycle_number=F32, ordering="z",
                 origin=None, neumann_sides=(), hierarchy=None):
        """origin (default 0): the corner of the box, for the coordinates x = origin + J (pos + xi) that compute_rhs and
        compute_l2_error of the finest fp64 operator evaluate sine products in; neumann_sides: the sides of the box
        (face numbers 2d+s) that are Neumann faces, on every level alike -- at least one side must stay Dirichlet.
        hierarchy (default None: every level has `degree`, level l the mesh refined l times, mgx_dg_plain_solver_create):
        the levels from coarsest to finest as (degree, refinement) pairs, starting on the mesh coarse_cells (refinement
        0); each step either refines the mesh once (same degree, refinement + 1) or raises the degree (same refinement);
        the last entry must be (degree, n_levels - 1), and n_levels may be None.  Built by mgx_dg_hp_solver_create;
        every level is a rediscretisation with its own degree and penalty."""
        self.ctx, self.lib = ctx, ctx.lib
        self.dim = dim = len(coarse_cells)
        if hierarchy is None:
            levels = [(int(degree), l) for l in range(n_levels)]
        else:
            levels = [(int(p), int(r)) for p, r in hierarchy]
            if not levels or levels[0][1] != 0:
                raise ValueError("hierarchy: the first level is on the mesh coarse_cells (refinement 0)")
            for l in range(1, len(levels)):
                (pc, rc), (pf, rf) = levels[l - 1], levels[l]
                if not ((pf == pc and rf == rc + 1) or (pf > pc and rf == rc)):
                    raise ValueError("hierarchy: the step from level %d %r to level %d %r neither refines the mesh once nor "
                                     "raises the degree" % (l - 1, levels[l - 1], l, levels[l]))
            if levels[-1][0] != degree or (n_levels is not None and levels[-1][1] != n_levels - 1):
                raise ValueError("hierarchy: the last level %r must be (degree, n_levels - 1)" % (levels[-1],))
        self.hierarchy = levels
        self.degree, self.basis, self.n_levels, self.vnumber = degree, basis, len(levels), vcycle_number
        jac0 = np.asarray(jacobian0, dtype=float).reshape(dim, dim)
        self.cells, self.cell_ijk, self.cell_gid, self.matrix, self.transfer = [], [], [], [], []
        self.matrix_dg_dp = self.h = None
        try:
            for l, (p, r) in enumerate(levels):
                cells = tuple(int(c) << r for c in coarse_cells)
                nb, ijk = dg_box_neighbours(cells, ordering, neumann_sides)
                self.cells.append(cells)
                self.cell_ijk.append(ijk)
                i64 = ijk.astype(np.int64)
                lex = i64[:, 0] + cells[0] * (i64[:, 1] + (cells[1] * i64[:, 2] if dim == 3 else 0))
                self.cell_gid.append(np.ascontiguousarray(lex, dtype=np.uint32))
                self.matrix.append(DGLaplaceOperator(ctx, p, basis, nb, jac0 / 2 ** r, vcycle_number, dim=dim))
                if l == len(levels) - 1:
                    self.matrix_dg_dp = DGLaplaceOperator(ctx, p, basis, nb, jac0 / 2 ** r, F64, dim=dim)
                    self.matrix_dg_dp.set_cell_positions(np.zeros(dim) if origin is None else origin, ijk)
                if l > 0 and levels[l - 1][1] < r:
                    self.transfer.append(DGLevelTransfer(ctx, p, basis, dg_box_children(self.cells[l - 1], ordering, ordering),
                                                         vcycle_number))
                elif l > 0:
                    self.transfer.append(DGDegreeTransfer(ctx, p, levels[l - 1][0], basis, len(ijk), vcycle_number, dim))
            n = len(levels)
            d = _lib.DGPlainSolverDesc() if hierarchy is None else _lib.DGHPSolverDesc()
            d.n_levels = n
            d.matrix = (_lib.vp * n)(*[m.h for m in self.matrix])
            d.matrix_dg_dp = self.matrix_dg_dp.h
            d.degree_pre = degree_pre
            d.cell_global_id = (_lib.u32p * n)(*[g.ctypes.data_as(_lib.u32p) for g in self.cell_gid])
            h = C.c_void_p()
            if hierarchy is None:
                d.transfer = (_lib.vp * max(1, n - 1))(*[t.h for t in self.transfer])
                check(self.lib.mgx_dg_plain_solver_create(ctx.h, C.byref(d), C.byref(h)))
            else:
                d.transfer = (_lib.vp * max(1, n - 1))(*[t.h if isinstance(t, DGLevelTransfer) else None for t in self.transfer])
                d.degree_transfer = (_lib.vp * max(1, n - 1))(*[t.h if isinstance(t, DGDegreeTransfer) else None
                                                                for t in self.transfer])
                check(self.lib.mgx_dg_hp_solver_create(ctx.h, C.byref(d), C.byref(h)))
            self.h = h
        except Exception:
            self.close()
            raise

    def m(self):
        return self.matrix[-1].m()

    def initialize_dof_vector(self, data=None):
        """fp64 vector of the finest level"""
        return self.matrix_dg_dp.initialize_dof_vector(data)

    def smoother_info(self, level):
        i = _lib.SmootherInfo()
        check(self.lib.mgx_dg_plain_solver_smoother_info(self.h, level, C.byref(i)))
        return dict(lambda_min=i.lambda_min, lambda_max=i.lambda_max, theta=i.theta, delta=i.delta,
                    degree=i.degree, cg_its=i.cg_iterations)

    def vmult(self, dst, src):
        """one V-cycle (multigrid_solver_dg_plain.h:322-334); fp64 vectors"""
        check(self.lib.mgx_dg_plain_solver_vmult(self.h, dst.ptr, src.ptr))

    def solve_cg(self, rhs, solution, tolerance=1e-9):
        """(iterations, reduction rate per iteration) of the V-cycle-preconditioned CG (:303-317)"""
        its, red = C.c_uint(), C.c_double()
        check(self.lib.mgx_dg_plain_solver_solve_cg(self.h, tolerance, rhs.ptr, solution.ptr, C.byref(its), C.byref(red)))
        return its.value, red.value

    def vmult_with_residual_update(self, residual, update, factor):
        """(:340-427) residual += factor update, update = V-cycle(residual); returns (mg.residual, mg.(factor update))"""
        out = np.empty(2)
        check(self.lib.mgx_dg_plain_solver_vmult_with_residual_update(self.h, residual.ptr, update.ptr, factor,
                                                                       out.ctypes.data_as(_lib.f64p)))
        return out

    def enable_timings(self, on=True):
        check(self.lib.mgx_dg_plain_solver_enable_timings(self.h, 1 if on else 0))

    def wall_times(self):
        """[n_levels, 6] seconds since the last call, the columns of the reference's timings[level] (print_wall_times)"""
        t = np.zeros((self.n_levels, 6))
        check(self.lib.mgx_dg_plain_solver_get_timings(self.h, t.ctypes.data_as(_lib.f64p)))
        return t

    def do_matvec(self):
        check(self.lib.mgx_dg_plain_solver_do_matvec(self.h))

    def do_matvec_smoother(self):
        check(self.lib.mgx_dg_plain_solver_do_matvec_smoother(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mgx_dg_plain_solver_destroy(self.h)
            self.h = None
        for t in self.transfer:
            t.clear()
        for m in self.matrix:
            m.clear()
        if self.matrix_dg_dp is not None:
            self.matrix_dg_dp.clear()
        self.transfer, self.matrix, self.matrix_dg_dp = [], [], None
