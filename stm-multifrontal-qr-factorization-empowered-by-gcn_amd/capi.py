"""ctypes binding of libstmmqr_hip.so (include/stmmqr_hip.h).

Mirrors the reference's operator interface for the hot path (STMMQR/include/SparseQR.h:127-268):
``qr_factorize``, ``qr_front``, ``qr_larftb``, ``qr_cpack``, ``qr_rhpack``, ``qr_assemble`` keep their names and
argument meaning; array arguments are numpy arrays (int64 = the reference's Long, float64).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
lib_path = _HERE / "libstmmqr_hip.so"

c_long_p = C.POINTER(C.c_long)
c_double_p = C.POINTER(C.c_double)
I64 = np.int64


class StmmqrError(RuntimeError):
    code = 0


ERR_RESCHEDULE = -6                        # STMMQR_ERR_RESCHEDULE (include/stmmqr_hip.h)
ERR_STALE = -7                             # STMMQR_ERR_STALE: SparseQR.refactorize, the singleton structure does not hold for the new values


if not lib_path.exists():
    raise ImportError(
        f"{lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  There is no CPU fallback for this path.")


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 (torch/lib, rpath $ORIGIN).  A
    process that loads /opt/rocm's runtime through this library FIRST and imports torch afterwards ends up with two runtimes:
    torch then reports "No HIP GPUs are available", and device pointers could not be handed from one to the other
    (sharded.py sends contribution blocks and panels from torch tensors).  So the runtime torch will use is loaded first, by
    path and without importing torch; the library's NEEDED libamdhip64.so.7 then binds to it (same soname).  Processes that
    never see torch (the C drivers, the relinked reference) use /opt/rocm's.  STMMQR_SYSTEM_HIP=1 skips this."""
    import importlib.util
    import os
    if os.environ.get("STMMQR_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    rt = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if rt.exists():
        C.CDLL(str(rt), mode=C.RTLD_GLOBAL)


_preload_torch_hip_runtime()
lib = C.CDLL(str(lib_path))


class SymbolicView(C.Structure):
    _fields_ = [(k, C.c_long) for k in ["m", "n", "anz", "nf", "maxfn", "rjsize", "hisize", "do_rank_detection"]] + \
               [(k, c_long_p) for k in ["Sp", "Sj", "Qfill", "PLinv", "Sleft", "Child", "Childp", "Super", "Rp", "Rj",
                                        "Post", "Hip", "Fm"]] + [("maxstack", C.c_long), ("r_only", C.c_long)]


class Stats(C.Structure):
    _fields_ = [(k, C.c_double) for k in ["flops", "ms_total", "ms_assemble", "ms_front", "ms_pack", "ms_h2d", "ms_d2h",
                                          "ms_host", "bytes_assemble", "bytes_pack", "flops_update", "ms_update"]] + \
               [("nlaunch", C.c_long), ("nlevels", C.c_long), ("ms_panel", C.c_double), ("ms_small", C.c_double),
                ("npanel_launch", C.c_long), ("nupdate_launch", C.c_long), ("nsteps", C.c_long),
                ("flops_update_pair", C.c_double), ("retries", C.c_long), ("device_bytes", C.c_double), ("reschedules", C.c_long)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Options(C.Structure):
    _fields_ = [("panel_width", C.c_int), ("big_front_cols", C.c_int), ("verbose", C.c_int), ("use_graph", C.c_int),
                ("panel_algo", C.c_int), ("split_update", C.c_int), ("tall_min_rows", C.c_int),
                ("lookahead", C.c_int), ("fused_update", C.c_int), ("pair_update", C.c_int)]


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_long_p)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


lib.stmmqr_last_error.restype = C.c_char_p
lib.stmmqr_version.restype = C.c_char_p
lib.stmmqr_device_name.restype = C.c_char_p
lib.stmmqr_device_name.argtypes = [C.c_int]
lib.stmmqr_plan_create.restype = C.c_void_p
lib.stmmqr_plan_create.argtypes = [C.POINTER(SymbolicView), C.c_int, C.POINTER(C.c_int)]
lib.stmmqr_plan_destroy.argtypes = [C.c_void_p]
lib.stmmqr_plan_destroy.restype = None
lib.stmmqr_plan_set_pattern.argtypes = [C.c_void_p, c_long_p, c_long_p]
lib.stmmqr_factorize_device.argtypes = [C.c_void_p, c_long_p, c_long_p, C.c_void_p, C.c_int, C.c_double, C.c_long,
                                        C.POINTER(Stats)]
lib.stmmqr_plan_result_sizes.argtypes = [C.c_void_p, c_long_p, c_long_p]
lib.stmmqr_plan_download.argtypes = [C.c_void_p, c_double_p, c_long_p, C.c_char_p, c_long_p, c_double_p, c_long_p,
                                     c_long_p, c_long_p, c_long_p, c_long_p, C.POINTER(Stats)]
lib.stmmqr_front.restype = C.c_long
lib.stmmqr_front.argtypes = [C.c_long, C.c_long, C.c_long, C.c_double, C.c_long, c_double_p, c_long_p, C.c_char_p,
                             c_double_p, c_double_p]
lib.stmmqr_larftb_qtx.argtypes = [C.c_long] * 5 + [c_double_p, c_double_p, c_double_p]
lib.stmmqr_larftb.argtypes = [C.c_int] + [C.c_long] * 5 + [c_double_p, c_double_p, c_double_p]
lib.qr_larftb.restype = None
lib.qr_larftb.argtypes = [C.c_int] + [C.c_long] * 5 + [c_double_p, c_double_p, c_double_p, c_double_p, C.c_void_p]
lib.stmmqr_last_seam_ms.restype = C.c_double
lib.stmmqr_last_seam_ms.argtypes = []
lib.qr_cpack.restype = C.c_long
lib.qr_cpack.argtypes = [C.c_long] * 4 + [c_double_p, c_double_p]
lib.qr_rhpack.restype = C.c_long
lib.qr_rhpack.argtypes = [C.c_int, C.c_long, C.c_long, C.c_long, c_long_p, c_double_p, c_double_p, c_long_p]
lib.qr_fcsize.restype = C.c_long
lib.qr_fcsize.argtypes = [C.c_long] * 4
lib.qr_assemble.restype = None
lib.qr_assemble.argtypes = [C.c_long, C.c_long, C.c_int] + [c_long_p] * 8 + [c_double_p, c_long_p, c_long_p,
                                                                             C.POINTER(c_double_p), c_long_p, c_long_p,
                                                                             c_long_p, c_long_p, c_double_p, c_long_p]
lib.stmmqr_plan_rsolve.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_long, c_double_p, C.c_long, C.c_long]
lib.stmmqr_read_matrix_market.argtypes = [C.c_char_p, c_long_p, c_long_p, c_long_p, C.POINTER(c_long_p), C.POINTER(c_long_p), C.POINTER(c_double_p)]
lib.qr_fsize.argtypes = [C.c_long] + [c_long_p] * 9
lib.stmmqr_factorize_begin.argtypes = [C.c_void_p, c_long_p, c_long_p, C.c_void_p, C.c_int, C.c_double, C.c_long]
lib.stmmqr_factorize_group.argtypes = [C.c_void_p, C.c_int, C.c_int]
lib.stmmqr_factorize_finish.argtypes = [C.c_void_p, C.POINTER(Stats)]
lib.stmmqr_plan_set_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
lib.stmmqr_plan_set_early_end.argtypes = [C.c_void_p, C.c_int]
lib.stmmqr_plan_front_info.argtypes = [C.c_void_p, C.c_long, c_long_p]
lib.stmmqr_plan_export_front.argtypes = [C.c_void_p, C.c_long, C.c_void_p, c_long_p, C.c_int]
lib.stmmqr_plan_import_front.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_long, C.c_void_p, c_long_p, C.c_int]
lib.stmmqr_plan_qmult.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_long, C.c_long]
lib.stmmqr_plan_group_steps.argtypes = [C.c_void_p, C.c_int]
lib.stmmqr_factorize_step.argtypes = [C.c_void_p] + [C.c_int] * 6
lib.stmmqr_plan_panel_doubles.argtypes = [C.c_void_p, C.c_long, c_long_p]
lib.stmmqr_plan_export_panel.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int]
lib.stmmqr_plan_import_panel.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int]
lib.stmmqr_plan_export_front_cols.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, c_long_p]
lib.stmmqr_plan_import_front_cols.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int]
lib.stmmqr_plan_front_rhoff.argtypes = [C.c_void_p, C.c_long, c_long_p]
lib.stmmqr_plan_front_kept.argtypes = [C.c_void_p, C.c_long]
lib.stmmqr_plan_front_flops.argtypes = [C.c_void_p, C.c_long, c_double_p]
lib.stmmqr_plan_device_bytes.argtypes = [C.c_void_p]
lib.stmmqr_plan_device_bytes.restype = C.c_double
lib.stmmqr_plan_solve.argtypes = [C.c_void_p, c_double_p, C.c_long, c_double_p, C.c_long, C.c_long]
lib.stmmqr_plan_keep_h.argtypes = [C.c_void_p]
lib.stmmqr_plan_spmv.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int]
lib.stmmqr_plan_solve_seminormal.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int,
                                             c_double_p]
lib.stmmqr_plan_solve_minnorm.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int]
lib.stmmqr_plan_solve_carried.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int]
lib.stmmqr_plan_covariance_diag.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_int]
lib.stmmqr_plan_rmult.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int]
lib.stmmqr_plan_condest.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_plan_leverage.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_plan_nullspace.argtypes = [C.c_void_p, C.c_long, c_long_p, C.c_void_p, C.c_long, C.c_int, C.c_int]
lib.stmmqr_plan_project_minnorm.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, c_double_p]
lib.stmmqr_plan_nullspace_times.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_plan_solve_lsminnorm.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, c_double_p]
lib.stmmqr_plan_covariance_entries.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_sparseqr_set_keep_h.argtypes = [C.c_void_p, C.c_int]
lib.stmmqr_sparseqr_solve_seminormal.argtypes = [C.c_void_p, c_long_p, c_long_p, c_double_p, c_double_p, C.c_long, C.c_long, c_double_p,
                                                 C.c_long, C.c_int, c_double_p]
lib.stmmqr_get_options.argtypes = [C.POINTER(Options)]
lib.stmmqr_set_options.argtypes = [C.POINTER(Options)]


class TransportC(C.Structure):
    """stmmqr_transport (include/stmmqr_hip.h): callbacks on device buffers, enqueued on the HIP stream they are given"""
    SEND = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    RECV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    GRP = C.CFUNCTYPE(C.c_int, C.c_void_p)
    _fields_ = [("ctx", C.c_void_p), ("send", SEND), ("recv", RECV), ("group_begin", GRP), ("group_end", GRP), ("rank", C.c_int),
                ("size", C.c_int)]


lib.stmmqr_factorize_shared_front.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(TransportC)]


class ShardPhasesC(C.Structure):
    """stmmqr_shard_phases (include/stmmqr_hip.h): what one rank does in each phase of a sharded factorization"""
    _LP, _IP = C.POINTER(C.c_long), C.POINTER(C.c_int)
    _fields_ = [("nphase", C.c_int), ("out_ptr", _LP), ("out_front", _LP), ("out_peer", _IP), ("in_ptr", _LP), ("in_front", _LP),
                ("in_peer", _IP), ("shared_front", _LP), ("shared_first", _IP), ("shared_span", _IP), ("has_group", _IP)]


lib.stmmqr_factorize_exchange.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int), C.c_long, C.POINTER(C.c_long),
                                          C.POINTER(C.c_int), C.POINTER(TransportC)]
lib.stmmqr_shared_front_gather.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.POINTER(TransportC)]
lib.stmmqr_factorize_phases.argtypes = [C.c_void_p, C.POINTER(ShardPhasesC), C.POINTER(TransportC)]
lib.stmmqr_rccl_unique_id.argtypes = [C.c_char_p]
lib.stmmqr_rccl_transport_create.argtypes = [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.POINTER(TransportC))]
lib.stmmqr_rccl_transport_destroy.restype = None
lib.stmmqr_rccl_transport_destroy.argtypes = [C.POINTER(TransportC)]
lib.stmmqr_transport_sendrecv.argtypes = [C.POINTER(TransportC), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
lib.stmmqr_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


class RcclTransport:
    """RCCL point-to-point transport of the native shared-front loop (stmmqr_rccl_transport_create).  `dist`: an initialised
    torch.distributed (any backend) that carries the 128-byte id from rank 0 to the others; the communicator itself is this
    library's own (ncclCommInitRank on the copy of librccl the process already holds)."""

    def __init__(self, dist, device=None):
        import torch
        rank, world = dist.get_rank(), dist.get_world_size()
        ident = C.create_string_buffer(128)
        if rank == 0:
            _check(lib.stmmqr_rccl_unique_id(ident), "stmmqr_rccl_unique_id")
        t = torch.frombuffer(bytearray(ident.raw), dtype=torch.uint8).clone()
        if device is not None and dist.get_backend() == "nccl":
            t = t.to(device)
        dist.broadcast(t, 0)
        raw = bytes(t.cpu().numpy().tobytes())
        self._p = C.POINTER(TransportC)()
        _check(lib.stmmqr_rccl_transport_create(world, rank, raw, C.byref(self._p)), "stmmqr_rccl_transport_create")
        self.rank, self.size = rank, world

    @property
    def ptr(self):
        return self._p

    def sendrecv(self, send_ptr, send_bytes, dst, recv_ptr, recv_bytes, src, stream=None):
        _check(lib.stmmqr_transport_sendrecv(self._p, send_ptr, send_bytes, dst, recv_ptr, recv_bytes, src, stream), "stmmqr_transport_sendrecv")

    def close(self):
        if self._p:
            lib.stmmqr_rccl_transport_destroy(self._p)
            self._p = C.POINTER(TransportC)()


class CallbackTransport:
    """A stmmqr_transport whose send / receive are Python callables (tests: the ranks of a group as threads on one GPU)"""

    def __init__(self, rank, size, send, recv):
        self._send = TransportC.SEND(lambda ctx, buf, nbytes, peer, stream: int(send(buf, nbytes, peer, stream) or 0))
        self._recv = TransportC.RECV(lambda ctx, buf, nbytes, peer, stream: int(recv(buf, nbytes, peer, stream) or 0))
        self._t = TransportC(None, self._send, self._recv, TransportC.GRP(), TransportC.GRP(), rank, size)
        self.rank, self.size = rank, size

    @property
    def ptr(self):
        return C.pointer(self._t)


def device_copy(dst: int, src: int, nbytes: int, stream=None):
    _check(lib.stmmqr_device_copy(C.c_void_p(dst), C.c_void_p(src), nbytes, stream), "stmmqr_device_copy")


def last_error() -> str:
    return lib.stmmqr_last_error().decode()


def device_count() -> int:
    return int(lib.stmmqr_device_count())


def device_name(i: int = 0) -> str:
    return lib.stmmqr_device_name(i).decode()


def get_options() -> dict:
    o = Options()
    lib.stmmqr_get_options(C.byref(o))
    return {k: getattr(o, k) for k, _ in o._fields_}


lib.stmmqr_device_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
lib.stmmqr_device_free.argtypes = [C.c_void_p]


def device_alloc(nbytes: int) -> int:
    """Device buffer from the HIP runtime the library is bound to (current device); release with device_free."""
    p = C.c_void_p()
    _check(lib.stmmqr_device_alloc(nbytes, C.byref(p)), "stmmqr_device_alloc")
    return p.value


def device_free(ptr: int):
    _check(lib.stmmqr_device_free(ptr), "stmmqr_device_free")


def set_options(**kw):
    o = Options()
    lib.stmmqr_get_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    lib.stmmqr_set_options(C.byref(o))


def _check(rc: int, what: str):
    if rc != 0:
        e = StmmqrError(f"{what} failed ({rc}): {last_error()}")
        e.code = int(rc)
        raise e


class QRNumeric:
    """Host copy of the reference's qr_numeric (STMMQR/include/SparseQR_struct.h:145-209), one stack."""

    def __init__(self, nf, n, m, rjsize, hisize, rh_total):
        self.Stack = np.zeros(max(rh_total, 1))
        self.Rblock_off = np.zeros(max(nf, 1), I64)
        self.Rdead = np.zeros(max(n, 1), np.int8)
        self.HStair = np.zeros(max(rjsize, 1), I64)
        self.HTau = np.zeros(max(rjsize, 1))
        self.Hii = np.zeros(max(hisize, 1), I64)
        self.HPinv = np.zeros(max(m, 1), I64)
        self.Hm = np.zeros(max(nf, 1), I64)
        self.Hr = np.zeros(max(nf, 1), I64)
        self.rh_total = rh_total
        self.rank = self.rank1 = self.maxfrank = self.maxfm = 0
        self.stats = {}


def _nullspace_array(call, what, ncol):
    """call(ndead, N, ldn) of a nullspace entry point with host arrays -> the ncol x d array (the count first, then the basis)"""
    nd = C.c_long(0)
    _check(call(C.byref(nd), None, max(ncol, 1)), what)
    N = np.zeros((max(ncol, 0), int(nd.value)), order="F")
    if N.size:
        _check(call(C.byref(nd), N.ctypes.data, max(ncol, 1)), what)
    return N


def _minnorm_info(v):
    return {"d": int(v[0]), "orth": float(v[1]), "norm_N": float(v[2]), "min_diag_L": float(v[3]), "built": bool(v[4])}


def _project(call, what, X, rows, with_info):
    """call(X, ldx, nrhs, info) of a projector entry point on a copy of X (rows or rows x nrhs)"""
    Xf = np.array(X, dtype=np.float64, order="F", copy=True).reshape(rows, -1, order="F")
    info = np.zeros(8)
    _check(call(Xf.ctypes.data, max(rows, 1), Xf.shape[1], _dp(info)), what)
    out = Xf[:, 0] if np.ndim(X) == 1 else Xf
    return (out, _minnorm_info(info)) if with_info else out


def _condest_dict(call, what, ncol, with_vector):
    """call(out, v) of a condest entry point with host arrays -> the dict HipQR.condest / LeastSquares.condest return"""
    out = np.zeros(8)
    v = np.zeros(max(ncol, 1)) if with_vector else None
    _check(call(out.ctypes.data, None if v is None else v.ctypes.data), what)
    d = {"cond": float(out[0]), "norm": float(out[1]), "inv_norm": float(out[2]), "rounds": int(out[3]), "r": int(out[4]), "kind": int(out[5])}
    if with_vector:
        d["v"] = v[:max(ncol, 0)]
    return d


class HipQR:
    """A device plan for one symbolic analysis (reusable across numeric factorizations).

    ``sym`` is a dict with the qr_symbolic arrays/scalars of the same names (int64 numpy arrays).
    """

    def __init__(self, sym: dict, device: int = -1):
        self._keep = {}
        v = SymbolicView()
        for k in ["m", "n", "anz", "nf", "maxfn", "rjsize", "hisize", "do_rank_detection"]:
            setattr(v, k, int(sym[k]))
        for k in ["Sp", "Sj", "Qfill", "PLinv", "Sleft", "Child", "Childp", "Super", "Rp", "Rj", "Post", "Hip", "Fm"]:
            a = sym.get(k)
            if a is not None and np.size(a) == 0 and k == "Qfill":
                a = None
            if a is not None:
                a = np.ascontiguousarray(a, dtype=I64)
                self._keep[k] = a
            setattr(v, k, _ip(a))
        v.maxstack = int(sym.get("maxstack", 0) or 0)
        v.r_only = 0 if sym.get("keepH") is None or int(sym["keepH"]) else 1     # (keepH = 0: R only, qr_rhpack's keepH = 0 layout)
        self.sym = {k: int(sym[k]) for k in ["m", "n", "anz", "nf", "maxfn", "rjsize", "hisize"]}
        st = C.c_int(0)
        self._h = lib.stmmqr_plan_create(C.byref(v), device, C.byref(st))
        if not self._h:
            raise StmmqrError(f"stmmqr_plan_create failed ({st.value}): {last_error()}")

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):          # (LeastSquares.plan(): the object owns the plan)
                lib.stmmqr_plan_destroy(self._h)
            self._h = None

    __del__ = close

    def set_pattern(self, Ap, Ai):
        Ap = np.ascontiguousarray(Ap, I64); Ai = np.ascontiguousarray(Ai, I64)
        _check(lib.stmmqr_plan_set_pattern(self._h, _ip(Ap), _ip(Ai)), "stmmqr_plan_set_pattern")

    def factorize(self, Ax, tol, ntol, Ap=None, Ai=None, device_ptr: int | None = None, detail=False) -> dict:
        """Numeric factorization; results stay in HBM.  Ax: numpy array, or device_ptr (int) of a device buffer."""
        st = Stats()
        if detail:
            st.nlaunch = -1
        if Ap is not None:
            Ap = np.ascontiguousarray(Ap, I64); Ai = np.ascontiguousarray(Ai, I64)
        if device_ptr is not None:
            rc = lib.stmmqr_factorize_device(self._h, _ip(Ap), _ip(Ai), C.c_void_p(device_ptr), 1, float(tol), int(ntol),
                                             C.byref(st))
        else:
            Ax = np.ascontiguousarray(Ax, np.float64)
            rc = lib.stmmqr_factorize_device(self._h, _ip(Ap), _ip(Ai), Ax.ctypes.data_as(C.c_void_p), 0, float(tol),
                                             int(ntol), C.byref(st))
        _check(rc, "stmmqr_factorize_device")
        return st.as_dict()

    # ---- phased interface / subtree sharding (include/stmmqr_hip.h, "Subtree sharding") ----
    def set_groups(self, group):
        g = np.ascontiguousarray(group, np.int32)
        assert g.size == self.sym["nf"]
        _check(lib.stmmqr_plan_set_groups(self._h, g.ctypes.data_as(C.POINTER(C.c_int))), "stmmqr_plan_set_groups")

    def set_early_end(self, mode: int):
        """1: the cut schedule under the phased interface (the caller handles ERR_RESCHEDULE at finish); 0: every panel a step"""
        _check(lib.stmmqr_plan_set_early_end(self._h, int(mode)), "stmmqr_plan_set_early_end")

    def begin(self, Ax, tol, ntol, Ap=None, Ai=None, device_ptr=None):
        if Ap is not None:
            Ap = np.ascontiguousarray(Ap, I64); Ai = np.ascontiguousarray(Ai, I64)
        if device_ptr is not None:
            rc = lib.stmmqr_factorize_begin(self._h, _ip(Ap), _ip(Ai), C.c_void_p(device_ptr), 1, float(tol), int(ntol))
        else:
            Ax = np.ascontiguousarray(Ax, np.float64)
            rc = lib.stmmqr_factorize_begin(self._h, _ip(Ap), _ip(Ai), Ax.ctypes.data_as(C.c_void_p), 0, float(tol), int(ntol))
        _check(rc, "stmmqr_factorize_begin")

    def run_group(self, g, detail=False):
        _check(lib.stmmqr_factorize_group(self._h, int(g), int(detail)), "stmmqr_factorize_group")

    def finish(self) -> dict:
        st = Stats()
        _check(lib.stmmqr_factorize_finish(self._h, C.byref(st)), "stmmqr_factorize_finish")
        return st.as_dict()

    def front_info(self, f) -> dict:
        info = np.zeros(6, I64)
        _check(lib.stmmqr_plan_front_info(self._h, int(f), _ip(info)), "stmmqr_plan_front_info")
        return dict(zip(["fm", "rank", "cm", "csize", "fn", "fp"], (int(x) for x in info)))

    def export_front(self, f):
        """-> (info, packed C [csize], row ids [cm]) of a factorized front (host arrays)."""
        info = self.front_info(f)
        Cb = np.zeros(max(info["csize"], 1)); rows = np.zeros(max(info["cm"], 1), I64)
        _check(lib.stmmqr_plan_export_front(self._h, int(f), Cb.ctypes.data_as(C.c_void_p), _ip(rows), 0),
               "stmmqr_plan_export_front")
        return info, Cb[:info["csize"]], rows[:info["cm"]]

    def export_front_dev(self, f, dev_ptr: int, info=None):
        """packed C of front f copied device-to-device into the buffer at dev_ptr (>= csize doubles); returns the row ids
        (host int64).  The contribution block never crosses PCIe (multi-GPU: it is then sent by RCCL from that buffer)."""
        info = info or self.front_info(f)
        rows = np.zeros(max(info["cm"], 1), I64)
        _check(lib.stmmqr_plan_export_front(self._h, int(f), C.c_void_p(dev_ptr), _ip(rows), 1), "stmmqr_plan_export_front")
        return rows[:info["cm"]]

    def import_front_dev(self, f, fm, rank, cm, dev_ptr: int, rows):
        rows = np.ascontiguousarray(rows, I64)
        _check(lib.stmmqr_plan_import_front(self._h, int(f), int(fm), int(rank), int(cm), C.c_void_p(dev_ptr), _ip(rows), 1),
               "stmmqr_plan_import_front")

    def import_front(self, f, fm, rank, cm, Cb, rows):
        Cb = np.ascontiguousarray(Cb, np.float64); rows = np.ascontiguousarray(rows, I64)
        _check(lib.stmmqr_plan_import_front(self._h, int(f), int(fm), int(rank), int(cm), Cb.ctypes.data_as(C.c_void_p),
                                            _ip(rows), 0), "stmmqr_plan_import_front")

    # ---- a front shared between plans (include/stmmqr_hip.h, "A front SHARED between plans") ----
    SHARED = 1 << 30
    PREP, PANEL, UPDATE, GRAM, POST = 1, 2, 4, 8, 16

    def group_steps(self, g) -> int:
        n = lib.stmmqr_plan_group_steps(self._h, int(g))
        if n < 0:
            raise StmmqrError(f"stmmqr_plan_group_steps failed: {last_error()}")
        return int(n)

    def run_step(self, g, step, what, cb_first=0, cb_stride=1, cb_count=-1):
        _check(lib.stmmqr_factorize_step(self._h, int(g), int(step), int(what), int(cb_first), int(cb_stride), int(cb_count)),
               "stmmqr_factorize_step")

    def shared_front_native(self, group, f, first_rank, nranks, transport):
        """the whole panel loop of a shared front in ONE native call (stmmqr_factorize_shared_front); transport: RcclTransport or
        CallbackTransport"""
        _check(lib.stmmqr_factorize_shared_front(self._h, int(group), int(f), int(first_rank), int(nranks), transport.ptr),
               "stmmqr_factorize_shared_front")

    def exchange_native(self, out, inn, transport):
        """the contribution blocks entering a phase, [(front, peer)] each way, in ONE native call (stmmqr_factorize_exchange)"""
        of, op = np.array([c for c, _ in out], I64), np.array([p for _, p in out], np.int32)
        nf, npr = np.array([c for c, _ in inn], I64), np.array([p for _, p in inn], np.int32)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))       # noqa: E731
        _check(lib.stmmqr_factorize_exchange(self._h, len(of), _ip(of), i32(op), len(nf), _ip(nf), i32(npr), transport.ptr),
               "stmmqr_factorize_exchange")

    def gather_native(self, f, first_rank, nranks, transport):
        _check(lib.stmmqr_shared_front_gather(self._h, int(f), int(first_rank), int(nranks), transport.ptr), "stmmqr_shared_front_gather")

    def phases_native(self, phases, transport):
        """every phase of a sharded factorization in ONE native call (stmmqr_factorize_phases); phases: ShardPlan.c_phases()"""
        _check(lib.stmmqr_factorize_phases(self._h, C.byref(phases[0]), transport.ptr), "stmmqr_factorize_phases")

    def panel_doubles(self, f) -> int:
        n = np.zeros(1, I64)
        _check(lib.stmmqr_plan_panel_doubles(self._h, int(f), _ip(n)), "stmmqr_plan_panel_doubles")
        return int(n[0])

    def export_panel(self, f, p):
        buf = np.zeros(self.panel_doubles(f))
        _check(lib.stmmqr_plan_export_panel(self._h, int(f), int(p), buf.ctypes.data_as(C.c_void_p), 0), "stmmqr_plan_export_panel")
        return buf

    def export_panel_dev(self, f, p, dev_ptr: int):
        _check(lib.stmmqr_plan_export_panel(self._h, int(f), int(p), C.c_void_p(dev_ptr), 1), "stmmqr_plan_export_panel")

    def import_panel(self, f, p, buf):
        buf = np.ascontiguousarray(buf, np.float64)
        assert buf.size >= self.panel_doubles(f)
        _check(lib.stmmqr_plan_import_panel(self._h, int(f), int(p), buf.ctypes.data_as(C.c_void_p), 0), "stmmqr_plan_import_panel")

    def import_panel_dev(self, f, p, dev_ptr: int):
        _check(lib.stmmqr_plan_import_panel(self._h, int(f), int(p), C.c_void_p(dev_ptr), 1), "stmmqr_plan_import_panel")

    def front_cols_doubles(self, f, part, nparts) -> int:
        n = np.zeros(1, I64)
        _check(lib.stmmqr_plan_export_front_cols(self._h, int(f), int(part), int(nparts), None, 0, _ip(n)), "stmmqr_plan_export_front_cols")
        return int(n[0])

    def export_front_cols(self, f, part, nparts):
        buf = np.zeros(max(self.front_cols_doubles(f, part, nparts), 1))
        n = np.zeros(1, I64)
        _check(lib.stmmqr_plan_export_front_cols(self._h, int(f), int(part), int(nparts), buf.ctypes.data_as(C.c_void_p), 0, _ip(n)),
               "stmmqr_plan_export_front_cols")
        return buf[:int(n[0])]

    def export_front_cols_dev(self, f, part, nparts, dev_ptr: int) -> int:
        n = np.zeros(1, I64)
        _check(lib.stmmqr_plan_export_front_cols(self._h, int(f), int(part), int(nparts), C.c_void_p(dev_ptr), 1, _ip(n)),
               "stmmqr_plan_export_front_cols")
        return int(n[0])

    def import_front_cols(self, f, part, nparts, buf):
        buf = np.ascontiguousarray(buf, np.float64)
        if buf.size:
            _check(lib.stmmqr_plan_import_front_cols(self._h, int(f), int(part), int(nparts), buf.ctypes.data_as(C.c_void_p), 0),
                   "stmmqr_plan_import_front_cols")

    def import_front_cols_dev(self, f, part, nparts, dev_ptr: int):
        _check(lib.stmmqr_plan_import_front_cols(self._h, int(f), int(part), int(nparts), C.c_void_p(dev_ptr), 1),
               "stmmqr_plan_import_front_cols")

    def front_rhoff(self, f, fn):
        off = np.zeros(int(fn) + 1, I64)
        _check(lib.stmmqr_plan_front_rhoff(self._h, int(f), _ip(off)), "stmmqr_plan_front_rhoff")
        return off

    def front_kept(self, f) -> int:
        """1: front f keeps its slab under slab recycling, 0: its packed block is staged; -1: no recycling or a bad f"""
        return int(lib.stmmqr_plan_front_kept(self._h, int(f)))

    def device_bytes(self) -> float:
        return float(lib.stmmqr_plan_device_bytes(self._h))

    def result_sizes(self):
        """-> (entries of the packed R+H, rank) of the factorization held"""
        rh, rk = C.c_long(0), C.c_long(0)
        _check(lib.stmmqr_plan_result_sizes(self._h, C.byref(rh), C.byref(rk)), "stmmqr_plan_result_sizes")
        return int(rh.value), int(rk.value)

    def front_flops(self, f):
        """-> (reference flop count of front f, the part done by trailing updates) of the factorization in progress / held"""
        v = np.zeros(2)
        _check(lib.stmmqr_plan_front_flops(self._h, int(f), _dp(v)), "stmmqr_plan_front_flops")
        return float(v[0]), float(v[1])

    def qmult(self, method: int, X: np.ndarray) -> np.ndarray:
        """QR_qmult (SparseQR.h:403-409) on the resident factors: method 0 = QR_QTX (Q'X), 1 = QR_QX (Q X) with X m or
        m x nrhs; 2 = QR_XQT (X Q'), 3 = QR_XQ (X Q) with X k x m.  Returns a new array (orders as in the reference: Q'X
        and X Q in the permuted order of the factorization)."""
        m = self.sym["m"]
        if method <= 1:
            Xf = np.array(X, dtype=np.float64, order="F", copy=True).reshape(m, -1, order="F")
            _check(lib.stmmqr_plan_qmult(self._h, int(method), _dp(Xf), m, Xf.shape[1]), "stmmqr_plan_qmult")
            return Xf.reshape(np.shape(X), order="F")
        Xf = np.array(X, dtype=np.float64, order="F", copy=True).reshape(-1, m, order="F")
        _check(lib.stmmqr_plan_qmult(self._h, int(method), _dp(Xf), Xf.shape[0], Xf.shape[0]), "stmmqr_plan_qmult")
        return Xf.reshape(np.shape(X), order="F")

    def rsolve(self, system: int, B: np.ndarray) -> np.ndarray:
        """QR_solve (SparseQR.h:411-417): system 0 RX=B, 1 RE'X=B (B m x nrhs in R's row order, X n x nrhs), 2 R'X=B,
        3 R'X=E'B (B n x nrhs, X m x nrhs)."""
        m, n = self.sym["m"], self.sym["n"]
        br, xr = (m, n) if system <= 1 else (n, m)
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(br, -1, order="F")
        X = np.zeros((xr, Bf.shape[1]), order="F")
        _check(lib.stmmqr_plan_rsolve(self._h, int(system), _dp(Bf), br, _dp(X), xr, Bf.shape[1]), "stmmqr_plan_rsolve")
        return X[:, 0] if np.ndim(B) == 1 else X

    @property
    def keep_h(self) -> bool:
        """False when the plan keeps R only (sym["keepH"] = 0)"""
        return bool(lib.stmmqr_plan_keep_h(self._h))

    def spmv(self, X: np.ndarray, trans: int = 0) -> np.ndarray:
        """A X (trans 0: X n or n x nrhs) or A' X (trans 1: X m or m x nrhs) on the device, with the values of the last
        factorization.  Deterministic: column j of a batch equals the single-vector call."""
        m, n = self.sym["m"], self.sym["n"]
        xr, yr = (m, n) if trans else (n, m)
        Xf = np.array(X, dtype=np.float64, order="F", copy=True).reshape(xr, -1, order="F")
        Y = np.zeros((yr, Xf.shape[1]), order="F")
        _check(lib.stmmqr_plan_spmv(self._h, int(trans), Xf.ctypes.data, xr, Y.ctypes.data, yr, Xf.shape[1], 0), "stmmqr_plan_spmv")
        return Y[:, 0] if np.ndim(X) == 1 else Y

    def solve_seminormal(self, B: np.ndarray, refine: int = 1):
        """Least squares with R only, by the corrected seminormal equations x = E R^-1 R^-T E' A'b plus `refine` correction steps.
        Returns (X, info), info = max over the columns of |A'r| / (|A|_F (|A|_F |x| + |b|)).  Accurate while cond(A)^2 u << 1."""
        m, n = self.sym["m"], self.sym["n"]
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(m, -1, order="F")
        X = np.zeros((n, Bf.shape[1]), order="F")
        info = C.c_double(0)
        _check(lib.stmmqr_plan_solve_seminormal(self._h, Bf.ctypes.data, m, X.ctypes.data, n, Bf.shape[1], int(refine), 0, C.byref(info)),
               "stmmqr_plan_solve_seminormal")
        return (X[:, 0] if np.ndim(B) == 1 else X), float(info.value)

    def solve_minnorm(self, B: np.ndarray, permuted: bool = False) -> np.ndarray:
        """With the plan holding the factorization of M (m x n): X = Q (R' \\ (E'B)) for B n or n x nrhs (permuted: B is already in
        R's column order, X = Q (R' \\ B)), the minimum-2-norm solution of M(:, live)' x = b(live) in M's row order; dead columns have
        no equation.  Both passes run on the device with nothing crossing to the host in between; qmult(1, rsolve(3, B)) bit for bit
        where that route works, and no limit on the width of a front where it refuses.  Needs H."""
        m, n = self.sym["m"], self.sym["n"]
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(n, -1, order="F")
        X = np.zeros((m, Bf.shape[1]), order="F")
        _check(lib.stmmqr_plan_solve_minnorm(self._h, Bf.ctypes.data, max(n, 1), X.ctypes.data, max(m, 1), Bf.shape[1], int(bool(permuted)), 0),
               "stmmqr_plan_solve_minnorm")
        return X[:, 0] if np.ndim(B) == 1 else X

    def rmult(self, X: np.ndarray, trans: int = 0, permuted: bool = False) -> np.ndarray:
        """Products with the whole rank x n factor R on the device (stmmqr_plan_rmult), dead pivot columns included.  trans = 0: X is n
        or n x nrhs, returns R (E'X) (permuted: X is in R's column order, R X) as m rows in R's row order -- what qmult(0, .) returns
        and qmult(1, .) takes; rows beyond the rank are zero.  trans = 1: X has m rows (those beyond the rank are ignored), returns
        E (R'X) or R'X.  Reads R only; column j of a batch carries the bits of the one-vector call."""
        m, n = self.sym["m"], self.sym["n"]
        xr, yr = (m, n) if trans else (n, m)
        Xf = np.array(X, dtype=np.float64, order="F", copy=True).reshape(xr, -1, order="F")
        Y = np.zeros((yr, Xf.shape[1]), order="F")
        _check(lib.stmmqr_plan_rmult(self._h, int(trans), Xf.ctypes.data, max(xr, 1), Y.ctypes.data, max(yr, 1), Xf.shape[1],
                                     int(bool(permuted)), 0), "stmmqr_plan_rmult")
        return Y[:, 0] if np.ndim(X) == 1 else Y

    def r_sparse(self, form: str = "csc", ncol=None, econ=None, device: bool = False):
        """R of the held factorization as a sparse matrix made on the device (stmmqr_plan_r_sparse): form "csc" (rows ascending within
        a column: the arrays of export_r, bit for bit) or "csr"; the leading ncol columns (default all) and the rows below econ
        (default all); exact zeros dropped.  Rows are numbered front by front over the live pivots, columns are those of the
        factorized matrix (apply Qfill).  device=False: {"ptr", "idx", "val", "shape", "info"} as numpy arrays, info = (nnz, stored
        entries visited, rows of R, 0); device=True: a torch.sparse_csc_tensor / sparse_csr_tensor (m, ncol) written on the plan's
        device -- nothing crosses the bus.  Reads R only."""
        return _r_sparse(self._h, self.sym["m"], self.sym["n"], form, ncol, econ, device)

    def h_sparse(self, device: bool = False) -> dict:
        """H of the held factorization made on the device (stmmqr_plan_h_sparse; needs keepH = 1): the Householder vectors as compressed
        columns Hp / Hi / Hx (unit diagonal stored first, exact zeros dropped, rows = the permuted row ids in front-row order), HTau and
        the row permutation HPinv -- the Hp / Hi / Hx / HTau of export_r and the HPinv of download(), bit for bit.  w[HPinv[i]] = x[i],
        then H_0 .. H_{nh-1} applied in order, gives qmult(0, x).  Returns {"Hp", "Hi", "Hx", "HTau", "HPinv", "shape": (m, nh),
        "info"}, info = (nh, hnz, entries visited before the zero test, m): numpy arrays, or with device=True torch tensors written on
        the plan's device -- nothing crosses the bus (info stays a numpy array).  No torch.sparse_csc_tensor is built: the rows of a
        column are not ascending, which that format asks for."""
        return _h_sparse(self._h, self.sym["m"], device)

    def condest(self, kind: int = 1, iters: int = 0, ncol=None, with_vector: bool = False) -> dict:
        """The condition of R over its live pivot columns -- of A(:, live) -- estimated on the device (stmmqr_plan_condest).  kind 1:
        the one-norm, exact |R_live|_1 times Hager / Higham's estimate of |R_live^-1|_1 (LAPACK's dtrcon convention); kind 2: the
        two-norm by `iters` (default 8) steps of the power iteration on R'R and on its inverse.  Both are lower bounds.  ncol as in
        covariance_diag.  Returns {"cond", "norm", "inv_norm", "rounds", "r", "kind"} and, with_vector, "v": an approximate null
        vector in the caller's column order with zeros on dead columns, unit norm of the kind and |R_live v| = 1 / inv_norm."""
        return _condest_dict(lambda out, v: lib.stmmqr_plan_condest(self._h, self.sym["n"] if ncol is None else int(ncol), int(kind), int(iters),
                                                                    out, v, 0),
                             "stmmqr_plan_condest", self.sym["n"] if ncol is None else int(ncol), with_vector)

    def nullspace(self, ncol=None, permuted: bool = False) -> np.ndarray:
        """The null-space basis N (ncol x d) of R over its first ncol columns (stmmqr_plan_nullspace): column k belongs to the k-th dead
        pivot column in R's column order, is exactly 1 there, exactly 0 on the other dead columns and -R11^-1 R12(:, k) on the live
        ones, so R N = 0 and |A E N(:, k)| <= tol + rounding.  Rows in the caller's column order (permuted: in R's).  ncol as in
        covariance_diag.  Reads R only."""
        ncol = self.sym["n"] if ncol is None else int(ncol)
        return _nullspace_array(lambda nd, N, ld: lib.stmmqr_plan_nullspace(self._h, ncol, nd, N, ld, int(bool(permuted)), 0),
                                "stmmqr_plan_nullspace", ncol)

    def nullspace_times(self) -> dict:
        """device ms of the last build of the basis held: {"N", "gram", "cholesky"} (stmmqr_plan_nullspace_times)"""
        v = np.zeros(3)
        _check(lib.stmmqr_plan_nullspace_times(self._h, _dp(v)), "stmmqr_plan_nullspace_times")
        return {"N": float(v[0]), "gram": float(v[1]), "cholesky": float(v[2])}

    def project_minnorm(self, X: np.ndarray, ncol=None, permuted: bool = False, with_info: bool = False):
        """(I - N G^-1 N')^2 X for X of ncol rows (a vector or ncol x nrhs), G = N'N: the component of X in the null space of R is
        removed, which turns the basic least-squares solution into the minimum-norm one (stmmqr_plan_project_minnorm).  Returns a new
        array; with_info also {"d", "orth": the largest |N'x_out| / (|N|_F |x_in|), "norm_N", "min_diag_L", "built"}."""
        ncol = self.sym["n"] if ncol is None else int(ncol)
        return _project(lambda Xp, ld, k, info: lib.stmmqr_plan_project_minnorm(self._h, ncol, Xp, ld, k, int(bool(permuted)), 0, info),
                        "stmmqr_plan_project_minnorm", X, ncol, with_info)

    def solve_lsminnorm(self, B: np.ndarray, with_info: bool = False):
        """The minimum-norm least-squares solution of min |A x - b| for B of m rows: solve() followed by the projector
        (stmmqr_plan_solve_lsminnorm).  Needs H.  with_info as project_minnorm."""
        m, n = self.sym["m"], self.sym["n"]
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(m, -1, order="F")
        X = np.zeros((n, Bf.shape[1]), order="F")
        info = np.zeros(8)
        _check(lib.stmmqr_plan_solve_lsminnorm(self._h, Bf.ctypes.data, max(m, 1), X.ctypes.data, max(n, 1), Bf.shape[1], 0, _dp(info)),
               "stmmqr_plan_solve_lsminnorm")
        out = X[:, 0] if np.ndim(B) == 1 else X
        return (out, _minnorm_info(info)) if with_info else out

    def solve_carried(self, nrhs: int):
        """Least squares with the right-hand sides carried through the factorization: the plan holds [A B] factorized with
        ntol = n (n = columns - nrhs, Qfill the identity on the B columns).  Returns (X, resid): X (n x nrhs) = E R11^-1 C with
        C = Q'B read from the last columns of R, resid[j] = |b_j - A x_j|_2 from the block below C.  Reads R only."""
        nrhs = int(nrhs)
        n = self.sym["n"] - nrhs
        X = np.zeros((max(n, 0), max(nrhs, 0)), order="F")
        resid = np.zeros(max(nrhs, 1))
        _check(lib.stmmqr_plan_solve_carried(self._h, nrhs, X.ctypes.data, max(n, 1), resid.ctypes.data, 0), "stmmqr_plan_solve_carried")
        return X, resid[:nrhs]

    def covariance_diag(self, ncol=None, dev_ptr=None) -> np.ndarray:
        """diag(((A E)_live' (A E)_live)^-1) in the caller's column order by selected inversion of R'R on the resident factors: the
        unscaled variances of the basic least-squares solution, 0 for dead columns.  ncol (default: every column of the plan) smaller
        than that: the plan holds [A B] as solve_carried expects it and the trailing columns take no part.  dev_ptr: a device
        pointer that receives the ncol doubles (returns None).  Reads R only; no limit on the width of a front."""
        ncol = self.sym["n"] if ncol is None else int(ncol)
        if dev_ptr is not None:
            _check(lib.stmmqr_plan_covariance_diag(self._h, ncol, C.c_void_p(int(dev_ptr)), 1), "stmmqr_plan_covariance_diag")
            return None
        var = np.zeros(max(ncol, 1))
        _check(lib.stmmqr_plan_covariance_diag(self._h, ncol, var.ctypes.data, 0), "stmmqr_plan_covariance_diag")
        return var[:max(ncol, 0)]

    def leverage(self, ncol=None, with_var=False, dev_ptr=None):
        """The leverages of the rows, lev[i] = a_i' ((A E)_live' (A E)_live)^-1 a_i in the caller's row order (the diagonal of the hat
        matrix; a_i: row i cut at ncol columns), read from the blocks of one selected inversion (stmmqr_plan_leverage).  with_var:
        returns (lev, var) with var the bits of covariance_diag(ncol), from the same inversion.  dev_ptr: a device pointer that
        receives the m doubles (returns None, or var alone with with_var)."""
        ncol = self.sym["n"] if ncol is None else int(ncol)
        m = self.sym["m"]
        var = np.zeros(max(ncol, 1)) if with_var else None
        vp = None if var is None else var.ctypes.data
        if dev_ptr is not None:
            if with_var:                                                     # (one call takes host or device pointers, not both)
                raise StmmqrError("HipQR.leverage: with_var needs host output (dev_ptr=None)")
            _check(lib.stmmqr_plan_leverage(self._h, ncol, C.c_void_p(int(dev_ptr)), None, 1), "stmmqr_plan_leverage")
            return None
        lev = np.zeros(max(m, 1))
        _check(lib.stmmqr_plan_leverage(self._h, ncol, lev.ctypes.data, vp, 0), "stmmqr_plan_leverage")
        return (lev[:m], var[:max(ncol, 0)]) if with_var else lev[:m]

    def covariance_entries(self, I, J, ncol=None) -> np.ndarray:
        """Z(I[p], J[p]) of Z = ((A E)_live' (A E)_live)^-1, column indices in the caller's order (stmmqr_plan_covariance_entries).
        Every pair must lie in the pattern of the selected inverse (two columns that share a row of A always do): the first one
        that does not raises StmmqrError (code -4) naming it."""
        ncol = self.sym["n"] if ncol is None else int(ncol)
        I = np.ascontiguousarray(I, I64).reshape(-1); J = np.ascontiguousarray(J, I64).reshape(-1)
        if I.size != J.size:
            raise StmmqrError("HipQR.covariance_entries: I and J must have the same length")
        out = np.zeros(max(I.size, 1))
        _check(lib.stmmqr_plan_covariance_entries(self._h, ncol, I.size, I.ctypes.data, J.ctypes.data, out.ctypes.data, 0),
               "stmmqr_plan_covariance_entries")
        return out[:I.size]

    def solve(self, B: np.ndarray) -> np.ndarray:
        """QR_solve(QR_RETX_EQUALS_B) (SparseQR.h:411-417): X = E R^-1 (Q'B)(1:n), least-squares solution; rank == n only."""
        m, n = self.sym["m"], self.sym["n"]
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(m, -1, order="F")
        X = np.zeros((n, Bf.shape[1]), order="F")
        _check(lib.stmmqr_plan_solve(self._h, _dp(Bf), m, _dp(X), n, Bf.shape[1]), "stmmqr_plan_solve")
        return X[:, 0] if np.ndim(B) == 1 else X

    def download(self) -> QRNumeric:
        rh = C.c_long(0); rk = C.c_long(0)
        _check(lib.stmmqr_plan_result_sizes(self._h, C.byref(rh), C.byref(rk)), "stmmqr_plan_result_sizes")
        s = self.sym
        N = QRNumeric(s["nf"], s["n"], s["m"], s["rjsize"], s["hisize"], rh.value)
        sc = np.zeros(4, I64)
        st = Stats()
        _check(lib.stmmqr_plan_download(self._h, _dp(N.Stack), _ip(N.Rblock_off),
                                        C.cast(N.Rdead.ctypes.data, C.c_char_p), _ip(N.HStair), _dp(N.HTau), _ip(N.Hii),
                                        _ip(N.HPinv), _ip(N.Hm), _ip(N.Hr), _ip(sc), C.byref(st)),
               "stmmqr_plan_download")
        N.rank, N.rank1, N.maxfrank, N.maxfm = (int(x) for x in sc)
        N.stats = st.as_dict()
        return N


def qr_factorize(sym: dict, Ap, Ai, Ax, tol, ntol) -> QRNumeric:
    """qr_factorize(&A, freeA, tol, ntol, QRsym, cc) on arrays (SparseQR.h:127-135)."""
    plan = HipQR(sym)
    try:
        stats = plan.factorize(Ax, tol, ntol, Ap, Ai)
        N = plan.download()
        N.stats = {**stats, **{k: v for k, v in N.stats.items() if k in ("ms_d2h", "ms_host")}}
        return N
    finally:
        plan.close()


class SeamNumeric:
    """What the exported qr_factorize (the drop-in seam with the reference's structs) returned: a view of the qr_numeric; the
    arrays are copied out on demand, close() releases it through stmmqr_free_numeric."""

    def __init__(self, ptr, nf, n, m, rjsize, hisize):
        self._p, self.nf, self.n, self.m, self.rjsize, self.hisize = ptr, nf, n, m, rjsize, hisize
        c = ptr.contents
        self.rank, self.rank1, self.maxfrank, self.maxfm = c.rank, c.rank1, c.maxfrank, c.maxfm
        self.rh_total = int(c.Stack_size[0])

    def arrays(self) -> dict:
        c = self._p.contents
        take = lambda ptr, cnt, ty: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ty)), shape=(max(cnt, 1),))[:cnt].copy()
        stacks = C.cast(c.Stacks, C.POINTER(c_double_p))
        base = C.cast(stacks[0], C.c_void_p).value
        rb = C.cast(c.Rblock, C.POINTER(C.c_void_p))
        return {"Stack": take(stacks[0], self.rh_total, C.c_double), "Rdead": take(c.Rdead, self.n, C.c_int8),
                "HStair": take(c.HStair, self.rjsize, C.c_long), "HTau": take(c.HTau, self.rjsize, C.c_double),
                "Hii": take(c.Hii, self.hisize, C.c_long), "HPinv": take(c.HPinv, self.m, C.c_long),
                "Hm": take(c.Hm, self.nf, C.c_long), "Hr": take(c.Hr, self.nf, C.c_long),
                "Rblock_off": np.array([((rb[f] or base) - base) // 8 for f in range(self.nf)], I64)}

    def close(self):
        if self._p:
            pp = C.POINTER(QrNumericC)(self._p.contents)
            lib.stmmqr_free_numeric(C.byref(pp), None)
            self._p = None

    __del__ = close


def qr_factorize_seam(sym: dict, Ap, Ai, Ax, tol, ntol) -> SeamNumeric:
    """ONE call of the exported qr_factorize -- the drop-in seam itself, with the reference's structs (sparse_csc **, freeA = 0,
    qr_symbolic *, cc = NULL), exactly what SparseQR.c:349 calls: plan (built or from the seam's cache), H2D, factorization, host
    allocation of the qr_numeric, D2H of the packed factors."""
    keep = {}
    S = QrSymbolicC()
    for k in ("m", "n", "anz", "nf", "maxfn", "rjsize", "do_rank_detection", "maxstack", "hisize", "keepH", "ntasks", "ns"):
        setattr(S, k, int(sym.get(k, 1 if k in ("keepH", "ntasks", "ns") else 0)))
    for k in ("Sp", "Sj", "Qfill", "PLinv", "Sleft", "Parent", "Child", "Childp", "Super", "Rp", "Rj", "Post", "Hip", "Fm", "Cm"):
        a = sym.get(k)
        if a is not None and len(a):
            keep[k] = np.ascontiguousarray(a, I64)
            setattr(S, k, _ip(keep[k]))
    keep["Ap"], keep["Ai"], keep["Ax"] = np.ascontiguousarray(Ap, I64), np.ascontiguousarray(Ai, I64), np.ascontiguousarray(Ax, np.float64)
    A = SparseCsc()
    A.nrow, A.ncol, A.nzmax = S.m, S.n, len(keep["Ax"])
    A.p, A.i, A.x = keep["Ap"].ctypes.data, keep["Ai"].ctypes.data, keep["Ax"].ctypes.data
    A.stype, A.itype, A.xtype, A.dtype, A.sorted, A.packed = 0, 2, 1, 0, 1, 1
    Ah = C.pointer(A)
    lib.qr_factorize.restype = C.POINTER(QrNumericC)
    lib.qr_factorize.argtypes = [C.POINTER(C.POINTER(SparseCsc)), C.c_long, C.c_double, C.c_long, C.POINTER(QrSymbolicC), C.c_void_p]
    lib.stmmqr_free_numeric.restype = None
    lib.stmmqr_free_numeric.argtypes = [C.POINTER(C.POINTER(QrNumericC)), C.c_void_p]
    N = lib.qr_factorize(C.byref(Ah), 0, float(tol), int(ntol), C.byref(S), None)
    if not N:
        raise StmmqrError("qr_factorize (seam) returned NULL: " + last_error())
    return SeamNumeric(N, S.nf, S.n, S.m, S.rjsize, S.hisize)


def plan_cache_clear():
    lib.stmmqr_plan_cache_clear()


def qr_front(m, n, npiv, tol, ntol, F, Stair):
    """qr_front (SparseQR.h:209-226).  F: (m,n) Fortran-ordered, modified in place; Stair int64, in/out.
    Returns (rank, Tau, Rdead, flops)."""
    assert F.flags.f_contiguous and F.dtype == np.float64 and F.shape == (m, n)
    assert Stair.dtype == I64
    Tau = np.zeros(max(n, 1)); Rdead = np.zeros(max(n, 1), np.int8); fl = C.c_double(0)
    r = lib.stmmqr_front(m, n, npiv, float(tol), int(ntol), _dp(F), _ip(Stair), C.cast(Rdead.ctypes.data, C.c_char_p),
                         _dp(Tau), C.byref(fl))
    if r < 0:
        raise StmmqrError(f"stmmqr_front failed: {last_error()}")
    return int(r), Tau[:n], Rdead[:min(n, max(npiv, 0))], fl.value


def last_seam_ms() -> float:
    """Device time (ms) of the kernels of the last qr_front / qr_assemble seam call (-1: none)."""
    return float(lib.stmmqr_last_seam_ms())


def qr_larftb(method, m, n, k, ldc, ldv, V, Tau, Cmat):
    """qr_larftb (SparseQR.h:255-268; SparseQR_factorize.c:1851-1904), C in place: method 0 QR_QTX C <- Q'C, 1 QR_QX
    C <- QC (C m x n, V m x k), 2 QR_XQT C <- CQ', 3 QR_XQ C <- CQ (C m x n, V n x k), Q = I - V T V'."""
    _check(lib.stmmqr_larftb(method, m, n, k, ldc, ldv, _dp(V), _dp(Tau), _dp(Cmat)), "stmmqr_larftb")


def qr_fcsize(m, n, npiv, g):
    return int(lib.qr_fcsize(m, n, npiv, g))


def qr_cpack(m, n, npiv, g, F):
    """qr_cpack (SparseQR.h:235-242): returns (cm, packed C)."""
    Cp = np.zeros(max(qr_fcsize(m, n, npiv, g), 1))
    cm = lib.qr_cpack(m, n, npiv, g, _dp(F), _dp(Cp))
    if cm < 0:
        raise StmmqrError("qr_cpack failed")
    return int(cm), Cp[:qr_fcsize(m, n, npiv, g)]


def qr_rhpack(m, n, npiv, Stair, F, keep_h=True):
    """qr_rhpack (SparseQR.h:244-253): returns (rsize, rm, packed R+H), or packed R only with keep_h=False."""
    R = np.zeros(max(m * n, 1)); rm = C.c_long(0)
    rs = lib.qr_rhpack(1 if keep_h else 0, m, n, npiv, _ip(Stair), _dp(F), _dp(R), C.byref(rm))
    if rs < 0:
        raise StmmqrError("qr_rhpack failed")
    return int(rs), int(rm.value), R[:rs]


class SparseCsc(C.Structure):
    """sparse_csc (STMMQR/include/SparseCore.h:514-556), the fields the seams read"""
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t), ("p", C.c_void_p), ("i", C.c_void_p),
                ("nz", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p), ("stype", C.c_int), ("itype", C.c_int),
                ("xtype", C.c_int), ("dtype", C.c_int), ("sorted", C.c_int), ("packed", C.c_int)]


class QrSymbolicC(C.Structure):
    """qr_symbolic (SparseQR_struct.h:26-137), field order of include/stmmqr_hip.h"""
    _fields_ = [("m", C.c_long), ("n", C.c_long), ("anz", C.c_long)] + \
               [(k, c_long_p) for k in ("Sp", "Sj", "Qfill", "PLinv", "Sleft")] + [("nf", C.c_long), ("maxfn", C.c_long)] + \
               [(k, c_long_p) for k in ("Parent", "Child", "Childp", "Super", "Rp", "Rj", "Post")] + \
               [(k, C.c_long) for k in ("rjsize", "do_rank_detection", "maxstack", "hisize", "keepH")] + [("Hip", c_long_p)] + \
               [("ntasks", C.c_long), ("ns", C.c_long)] + \
               [(k, c_long_p) for k in ("TaskChildp", "TaskChild", "TaskStack", "TaskFront", "TaskFrontp", "On_stack",
                                        "Stack_maxstack", "Fm", "Cm")]


class QrNumericC(C.Structure):
    """qr_numeric (SparseQR_struct.h:145-209)"""
    _fields_ = [("Rblock", C.c_void_p), ("Stacks", C.c_void_p), ("Stack_size", c_long_p)] + \
               [(k, C.c_long) for k in ("hisize", "n", "m", "nf", "ntasks", "ns", "maxstack")] + [("Rdead", C.c_char_p)] + \
               [(k, C.c_long) for k in ("rank", "rank1", "maxfrank")] + [("norm_E_fro", C.c_double)] + \
               [("keepH", C.c_long), ("rjsize", C.c_long), ("HStair", c_long_p), ("HTau", c_double_p)] + \
               [(k, c_long_p) for k in ("Hii", "HPinv", "Hm", "Hr")] + [("maxfm", C.c_long)]


class Relax(C.Structure):
    _fields_ = [("nrelax", C.c_long * 3), ("zrelax", C.c_double * 3)]


lib.stmmqr_relax_for_qr.restype = None
lib.stmmqr_relax_for_qr.argtypes = [C.c_long, C.c_long, C.POINTER(Relax)]
lib.stmmqr_analyze.argtypes = [C.c_long, C.c_long, c_long_p, c_long_p, c_long_p, C.c_int, C.POINTER(Relax), C.POINTER(C.c_void_p)]
lib.stmmqr_analysis_symbolic.restype = C.POINTER(QrSymbolicC)
lib.stmmqr_analysis_symbolic.argtypes = [C.c_void_p]
lib.stmmqr_analysis_info.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_analysis_free.restype = None
lib.stmmqr_analysis_free.argtypes = [C.c_void_p]


def relax_for_qr(n: int, nnz: int) -> Relax:
    """Relaxfactor_setting(n, nnz, RELAX_FOR_QR) (SparseCore_common.c:1172-1203, called by the driver at qrtest.c:153)."""
    r = Relax()
    lib.stmmqr_relax_for_qr(n, nnz, C.byref(r))
    return r


def analyze(m: int, n: int, Ap, Ai, Qfill=None, do_rank_detection: bool = True, relax: Relax | None = None) -> dict:
    """qr_analyze (SparseQR_analyze.c:20-700) on plain arrays: the whole qr_symbolic as a dict of numpy arrays / ints,
    plus 'info' = [flop bound, fl, lnz, QR_CHUNK_FLAG, nnz(R) bound, nnz(H) bound, maxstack, nf].  Host-only."""
    Ap = np.ascontiguousarray(Ap, I64)
    Ai = np.ascontiguousarray(Ai, I64)
    Q = None if Qfill is None else np.ascontiguousarray(Qfill, I64)
    h = C.c_void_p()
    _check(lib.stmmqr_analyze(m, n, _ip(Ap), _ip(Ai), _ip(Q), 1 if do_rank_detection else 0,
                              None if relax is None else C.byref(relax), C.byref(h)), "stmmqr_analyze")
    try:
        S = lib.stmmqr_analysis_symbolic(h).contents
        nf, anz = S.nf, S.anz
        out = {k: int(getattr(S, k)) for k in ("m", "n", "anz", "nf", "maxfn", "rjsize", "do_rank_detection", "maxstack", "hisize",
                                               "keepH", "ntasks", "ns")}
        sizes = {"Sp": m + 1, "Sj": anz, "Qfill": n, "PLinv": m, "Sleft": n + 2, "Parent": nf + 1, "Child": nf + 1,
                 "Childp": nf + 2, "Super": nf + 1, "Rp": nf + 1, "Rj": S.Rp[nf] if nf > 0 else 0, "Post": nf + 1, "Hip": nf + 1,
                 "Fm": nf + 1, "Cm": nf + 1}
        for k, cnt in sizes.items():
            ptr = getattr(S, k)
            out[k] = np.ctypeslib.as_array(ptr, shape=(cnt,)).copy() if cnt > 0 else np.zeros(0, I64)
        info = np.zeros(8)
        _check(lib.stmmqr_analysis_info(h, _dp(info)), "stmmqr_analysis_info")
        out["info"] = info
        return out
    finally:
        lib.stmmqr_analysis_free(h)


lib.stmmqr_sparseqr.argtypes = [C.c_int, C.c_double, C.c_long, C.c_long, c_long_p, c_long_p, c_double_p, c_long_p, C.POINTER(Relax), C.c_int,
                                C.POINTER(C.c_void_p)]
lib.stmmqr_sparseqr_symbolic.argtypes = [C.c_int, C.c_double, C.c_long, C.c_long, c_long_p, c_long_p, c_double_p, c_long_p, C.POINTER(Relax),
                                         C.POINTER(C.c_void_p)]
lib.stmmqr_sparseqr_numeric.argtypes = [C.c_void_p, C.c_int]
lib.stmmqr_sparseqr_free.restype = None
lib.stmmqr_sparseqr_free.argtypes = [C.c_void_p]
lib.stmmqr_sparseqr_info.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_sparseqr_q1fill.restype = c_long_p
lib.stmmqr_sparseqr_q1fill.argtypes = [C.c_void_p]
lib.stmmqr_sparseqr_symbolic_view.restype = C.POINTER(QrSymbolicC)
lib.stmmqr_sparseqr_symbolic_view.argtypes = [C.c_void_p]
lib.stmmqr_sparseqr_y.argtypes = [C.c_void_p, C.POINTER(c_long_p), C.POINTER(c_long_p), C.POINTER(c_double_p)]
lib.stmmqr_sparseqr_qmult.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_long, C.c_long, C.c_long, c_double_p, C.c_long]
lib.stmmqr_sparseqr_solve.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_long, C.c_long, c_double_p, C.c_long]
lib.stmmqr_sparseqr_min2norm.argtypes = [C.c_void_p, c_double_p, C.c_long, C.c_long, c_double_p, C.c_long]
lib.stmmqr_sparseqr_tol.restype = C.c_double
lib.stmmqr_sparseqr_tol.argtypes = [C.c_void_p]
lib.stmmqr_sparseqr_refactorize.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_sparseqr_refactor_info.argtypes = [C.c_void_p, c_double_p]
c_int_p = C.POINTER(C.c_int)
lib.stmmqr_sparseqr_refactor_maps.argtypes = [C.c_void_p, c_long_p, C.POINTER(c_int_p), C.POINTER(c_int_p), C.POINTER(c_int_p)]


lib.stmmqr_sparseqr_plan.restype = C.c_void_p
lib.stmmqr_sparseqr_plan.argtypes = [C.c_void_p]
lib.stmmqr_plan_export_r.argtypes = [C.c_void_p, C.POINTER(QrSymbolicC), C.c_long, C.POINTER(c_long_p), C.POINTER(c_long_p),
                                     C.POINTER(c_double_p), c_long_p, C.POINTER(c_long_p), C.POINTER(c_long_p), C.POINTER(c_double_p),
                                     C.POINTER(c_double_p)]
lib.stmmqr_plan_r_sparse.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, c_long_p, C.c_int]
lib.stmmqr_plan_device_index.argtypes = [C.c_void_p]
lib.stmmqr_plan_h_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_long, c_long_p, C.c_int]
lib.stmmqr_sparselq.argtypes = [C.c_int, C.c_double, C.c_long, C.c_long, c_long_p, c_long_p, c_double_p, C.POINTER(Relax), C.c_int,
                                C.POINTER(C.c_void_p)]
lib.stmmqr_free.restype = None
lib.stmmqr_free.argtypes = [C.c_void_p]


def _take(ptr, count, dtype):
    out = np.ctypeslib.as_array(ptr, shape=(max(count, 1),))[:count].astype(dtype, copy=True)
    lib.stmmqr_free(C.cast(ptr, C.c_void_p))
    return out


R_SPARSE_FORMS = {"csc": 0, "csr": 1}


def _r_sparse(plan, m, n, form, ncol, econ, device):
    """stmmqr_plan_r_sparse on a plan handle of an m x n factorization: the count call, the arrays, the fill call.  device=False:
    {"ptr", "idx", "val", "shape", "info"} as numpy arrays; device=True: a torch.sparse_csc_tensor / sparse_csr_tensor of shape
    (m, ncol) whose int64 / float64 tensors live on the plan's device and were written there."""
    if form not in R_SPARSE_FORMS:
        raise StmmqrError(f"r_sparse: form {form!r} is neither 'csc' nor 'csr'")
    code = R_SPARSE_FORMS[form]
    ncol = n if ncol is None else int(ncol)
    econ = m if econ is None else int(econ)
    nptr = max((ncol if code == 0 else m) + 1, 1)
    info = np.zeros(4, I64)
    ptr = np.zeros(nptr, I64)
    _check(lib.stmmqr_plan_r_sparse(plan, code, ncol, econ, ptr.ctypes.data, None, None, 0, _ip(info), 0), "stmmqr_plan_r_sparse")
    nnz = int(info[0])
    if not device:
        idx, val = np.zeros(max(nnz, 1), I64), np.zeros(max(nnz, 1))
        _check(lib.stmmqr_plan_r_sparse(plan, code, ncol, econ, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz, _ip(info), 0),
               "stmmqr_plan_r_sparse")
        return {"ptr": ptr, "idx": idx[:nnz], "val": val[:nnz], "shape": (m, ncol), "info": info}
    import torch
    dev = torch.device("cuda", int(lib.stmmqr_plan_device_index(plan)))
    tptr = torch.empty(nptr, dtype=torch.int64, device=dev)
    tidx = torch.empty(max(nnz, 1), dtype=torch.int64, device=dev)
    tval = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _check(lib.stmmqr_plan_r_sparse(plan, code, ncol, econ, tptr.data_ptr(), tidx.data_ptr(), tval.data_ptr(), nnz, _ip(info), 1),
           "stmmqr_plan_r_sparse")
    make = torch.sparse_csc_tensor if code == 0 else torch.sparse_csr_tensor
    return make(tptr, tidx[:nnz], tval[:nnz], size=(m, ncol))


def _h_sparse(plan, m, device):
    """stmmqr_plan_h_sparse on a plan handle of a factorization with m rows: the count call, the arrays, the fill call.  device=False:
    {"Hp", "Hi", "Hx", "HTau", "HPinv", "shape": (m, nh), "info"} as numpy arrays; device=True: the same keys as int64 / float64 torch
    tensors that live on the plan's device and were written there (info stays a numpy array)."""
    info = np.zeros(4, I64)
    _check(lib.stmmqr_plan_h_sparse(plan, None, None, None, None, None, 0, 0, _ip(info), 0), "stmmqr_plan_h_sparse")
    nh, hnz = int(info[0]), int(info[1])
    if not device:
        Hp, Hi, Hx = np.zeros(nh + 1, I64), np.zeros(max(hnz, 1), I64), np.zeros(max(hnz, 1))
        HTau, HPinv = np.zeros(max(nh, 1)), np.zeros(max(m, 1), I64)
        _check(lib.stmmqr_plan_h_sparse(plan, Hp.ctypes.data, Hi.ctypes.data, Hx.ctypes.data, HTau.ctypes.data, HPinv.ctypes.data, nh, hnz,
                                        _ip(info), 0), "stmmqr_plan_h_sparse")
        return {"Hp": Hp, "Hi": Hi[:hnz], "Hx": Hx[:hnz], "HTau": HTau[:nh], "HPinv": HPinv[:m], "shape": (m, nh), "info": info}
    import torch
    dev = torch.device("cuda", int(lib.stmmqr_plan_device_index(plan)))
    tHp = torch.empty(nh + 1, dtype=torch.int64, device=dev)
    tHi = torch.empty(max(hnz, 1), dtype=torch.int64, device=dev)
    tHx = torch.empty(max(hnz, 1), dtype=torch.float64, device=dev)
    tTau = torch.empty(max(nh, 1), dtype=torch.float64, device=dev)
    tPinv = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _check(lib.stmmqr_plan_h_sparse(plan, tHp.data_ptr(), tHi.data_ptr(), tHx.data_ptr(), tTau.data_ptr(), tPinv.data_ptr(), nh, hnz,
                                    _ip(info), 1), "stmmqr_plan_h_sparse")
    return {"Hp": tHp, "Hi": tHi[:hnz], "Hx": tHx[:hnz], "HTau": tTau[:nh], "HPinv": tPinv[:m], "shape": (m, nh), "info": info}


def _symbolic_dict(S, m, n) -> dict:
    nf, anz = S.nf, S.anz
    out = {k: int(getattr(S, k)) for k in ("m", "n", "anz", "nf", "maxfn", "rjsize", "do_rank_detection", "maxstack", "hisize", "keepH",
                                           "ntasks", "ns")}
    sizes = {"Sp": m + 1, "Sj": anz, "Qfill": n, "PLinv": m, "Sleft": n + 2, "Parent": nf + 1, "Child": nf + 1, "Childp": nf + 2,
             "Super": nf + 1, "Rp": nf + 1, "Rj": S.Rp[nf] if nf > 0 else 0, "Post": nf + 1, "Hip": nf + 1, "Fm": nf + 1, "Cm": nf + 1}
    for k, cnt in sizes.items():
        out[k] = np.ctypeslib.as_array(getattr(S, k), shape=(cnt,)).copy() if cnt > 0 else np.zeros(0, I64)
    return out


class SparseQR:
    """SparseQR() / QR_qmult / QR_solve / SparseQR_free of the reference (STMMQR/include/SparseQR.h:25-36,403-417) on this library
    alone: singletons + COLAMD + symbolic analysis on the host, numeric factorization and the Q / R operations on the device.
    symbolic_only=True stops after the host half (no GPU needed)."""

    def __init__(self, m, n, Ap, Ai, Ax, ordering=7, tol=-2.0, relax: Relax | None = None, Quser=None, device=-1, symbolic_only=False,
                 keep_h=True):
        """keep_h=False: the numeric phase keeps R only (keepH = 0): solve works, qmult and export_r's H do not."""
        self.m, self.n = int(m), int(n)
        self._A = (np.ascontiguousarray(Ap, I64), np.ascontiguousarray(Ai, I64), np.ascontiguousarray(Ax, np.float64))
        Q = None if Quser is None else np.ascontiguousarray(Quser, I64)
        self._h = C.c_void_p()
        self._args = dict(ordering=ordering, tol=tol, relax=relax, Quser=Quser, device=device, keep_h=keep_h)   # (refactorize(rebuild=True))
        self._rebuilt = 0
        rp = None if relax is None else C.byref(relax)
        if symbolic_only or not keep_h:
            _check(lib.stmmqr_sparseqr_symbolic(ordering, tol, m, n, _ip(self._A[0]), _ip(self._A[1]), _dp(self._A[2]), _ip(Q), rp,
                                                C.byref(self._h)), "stmmqr_sparseqr_symbolic")
            if not keep_h:
                _check(lib.stmmqr_sparseqr_set_keep_h(self._h, 0), "stmmqr_sparseqr_set_keep_h")
                if not symbolic_only:
                    self.numeric(device)
        else:
            _check(lib.stmmqr_sparseqr(ordering, tol, m, n, _ip(self._A[0]), _ip(self._A[1]), _dp(self._A[2]), _ip(Q), rp, device,
                                       C.byref(self._h)), "stmmqr_sparseqr")

    def numeric(self, device=-1):
        _check(lib.stmmqr_sparseqr_numeric(self._h, device), "stmmqr_sparseqr_numeric")

    def close(self):
        if self._h:
            lib.stmmqr_sparseqr_free(self._h)
            self._h = None

    __del__ = close

    @property
    def info(self) -> dict:
        v = np.zeros(12)
        _check(lib.stmmqr_sparseqr_info(self._h, _dp(v)), "stmmqr_sparseqr_info")
        keys = ["rank", "n1rows", "n1cols", "nf", "ana_seconds", "fac_seconds", "flops", "flop_bound", "ms_device", "ordering", "chunk_flag",
                "retries"]
        return dict(zip(keys, v.tolist()))

    @property
    def Q1fill(self):
        return np.ctypeslib.as_array(lib.stmmqr_sparseqr_q1fill(self._h), shape=(max(self.n, 1),))[:self.n].copy()

    def symbolic(self) -> dict:
        S = lib.stmmqr_sparseqr_symbolic_view(self._h).contents
        return _symbolic_dict(S, S.m, S.n)

    def Y(self):
        """(Yp, Yi, Yx) of the matrix handed to the numeric phase when singletons were removed, else None"""
        p, i, x = c_long_p(), c_long_p(), c_double_p()
        _check(lib.stmmqr_sparseqr_y(self._h, C.byref(p), C.byref(i), C.byref(x)), "stmmqr_sparseqr_y")
        if not p:
            return None
        n2 = self.n - int(self.info["n1cols"])
        Yp = np.ctypeslib.as_array(p, shape=(n2 + 1,)).copy()
        nz = int(Yp[-1])
        return Yp, np.ctypeslib.as_array(i, shape=(max(nz, 1),))[:nz].copy(), np.ctypeslib.as_array(x, shape=(max(nz, 1),))[:nz].copy()

    def export_r(self, econ=None, with_h=True) -> dict:
        """qr_rcount + qr_rconvert (SparseLQ.c:102-517) on the factors resident in HBM: R of the multifrontal part as CSC over
        the columns of the factorized matrix (Rp, Ri, Rx) and, with_h, H as CSC (Hp, Hi, Hx) + HTau."""
        Sptr = lib.stmmqr_sparseqr_symbolic_view(self._h)
        S = Sptr.contents
        econ = S.m if econ is None else econ
        Rp, Ri, Hp, Hi = c_long_p(), c_long_p(), c_long_p(), c_long_p()
        Rx, Hx, Ht = c_double_p(), c_double_p(), c_double_p()
        nh = C.c_long(0)
        _check(lib.stmmqr_plan_export_r(lib.stmmqr_sparseqr_plan(self._h), Sptr, econ, C.byref(Rp), C.byref(Ri), C.byref(Rx),
                                        C.byref(nh) if with_h else None, C.byref(Hp) if with_h else None, C.byref(Hi) if with_h else None,
                                        C.byref(Hx) if with_h else None, C.byref(Ht) if with_h else None), "stmmqr_plan_export_r")
        n = S.n
        out = {"Rp": _take(Rp, n + 1, I64)}
        out["Ri"], out["Rx"] = _take(Ri, int(out["Rp"][-1]), I64), _take(Rx, int(out["Rp"][-1]), np.float64)
        if with_h:
            out["Hp"] = _take(Hp, nh.value + 1, I64)
            hnz = int(out["Hp"][-1])
            out["Hi"], out["Hx"], out["HTau"] = _take(Hi, hnz, I64), _take(Hx, hnz, np.float64), _take(Ht, nh.value, np.float64)
        return out

    def r_sparse(self, form: str = "csc", ncol=None, econ=None, device: bool = False):
        """HipQR.r_sparse on the object's plan: R of the multifrontal part, as export_r gives it (R1 of the singletons is not part of
        it), without the download -- and with device=True as a torch sparse tensor that never left the device."""
        S = lib.stmmqr_sparseqr_symbolic_view(self._h).contents
        return _r_sparse(lib.stmmqr_sparseqr_plan(self._h), int(S.m), int(S.n), form, ncol, econ, device)

    def h_sparse(self, device: bool = False) -> dict:
        """HipQR.h_sparse on the object's plan: H, HTau and HPinv of the multifrontal part, as export_r gives them (the singleton rows
        are not part of it), without the download -- and with device=True as torch tensors that never left the device (no
        torch.sparse_csc_tensor: the rows of a column of H are not ascending)."""
        S = lib.stmmqr_sparseqr_symbolic_view(self._h).contents
        return _h_sparse(lib.stmmqr_sparseqr_plan(self._h), int(S.m), device)

    @classmethod
    def lq(cls, m, n, Ap, Ai, Ax, tol=-2.0, relax: Relax | None = None, device=-1):
        """SparseLQ (SparseLQ.c:691-734): the QR object of A' (L = R').  min2norm(b) on it is the minimum-2-norm solution of A x = b."""
        self = cls.__new__(cls)
        self._is_lq = True                                   # (the QR object of A': solve_seminormal would need A' as the matrix)
        self.m, self.n = int(n), int(m)
        self._A = (np.ascontiguousarray(Ap, I64), np.ascontiguousarray(Ai, I64), np.ascontiguousarray(Ax, np.float64))
        self._h = C.c_void_p()
        self._args = dict(tol=tol, relax=relax, device=device)
        self._rebuilt = 0
        _check(lib.stmmqr_sparselq(7, tol, m, n, _ip(self._A[0]), _ip(self._A[1]), _dp(self._A[2]), None if relax is None else C.byref(relax),
                                   device, C.byref(self._h)), "stmmqr_sparselq")
        return self

    def refactorize(self, Ax=None, dev_ptr=None, rebuild=False):
        """New values of the same pattern (stmmqr_sparseqr_refactorize): Ax, a numpy array in the storage order of the matrix the
        object was made from (A itself also for SparseQR.lq objects), or dev_ptr, a device pointer to such values (tensor.data_ptr()).
        Column order, singletons, analysis, plan and arenas stay; tolerance, R1, Y, factors, rank are made again.  Raises
        StmmqrError with code ERR_STALE, the object unchanged, when a singleton of the first values has no pivot above the new
        tolerance -- unless rebuild=True, which then makes a new native object with the same arguments from Ax and swaps it in
        (refactor_info["rebuilt"] counts that; needs Ax: there is no host copy of device values to analyse).  Returns self."""
        if (Ax is None) == (dev_ptr is None):
            raise StmmqrError("refactorize: give Ax (a host array) or dev_ptr (a device pointer), one of them")
        if dev_ptr is not None:
            if rebuild:
                raise StmmqrError("refactorize: rebuild=True needs host values (Ax): a device pointer leaves nothing to analyse on the host")
            _check(lib.stmmqr_sparseqr_refactorize(self._h, C.c_void_p(int(dev_ptr)), 1), "stmmqr_sparseqr_refactorize")
            self._A = (self._A[0], self._A[1], None)                 # (solve_seminormal needs A's values on the host)
            return self
        Ax = np.ascontiguousarray(Ax, np.float64)
        if Ax.size != int(self._A[0][-1]):
            raise StmmqrError("refactorize: Ax must hold one value per entry of the pattern")
        rc = lib.stmmqr_sparseqr_refactorize(self._h, Ax.ctypes.data if Ax.size else None, 0)
        if rc == ERR_STALE and rebuild:
            a = self._args
            if getattr(self, "_is_lq", False):
                new = SparseQR.lq(self.n, self.m, self._A[0], self._A[1], Ax, **a)
            else:
                new = SparseQR(self.m, self.n, self._A[0], self._A[1], Ax, **a)
            old, self._h, new._h = self._h, new._h, None
            lib.stmmqr_sparseqr_free(old)
            self._A, self._rebuilt = new._A, self._rebuilt + 1
            return self
        _check(rc, "stmmqr_sparseqr_refactorize")
        self._A = (self._A[0], self._A[1], Ax.copy())
        return self

    @property
    def refactor_info(self) -> dict:
        """stmmqr_sparseqr_refactor_info, and "rebuilt": how often refactorize(rebuild=True) had to make a new native object"""
        v = np.zeros(8)
        _check(lib.stmmqr_sparseqr_refactor_info(self._h, _dp(v)), "stmmqr_sparseqr_refactor_info")
        keys = ["tol", "ms_values", "ms_factorize", "seconds", "refactorizations", "stale", "analyses_and_plans", "device_bytes"]
        return {**dict(zip(keys, v.tolist())), **{i: float(v[i]) for i in range(8)}, "rebuilt": self._rebuilt}

    def refactor_maps(self) -> dict:
        """stmmqr_sparseqr_refactor_maps: counts = [nz, nnz(Y), nnz(R1), n1rows] and ysrc / r1src / pivsrc (None where the native
        pointer is NULL: no singletons and no LQ object), positions in the caller's storage order"""
        cnt = np.zeros(4, I64)
        y, r, p = c_int_p(), c_int_p(), c_int_p()
        _check(lib.stmmqr_sparseqr_refactor_maps(self._h, _ip(cnt), C.byref(y), C.byref(r), C.byref(p)), "stmmqr_sparseqr_refactor_maps")

        def arr(ptr, k):
            return np.ctypeslib.as_array(ptr, shape=(max(int(k), 1),))[:int(k)].copy() if ptr else None
        return {"counts": cnt, "ysrc": arr(y, cnt[1]), "r1src": arr(r, cnt[2]), "pivsrc": arr(p, cnt[3])}

    @property
    def tol(self) -> float:
        """the tolerance the factorization really used (stmmqr_sparseqr_tol)"""
        return float(lib.stmmqr_sparseqr_tol(self._h))

    def qmult(self, method, X):
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1, order="F")
        Y = np.zeros_like(X, order="F")
        _check(lib.stmmqr_sparseqr_qmult(self._h, method, _dp(X), X.shape[0], X.shape[0], X.shape[1], _dp(Y), Y.shape[0]), "stmmqr_sparseqr_qmult")
        return Y

    def solve_seminormal(self, B, refine=1):
        """Least squares by the corrected seminormal equations with R only (also without H), products with this object's full A on
        the device.  Returns (X, info), info = max over the columns of |A'r| / (|A|_F (|A|_F |x| + |b|))."""
        if getattr(self, "_is_lq", False):
            raise StmmqrError("solve_seminormal: not on the LQ object")
        if self._A[2] is None:
            raise StmmqrError("solve_seminormal: the object was last refactorized from a device pointer and has no host copy of A's values; "
                              "refactorize with a host array (Ax=...) first")
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B.reshape(-1, 1, order="F")
        X = np.zeros((self.n, B.shape[1]), order="F")
        info = C.c_double(0)
        _check(lib.stmmqr_sparseqr_solve_seminormal(self._h, _ip(self._A[0]), _ip(self._A[1]), _dp(self._A[2]), _dp(B), B.shape[0],
                                                    B.shape[1], _dp(X), self.n, int(refine), C.byref(info)),
               "stmmqr_sparseqr_solve_seminormal")
        return X, float(info.value)

    def min2norm(self, B):
        """On the QR object of A' (SparseQR.lq(A), or SparseQR of the transpose): the minimum-2-norm solution of A x = b,
        x = Q (R' \\ (E'b)), for B self.n or self.n x nrhs -> self.m x nrhs.  The multifrontal part runs on the device in one call
        (HipQR.solve_minnorm): unlike qmult(1, solve(3, B)) it has no limit on the width of a front.  Needs H."""
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B.reshape(-1, 1, order="F")
        X = np.zeros((self.m, B.shape[1]), order="F")
        _check(lib.stmmqr_sparseqr_min2norm(self._h, _dp(B), B.shape[0], B.shape[1], _dp(X), max(self.m, 1)), "stmmqr_sparseqr_min2norm")
        return X

    def solve(self, system, B):
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B.reshape(-1, 1, order="F")
        rows = self.n if system <= 1 else self.m
        X = np.zeros((rows, B.shape[1]), order="F")
        _check(lib.stmmqr_sparseqr_solve(self._h, system, _dp(B), B.shape[0], B.shape[1], _dp(X), rows), "stmmqr_sparseqr_solve")
        return X


lib.stmmqr_ls_create.argtypes = [C.c_int, C.c_double, C.c_long, C.c_long, c_long_p, c_long_p, c_double_p, C.c_long, c_long_p, C.POINTER(Relax),
                                 C.c_int, C.POINTER(C.c_void_p)]
lib.stmmqr_ls_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int]
lib.stmmqr_ls_symbolic_view.restype = C.POINTER(QrSymbolicC)
lib.stmmqr_ls_symbolic_view.argtypes = [C.c_void_p]
lib.stmmqr_ls_plan.restype = C.c_void_p
lib.stmmqr_ls_plan.argtypes = [C.c_void_p]
lib.stmmqr_ls_info.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_ls_resid.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_ls_covariance_diag.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_ls_leverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_ls_covariance_entries.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_ls_condest.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
lib.stmmqr_ls_nullspace.argtypes = [C.c_void_p, c_long_p, C.c_void_p, C.c_long, C.c_int]
lib.stmmqr_ls_project_minnorm.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, c_double_p]
lib.stmmqr_ls_free.restype = None
lib.stmmqr_ls_free.argtypes = [C.c_void_p]


class LsDamping(C.Structure):
    """stmmqr_ls_damping (include/stmmqr_hip.h)"""
    _fields_ = [("w", C.c_void_p), ("d", C.c_void_p), ("lam", C.c_double), ("scale", C.c_int), ("scale_min", C.c_double),
                ("scale_max", C.c_double), ("D_out", C.c_void_p), ("dnorm", C.c_void_p)]


lib.stmmqr_ls_create_damped.argtypes = lib.stmmqr_ls_create.argtypes
lib.stmmqr_ls_solve_damped.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LsDamping), C.c_void_p, C.c_long, C.c_void_p, C.c_long,
                                       C.c_void_p, C.c_int]
lib.stmmqr_ls_dims.argtypes = [C.c_void_p, c_long_p]
lib.stmmqr_ls_damped_info.argtypes = [C.c_void_p, c_double_p]
lib.stmmqr_ls_adjoint.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_long, C.c_void_p, C.c_void_p, C.c_int, c_double_p]
lib.stmmqr_ls_adjoint_z.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int]
_ADJOINT_INFO = ["live", "refine_steps", "normal_resid", "ms", "ms_passes", "bytes_added"]


class LsRobust(C.Structure):
    """stmmqr_ls_robust (include/stmmqr_hip.h)"""
    _fields_ = [("loss", C.c_int), ("cc", C.c_double), ("sigma", C.c_double), ("mad_factor", C.c_double), ("sigma_min", C.c_double),
                ("w0", C.c_void_p)]


ROBUST_LOSSES = {"l2": 0, "huber": 1, "cauchy": 2, "tukey": 3, "l1": 4}
lib.stmmqr_median_abs.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
lib.stmmqr_ls_robust_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LsRobust), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, c_double_p]
lib.stmmqr_ls_solve_robust.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LsRobust), C.POINTER(LsDamping), C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_double_p, c_double_p]
lib.stmmqr_ls_robust_times.argtypes = [C.c_void_p, c_double_p]
_ROBUST_STAT = ["sigma", "lo", "hi", "count", "loss", "rejected", "unit", "flags"]
_ROBUST_INFO = ["solves", "converged", "step_ratio", "sigma", "loss", "rejected", "ms_reweight", "robust_bytes"]


def median_abs(v, mask=None, device=-1):
    """the exact median of |v| (mask None) or of |mask * v| over the entries with mask != 0, found on the device by a radix select
    (stmmqr_median_abs) -> {"median": 0.5 * (lo + hi), "lo", "hi", "count"}; all 0 for no entry"""
    v = np.ascontiguousarray(v, np.float64).reshape(-1)
    if mask is not None:
        mask = np.ascontiguousarray(mask, np.float64).reshape(-1)
        if mask.size != v.size:
            raise StmmqrError("median_abs: mask must hold one value per entry of v")
    out = np.zeros(4)
    _check(lib.stmmqr_median_abs(v.ctypes.data if v.size else None, None if mask is None else mask.ctypes.data, v.size, int(device), 0,
                                 out.ctypes.data), "stmmqr_median_abs")
    return {"median": float(out[0]), "lo": float(out[1]), "hi": float(out[2]), "count": int(out[3])}


def median_abs_dev(v_ptr: int, length: int, out_ptr: int, mask_ptr=None, device=-1):
    """device pointers: v [length], mask [length] or None, out [4] receives the median, lo, hi and the count"""
    _check(lib.stmmqr_median_abs(C.c_void_p(int(v_ptr)), None if mask_ptr is None else C.c_void_p(int(mask_ptr)), int(length), int(device),
                                 1, C.c_void_p(int(out_ptr))), "stmmqr_median_abs")


def _robust_rule(loss, cc, sigma, mad_factor, sigma_min, w0_ptr):
    if isinstance(loss, str):
        if loss not in ROBUST_LOSSES:
            raise StmmqrError(f"robust fit: unknown loss {loss!r} (one of {sorted(ROBUST_LOSSES)})")
        loss = ROBUST_LOSSES[loss]
    return LsRobust(int(loss), 0.0 if cc is None else float(cc), float(sigma), float(mad_factor), float(sigma_min), w0_ptr)


def _robust_info(info, hist, resid=None):
    d = dict(zip(_ROBUST_INFO, info.tolist()))
    d["solves"], d["converged"] = int(d["solves"]), bool(d["converged"])
    d["hist"] = hist[:d["solves"]].copy()                  # per solve: sigma, loss, step, resid
    if resid is not None:
        d["resid"] = float(resid[0])
    return d



def _adjoint_info(v):
    return dict(zip(_ADJOINT_INFO, v[:6].tolist()))


class LeastSquares:
    """min |A x - b| for nrhs right-hand sides with the right-hand sides carried through the factorization (stmmqr_ls_*): the
    columns of A are ordered as SparseQR orders them, [A B] is analysed once and factorized with ntol = n at every solve, and
    x = E R11^-1 C comes from R alone -- Q is never stored (an R-only plan).  Column singletons are not removed in this mode.
    solve() may be called again with new values and a new B (a Gauss-Newton loop): nothing is analysed or planned again.
    symbolic_only=True stops after the host half (no GPU needed)."""

    _create = "stmmqr_ls_create"

    def __init__(self, m, n, Ap, Ai, Ax, nrhs=1, ordering=7, tol=-2.0, relax: Relax | None = None, Quser=None, device=-1,
                 symbolic_only=False):
        self.m, self.n, self.nrhs = int(m), int(n), int(nrhs)
        Ap = np.ascontiguousarray(Ap, I64); Ai = np.ascontiguousarray(Ai, I64); Ax = np.ascontiguousarray(Ax, np.float64)
        Q = None if Quser is None else np.ascontiguousarray(Quser, I64)
        if Q is not None and Q.size != self.n:
            raise StmmqrError("LeastSquares: Quser must hold one entry per column of A")
        self.anz = int(Ap[-1])
        self._h = C.c_void_p()
        _check(getattr(lib, self._create)(int(ordering), float(tol), self.m, self.n, _ip(Ap), _ip(Ai), _dp(Ax), self.nrhs, _ip(Q),
                                          None if relax is None else C.byref(relax), -2 if symbolic_only else int(device),
                                          C.byref(self._h)), self._create)

    def close(self):
        if getattr(self, "_h", None):
            lib.stmmqr_ls_free(self._h)
            self._h = None

    __del__ = close

    def symbolic(self) -> dict:
        """the qr_symbolic of [A B] (n = columns of A + nrhs; Qfill = A's order, then the identity)"""
        S = lib.stmmqr_ls_symbolic_view(self._h).contents
        return _symbolic_dict(S, S.m, S.n)

    def plan(self) -> HipQR:
        """the R-only device plan of [A B] as a HipQR (borrowed: valid until close(); download / rsolve / solve_carried / device_bytes)"""
        h = lib.stmmqr_ls_plan(self._h)
        if not h:
            raise StmmqrError("LeastSquares.plan: the object holds the host half only")
        S = lib.stmmqr_ls_symbolic_view(self._h).contents
        p = HipQR.__new__(HipQR)
        p._keep, p._borrowed, p._h = {}, True, h
        p.sym = {k: int(getattr(S, k)) for k in ["m", "n", "anz", "nf", "maxfn", "rjsize", "hisize"]}
        return p

    @property
    def dims(self) -> dict:
        """m and n of A, nrhs, and whether the object is a damped one (stmmqr_ls_dims)"""
        v = np.zeros(4, I64)
        _check(lib.stmmqr_ls_dims(self._h, _ip(v)), "stmmqr_ls_dims")
        return {"m": int(v[0]), "n": int(v[1]), "nrhs": int(v[2]), "damped": bool(v[3])}

    @property
    def info(self) -> dict:
        v = np.zeros(14)
        _check(lib.stmmqr_ls_info(self._h, _dp(v)), "stmmqr_ls_info")
        keys = ["rank", "nf", "flops", "flop_bound", "ms_factorize", "ms_solve", "device_bytes", "retries", "reschedules", "analyses",
                "plans", "solves", "tol", "nrhs"]
        return dict(zip(keys, v.tolist()))

    def solve(self, B, Ax=None):
        """-> (X, resid): X n x nrhs (a vector for a vector B), resid[j] = |b_j - A x_j|_2.  Ax: new values of A (same pattern)."""
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(self.m, -1, order="F")
        if Bf.shape[1] != self.nrhs:
            raise StmmqrError(f"LeastSquares.solve: B has {Bf.shape[1]} columns, the object was created for {self.nrhs}")
        if Ax is not None:
            Ax = np.ascontiguousarray(Ax, np.float64)
            if Ax.size != self.anz:
                raise StmmqrError("LeastSquares.solve: Ax must hold one value per entry of A's pattern")
        X = np.zeros((self.n, self.nrhs), order="F")
        resid = np.zeros(self.nrhs)
        _check(lib.stmmqr_ls_solve(self._h, None if Ax is None else Ax.ctypes.data, 0, Bf.ctypes.data, max(self.m, 1), X.ctypes.data,
                                   max(self.n, 1), resid.ctypes.data, 0), "stmmqr_ls_solve")
        return (X[:, 0] if np.ndim(B) == 1 else X), resid

    def solve_dev(self, b_ptr: int, x_ptr: int, ax_ptr: int | None = None, resid=True):
        """device pointers: B (m x nrhs, ld m), X (n x nrhs, ld n), optionally A's values.  resid: True -> the residual norms as a
        numpy array, an int -> a device pointer that receives them (returns None), False / None -> not asked for."""
        rd = None if resid is True or resid in (False, None) else C.c_void_p(int(resid))
        _check(lib.stmmqr_ls_solve(self._h, None if ax_ptr is None else C.c_void_p(int(ax_ptr)), 1, C.c_void_p(int(b_ptr)), max(self.m, 1),
                                   C.c_void_p(int(x_ptr)), max(self.n, 1), rd, 1), "stmmqr_ls_solve")
        if resid is True:
            out = np.zeros(self.nrhs)
            _check(lib.stmmqr_ls_resid(self._h, _dp(out)), "stmmqr_ls_resid")
            return out
        return None

    def _adjoint_in(self, what, X, Xbar):
        n, k = max(self.n, 1), self.nrhs
        out = []
        for name, a in (("X", X), ("Xbar", Xbar)):
            a = np.asarray(a, np.float64)
            if a.size != self.n * k:
                raise StmmqrError(f"{what}: {name} must hold n x nrhs = {self.n} x {k} values")
            f = np.zeros((n, k), order="F")
            f[:self.n] = a.reshape(self.n, k)
            out.append(f)
        return out

    def adjoint(self, X, Xbar, refine=1):
        """after solve(): the backward pass of that solve (stmmqr_ls_adjoint).  X: the solution it returned, Xbar = dL/dX, both n x nrhs
        (or vectors).  -> (Axbar [anz], the gradient on A's pattern; Bbar, shaped as B was; info).  Dead columns: exactly 0."""
        Xf, Xb = self._adjoint_in("LeastSquares.adjoint", X, Xbar)
        Axbar, Bbar, info = np.zeros(max(self.anz, 1)), np.zeros((max(self.m, 1), self.nrhs), order="F"), np.zeros(8)
        _check(lib.stmmqr_ls_adjoint(self._h, Xf.ctypes.data, max(self.n, 1), Xb.ctypes.data, max(self.n, 1), None, int(refine),
                                     Axbar.ctypes.data, Bbar.ctypes.data, max(self.m, 1), None, None, 0, _dp(info)), "stmmqr_ls_adjoint")
        Bbar = Bbar[:self.m]
        return Axbar[:self.anz], (Bbar[:, 0] if np.ndim(X) == 1 else Bbar), _adjoint_info(info)

    def adjoint_dev(self, x_ptr: int, xbar_ptr: int, axbar_ptr=None, bbar_ptr=None, refine=1) -> dict:
        """device pointers: X and Xbar (n x nrhs, ld n); where Axbar [anz] and Bbar (m x nrhs, ld m) go, None = not asked for.
        Returns info."""
        vp = lambda p: None if p is None else C.c_void_p(int(p))                                             # noqa: E731
        info = np.zeros(8)
        _check(lib.stmmqr_ls_adjoint(self._h, vp(x_ptr), max(self.n, 1), vp(xbar_ptr), max(self.n, 1), None, int(refine), vp(axbar_ptr),
                                     vp(bbar_ptr), max(self.m, 1), None, None, 1, _dp(info)), "stmmqr_ls_adjoint")
        return _adjoint_info(info)

    def adjoint_z(self, dev_ptr=None):
        """after adjoint(): its z = (C'C)^-1 xbar, n x nrhs, zero on dead columns (stmmqr_ls_adjoint_z).  dev_ptr: a device pointer
        that receives it with leading dimension n (returns None)."""
        if dev_ptr is not None:
            _check(lib.stmmqr_ls_adjoint_z(self._h, C.c_void_p(int(dev_ptr)), max(self.n, 1), 1), "stmmqr_ls_adjoint_z")
            return None
        Z = np.zeros((max(self.n, 1), self.nrhs), order="F")
        _check(lib.stmmqr_ls_adjoint_z(self._h, Z.ctypes.data, max(self.n, 1), 0), "stmmqr_ls_adjoint_z")
        return Z[:self.n]

    def variances(self, dev_ptr=None):
        """after solve(): diag((A_live' A_live)^-1) in A's column order, 0 for dead columns (stmmqr_ls_covariance_diag).  dev_ptr: a
        device pointer that receives the n doubles (returns None)."""
        if dev_ptr is not None:
            _check(lib.stmmqr_ls_covariance_diag(self._h, C.c_void_p(int(dev_ptr)), 1), "stmmqr_ls_covariance_diag")
            return None
        var = np.zeros(max(self.n, 1))
        _check(lib.stmmqr_ls_covariance_diag(self._h, var.ctypes.data, 0), "stmmqr_ls_covariance_diag")
        return var[:self.n]

    def condest(self, kind: int = 1, iters: int = 0, with_vector: bool = False) -> dict:
        """after solve(): the condition of A(:, live) from the R the object holds (stmmqr_ls_condest; HipQR.condest with ncol = n)"""
        return _condest_dict(lambda out, v: lib.stmmqr_ls_condest(self._h, int(kind), int(iters), out, v, 0), "stmmqr_ls_condest", self.n,
                             with_vector)

    def r_sparse(self, form: str = "csc", ncol=None, econ=None, device: bool = False):
        """after solve(): R of A -- the leading n columns of the R of [A B] the object holds (HipQR.r_sparse, ncol = n by default) -- in
        the column order of the factorization"""
        S = lib.stmmqr_ls_symbolic_view(self._h).contents
        return _r_sparse(lib.stmmqr_ls_plan(self._h), int(S.m), int(S.n), form, self.n if ncol is None else ncol, econ, device)

    def nullspace(self) -> np.ndarray:
        """after solve(): the null vectors of A as the rank test saw it, n x d in A's column order (stmmqr_ls_nullspace; HipQR.nullspace
        with ncol = n)"""
        return _nullspace_array(lambda nd, N, ld: lib.stmmqr_ls_nullspace(self._h, nd, N, ld, 0), "stmmqr_ls_nullspace", self.n)

    def project_minnorm(self, X, with_info: bool = False):
        """after solve(): the minimum-norm solution from the basic one that solve() returns (X of n rows; stmmqr_ls_project_minnorm).
        The residuals do not change."""
        return _project(lambda Xp, ld, k, info: lib.stmmqr_ls_project_minnorm(self._h, Xp, ld, k, 0, info), "stmmqr_ls_project_minnorm",
                        X, self.n, with_info)

    def diagnostics(self):
        """after solve(): (leverages, variances) from ONE selected inversion (stmmqr_ls_leverage): the leverages of the m rows of A
        and the bits of variances()."""
        lev, var = np.zeros(max(self.m, 1)), np.zeros(max(self.n, 1))
        _check(lib.stmmqr_ls_leverage(self._h, lev.ctypes.data, var.ctypes.data, 0), "stmmqr_ls_leverage")
        return lev[:self.m], var[:self.n]

    def leverages(self, dev_ptr=None):
        """after solve(): h_i = a_i' (A_live' A_live)^-1 a_i for the m rows of A, the diagonal of the hat matrix (0 <= h_i <= 1, their sum
        is the rank).  dev_ptr: a device pointer that receives the m doubles (returns None)."""
        if dev_ptr is not None:
            _check(lib.stmmqr_ls_leverage(self._h, C.c_void_p(int(dev_ptr)), None, 1), "stmmqr_ls_leverage")
            return None
        lev = np.zeros(max(self.m, 1))
        _check(lib.stmmqr_ls_leverage(self._h, lev.ctypes.data, None, 0), "stmmqr_ls_leverage")
        return lev[:self.m]

    def covariance(self, I, J) -> np.ndarray:
        """after solve(): the entries (I[p], J[p]) of (A_live' A_live)^-1, A's column order; pairs outside the pattern of the selected
        inverse are refused (stmmqr_ls_covariance_entries).  The correlation of x_i and x_j is cov(i, j) / sqrt(var_i var_j)."""
        I = np.ascontiguousarray(I, I64).reshape(-1); J = np.ascontiguousarray(J, I64).reshape(-1)
        if I.size != J.size:
            raise StmmqrError("LeastSquares.covariance: I and J must have the same length")
        out = np.zeros(max(I.size, 1))
        _check(lib.stmmqr_ls_covariance_entries(self._h, I.size, I.ctypes.data, J.ctypes.data, out.ctypes.data, 0),
               "stmmqr_ls_covariance_entries")
        return out[:I.size]

    def _vec(self, what, name, a, size):
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        if a.size != size:
            raise StmmqrError(f"{what}: {name} must hold {size} values")
        return a

    def robust_weights(self, B, X, loss="huber", cc=None, sigma=0.0, w0=None, mad_factor=0.0, sigma_min=0.0, Ax=None):
        """one reweighting of a robust fit from a given x (stmmqr_ls_robust_weights; nrhs must be 1) -> (r, w, stat): the unweighted
        residual b - A x, the row multipliers w = w0 * f(|w0 r| / sigma), and sigma, lo, hi, count, loss, rejected, unit, flags.
        sigma = 0: mad_factor * median |w0 r| over w0 != 0, floored at sigma_min."""
        what = type(self).__name__ + ".robust_weights"
        keep = {"B": self._vec(what, "B", B, self.m), "X": self._vec(what, "X", X, self.n)}
        if w0 is not None:
            keep["w0"] = self._vec(what, "w0", w0, self.m)
        if Ax is not None:
            keep["Ax"] = self._vec(what, "Ax", Ax, self.anz)
        ptr = lambda k: keep[k].ctypes.data if k in keep else None                                           # noqa: E731
        rb = _robust_rule(loss, cc, sigma, mad_factor, sigma_min, ptr("w0"))
        r, w, stat = np.zeros(max(self.m, 1)), np.zeros(max(self.m, 1)), np.zeros(8)
        _check(lib.stmmqr_ls_robust_weights(self._h, ptr("Ax"), 0, C.byref(rb), ptr("B"), ptr("X"), r.ctypes.data, w.ctypes.data, 0,
                                            _dp(stat)), "stmmqr_ls_robust_weights")
        return r[:self.m], w[:self.m], dict(zip(_ROBUST_STAT, stat.tolist()))

    def robust_weights_dev(self, b_ptr: int, x_ptr: int, r_ptr=None, w_ptr=None, loss="huber", cc=None, sigma=0.0, w0_ptr=None,
                           mad_factor=0.0, sigma_min=0.0, ax_ptr=None) -> dict:
        """device pointers: B [m], X [n], optionally w0 [m] and A's values; where r [m] and w [m] go, None = not asked for.  Returns stat."""
        vp = lambda p: None if p is None else C.c_void_p(int(p))                                             # noqa: E731
        rb = _robust_rule(loss, cc, sigma, mad_factor, sigma_min, None if w0_ptr is None else int(w0_ptr))
        stat = np.zeros(8)
        _check(lib.stmmqr_ls_robust_weights(self._h, vp(ax_ptr), 1, C.byref(rb), vp(b_ptr), vp(x_ptr), vp(r_ptr), vp(w_ptr), 1, _dp(stat)),
               "stmmqr_ls_robust_weights")
        return dict(zip(_ROBUST_STAT, stat.tolist()))

    def robust_times(self) -> dict:
        """device ms of the last reweighting: residual, selection, weights, and their sum (stmmqr_ls_robust_times)"""
        v = np.zeros(4)
        _check(lib.stmmqr_ls_robust_times(self._h, _dp(v)), "stmmqr_ls_robust_times")
        return dict(zip(["residual", "selection", "weights", "total"], v.tolist()))

    def _solve_robust(self, dmp, keep, B, loss, cc, sigma, w0, x0, max_iter, rtol, sigma_iters, Ax, mad_factor, sigma_min):
        what = type(self).__name__ + ".solve_robust"
        keep["B"] = self._vec(what, "B", B, self.m)
        for name, a, size in (("w0", w0, self.m), ("x0", x0, self.n), ("Ax", Ax, self.anz)):
            if a is not None:
                keep[name] = self._vec(what, name, a, size)
        ptr = lambda k: keep[k].ctypes.data if k in keep else None                                           # noqa: E731
        rb = _robust_rule(loss, cc, sigma, mad_factor, sigma_min, ptr("w0"))
        X, w, resid = np.zeros(max(self.n, 1)), np.zeros(max(self.m, 1)), np.zeros(1)
        hist, info = np.zeros((max(int(max_iter), 1), 4)), np.zeros(8)
        _check(lib.stmmqr_ls_solve_robust(self._h, ptr("Ax"), 0, C.byref(rb), None if dmp is None else C.byref(dmp), ptr("B"), ptr("x0"),
                                          int(max_iter), float(rtol), int(sigma_iters), X.ctypes.data, w.ctypes.data, resid.ctypes.data, 0,
                                          _dp(hist), _dp(info)), "stmmqr_ls_solve_robust")
        return X[:self.n], w[:self.m], _robust_info(info, hist, resid)

    def _solve_robust_dev(self, dmp, b_ptr, x_ptr, w_ptr, loss, cc, sigma, w0_ptr, x0_ptr, max_iter, rtol, sigma_iters, ax_ptr, mad_factor,
                          sigma_min, resid_ptr):
        vp = lambda p: None if p is None else C.c_void_p(int(p))                                             # noqa: E731
        rb = _robust_rule(loss, cc, sigma, mad_factor, sigma_min, None if w0_ptr is None else int(w0_ptr))
        hist, info = np.zeros((max(int(max_iter), 1), 4)), np.zeros(8)
        _check(lib.stmmqr_ls_solve_robust(self._h, vp(ax_ptr), 1, C.byref(rb), None if dmp is None else C.byref(dmp), vp(b_ptr), vp(x0_ptr),
                                          int(max_iter), float(rtol), int(sigma_iters), vp(x_ptr), vp(w_ptr), vp(resid_ptr), 1, _dp(hist),
                                          _dp(info)), "stmmqr_ls_solve_robust")
        return _robust_info(info, hist)

    def solve_robust(self, B, loss="huber", cc=None, sigma=0.0, w0=None, x0=None, max_iter=50, rtol=1e-8, sigma_iters=-1, Ax=None,
                     mad_factor=0.0, sigma_min=0.0):
        """a robust fit by iteratively reweighted solves, everything between two solves on the device (stmmqr_ls_solve_robust; nrhs
        must be 1) -> (X, w, info): the solution, the row multipliers of the last solve, and solves, converged, step_ratio, sigma,
        loss, rejected, ms_reweight, robust_bytes, resid and hist (per solve: sigma, loss, step, resid).  loss: "l2", "huber",
        "cauchy", "tukey", "l1" (or 0 .. 4); cc None: the default of the loss; sigma = 0: the MAD of the residuals, re-estimated in
        the first sigma_iters reweightings (< 0: always); w0: prior row multipliers; x0: where the first weights come from (None: the
        L2 start).  Every solve is solve(w * b, Ax = w[Ai] * Ax): afterwards the object's values are weighted ones."""
        return self._solve_robust(None, {}, B, loss, cc, sigma, w0, x0, max_iter, rtol, sigma_iters, Ax, mad_factor, sigma_min)

    def solve_robust_dev(self, b_ptr: int, x_ptr: int, w_ptr=None, loss="huber", cc=None, sigma=0.0, w0_ptr=None, x0_ptr=None, max_iter=50,
                         rtol=1e-8, sigma_iters=-1, ax_ptr=None, mad_factor=0.0, sigma_min=0.0, resid_ptr=None) -> dict:
        """device pointers: B [m], where X [n] and w [m] go, optionally w0 [m], x0 [n], A's values, resid [1].  Returns info."""
        return self._solve_robust_dev(None, b_ptr, x_ptr, w_ptr, loss, cc, sigma, w0_ptr, x0_ptr, max_iter, rtol, sigma_iters, ax_ptr,
                                      mad_factor, sigma_min, resid_ptr)

    def std_errors(self) -> np.ndarray:
        """after solve(): the standard errors of x, n x nrhs: sqrt(var * resid_j^2 / (m - rank)) for right-hand side j; inf where
        m == rank (no degree of freedom left)."""
        var = self.variances()
        resid = np.zeros(self.nrhs)
        _check(lib.stmmqr_ls_resid(self._h, _dp(resid)), "stmmqr_ls_resid")
        dof = self.m - int(self.info["rank"])
        if dof <= 0:
            return np.full((self.n, self.nrhs), np.inf)
        return np.sqrt(var[:, None] * (resid[None, :] ** 2 / dof))


class DampedLeastSquares(LeastSquares):
    """min |W (A x - b)|^2 + |D x|^2 with W = diag(w) and D = diag(sqrt(lam) * s) (stmmqr_ls_create_damped / stmmqr_ls_solve_damped):
    Levenberg-Marquardt and trust-region steps, ridge regression, reweighted fits.  The columns of A are ordered as LeastSquares orders
    them, [A; I | B; 0] is analysed once, and every solve() builds the values of [W A; D | W B; 0] on the device and factorizes them:
    w, D, A's values and B may all change from call to call, nothing is analysed or planned again.  The object is the LeastSquares of
    that (m + n) x n matrix, so after a solve variances() is diag((A'W^2 A + D^2)^-1), leverages() has m + n entries (the first m: the
    diagonal of the ridge hat matrix, their sum the effective degrees of freedom) and condest() is the condition of [W A; D]."""

    _create = "stmmqr_ls_create_damped"

    def _damping(self, w, d, lam, scale, scale_min, scale_max, D_out, dnorm):
        return LsDamping(w, d, float(lam), int(scale), float(scale_min), float(scale_max), D_out, dnorm)

    @property
    def damped_info(self) -> dict:
        v = np.zeros(2)
        _check(lib.stmmqr_ls_damped_info(self._h, _dp(v)), "stmmqr_ls_damped_info")
        return {"ms_build": float(v[0]), "damped_bytes": float(v[1])}

    def solve(self, B, Ax=None, w=None, d=None, lam=0.0, scale=0, scale_min=1e-6, scale_max=1e32):
        """-> (X, resid, dnorm, D): X n x nrhs (a vector for a vector B), resid[j] = sqrt(|W (b_j - A x_j)|^2 + |D x_j|^2),
        dnorm[j] = |D x_j|, D [n] the diagonal used.  Ax: new values of A (same pattern); w [m] row weights; d [n] column scales s_j, or
        scale = 0 (s_j = 1) / 1 (s_j = |W A(:,j)| clamped to [scale_min, scale_max]); D_jj = sqrt(lam) * s_j."""
        Bf = np.array(B, dtype=np.float64, order="F", copy=True).reshape(self.m, -1, order="F")
        if Bf.shape[1] != self.nrhs:
            raise StmmqrError(f"DampedLeastSquares.solve: B has {Bf.shape[1]} columns, the object was created for {self.nrhs}")
        keep = {}
        for name, a, size in (("Ax", Ax, self.anz), ("w", w, self.m), ("d", d, self.n)):
            if a is not None:
                keep[name] = np.ascontiguousarray(a, np.float64).reshape(-1)
                if keep[name].size != size:
                    raise StmmqrError(f"DampedLeastSquares.solve: {name} must hold {size} values")
        ptr = lambda k: keep[k].ctypes.data if k in keep else None                                           # noqa: E731
        X = np.zeros((max(self.n, 1), self.nrhs), order="F")
        resid, dnorm, D = np.zeros(self.nrhs), np.zeros(self.nrhs), np.zeros(max(self.n, 1))
        dmp = self._damping(ptr("w"), ptr("d"), lam, scale, scale_min, scale_max, D.ctypes.data, dnorm.ctypes.data)
        _check(lib.stmmqr_ls_solve_damped(self._h, ptr("Ax"), 0, C.byref(dmp), Bf.ctypes.data, max(self.m, 1), X.ctypes.data, max(self.n, 1),
                                          resid.ctypes.data, 0), "stmmqr_ls_solve_damped")
        X = X[:self.n]
        return (X[:, 0] if np.ndim(B) == 1 else X), resid, dnorm, D[:self.n]

    def solve_dev(self, b_ptr: int, x_ptr: int, ax_ptr=None, w_ptr=None, d_ptr=None, lam=0.0, scale=0, scale_min=1e-6, scale_max=1e32,
                  resid_ptr=None, dnorm_ptr=None, D_ptr=None):
        """device pointers for every array: B (m x nrhs, ld m), X (n x nrhs, ld n), optionally A's values, w [m], d [n], and where
        resid [nrhs], dnorm [nrhs] and D [n] go.  Returns the residual norms as a numpy array (stmmqr_ls_resid)."""
        vp = lambda p: None if p is None else C.c_void_p(int(p))                                             # noqa: E731
        dmp = self._damping(vp(w_ptr), vp(d_ptr), lam, scale, scale_min, scale_max, vp(D_ptr), vp(dnorm_ptr))
        _check(lib.stmmqr_ls_solve_damped(self._h, vp(ax_ptr), 1, C.byref(dmp), vp(b_ptr), max(self.m, 1), vp(x_ptr), max(self.n, 1),
                                          vp(resid_ptr), 1), "stmmqr_ls_solve_damped")
        out = np.zeros(self.nrhs)
        _check(lib.stmmqr_ls_resid(self._h, _dp(out)), "stmmqr_ls_resid")
        return out

    def adjoint(self, X, Xbar, w=None, refine=1):
        """after solve(): the backward pass of that solve (stmmqr_ls_adjoint).  X: the solution it returned, Xbar = dL/dX, w: the
        weights of that solve (None: all 1).  -> (Axbar [anz], Bbar as B was shaped, wbar [m], Dbar [n], info); Dbar is the gradient
        for the D_jj used: dbar = sqrt(lam) * Dbar, lambdabar = sum_j s_j Dbar_j / (2 sqrt(lam)) (autograd.py has the form that is
        finite at lam = 0)."""
        Xf, Xb = self._adjoint_in("DampedLeastSquares.adjoint", X, Xbar)
        wf = None
        if w is not None:
            wf = np.ascontiguousarray(w, np.float64).reshape(-1)
            if wf.size != self.m:
                raise StmmqrError(f"DampedLeastSquares.adjoint: w must hold {self.m} values")
        Axbar, Bbar = np.zeros(max(self.anz, 1)), np.zeros((max(self.m, 1), self.nrhs), order="F")
        wbar, Dbar, info = np.zeros(max(self.m, 1)), np.zeros(max(self.n, 1)), np.zeros(8)
        _check(lib.stmmqr_ls_adjoint(self._h, Xf.ctypes.data, max(self.n, 1), Xb.ctypes.data, max(self.n, 1),
                                     None if wf is None else wf.ctypes.data, int(refine), Axbar.ctypes.data, Bbar.ctypes.data, max(self.m, 1),
                                     wbar.ctypes.data, Dbar.ctypes.data, 0, _dp(info)), "stmmqr_ls_adjoint")
        Bbar = Bbar[:self.m]
        return Axbar[:self.anz], (Bbar[:, 0] if np.ndim(X) == 1 else Bbar), wbar[:self.m], Dbar[:self.n], _adjoint_info(info)

    def adjoint_dev(self, x_ptr: int, xbar_ptr: int, w_ptr=None, axbar_ptr=None, bbar_ptr=None, wbar_ptr=None, dbar_ptr=None,
                    refine=1) -> dict:
        """device pointers for every array: X and Xbar (n x nrhs, ld n), w [m] of the solve; where Axbar [anz], Bbar (m x nrhs, ld m),
        wbar [m] and Dbar [n] go, None = not asked for.  Returns info."""
        vp = lambda p: None if p is None else C.c_void_p(int(p))                                             # noqa: E731
        info = np.zeros(8)
        _check(lib.stmmqr_ls_adjoint(self._h, vp(x_ptr), max(self.n, 1), vp(xbar_ptr), max(self.n, 1), vp(w_ptr), int(refine),
                                     vp(axbar_ptr), vp(bbar_ptr), max(self.m, 1), vp(wbar_ptr), vp(dbar_ptr), 1, _dp(info)),
               "stmmqr_ls_adjoint")
        return _adjoint_info(info)

    def diagnostics(self):
        """after solve(): (leverages [m + n], variances [n]) from ONE selected inversion (stmmqr_ls_leverage)"""
        lev, var = np.zeros(max(self.m + self.n, 1)), np.zeros(max(self.n, 1))
        _check(lib.stmmqr_ls_leverage(self._h, lev.ctypes.data, var.ctypes.data, 0), "stmmqr_ls_leverage")
        return lev[:self.m + self.n], var[:self.n]

    def leverages(self, dev_ptr=None):
        """after solve(): the m + n leverages of the rows of [W A; D].  The first m are the diagonal of the ridge hat matrix
        W A (A'W^2 A + D^2)^-1 A'W, whose sum is the effective degrees of freedom; all m + n sum to the number of live columns.
        dev_ptr: a device pointer that receives the m + n doubles (returns None)."""
        if dev_ptr is not None:
            _check(lib.stmmqr_ls_leverage(self._h, C.c_void_p(int(dev_ptr)), None, 1), "stmmqr_ls_leverage")
            return None
        lev = np.zeros(max(self.m + self.n, 1))
        _check(lib.stmmqr_ls_leverage(self._h, lev.ctypes.data, None, 0), "stmmqr_ls_leverage")
        return lev[:self.m + self.n]

    def solve_robust(self, B, loss="huber", cc=None, sigma=0.0, w0=None, x0=None, max_iter=50, rtol=1e-8, sigma_iters=-1, Ax=None,
                     mad_factor=0.0, sigma_min=0.0, d=None, lam=0.0, scale=0, scale_min=1e-6, scale_max=1e32):
        """LeastSquares.solve_robust with the damping of solve(): every solve is solve(w=...) with the device's multipliers.  info also
        holds dnorm and D of the last solve."""
        keep = {}
        if d is not None:
            keep["d"] = self._vec("DampedLeastSquares.solve_robust", "d", d, self.n)
        dnorm, D = np.zeros(1), np.zeros(max(self.n, 1))
        dmp = self._damping(None, keep["d"].ctypes.data if d is not None else None, lam, scale, scale_min, scale_max, D.ctypes.data,
                            dnorm.ctypes.data)
        X, w, info = self._solve_robust(dmp, keep, B, loss, cc, sigma, w0, x0, max_iter, rtol, sigma_iters, Ax, mad_factor, sigma_min)
        info["dnorm"], info["D"] = float(dnorm[0]), D[:self.n]
        return X, w, info

    def solve_robust_dev(self, b_ptr: int, x_ptr: int, w_ptr=None, loss="huber", cc=None, sigma=0.0, w0_ptr=None, x0_ptr=None, max_iter=50,
                         rtol=1e-8, sigma_iters=-1, ax_ptr=None, mad_factor=0.0, sigma_min=0.0, resid_ptr=None, d_ptr=None, lam=0.0,
                         scale=0, scale_min=1e-6, scale_max=1e32, dnorm_ptr=None, D_ptr=None) -> dict:
        """device pointers for every array, the damping's d [n], dnorm [1] and D [n] included.  Returns info."""
        vp = lambda p: None if p is None else int(p)                                                          # noqa: E731
        dmp = self._damping(None, vp(d_ptr), lam, scale, scale_min, scale_max, vp(D_ptr), vp(dnorm_ptr))
        return self._solve_robust_dev(dmp, b_ptr, x_ptr, w_ptr, loss, cc, sigma, w0_ptr, x0_ptr, max_iter, rtol, sigma_iters, ax_ptr,
                                      mad_factor, sigma_min, resid_ptr)

    def std_errors(self):
        raise StmmqrError("DampedLeastSquares.std_errors: not defined for a damped fit (use variances() and the residuals)")


def read_matrix_market(path):
    """The driver's Matrix Market reader (SparseCore_read_matrix with prefer = 1, qrtest.c:112): (m, n, Ap, Ai, Ax) of the
    unsymmetric CSC with both triangles."""
    m, n, nz = C.c_long(0), C.c_long(0), C.c_long(0)
    pp, pi, px = c_long_p(), c_long_p(), c_double_p()
    lib.stmmqr_mm_last_error.restype = C.c_char_p
    rc = lib.stmmqr_read_matrix_market(str(path).encode(), C.byref(m), C.byref(n), C.byref(nz), C.byref(pp), C.byref(pi), C.byref(px))
    if rc != 0:
        raise StmmqrError(f"stmmqr_read_matrix_market({path}): {lib.stmmqr_mm_last_error().decode()}")
    try:
        Ap = np.ctypeslib.as_array(pp, shape=(n.value + 1,)).copy()
        Ai = np.ctypeslib.as_array(pi, shape=(max(nz.value, 1),))[:nz.value].copy()
        Ax = np.ctypeslib.as_array(px, shape=(max(nz.value, 1),))[:nz.value].copy()
    finally:
        lib.stmmqr_free.argtypes = [C.c_void_p]
        for q in (pp, pi, px):
            lib.stmmqr_free(C.cast(q, C.c_void_p))
    return m.value, n.value, Ap, Ai, Ax


def qr_fsize(f, Super, Rp, Rj, Sleft, Child, Childp, Cm, Fmap, Stair):
    """qr_fsize (SparseQR.h:159-176 / SparseQR_factorize.c:1066-1145): Fmap and Stair are written; returns fm"""
    a = [np.ascontiguousarray(x, I64) for x in (Super, Rp, Rj, Sleft, Child, Childp, Cm)]
    assert Fmap.dtype == I64 and Stair.dtype == I64
    lib.qr_fsize.restype = C.c_long
    return int(lib.qr_fsize(C.c_long(int(f)), *[_ip(x) for x in a], _ip(Fmap), _ip(Stair)))


def qr_stranspose2(m, n, Ap, Ai, Ax, Qfill, Sp, PLinv):
    """qr_stranspose2 (SparseQR_factorize.c:755-785): returns Sx, the values of S = A(P,Q) in row form"""
    Ap = np.ascontiguousarray(Ap, I64); Ai = np.ascontiguousarray(Ai, I64); Ax = np.ascontiguousarray(Ax, np.float64)
    Sp = np.ascontiguousarray(Sp, I64); PLinv = np.ascontiguousarray(PLinv, I64)
    Qf = None if Qfill is None else np.ascontiguousarray(Qfill, I64)
    A = SparseCsc(m, n, Ax.size, Ap.ctypes.data, Ai.ctypes.data, None, Ax.ctypes.data, None, 0, 2, 1, 0, 1, 1)
    Sx = np.zeros(max(Ax.size, 1)); W = np.zeros(max(m, 1), I64)
    lib.qr_stranspose2.restype = None
    lib.qr_stranspose2(C.byref(A), _ip(Qf), _ip(Sp), _ip(PLinv), _dp(Sx), _ip(W))
    return Sx[:Ax.size]


def qr_hpinv(sym: dict, Hm, Hr, Hii):
    """qr_hpinv (SparseQR_factorize.c:991-1060): Hii is rewritten in place; returns (HPinv, maxfm)"""
    keep = {k: np.ascontiguousarray(sym[k], I64) for k in ("Sleft", "Super", "Rp", "Hip", "PLinv")}
    S = QrSymbolicC()
    S.m, S.n, S.nf = int(sym["m"]), int(sym["n"]), int(sym["nf"])
    for k, a in keep.items():
        setattr(S, k, _ip(a))
    Hm = np.ascontiguousarray(Hm, I64); Hr = np.ascontiguousarray(Hr, I64)
    assert Hii.dtype == I64 and Hii.flags.c_contiguous
    HPinv = np.zeros(max(S.m, 1), I64); W = np.zeros(max(S.m, 1), I64)
    N = QrNumericC()
    N.m, N.n, N.nf = S.m, S.n, S.nf
    N.Hm, N.Hr, N.Hii, N.HPinv = _ip(Hm), _ip(Hr), _ip(Hii), _ip(HPinv)
    lib.qr_hpinv.restype = None
    lib.qr_hpinv(C.byref(S), C.byref(N), _ip(W))
    return HPinv[:S.m], int(N.maxfm)


def qr_assemble(f, fm, Super, Rp, Rj, Sp, Sj, Sleft, Child, Childp, Sx, Fmap, Cm, Cblocks: dict, Hr, Stair, Hii, Hip):
    """qr_assemble (SparseQR.h:178-200).  Cblocks: {child: packed C array}.  Returns (F, Cmap); Stair/Hii in place."""
    nf = len(Rp) - 1
    fn = int(Rp[f + 1] - Rp[f])
    F = np.zeros((fm, fn), order="F")
    Cmap = np.zeros(max(fn, 1), I64)
    ptrs = (c_double_p * (nf + 1))()
    keep = {}
    for c, a in Cblocks.items():
        keep[c] = np.ascontiguousarray(a, np.float64)
        ptrs[c] = _dp(keep[c])
    arrs = [np.ascontiguousarray(a, I64) for a in (Super, Rp, Rj, Sp, Sj, Sleft, Child, Childp)]
    Sx = np.ascontiguousarray(Sx, np.float64)
    Fmap = np.ascontiguousarray(Fmap, I64); Cm = np.ascontiguousarray(Cm, I64); Hr = np.ascontiguousarray(Hr, I64)
    Hip = np.ascontiguousarray(Hip, I64)
    lib.qr_assemble(f, fm, 1, *[_ip(a) for a in arrs], _dp(Sx), _ip(Fmap), _ip(Cm), ptrs, _ip(Hr), _ip(Stair), _ip(Hii),
                    _ip(Hip), _dp(F), _ip(Cmap))
    return F, Cmap
