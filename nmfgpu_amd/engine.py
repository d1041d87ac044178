"""ctypes wrapper of include/nmfgpu_amd.h: the device-resident engine and the single-kernel ops."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._lib import library

ALGORITHMS = {"mu": 0, "gdcls": 1, "als": 2, "acls": 3, "ahcls": 4, "nsnmf": 5, "hals": 6, "nenmf": 7}
MISSING_SOLVERS = {"mu": 0, "cd": 1}      # Engine.set_missing_solver (docs/MISSING.md, "Coordinate descent")
_STATUS = {0: "ok", 1: "invalid argument", 2: "out of device memory", 3: "out of host memory", 4: "HIP error", 5: "no HIP device",
           6: "values outside the exact range of the split-operand product"}


class EngineError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        super().__init__(f"{what}: {_STATUS.get(status, status)}{(' (' + detail + ')') if detail else ''}")
        self.status = status


class _Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lam", "lambdaW", "lambdaH", "alphaW", "alphaH", "theta", "divergence", "sparse_compute", "precision",
                                          "missing_values")]


class _ParamsV2(C.Structure):
    """nmfamd_params_v2: the frozen struct followed by the fields added since (nmfamd_engine_create_v2 takes it with its size)."""
    _fields_ = [("base", _Params), ("dense_compute", C.c_double)]


class _ParamsV3(C.Structure):
    """nmfamd_params_v3: nmfamd_params_v2 (which keeps its size) followed by the fields added since."""
    _fields_ = [("v2", _ParamsV2), ("beta", C.c_double)]


class _ParamsV4(C.Structure):
    """nmfamd_params_v4: nmfamd_params_v3 (which keeps its size) followed by the fields added since."""
    _fields_ = [("v3", _ParamsV3), ("weighted", C.c_double)]


class _ParamsV5(C.Structure):
    """nmfamd_params_v5: nmfamd_params_v4 (which keeps its size) followed by the fields added since."""
    _fields_ = [("v4", _ParamsV4), ("mixed_precision", C.c_double)]


class _ParamsV6(C.Structure):
    """nmfamd_params_v6: nmfamd_params_v5 (which keeps its size) followed by the fields added since."""
    _fields_ = [("v5", _ParamsV5), ("batch_size", C.c_double), ("forget_factor", C.c_double)]


class _ParamsV7(C.Structure):
    """nmfamd_params_v7: nmfamd_params_v6 (which keeps its size) followed by the fields added since."""
    _fields_ = [("v6", _ParamsV6), ("missing_divergence", C.c_double), ("missing_beta", C.c_double)]


class _Geometry(C.Structure):
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("r", C.c_int), ("padded_rank", C.c_int),
                ("padded_m", C.c_long), ("padded_n", C.c_long), ("slabs_h", C.c_int), ("slabs_w", C.c_int),
                ("exchange_count", C.c_long), ("product_kernel", C.c_int), ("resident_images", C.c_int), ("one_pass", C.c_int),
                ("kl_blocks_w", C.c_int), ("kl_blocks_h", C.c_int), ("gram_k_slices", C.c_int), ("w_col_split", C.c_int),
                ("fused_launches", C.c_int), ("sparse_setup", C.c_int), ("gram_ride_slices_h", C.c_int), ("gram_ride_slices_w", C.c_int)]


def device_count() -> int:
    fn = library().nmfamd_device_count
    fn.restype = C.c_int
    return int(fn())


def _f(a: np.ndarray) -> np.ndarray:
    if a.ndim != 2 or not a.flags.f_contiguous:
        raise ValueError("matrices must be 2-D Fortran-ordered arrays")
    return a


def _ld(a: np.ndarray) -> int:
    return a.strides[1] // a.itemsize if a.shape[1] > 1 else max(a.shape[0], 1)


COLUMN_MAJOR, ROW_MAJOR = 0, 1


def device_matrix(obj, shape, dtype, writable: bool = False):
    """(ptr, ld, layout) of a 2-D device array for the device entries of Engine (docs/DEVICE_IO.md): ptr the address of element (0, 0), ld the leading dimension in
    elements, layout COLUMN_MAJOR or ROW_MAJOR.  obj: anything with __cuda_array_interface__ (a torch tensor on the GPU, a cupy array); nothing is imported and no
    library is called.  Accepted: no strides or C-contiguous strides (row-major, ld = columns), and exactly one unit stride with the other one at least the inner
    extent (that layout with that ld: a .T view, a slice of a taller or wider array).  TypeError for an object without the interface, another dtype, and a
    read-only array with writable=True; ValueError for another shape and for strides no (ptr, ld, layout) describes."""
    iface = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(iface, dict):
        raise TypeError(f"a device array with __cuda_array_interface__ is needed, got {type(obj).__name__}")
    dt = np.dtype(dtype)
    try:
        have = np.dtype(iface["typestr"])
    except TypeError:
        have = None
    if have != dt:
        raise TypeError(f"the device array must be {dt}, got {iface.get('typestr')!r}")
    shape = tuple(int(s) for s in shape)
    if tuple(iface["shape"]) != shape or len(shape) != 2:
        raise ValueError(f"the device array must have shape {shape}, got {tuple(iface['shape'])}")
    ptr, read_only = iface["data"]
    if writable and read_only:
        raise TypeError("the device array is read-only")
    rows, cols = shape
    strides = iface.get("strides")
    if strides is None:
        return int(ptr or 0), max(cols, 1), ROW_MAJOR
    if len(strides) != 2:
        raise ValueError(f"two strides are needed, got {strides!r}")
    if any(s <= 0 for s in strides):
        raise ValueError(f"strides must be positive, got {tuple(strides)}")
    if any(s % dt.itemsize for s in strides):
        raise ValueError(f"strides must be multiples of the item size {dt.itemsize}, got {tuple(strides)}")
    sr, sc = (s // dt.itemsize for s in strides)
    if sc == 1 and sr != 1 and sr >= cols:
        return int(ptr or 0), sr, ROW_MAJOR
    if sr == 1 and sc != 1 and sc >= rows:
        return int(ptr or 0), sc, COLUMN_MAJOR
    if sr == 1 and sc == 1:      # (a single row or a single column: either layout describes it)
        if rows == 1:
            return int(ptr or 0), 1, COLUMN_MAJOR
        if cols == 1:
            return int(ptr or 0), 1, ROW_MAJOR
    raise ValueError(f"strides {tuple(strides)} (bytes) of a {shape} array: exactly one of them has to be the item size and the other one at least the inner extent")


def device_vector(obj, dtype, count: Optional[int] = None):
    """(ptr, count) of a 1-D device array for the sparse device entry of Engine (docs/DEVICE_IO.md), the sibling of device_matrix: obj is anything with
    __cuda_array_interface__ (nothing is imported, no library is called) that is contiguous -- no strides, or a stride equal to the item size -- or a raw
    (ptr, count) pair, which the library checks.  TypeError for an object without the interface and for another dtype (an int64 index array -- torch's CSR default
    -- has to be converted to int32); ValueError for another rank, a non-unit stride and a count other than `count`."""
    dt = np.dtype(dtype)
    if isinstance(obj, tuple) and len(obj) == 2:
        ptr, have = int(obj[0] or 0), int(obj[1])
    else:
        iface = getattr(obj, "__cuda_array_interface__", None)
        if not isinstance(iface, dict):
            raise TypeError(f"a device array with __cuda_array_interface__ is needed, got {type(obj).__name__}")
        try:
            got = np.dtype(iface["typestr"])
        except TypeError:
            got = None
        if got != dt:
            hint = " (convert the index array to int32: tensor.to(torch.int32))" if got == np.dtype(np.int64) and dt == np.dtype(np.int32) else ""
            raise TypeError(f"the device array must be {dt}, got {iface.get('typestr')!r}{hint}")
        shape = tuple(iface["shape"])
        if len(shape) != 1:
            raise ValueError(f"a 1-D device array is needed, got shape {shape}")
        strides = iface.get("strides")
        if strides is not None and shape[0] > 1 and tuple(strides) != (dt.itemsize,):
            raise ValueError(f"the device array must be contiguous (stride {dt.itemsize} bytes), got strides {tuple(strides)}")
        ptr, have = int(iface["data"][0] or 0), int(shape[0])
    if count is not None and have != int(count):
        raise ValueError(f"the device array must have {int(count)} elements, got {have}")
    return ptr, have


def device_pointer_info(ptr: int) -> dict:
    """What the pointer check of the device entries sees (nmfamd_device_pointer_info; no kernel, no engine): {"kind": "unknown" | "device" | "pinned" | "other",
    "device": index or -1, "bytes_from_p": bytes from ptr to the end of its allocation (0 unless "device")}."""
    lib = library()
    kind, dev, avail = C.c_int(), C.c_int(), C.c_ulonglong()
    st = lib.nmfamd_device_pointer_info(C.c_void_p(int(ptr)), C.byref(kind), C.byref(dev), C.byref(avail))
    if st != 0:
        raise EngineError(st, "nmfamd_device_pointer_info")
    return {"kind": ("unknown", "device", "pinned", "other")[kind.value], "device": dev.value, "bytes_from_p": int(avail.value)}


def _count(v) -> int:
    """A sweep count as the C int it travels as; anything that is not a whole number is refused here, since the C side would only see it truncated."""
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"a sweep count must be an integer, got {v!r}")
    return int(v)


def _param_values(lam=0.0, lambda_w=0.0, lambda_h=0.0, alpha_w=0.0, alpha_h=0.0, theta=0.0, divergence="frobenius", sparse_compute=False, precision="native",
                  missing_values=False, dense_compute=False, beta=None, weighted=False, mixed_precision=False, batch_size=None, forget_factor=0.7,
                  missing_divergence="frobenius", missing_beta=None) -> list:
    """The eighteen doubles of nmfamd_params_v7, in its order, from the keyword arguments of Engine (and of plan_geometry)."""
    if missing_beta is not None and missing_divergence != "beta":
        raise ValueError('missing_beta needs missing_divergence="beta"')
    if missing_divergence == "beta" and missing_beta is None:
        raise ValueError('missing_divergence="beta" needs a missing_beta')
    if not batch_size:
        batch_size, forget_factor = 0.0, 0.0
    if beta is not None and divergence != "beta":
        raise ValueError('beta needs divergence="beta"')
    if divergence == "beta" and beta is None:
        raise ValueError('divergence="beta" needs a beta')
    return [lam, lambda_w, lambda_h, alpha_w, alpha_h, theta, {"frobenius": 0.0, "kl": 1.0, "is": 2.0, "beta": 3.0}[divergence],
            float(sparse_compute or missing_values), {"native": 0.0, "bf16": 1.0, "fp32_mfma": -1.0}[precision],
            float(missing_values), float(dense_compute), float(beta or 0.0), float(weighted), float(mixed_precision), float(batch_size), float(forget_factor),
            {"frobenius": 0.0, "kl": 1.0, "is": 2.0, "beta": 3.0}[missing_divergence], float(missing_beta or 0.0)]


def _params_struct(v: list) -> _ParamsV7:
    """v: the values of _param_values; a list of sixteen (nmfamd_params_v6) leaves the two fields added since at 0."""
    v = list(v) + [0.0] * (18 - len(v))
    return _ParamsV7(_ParamsV6(_ParamsV5(_ParamsV4(_ParamsV3(_ParamsV2(_Params(*v[:10]), v[10]), v[11]), v[12]), v[13]), v[14], v[15]), v[16], v[17])


def plan_geometry(m: int, n: int, r: int, algorithm: str = "mu", dtype=np.float32, *, num_cus: int, memory_side_cache_bytes: int, free_bytes: int,
                  row_blocks: int = 1, **params) -> dict:
    """Engine(m, n, r, algorithm, dtype, row_blocks=row_blocks, **params).geometry() as it would be on a device with num_cus compute units, a memory-side cache of
    memory_side_cache_bytes and free_bytes of free memory -- without a device (nmfamd_plan_geometry: the parameter checks and the planning step of engine creation,
    no allocation).  params: the keyword arguments of Engine that travel in nmfamd_params (lam ... forget_factor).  Raises EngineError where creation would refuse."""
    lib = library()
    p = _params_struct(_param_values(**params))
    g = _Geometry()
    st = lib.nmfamd_plan_geometry(int(m), int(n), int(r), ALGORITHMS[algorithm], C.byref(p), C.c_ulong(C.sizeof(p)), np.dtype(dtype).itemsize, int(row_blocks),
                                  int(num_cus), C.c_ulonglong(memory_side_cache_bytes), C.c_ulonglong(free_bytes), C.byref(g), C.c_ulong(C.sizeof(g)))
    if st != 0:
        lib.nmfamd_engine_last_error.restype = C.c_char_p
        raise EngineError(st, "nmfamd_plan_geometry", (lib.nmfamd_engine_last_error(None) or b"").decode())
    return {k: getattr(g, k) for k, _ in _Geometry._fields_}


class Engine:
    """One factorisation resident on the current HIP device (see include/nmfgpu_amd.h)."""

    def __init__(self, m: int, n: int, r: int, algorithm: str = "mu", dtype=np.float32, stream: int = 0,
                 lam=0.0, lambda_w=0.0, lambda_h=0.0, alpha_w=0.0, alpha_h=0.0, theta=0.0, divergence: str = "frobenius",
                 sparse_compute: bool = False, precision: str = "native", row_blocks: int = 1, missing_values: bool = False,
                 l1_w=0.0, l1_h=0.0, l2_w=0.0, l2_h=0.0, dense_compute: bool = False, beta=None, weighted: bool = False, mixed_precision: bool = False,
                 batch_size=None, forget_factor=0.7, sweeps_h: int = 1, sweeps_w: int = 1, sweep_tolerance: float = 0.0,
                 steps_h: Optional[int] = None, steps_w: Optional[int] = None, step_tolerance: Optional[float] = None,
                 missing_divergence: str = "frobenius", missing_beta=None, missing_solver: Optional[str] = None, missing_sweeps_h: int = 1, missing_sweeps_w: int = 1):
        """divergence: "frobenius", "kl" (generalised KL over the stored entries of a sparse image of V; with dense_compute=True on a dense resident V),
        "is" (Itakura-Saito, always dense: every entry of V > 0) or "beta" (the beta-divergence at `beta`, any finite value, always dense: scikit-learn's
        solver="mu" with beta_loss=beta; beta=0.0 and beta=1.0 are the "is" and the dense "kl" engines; beta <= 0 needs every entry of V > 0) --
        docs/DIVERGENCE.md.  The dense divergence engines are "mu" only, rank <= 256, single GPU; divergence_value reports their objective.

        missing_values=True: fit the observed entries only (docs/MISSING.md) -- the stored entries of upload_sparse, the non-NaN entries of
        upload (zeros included).  Multiplicative update ("mu") only; implies sparse_compute.  missing_divergence: the objective over the observed entries --
        "frobenius" (the default), "kl", "is" or "beta" at missing_beta (any finite value; 0.0 and 1.0 are "is" and "kl"), docs/MISSING.md "Beta-divergence": the
        weighted update at 0 / 1 weights in O(nnz r) per iteration.  beta <= 0 needs every stored value > 0, beta > 0 takes stored zeros as observations; such an
        engine takes l1_w ... l2_h (set_penalties) and constant_w, and divergence_value reports its objective.  `divergence` itself stays refused beside
        missing_values.

        missing_solver ("mu" or "cd"; missing_values=True with the "frobenius" objective only; None = never set, the multiplicative update): "cd" fits the observed
        entries by coordinate descent (docs/MISSING.md, "Coordinate descent") with missing_sweeps_h / missing_sweeps_w sweeps (1 ... 64) per half-step; rank <= 128.
        With a missing_solver the penalties l1_w ... l2_h are the solver's (set_missing_solver), not set_penalties'.

        l1_w, l1_h, l2_w, l2_h: the L1 / L2 penalties on W and H of scikit-learn's coordinate descent ("hals", docs/HALS.md) and of its multiplicative update
        (the dense divergence engines, docs/DIVERGENCE.md); see set_penalties.  sparse_compute=True is available for "mu" and "hals" (rank <= 256).

        weighted=True: weighted NMF on a dense divergence engine ("is", "beta", or "kl" with dense_compute) -- the objective is sum w_ij d_beta(v_ij | (W H)_ij) with a
        matrix of weights >= 0 given to upload(V, weights=...).  A weight of 0 means the entry is missing (V may hold anything there, NaN included); rmsd divides by
        the sum of the weights (docs/DIVERGENCE.md, "Weighted update").

        mixed_precision=True: a float32 dense divergence engine multiplies with bf16 operands (W, H and the mapped V .* P^(beta - 2), P^(beta - 1) rounded to
        nearest even; V, the element-wise map, every sum and the factors themselves stay float32) -- faster, with a relative error of a few 2^-9 per update
        (docs/DIVERGENCE.md, "Mixed precision").  Not with float64, not with weighted=True; precision="bf16" stays refused on these engines.

        batch_size=b (a positive multiple of 128): the minibatch (online) form of a dense divergence engine, scikit-learn's MiniBatchNMF with the samples as the
        columns of V (docs/DIVERGENCE.md, "Minibatch update").  One iterate() step is one pass over the column blocks [0, b), [b, 2 b), ... in order; W moves
        once per block, from numerator and denominator panels accumulated with rho = forget_factor^(min(b, n) / n); set_factors and randomize start them again.
        No normalisation, no constant_w; frobenius / rmsd / divergence_value refer to (W, H) after the pass.  None or 0: the full-batch engine, where
        forget_factor is not looked at.

        sweeps_h, sweeps_w ("hals" only; 1 ... 64): accelerated HALS, that many sweeps per product in the H step and in the W step (docs/HALS.md, "Inner
        sweeps"); see set_sweeps.

        sweep_tolerance ("hals" only; in [0, 1)): per-column dynamic stopping of the inner sweeps, with sweeps_h / sweeps_w as maximum counts (docs/HALS.md, "Dynamic
        stopping"); 0 keeps the static counts; see set_sweep_tolerance.

        steps_h, steps_w ("nenmf" only; 1 ... 256, None = the library's 8): NeNMF, that many accelerated projected-gradient steps per product in the H step and
        in the W step (docs/NENMF.md); see set_steps.  "nenmf" takes the penalties and sparse_compute of "hals"; rank <= 128.

        step_tolerance ("nenmf" only; in [0, 1), None = 0): per-column dynamic stopping of those steps, with steps_h / steps_w as maximum counts (docs/NENMF.md,
        "Dynamic stopping"); 0 keeps the static counts; see set_step_tolerance."""
        self._bind(m, n, r, dtype)
        solver = None
        if missing_solver is not None:
            solver = [missing_solver, _count(missing_sweeps_h), _count(missing_sweeps_w), float(l1_w), float(l1_h), float(l2_w), float(l2_h)]
            l1_w = l1_h = l2_w = l2_h = 0.0
        elif missing_sweeps_h != 1 or missing_sweeps_w != 1:
            raise ValueError("missing_sweeps_h / missing_sweeps_w need a missing_solver")
        self._ctor = dict(algorithm=algorithm, stream=stream, row_blocks=row_blocks, missing_solver=solver,
                          params=_param_values(lam, lambda_w, lambda_h, alpha_w, alpha_h, theta, divergence, sparse_compute, precision, missing_values, dense_compute, beta,
                                               weighted, mixed_precision, batch_size, forget_factor, missing_divergence, missing_beta),
                          penalties=[float(l1_w), float(l1_h), float(l2_w), float(l2_h)], sweeps=[_count(sweeps_h), _count(sweeps_w)],
                          sweep_tolerance=float(sweep_tolerance), step_tolerance=None if step_tolerance is None else float(step_tolerance),
                          steps=None if steps_h is None and steps_w is None else [_count(8 if steps_h is None else steps_h), _count(8 if steps_w is None else steps_w)])
        self._create()

    def _bind(self, m, n, r, dtype):
        self._lib = library()
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("float32 or float64")
        self.m, self.n, self.r = m, n, r
        self._ctor = None
        self._h = None
        self._lib.nmfamd_engine_frobenius.restype = C.c_double
        self._lib.nmfamd_engine_rmsd.restype = C.c_double
        self._lib.nmfamd_engine_kl_divergence.restype = C.c_double
        self._lib.nmfamd_engine_last_error.restype = C.c_char_p
        self._lib.nmfamd_engine_error_terms.restype = C.c_long

    @classmethod
    def from_handle(cls, handle, m: int, n: int, r: int, dtype=np.float32):
        """The wrapper around an nmfamd_engine* that the caller created through the C interface (nmfamd_engine_create*), which it owns from here on (close()
        destroys it).  Such an engine is never recreated: an upload the C side answers with NMFAMD_VALUE_RANGE raises instead of switching the product form."""
        self = cls.__new__(cls)
        self._bind(m, n, r, dtype)
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        return self

    def _create(self):
        c = self._ctor
        p = _params_struct(c["params"])
        h = C.c_void_p()
        # row_blocks > 1: the padded row count is a multiple of 128 * row_blocks (row-block form of the sharded W step)
        if not hasattr(self._lib, "nmfamd_engine_create_v2"):
            # (NMFAMD_LIBRARY names a build from before the sized entry -- tools/time_beta.py times such a build: it reads the frozen struct only)
            st = self._lib.nmfamd_engine_create_blocks(self.m, self.n, self.r, ALGORITHMS[c["algorithm"]], C.byref(p.v6.v5.v4.v3.v2.base), self.dtype.itemsize,
                                                       C.c_void_p(c["stream"]), int(c["row_blocks"]), C.byref(h))
        else:
            st = self._lib.nmfamd_engine_create_v2(self.m, self.n, self.r, ALGORITHMS[c["algorithm"]], C.byref(p), C.c_ulong(C.sizeof(p)), self.dtype.itemsize,
                                                   C.c_void_p(c["stream"]), int(c["row_blocks"]), C.byref(h))
        if st != 0:
            raise EngineError(st, "nmfamd_engine_create", (self._lib.nmfamd_engine_last_error(None) or b"").decode())
        self._h = h
        # (the penalties are engine state, not part of nmfamd_params: an engine recreated by _upload gets them again)
        try:
            self.set_penalties(*c["penalties"])
            if c["sweeps"] != [1, 1]:      # (the default needs no call: a library from before the counts has no such entry)
                self.set_sweeps(*c["sweeps"])
            if c["sweep_tolerance"] != 0.0:      # (likewise)
                self.set_sweep_tolerance(c["sweep_tolerance"])
            if c.get("steps") is not None:      # (likewise; given counts go to the library whatever the algorithm, which refuses them on any but "nenmf")
                self.set_steps(*c["steps"])
            if c.get("step_tolerance") is not None:      # (likewise)
                self.set_step_tolerance(c["step_tolerance"])
            if c.get("missing_solver") is not None:      # (likewise)
                self.set_missing_solver(*c["missing_solver"])
        except EngineError:
            self.close()
            raise

    def _check(self, st: int, what: str):
        if st != 0:
            raise EngineError(st, what, (self._lib.nmfamd_engine_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, V: np.ndarray, weights: Optional[np.ndarray] = None):
        """weights (engines created with weighted=True, which take no upload without them): Fortran-ordered, of V's dtype and shape, finite and >= 0 with at
        least one entry > 0; where a weight is 0, V is not looked at.  A second upload replaces both matrices."""
        V = _f(V)
        if V.dtype != self.dtype:
            raise TypeError(f"V must be {self.dtype}, got {V.dtype}")
        if V.shape != (self.m, self.n):
            raise ValueError(f"V must have shape {(self.m, self.n)}, got {V.shape}")
        if weights is not None:
            weights = _f(weights)
            if weights.dtype != self.dtype:
                raise TypeError(f"weights must be {self.dtype}, got {weights.dtype}")
            if weights.shape != (self.m, self.n):
                raise ValueError(f"weights must have shape {(self.m, self.n)}, got {weights.shape}")
            self._check(self._lib.nmfamd_engine_upload_dense_weighted(self._h, C.c_void_p(V.ctypes.data), C.c_long(_ld(V)), C.c_void_p(weights.ctypes.data),
                                                                      C.c_long(_ld(weights))), "upload_dense_weighted")
            return
        self._upload(lambda: self._lib.nmfamd_engine_upload_dense(self._h, C.c_void_p(V.ctypes.data), C.c_long(_ld(V))), "upload_dense")

    def _upload(self, call, what: str):
        st = call()
        # (missing values: NaN marks a missing entry and the sparse images never see it -- no retry)
        if st == 6 and self._ctor is not None and self._ctor["params"][8] == 0.0 and self._ctor["params"][9] == 0.0:
            # NMFAMD_VALUE_RANGE: infinities, NaN, |v| > 2^126 or 0 < |v| < 2^-100 in V -- the split-operand product is not the
            # fp32 product there; recreate the engine on the native fp32 MFMA instructions, as nmfgpu::compute does.
            # The handle changes: anything created from the old one (a ShardedRun, w_panel_ptr()) is void -- upload V before
            # creating those.  Column-sharded callers must make this switch on every rank together (EngineShard does).
            self.close()
            self._ctor["params"][8] = -1.0
            self._create()
            st = call()
        self._check(st, what)

    def _dev(self, obj, shape, writable=False):
        """(ptr, ld, layout) of a device array (device_matrix), or the triple itself where the caller holds a raw device pointer: the library checks that one."""
        if isinstance(obj, tuple) and len(obj) == 3:
            return int(obj[0] or 0), int(obj[1]), int(obj[2])
        return device_matrix(obj, shape, self.dtype, writable)

    def upload_device(self, V, weights=None):
        """upload() for a V that lies in the memory of the engine's GPU (docs/DEVICE_IO.md): V, and weights on a weighted engine, are device arrays of the engine's
        dtype and shape (m, n) with __cuda_array_interface__ -- torch tensors, row-major or column-major, views with a leading dimension included (device_matrix) --
        or raw (ptr, ld, layout) triples.  They are read where they lie, never written, and everything that follows equals upload() of the same values bit for
        bit (rmsd of a weighted engine: within m n 2^-53).  Work enqueued on any stream of the device is waited for first.  Engines with sparse_compute or
        missing_values refuse it: upload_device_stored is their entry."""
        vp, vld, vlay = self._dev(V, (self.m, self.n))
        if weights is not None:
            wp, wld, wlay = self._dev(weights, (self.m, self.n))
            self._check(self._lib.nmfamd_engine_upload_dense_weighted_device(self._h, C.c_void_p(vp), C.c_long(vld), vlay, C.c_void_p(wp), C.c_long(wld), wlay),
                        "upload_dense_weighted_device")
            return
        self._upload(lambda: self._lib.nmfamd_engine_upload_dense_device(self._h, C.c_void_p(vp), C.c_long(vld), vlay), "upload_dense_device")

    def upload_device_stored(self, V):
        """upload() of a dense V that lies in the memory of the engine's GPU, for the engines upload_device refuses: sparse_compute (the entries != 0 are stored) and
        missing_values (every entry that is not NaN is observed, zeros included).  V as for upload_device.  The CSR and CSC images are compacted on the device
        (docs/DEVICE_IO.md, "Dense input on the sparse engines") and equal those of upload() of the same values bit for bit; any other engine refuses the call."""
        vp, vld, vlay = self._dev(V, (self.m, self.n))
        self._upload(lambda: self._lib.nmfamd_engine_upload_dense_device_stored(self._h, C.c_void_p(vp), C.c_long(vld), vlay), "upload_dense_device_stored")

    def upload_sparse_device(self, fmt: int, values, a, b, base: int = 0):
        """upload_sparse() for arrays that lie in the memory of the engine's GPU (docs/DEVICE_IO.md, "Sparse input"): values of the engine's dtype, a and b int32
        (torch's CSR tensors hold int64 indices: convert them), each a contiguous 1-D device array with __cuda_array_interface__ (device_vector) or a raw
        (ptr, count) pair.  fmt 1 CSR (a: m + 1 row pointers, b: column indices), 2 CSC (a: n + 1 column pointers, b: row indices), 3 COO (a: rows, b: columns).
        The arrays are read where they lie, never written and not kept; everything that follows equals upload_sparse() of the same values."""
        vp, nnz = device_vector(values, self.dtype)
        na = {1: self.m + 1, 2: self.n + 1, 3: nnz}.get(fmt)      # (another format: the library refuses it, as it refuses upload_sparse's)
        ap, _ = device_vector(a, np.int32, na)
        bp, _ = device_vector(b, np.int32, nnz)
        self._upload(lambda: self._lib.nmfamd_engine_upload_sparse_device(self._h, int(fmt), C.c_void_p(vp), C.c_void_p(ap), C.c_void_p(bp), C.c_long(nnz), int(base)),
                     "upload_sparse_device")

    def set_factors_device(self, W, H):
        """set_factors() from device arrays (W: (m, r), H: (r, n), either layout, see upload_device); None leaves that factor."""
        wp, wld, wlay = self._dev(W, (self.m, self.r)) if W is not None else (None, 0, 0)
        hp, hld, hlay = self._dev(H, (self.r, self.n)) if H is not None else (None, 0, 0)
        self._check(self._lib.nmfamd_engine_set_factors_device(self._h, C.c_void_p(wp), C.c_long(wld), wlay, C.c_void_p(hp), C.c_long(hld), hlay), "set_factors_device")

    def get_factors_device(self, W_out, H_out):
        """get_factors() into caller-supplied writable device arrays (W_out: (m, r), H_out: (r, n), either layout); None skips that factor.  Only the m x r / r x n
        elements are written.  Returns after the engine's stream is idle: any stream may read the arrays."""
        wp, wld, wlay = self._dev(W_out, (self.m, self.r), True) if W_out is not None else (None, 0, 0)
        hp, hld, hlay = self._dev(H_out, (self.r, self.n), True) if H_out is not None else (None, 0, 0)
        self._check(self._lib.nmfamd_engine_get_factors_device(self._h, C.c_void_p(wp), C.c_long(wld), wlay, C.c_void_p(hp), C.c_long(hld), hlay), "get_factors_device")

    # ---- predict and score entries of W H (docs/PREDICT.md) ----
    def _entries(self, rows, cols, values):
        """The coordinate list of predict / score as C arguments: (on_device, rows, cols, values, nnz), host arrays converted to contiguous int32 / the engine's dtype,
        device arrays (anything with __cuda_array_interface__: all of them or none) as pointers.  ValueError for mismatched lengths."""
        given = [a for a in (rows, cols, values) if a is not None]
        on_device = [hasattr(a, "__cuda_array_interface__") for a in given]
        if any(on_device) != all(on_device):
            raise TypeError("rows, cols and values: all of them device arrays, or none")
        if on_device[0]:
            rp, nnz = device_vector(rows, np.int32)
            try:
                cp, _ = device_vector(cols, np.int32, nnz)
                vp = device_vector(values, self.dtype, nnz)[0] if values is not None else None
            except ValueError as exc:
                raise ValueError(f"rows, cols and values must have the same length: {exc}") from None
            return True, rp, cp, vp, nnz
        rows = np.ascontiguousarray(rows, dtype=np.int32); cols = np.ascontiguousarray(cols, dtype=np.int32)
        if rows.ndim != 1 or cols.shape != rows.shape:
            raise ValueError(f"rows and cols must be 1-D arrays of the same length, got {rows.shape} and {cols.shape}")
        if values is not None:
            values = np.ascontiguousarray(values, dtype=self.dtype)
            if values.shape != rows.shape:
                raise ValueError(f"values must have the same length as rows and cols ({rows.shape[0]}), got {values.shape}")
        return False, rows, cols, values, int(rows.shape[0])

    def _device_out(self, like, nnz: int, dtype=None):
        """(tensor, ptr): a new torch tensor of nnz values of the engine's dtype (or `dtype`) on the device of `like` (a torch tensor).  Nothing is imported: the
        library is the one the caller's tensor brought along."""
        import sys
        dt = self.dtype if dtype is None else np.dtype(dtype)
        lib = sys.modules[type(like).__module__.partition(".")[0]]
        out = like.new_empty((int(nnz),), dtype=getattr(lib, dt.name))
        return out, device_vector(out, dt, int(nnz))[0]

    def predict(self, rows, cols, base: int = 0):
        """out[p] = sum_k W(rows[p], k) H(k, cols[p]) for W, H = what get_factors() would return now (nsNMF: W S), in the engine's precision (docs/PREDICT.md).  rows,
        cols: nnz >= 1 coordinates of index base `base` (0 or 1), unsorted, duplicates allowed -- numpy arrays (an ndarray comes back) or int32 device arrays with
        __cuda_array_interface__ such as torch tensors on the engine's GPU (a device tensor comes back; nothing crosses to the host).  The engine is left as
        get_factors() leaves it.  EngineError for a coordinate outside the matrix (no kernel gathers with an unchecked index), for an engine with row blocks or of
        a sharded run, and before the factors were set."""
        dev, r, c, _, nnz = self._entries(rows, cols, None)
        if dev:
            out, op = self._device_out(rows, nnz)
            self._check(self._lib.nmfamd_engine_predict_device(self._h, C.c_void_p(r), C.c_void_p(c), C.c_long(nnz), int(base), C.c_void_p(op)), "predict_device")
            return out
        out = np.empty(nnz, dtype=self.dtype)
        self._check(self._lib.nmfamd_engine_predict(self._h, _p(r), _p(c), C.c_long(nnz), int(base), _p(out)), "predict")
        return out

    def score(self, rows, cols, values, beta: Optional[float] = None, base: int = 0, return_predictions: bool = False) -> dict:
        """The error of W H over the entries (rows[p], cols[p]) with values[p] (docs/PREDICT.md): {"sq": sum (v - p)^2, "rmsd": sqrt(sq / nnz), "div": sum
        d_beta(v | p + eps), "abs_div": the sum of the absolute values of the summands of d_beta (the scale of div's rounding), "count": nnz} and, with
        return_predictions, "predictions" (as predict returns them).  beta=None: no divergence wanted -- div and abs_div are NaN, any finite value is taken;
        otherwise beta <= 0 needs every value finite and > 0 and beta > 0 finite and >= 0 (EngineError).  Arrays as for predict.  Bit-identical between calls and
        between host and device arrays."""
        dev, r, c, v, nnz = self._entries(rows, cols, values)
        b = C.c_double(float("nan") if beta is None else float(beta))
        sums = (C.c_double * 4)()
        out = None
        if dev:
            out, op = self._device_out(values, nnz) if return_predictions else (None, None)
            self._check(self._lib.nmfamd_engine_score_device(self._h, C.c_void_p(r), C.c_void_p(c), C.c_void_p(v), C.c_long(nnz), int(base), b, C.c_void_p(op), sums),
                        "score_device")
        else:
            if return_predictions:
                out = np.empty(nnz, dtype=self.dtype)
            self._check(self._lib.nmfamd_engine_score(self._h, _p(r), _p(c), _p(v), C.c_long(nnz), int(base), b, _p(out), sums), "score")
        res = {"sq": sums[0], "rmsd": sums[3], "div": sums[1], "abs_div": sums[2], "count": nnz}
        if return_predictions:
            res["predictions"] = out
        return res

    # ---- the k best candidates of W H per query (docs/TOPK.md) ----
    def top_k(self, queries, k: int, axis: int = 0, exclude=None, base: int = 0):
        """(indices, scores), each (nq, k): per query the k candidates with the highest score of W H, W and H being what get_factors() would return now
        (docs/TOPK.md).  axis=0: a query is a row of V and the candidates are the n columns; axis=1: a query is a column and the candidates are the m rows.
        Candidates are ordered by score descending, equal scores by ascending index; indices are int32 in the caller's base, scores in the engine's precision.
        exclude: a pair (excl_ptr, excl_idx) -- int64 offsets of nq + 1 entries and int32 candidate indices, as exclusion_lists builds them -- of candidates that are
        not eligible for a query; where fewer than k are eligible the remaining slots hold index -1 and score -inf.  1 <= k <= TOPK_MAX_K.  queries: a numpy array
        (ndarrays come back) or an int32 device array with __cuda_array_interface__ such as a torch tensor on the engine's GPU (device tensors come back, exclude
        is then a pair of device arrays, and nothing crosses to the host).  The engine is left as get_factors() leaves it.  EngineError for a query or an excluded
        index outside its range, a malformed excl_ptr, and the engines predict refuses."""
        k = int(k)
        if hasattr(queries, "__cuda_array_interface__"):
            qp, nq = device_vector(queries, np.int32)
            ep = ip = None
            ennz = 0
            if exclude is not None:
                ep, np1 = device_vector(exclude[0], np.int64)
                if np1 != nq + 1:
                    raise ValueError(f"exclude[0] must hold nq + 1 = {nq + 1} offsets, got {np1}")
                ip, ennz = device_vector(exclude[1], np.int32)
            idx, xp = self._device_out(queries, max(nq * k, 0), np.int32)
            sc, sp = self._device_out(queries, max(nq * k, 0))
            self._check(self._lib.nmfamd_engine_top_k_device(self._h, C.c_void_p(qp), C.c_long(nq), k, int(axis), int(base), C.c_void_p(ep), C.c_void_p(ip), C.c_long(ennz),
                                                             C.c_void_p(xp), C.c_void_p(sp)), "top_k_device")
            return idx.view(nq, k), sc.view(nq, k)
        q = np.ascontiguousarray(queries, dtype=np.int32)
        if q.ndim != 1:
            raise ValueError(f"queries must be a 1-D array, got {q.shape}")
        nq = int(q.shape[0])
        ep = ip = None
        if exclude is not None:
            ep = np.ascontiguousarray(exclude[0], dtype=np.int64); ip = np.ascontiguousarray(exclude[1], dtype=np.int32)
            if ep.shape != (nq + 1,) or ip.ndim != 1:
                raise ValueError(f"exclude: (excl_ptr of nq + 1 = {nq + 1} offsets, excl_idx), got {ep.shape} and {ip.shape}")
            if ep[0] == 0 and (np.diff(ep) >= 0).all() and ep[-1] > ip.shape[0]:
                raise ValueError(f"exclude: excl_ptr names {int(ep[-1])} entries, excl_idx holds {ip.shape[0]}")
        idx = np.empty((nq, max(k, 0)), dtype=np.int32); sc = np.empty((nq, max(k, 0)), dtype=self.dtype)
        self._check(self._lib.nmfamd_engine_top_k(self._h, _p(q), C.c_long(nq), k, int(axis), int(base), _p(ep), _p(ip), _p(idx), _p(sc)), "top_k")
        return idx, sc

    def upload_sparse(self, fmt: int, values: np.ndarray, a: np.ndarray, b: np.ndarray, base: int = 0):
        values = np.ascontiguousarray(values, dtype=self.dtype)
        a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
        self._upload(lambda: self._lib.nmfamd_engine_upload_sparse(self._h, fmt, C.c_void_p(values.ctypes.data), C.c_void_p(a.ctypes.data),
                                                                   C.c_void_p(b.ctypes.data), C.c_long(len(values)), base), "upload_sparse")

    def set_factors(self, W: Optional[np.ndarray], H: Optional[np.ndarray]):
        # the C side sees raw pointers and leading dimensions only: a float64 W on a float32 engine, or a wrong shape,
        # would be reinterpreted (or read out of bounds) silently
        for name, a, shape in (("W", W, (self.m, self.r)), ("H", H, (self.r, self.n))):
            if a is None:
                continue
            if not isinstance(a, np.ndarray) or a.dtype != self.dtype:
                raise TypeError(f"{name} must be a {self.dtype} ndarray, got {getattr(a, 'dtype', type(a))}")
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
        wp = C.c_void_p(_f(W).ctypes.data) if W is not None else None
        hp = C.c_void_p(_f(H).ctypes.data) if H is not None else None
        self._check(self._lib.nmfamd_engine_set_factors(self._h, wp, C.c_long(_ld(W) if W is not None else 0),
                                                        hp, C.c_long(_ld(H) if H is not None else 0)), "set_factors")

    def get_factors(self):
        W = np.zeros((self.m, self.r), dtype=self.dtype, order="F")
        H = np.zeros((self.r, self.n), dtype=self.dtype, order="F")
        self._check(self._lib.nmfamd_engine_get_factors(self._h, C.c_void_p(W.ctypes.data), C.c_long(self.m),
                                                        C.c_void_p(H.ctypes.data), C.c_long(self.r)), "get_factors")
        return W, H

    def randomize(self, seed: int, w: bool = True, h: bool = True):
        self._check(self._lib.nmfamd_engine_randomize(self._h, C.c_uint(seed), int(w), int(h)), "randomize")

    def iterate(self, count: int, first_iteration: int = 1, error_every: int = 10, last_iteration: int = 0, constant_w: bool = False):
        self._check(self._lib.nmfamd_engine_iterate(self._h, count, first_iteration, error_every, last_iteration, int(constant_w)), "iterate")

    def synchronize(self):
        self._check(self._lib.nmfamd_engine_synchronize(self._h), "synchronize")

    def set_penalties(self, l1_w=0.0, l1_h=0.0, l2_w=0.0, l2_h=0.0):
        """HALS: the iterations that follow minimise 1/2 ||V - W H||^2 + l1_w ||W||_1 + l1_h ||H||_1 + 1/2 l2_w ||W||^2 + 1/2 l2_h ||H||^2
        (nmfamd_engine_set_hals_penalties; docs/HALS.md has the mapping from scikit-learn's alpha_W, alpha_H, l1_ratio).  Dense divergence engines: the
        same four terms added to the divergence (scikit-learn's multiplicative update, docs/DIVERGENCE.md); masked divergence engines (missing_divergence): likewise, over
        the observed entries (docs/MISSING.md).  Valid between iterations; all zeros restores
        the unpenalised iteration, normalisation included.  frobenius / rmsd / divergence_value keep reporting the unpenalised figures."""
        vals = [float(l1_w), float(l1_h), float(l2_w), float(l2_h)]
        self._check(self._lib.nmfamd_engine_set_hals_penalties(self._h, *(C.c_double(v) for v in vals)), "set_hals_penalties")
        if self._ctor is not None:
            self._ctor["penalties"] = vals

    def set_missing_solver(self, solver: str = "cd", sweeps_h: int = 1, sweeps_w: int = 1, l1_w=0.0, l1_h=0.0, l2_w=0.0, l2_h=0.0):
        """Missing values under the Frobenius objective: the solver of the iterations that follow (nmfamd_engine_set_missing_solver; docs/MISSING.md, "Coordinate
        descent").  "mu": the multiplicative update, which takes sweeps 1 and penalties 0 only.  "cd": coordinate descent over the observed entries -- every column
        of H, then every row of W, against its own Gram matrix with sweeps_h / sweeps_w HALS sweeps (1 ... 64) and the penalties of set_penalties' objective, the
        squared error summed over the observed entries; no normalisation; rank <= 128.  Valid between iterations; the factors stay as they are.  frobenius / rmsd
        keep reporting the unpenalised error over the observed entries."""
        if solver not in MISSING_SOLVERS:
            raise ValueError(f'missing_solver: "mu" or "cd", got {solver!r}')
        vals = [solver, _count(sweeps_h), _count(sweeps_w), float(l1_w), float(l1_h), float(l2_w), float(l2_h)]
        if not hasattr(self._lib, "nmfamd_engine_set_missing_solver"):
            raise EngineError(1, "set_missing_solver", "the loaded library has no missing-value solver setting")
        self._check(self._lib.nmfamd_engine_set_missing_solver(self._h, MISSING_SOLVERS[solver], C.c_int(vals[1]), C.c_int(vals[2]), *(C.c_double(v) for v in vals[3:])),
                    "set_missing_solver")
        if self._ctor is not None:
            self._ctor["missing_solver"] = vals

    def set_sweeps(self, h: int = 1, w: int = 1):
        """HALS: the iterations that follow run h sweeps per H step and w sweeps per W step against one set of products each (accelerated HALS,
        nmfamd_engine_set_hals_sweeps; docs/HALS.md, "Inner sweeps").  Integers in 1 ... 64; (1, 1) restores the plain iteration.  Valid between
        iterations; with constant_w only h matters."""
        vals = [_count(h), _count(w)]
        self._check(self._lib.nmfamd_engine_set_hals_sweeps(self._h, *(C.c_int(v) for v in vals)), "set_hals_sweeps")
        if self._ctor is not None:
            self._ctor["sweeps"] = vals

    def set_steps(self, h: int = 8, w: int = 8):
        """NeNMF: the iterations that follow take h accelerated projected-gradient steps per H step and w per W step against one set of products each
        (nmfamd_engine_set_nenmf_steps; docs/NENMF.md).  Integers in 1 ... 256.  Valid between iterations; with constant_w only h matters.  Raises EngineError
        on an engine of another algorithm."""
        vals = [_count(h), _count(w)]
        self._check(self._lib.nmfamd_engine_set_nenmf_steps(self._h, *(C.c_int(v) for v in vals)), "set_nenmf_steps")
        if self._ctor is not None:
            self._ctor["steps"] = vals

    def set_sweep_tolerance(self, tol: float = 0.0):
        """HALS: per-column dynamic stopping of the inner sweeps in the iterations that follow (nmfamd_engine_set_hals_sweep_tolerance; docs/HALS.md, "Dynamic
        stopping").  With tol in (0, 1) the counts of set_sweeps are maximum counts: within a step a column is frozen after its sweep t when the squared step of
        that sweep is at most tol^2 times the squared step of its first sweep.  0 restores the static counts, bit for bit.  Valid between iterations."""
        tol = float(tol)
        self._check(self._lib.nmfamd_engine_set_hals_sweep_tolerance(self._h, C.c_double(tol)), "set_hals_sweep_tolerance")
        if self._ctor is not None:
            self._ctor["sweep_tolerance"] = tol

    def set_step_tolerance(self, tol: float = 0.0):
        """NeNMF: per-column dynamic stopping of the projected-gradient steps in the iterations that follow (nmfamd_engine_set_nenmf_step_tolerance; docs/NENMF.md,
        "Dynamic stopping").  With tol in (0, 1) the counts of set_steps are maximum counts: within a step launch a column is frozen after its step t when
        |P_{t+1} - Y_t|^2 of that step is at most tol^2 times that of its first step.  0 restores the static counts, bit for bit.  Valid between iterations.
        Raises EngineError on an engine of another algorithm."""
        tol = float(tol)
        self._check(self._lib.nmfamd_engine_set_nenmf_step_tolerance(self._h, C.c_double(tol)), "set_nenmf_step_tolerance")
        if self._ctor is not None:
            self._ctor["step_tolerance"] = tol

    def step_counts(self, which: int) -> np.ndarray:
        """NeNMF: the steps applied to each column of H (which = 0, n values) or row of W (which = 1, m values) by the most recent step launch of that factor, as
        np.int32 (nmfamd_engine_nenmf_step_counts; synchronises), with the contract of sweep_counts."""
        out = np.zeros(self.n if which == 0 else self.m, dtype=np.int32)
        fn = self._lib.nmfamd_engine_nenmf_step_counts
        fn.restype = C.c_long
        got = fn(self._h, int(which), C.c_void_p(out.ctypes.data), C.c_long(out.size))
        if got < 0:
            raise EngineError(1, "nenmf_step_counts", (self._lib.nmfamd_engine_last_error(self._h) or b"").decode())
        return out[:got]

    def sweep_counts(self, which: int) -> np.ndarray:
        """HALS: the sweeps applied to each column of H (which = 0, n values) or row of W (which = 1, m values) by the most recent step of that factor, as np.int32
        (nmfamd_engine_hals_sweep_counts; synchronises).  Raises EngineError on an engine of another algorithm and before any step of that factor -- with
        constant_w no W step runs, so which = 1 keeps what the last W step left, or raises if there was none."""
        out = np.zeros(self.n if which == 0 else self.m, dtype=np.int32)
        fn = self._lib.nmfamd_engine_hals_sweep_counts
        fn.restype = C.c_long
        got = fn(self._h, int(which), C.c_void_p(out.ctypes.data), C.c_long(out.size))
        if got < 0:
            raise EngineError(1, "hals_sweep_counts", (self._lib.nmfamd_engine_last_error(self._h) or b"").decode())
        return out[:got]

    @property
    def frobenius(self) -> float:
        return float(self._lib.nmfamd_engine_frobenius(self._h))

    @property
    def kl_divergence(self) -> float:
        return float(self._lib.nmfamd_engine_kl_divergence(self._h))

    @property
    def divergence_value(self) -> float:
        """The objective of whichever divergence the engine has (generalised KL, Itakura-Saito or the beta-divergence at the engine's beta), of the most
        recent error iteration: the divergence alone, without penalty terms."""
        fn = self._lib.nmfamd_engine_divergence
        fn.restype = C.c_double
        return float(fn(self._h))

    @property
    def rmsd(self) -> float:
        return float(self._lib.nmfamd_engine_rmsd(self._h))

    def kernel_timing(self, every: int):
        """every = k > 0: time the factor-product launches of every k-th iteration; 0: off."""
        self._check(self._lib.nmfamd_engine_kernel_timing(self._h, int(every)), "kernel_timing")

    def kernel_timing_read(self):
        ms = C.c_double(0); cnt = C.c_long(0)
        self._check(self._lib.nmfamd_engine_kernel_timing_read(self._h, C.byref(ms), C.byref(cnt)), "kernel_timing_read")
        return ms.value, cnt.value

    def kernel_timing_read2(self):
        """(total ms, launches, ms an empty event pair reports on the idle stream)."""
        ms = C.c_double(0); cnt = C.c_long(0); ov = C.c_double(0)
        self._check(self._lib.nmfamd_engine_kernel_timing_read2(self._h, C.byref(ms), C.byref(cnt), C.byref(ov)), "kernel_timing_read2")
        return ms.value, cnt.value, ov.value

    def kernel_timing_read3(self):
        """(total_ms, launches, idle_pair_ms, (ms_h, ms_w), (launches_h, launches_w)): the product launches split into the H side (W^T V) and the W side (V H^T)."""
        ms, cnt, ov = C.c_double(0), C.c_long(0), C.c_double(0)
        km, kc = (C.c_double * 2)(), (C.c_long * 2)()
        self._check(self._lib.nmfamd_engine_kernel_timing_read3(self._h, C.byref(ms), C.byref(cnt), C.byref(ov), km, kc), "kernel_timing_read3")
        return ms.value, cnt.value, ov.value, (km[0], km[1]), (kc[0], kc[1])

    def geometry(self) -> dict:
        # (the sized getter: a library older or newer than this mirror never writes past the struct, include/nmfgpu_amd.h)
        g = _Geometry()
        self._check(self._lib.nmfamd_engine_geometry_sized(self._h, C.byref(g), C.c_ulong(C.sizeof(g))), "geometry")
        return {k: getattr(g, k) for k, _ in _Geometry._fields_}

    # ---- column-sharded form ----
    def h_step(self, compute_error: bool = False):
        self._check(self._lib.nmfamd_engine_h_step(self._h, int(compute_error)), "h_step")

    def set_sole_rank(self, sole: bool):
        """A team of one rank: the exchange buffer goes from w_products to w_finish unchanged (nmfamd_engine_set_sole_rank)."""
        self._check(self._lib.nmfamd_engine_set_sole_rank(self._h, int(bool(sole))), "set_sole_rank")

    def w_products(self, exchange_ptr: int):
        self._check(self._lib.nmfamd_engine_w_products(self._h, C.c_void_p(exchange_ptr)), "w_products")

    def w_finish(self, exchange_ptr: int, compute_error: bool = False):
        self._check(self._lib.nmfamd_engine_w_finish(self._h, C.c_void_p(exchange_ptr), int(compute_error)), "w_finish")

    # ---- row-block form of the sharded W step (engine created with row_blocks = world) ----
    def w_update_rows(self, num_rows_ptr: int, hht_ptr: int, row0: int, rows: int, compute_error: bool, colsq_ptr: int):
        self._check(self._lib.nmfamd_engine_w_update_rows(self._h, C.c_void_p(num_rows_ptr), C.c_void_p(hht_ptr), C.c_long(row0), C.c_long(rows),
                                                          int(compute_error), C.c_void_p(colsq_ptr)), "w_update_rows")

    def w_normalize_rows(self, row0: int, rows: int, colsq_ptr: int):
        self._check(self._lib.nmfamd_engine_w_normalize_rows(self._h, C.c_long(row0), C.c_long(rows), C.c_void_p(colsq_ptr)), "w_normalize_rows")

    def w_rows_replaced(self):
        self._check(self._lib.nmfamd_engine_w_rows_replaced(self._h), "w_rows_replaced")

    def w_panel_ptr(self) -> int:
        fn = self._lib.nmfamd_engine_w_panel
        fn.restype = C.c_void_p
        return int(fn(self._h))

    def error_terms(self, which: int) -> np.ndarray:
        cap = max(self.n, self.r)
        out = np.zeros(cap, dtype=self.dtype)
        cnt = self._lib.nmfamd_engine_error_terms(self._h, which, C.c_void_p(out.ctypes.data), C.c_long(cap))
        if cnt < 0:
            raise EngineError(1, "error_terms")
        return out[:cnt]

    def error_terms_to_device(self, dst_ptr: int, capacity: int) -> int:
        """[n_local tr(H^T W^T V) terms | r tr(H H^T W^T W) terms] of the last error iteration -> device buffer (async)."""
        fn = self._lib.nmfamd_engine_error_terms_to_device
        fn.restype = C.c_long
        cnt = fn(self._h, C.c_void_p(dst_ptr), C.c_long(capacity))
        if cnt < 0:
            raise EngineError(1, "error_terms_to_device")
        return int(cnt)

    def debug_read(self, which: int, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=self.dtype)
        self._check(self._lib.nmfamd_engine_debug_read(self._h, which, C.c_void_p(out.ctypes.data), C.c_long(count)), "debug_read")
        return out


class RcclComm:
    """One rank of an RCCL clique, created through RCCL's C API inside libnmfgpu64.so (no torch).  Rank 0 calls
    RcclComm.unique_id() and hands the 128 bytes to the other ranks; every rank then constructs its communicator with
    its HIP device current (blocks until all ranks have arrived)."""

    def __init__(self, unique_id: bytes, world: int, rank: int):
        self._lib = library()
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id has 128 bytes")
        h = C.c_void_p()
        st = self._lib.nmfamd_comm_create_rccl(C.c_char_p(unique_id), int(world), int(rank), C.byref(h))
        if st != 0:
            raise EngineError(st, "nmfamd_comm_create_rccl")
        self._h = h
        self.world, self.rank = int(world), int(rank)

    @staticmethod
    def available() -> bool:
        return bool(library().nmfamd_comm_rccl_available())

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        st = library().nmfamd_comm_unique_id(buf)
        if st != 0:
            raise EngineError(st, "nmfamd_comm_unique_id")
        return buf.raw

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalGroup:
    """Shared state of the rank THREADS of one process (include/nmfgpu_amd.h, nmfamd_local_group_*): create one, hand it to every rank
    thread, each constructs its LocalComm with its own HIP device current."""

    def __init__(self, world: int):
        self._lib = library()
        h = C.c_void_p()
        st = self._lib.nmfamd_local_group_create(int(world), C.byref(h))
        if st != 0:
            raise EngineError(st, "nmfamd_local_group_create")
        self._h, self.world = h, int(world)

    def abort(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_local_group_abort(self._h)

    def selftest_report(self) -> str:
        """One line about the transport's set-up self-test (empty before the ranks have joined, or when NMFAMD_SELFTEST=0 skipped it)."""
        if not getattr(self, "_h", None):
            return ""
        self._lib.nmfamd_local_group_selftest.restype = C.c_char_p
        return (self._lib.nmfamd_local_group_selftest(self._h) or b"").decode()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_local_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalComm:
    """One rank of the in-process transport: the ranks' kernels read each other's buffers where they lie (same device, or peer-mapped devices over xGMI).
    The constructor blocks until every rank of the group has joined."""

    def __init__(self, group: LocalGroup, rank: int):
        self._lib = library()
        self.group = group                       # keep it alive
        h = C.c_void_p()
        st = self._lib.nmfamd_comm_create_local(group._h, int(rank), C.byref(h))
        if st != 0:
            self._lib.nmfamd_local_group_last_error.restype = C.c_char_p
            why = (self._lib.nmfamd_local_group_last_error(group._h) or b"").decode()
            raise EngineError(st, "nmfamd_comm_create_local", why or "a rank of the group failed or the group was aborted")
        self._h = h
        self.world, self.rank = group.world, int(rank)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SHARD_ROW_BLOCKS, SHARD_REPLICATED = 0, 1


class ShardedRun:
    """The column-sharded iteration driven natively (include/nmfgpu_amd.h, nmfamd_sharded_*): `engine` holds this rank's
    columns [total_columns * rank / world, total_columns * (rank + 1) / world) and was created with row_blocks = world."""

    def __init__(self, engine: Engine, comm: RcclComm, rows: int, total_columns: int, mode: int = SHARD_ROW_BLOCKS):
        self._lib = library()
        self.engine, self.comm = engine, comm          # keep both alive
        h = C.c_void_p()
        st = self._lib.nmfamd_sharded_create(engine._h, comm._h, int(mode), C.c_long(rows), C.c_long(total_columns), C.byref(h))
        if st != 0:
            raise EngineError(st, "nmfamd_sharded_create")
        self._h = h
        self._lib.nmfamd_sharded_frobenius.restype = C.c_double
        self._lib.nmfamd_sharded_rmsd.restype = C.c_double
        self._lib.nmfamd_sharded_last_error.restype = C.c_char_p

    def iterate(self, count: int, first_iteration: int = 1, error_every: int = 10, last_iteration: int = 0):
        st = self._lib.nmfamd_sharded_iterate(self._h, int(count), int(first_iteration), int(error_every), int(last_iteration))
        if st != 0:
            raise EngineError(st, "nmfamd_sharded_iterate", (self._lib.nmfamd_sharded_last_error(self._h) or b"").decode())

    def gather_w(self):
        """Row-block mode with the bf16 fragment exchange: gathers the fp32 rows of every rank's block (a collective: every rank calls it)."""
        st = self._lib.nmfamd_sharded_gather_w(self._h)
        if st != 0:
            raise EngineError(st, "nmfamd_sharded_gather_w", (self._lib.nmfamd_sharded_last_error(self._h) or b"").decode())

    @property
    def frobenius(self) -> float:
        return float(self._lib.nmfamd_sharded_frobenius(self._h))

    @property
    def rmsd(self) -> float:
        return float(self._lib.nmfamd_sharded_rmsd(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmfamd_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_columns(total: int, world: int, rank: int):
    """(first, count) of the columns rank `rank` holds when `total` columns are dealt to `world` ranks (sharded.h)."""
    a, b = (total * rank) // world, (total * (rank + 1)) // world
    return a, b - a


def resolve_frobenius(vtv_sorted: np.ndarray, htwtv: np.ndarray, hhtwtw: np.ndarray) -> float:
    lib = library()
    sfx = "f32" if vtv_sorted.dtype == np.float32 else "f64"
    fn = getattr(lib, f"nmfamd_resolve_frobenius_{sfx}")
    fn.restype = C.c_double
    a = np.ascontiguousarray(vtv_sorted); b = np.array(htwtv, dtype=a.dtype); c = np.array(hhtwtw, dtype=a.dtype)
    return float(fn(C.c_void_p(a.ctypes.data), C.c_long(len(a)), C.c_void_p(b.ctypes.data), C.c_long(len(b)),
                    C.c_void_p(c.ctypes.data), C.c_long(len(c))))


def op_factor_product(A: np.ndarray, F: np.ndarray, use_valu: bool = False):
    """OUT (r x X) = F (r x Y) A^T for a host X x Y matrix A.  Returns (OUT, slabs)."""
    A = _f(A); F = _f(F)
    X, Y = A.shape
    r = F.shape[0]
    assert F.shape[1] == Y and A.dtype == F.dtype
    out = np.zeros((r, X), dtype=A.dtype, order="F")
    lib = library()
    if A.dtype == np.float32:
        slabs = C.c_int(0)
        st = lib.nmfamd_op_factor_product_f32(C.c_void_p(A.ctypes.data), C.c_long(_ld(A)), X, Y, C.c_void_p(F.ctypes.data), C.c_long(_ld(F)), r,
                                              C.c_void_p(out.ctypes.data), C.c_long(r), int(use_valu), C.byref(slabs))
        if st != 0:
            raise EngineError(st, "nmfamd_op_factor_product_f32")
        return out, slabs.value
    slabs = C.c_int(0)
    st = lib.nmfamd_op_factor_product_f64(C.c_void_p(A.ctypes.data), C.c_long(_ld(A)), X, Y, C.c_void_p(F.ctypes.data), C.c_long(_ld(F)), r,
                                          C.c_void_p(out.ctypes.data), C.c_long(r), int(use_valu), C.byref(slabs))
    if st != 0:
        raise EngineError(st, "nmfamd_op_factor_product_f64")
    return out, slabs.value


def op_factor_product_bf16(A: np.ndarray, F: np.ndarray) -> np.ndarray:
    """OUT (r x X) = F A^T with both operands rounded to bf16 and fp32 accumulation (any r)."""
    A = _f(A); F = _f(F)
    X, Y = A.shape
    r = F.shape[0]
    out = np.zeros((r, X), dtype=np.float32, order="F")
    st = library().nmfamd_op_factor_product_bf16(C.c_void_p(A.ctypes.data), C.c_long(_ld(A)), X, Y, C.c_void_p(F.ctypes.data), C.c_long(_ld(F)), r,
                                                 C.c_void_p(out.ctypes.data), C.c_long(r))
    if st != 0:
        raise EngineError(st, "nmfamd_op_factor_product_bf16")
    return out


def op_factor_product_x3(A: np.ndarray, F: np.ndarray, reps: int = 0):
    """OUT (r x X) = F A^T at fp32 accuracy on the bf16 matrix pipe: both operands split exactly into three bf16
    terms, six cross products, fp32 accumulation (any r).  Returns OUT, or (OUT, microseconds per launch) if reps > 0."""
    A = _f(A); F = _f(F)
    X, Y = A.shape
    r = F.shape[0]
    out = np.zeros((r, X), dtype=np.float32, order="F")
    us = C.c_double(0.0)
    st = library().nmfamd_op_factor_product_x3(C.c_void_p(A.ctypes.data), C.c_long(_ld(A)), X, Y, C.c_void_p(F.ctypes.data), C.c_long(_ld(F)), r,
                                               C.c_void_p(out.ctypes.data), C.c_long(r), int(reps), C.byref(us))
    if st != 0:
        raise EngineError(st, "nmfamd_op_factor_product_x3")
    return (out, us.value) if reps > 0 else out


def op_gram(P: np.ndarray) -> np.ndarray:
    P = _f(P)
    r, length = P.shape
    G = np.zeros((r, r), dtype=P.dtype, order="F")
    fn = library().nmfamd_op_gram_f32 if P.dtype == np.float32 else library().nmfamd_op_gram_f64
    st = fn(C.c_void_p(P.ctypes.data), C.c_long(_ld(P)), r, length, C.c_void_p(G.ctypes.data), C.c_long(r))
    if st != 0:
        raise EngineError(st, "nmfamd_op_gram")
    return G


GRAM_SPREAD_SLICES, GRAM_KSPLIT_MAX, GRAM_REDUCE_BLOCKS, GRAM_IMAGE_TILES = 3, 8, 16, 10        # csrc/kernels.h


def _ride_args(product, rows: int):
    """(A_prod X x Y, F_prod rows x Y) in float32, Fortran order -> the trailing arguments of a riding test entry, OUT_plain, OUT_ride."""
    if product is None:
        return [None, C.c_long(0), 0, 0, None, C.c_long(0)], None, None
    Ap, Fp = _f(product[0]), _f(product[1])
    X, Y = Ap.shape
    if Ap.dtype != np.float32 or Fp.dtype != np.float32 or Fp.shape != (rows, Y):
        raise ValueError(f"product = (A_prod X x Y, F_prod {rows} x Y) in float32, Fortran order")
    plain = np.full((rows, X), np.nan, dtype=np.float32, order="F")
    ride = np.full((rows, X), np.nan, dtype=np.float32, order="F")
    return [_p(Ap), C.c_long(_ld(Ap)), X, Y, _p(Fp), C.c_long(_ld(Fp))], plain, ride


def split_image_bytes(ks: int, RP: int) -> int:
    """Bytes of the split (3 x bf16) image of ks K-steps of an RP-column panel plus the all-zero step that closes it (k_pack_panel_x3)."""
    return 3 * 16 * (ks + 1) * (RP // 32) * 64


def op_gram_image(P: Optional[np.ndarray], *, colsq_part: Optional[np.ndarray] = None, normalize: int = 0, ksplit: int = 0, spread: int = 0, finish: bool = False,
                  ride: int = 0, launches: int = 1, product=None, with_scale: bool = True, counter: int = 0, length: int = 16, fill=np.nan, guard_slices: int = 1):
    """The rank-64 Gram matrix from the split image of the panel P ((len, 64) float32, C order; None: no image) by one launch, or `launches` in a row into the same
    buffers (nmfamd_op_gram_image_f32, docs/GRAM.md).  ride 0: launch_gram_image_args; 1 / 2: as passengers of the x-tiled / y-tiled split-operand product of
    product = (A_prod X x Y, F_prod 64 x Y) over the 16-row image; 3: of the col_split product (128 x 32 workgroups over 128-row tiles, one slab).  Every output starts as `fill` -- except the pieces of the spread form, which start as the zeros of the one clear its
    contract asks for -- plus `guard_slices` matrices of `fill` behind the last one the form may write.  Returns a dict: `G` ((slices + guard_slices, 64, 64)),
    `scale` (64, or None), `spread_out` ((launches, 64, 64)), `counter` (the word after each launch), `slices`, `workgroups`, `pairs`, `image_ks`, and riding `out_plain`,
    `out_ride`, `xtiles`, `splits`."""
    if P is not None:
        P = np.ascontiguousarray(P, dtype=np.float32)
        if P.ndim != 2 or P.shape[1] != 64:
            raise ValueError("P: (len, 64) panel rows")
        length = P.shape[0]
    cs = None
    if colsq_part is not None:
        cs = np.ascontiguousarray(colsq_part, dtype=np.float32)
        if cs.ndim != 2 or cs.shape[1] != 64:
            raise ValueError("colsq_part: (parts, 64)")
    slices = GRAM_SPREAD_SLICES if spread > 0 else (min(ksplit, GRAM_KSPLIT_MAX) if ksplit > 1 else 1)
    G = np.full((slices + guard_slices, 64, 64), fill, np.float32)
    if spread > 0:
        G[:slices] = 0.0
    scale = np.full(64, fill, np.float32) if with_scale else None
    out = np.full((launches, 64, 64), fill, np.float32)
    cnt = (C.c_uint * (1 + launches))(int(counter))
    plan = (C.c_int * 6)()
    prod, plain, rode = _ride_args(product if ride else None, 64)
    st = library().nmfamd_op_gram_image_f32(_p(P), int(length), _p(cs), 0 if cs is None else int(cs.shape[0]), int(normalize), int(ksplit), int(spread), int(bool(finish)),
                                            int(ride), int(launches), _p(G), C.c_long(G.size), _p(scale), _p(out), cnt, plan, *prod, _p(plain), _p(rode), C.c_long(64))
    if st != 0:
        raise EngineError(st, "nmfamd_op_gram_image_f32")
    return {"G": G, "scale": scale, "spread_out": out, "counter": [int(cnt[1 + i]) for i in range(launches)], "slices": plan[0], "workgroups": plan[1], "pairs": plan[2],
            "image_ks": plan[3], "xtiles": plan[4], "splits": plan[5], "out_plain": plain, "out_ride": rode}


def op_gram64_partials(route: int, *, P: Optional[np.ndarray] = None, partials: Optional[np.ndarray] = None, normalize: int = 0, sumsq_part: Optional[np.ndarray] = None,
                       with_scale: bool = True, x3_ks: Optional[int] = None, product=None, fill=np.nan):
    """The rank-64 Gram matrix from partial 64 x 64 matrices, one launcher per route (nmfamd_op_gram64_partials_f32, docs/GRAM.md): 0 launch_mu64_gram_partials of the
    panel P ((len_pad, 64), len_pad a multiple of 64); 1 launch_mu64_gram_reduce; 2 its riding twin on the split-operand product of product = (A_prod, F_prod 64 x Y),
    6 the same on the col_split product launch;
    3 launch_gram64_from_partials; 4 launch_gram64_normalize_all; 5 launch_gram64_reduce_scale_all.  partials: (parts, 64, 64).  Outputs start as `fill`.
    Returns a dict: `partials`, `G`, `Graw`, `scale`, `P` (the panel after the launch), `x3` (the image's bytes as uint16: bf16 bit patterns), `out_plain`, `out_ride`."""
    len_pad, parts = 0, 0
    if P is not None:
        P = np.array(P, dtype=np.float32, order="C")
        if P.ndim != 2 or P.shape[1] != 64:
            raise ValueError("P: (len_pad, 64)")
        len_pad = P.shape[0]
    if route == 0:
        parts = len_pad // 64
        partials = np.full((max(parts, 1), 64, 64), fill, np.float32)
    else:
        partials = np.ascontiguousarray(partials, dtype=np.float32)
        if partials.ndim != 3 or partials.shape[1:] != (64, 64):
            raise ValueError("partials: (parts, 64, 64)")
        parts = partials.shape[0]
    sq = None if sumsq_part is None else np.ascontiguousarray(sumsq_part, dtype=np.float32)
    if sq is not None and (sq.ndim != 2 or sq.shape[1] != 64):
        raise ValueError("sumsq_part: (sq_parts, 64)")
    G = None if route == 0 else np.full((64, 64), fill, np.float32)
    Graw = np.full((64, 64), fill, np.float32) if route == 4 else None
    scale = np.full(64, fill, np.float32) if (route in (4, 5) or (route != 0 and with_scale)) else None
    x3 = np.full(split_image_bytes(len_pad // 16, 64) // 2, 0x7FC0, np.uint16) if route in (4, 5) else None          # (bf16 NaN)
    ks = len_pad // 16 if x3_ks is None else int(x3_ks)
    prod, plain, rode = _ride_args(product if route in (2, 6) else None, 64)
    st = library().nmfamd_op_gram64_partials_f32(int(route), _p(P), int(len_pad), _p(partials), int(parts), int(normalize), _p(sq), 0 if sq is None else int(sq.shape[0]),
                                                 _p(Graw), _p(G), _p(scale), _p(x3), ks, *prod, _p(plain), _p(rode), C.c_long(64))
    if st != 0:
        raise EngineError(st, "nmfamd_op_gram64_partials_f32")
    return {"partials": partials, "G": G, "Graw": Graw, "scale": scale, "P": P, "x3": x3, "out_plain": plain, "out_ride": rode}


def op_gram_wide(route: int, RP: int, *, P: Optional[np.ndarray] = None, parts: int = 16, partial: Optional[np.ndarray] = None, slices_alloc: Optional[int] = None,
                 sumsq_part: Optional[np.ndarray] = None, with_qx3: bool = True, product=None, fill=np.nan):
    """The fp32 Gram matrix at padded ranks 128 ... 512, one launcher per route (nmfamd_op_gram_wide_f32, docs/GRAM.md): 0 launch_gram_wide_f32; 1
    launch_gram_wide_fused_f32; 2 launch_gram_reduce_x3 alone on the caller's `partial` ((slices, RP, RP), `parts` of them read); 3 the slices as passengers of the
    split-operand product of product = (A_prod X x Y, F_prod r_prod x Y).  P: (len, RP) float32.  The slice buffer starts as `fill` with room for slices_alloc
    matrices (default: parts + 1, so one matrix behind the last slice shows what is left alone).  Returns a dict: `partial`, `G`, `qx3` (uint16 bf16 bit patterns),
    `scale` (RP values, or None without sumsq_part), `parts` (the slice count the launcher settled on), `out_plain`, `out_ride`."""
    length = 0
    if P is not None:
        P = np.ascontiguousarray(P, dtype=np.float32)
        if P.ndim != 2 or P.shape[1] != RP:
            raise ValueError("P: (len, RP)")
        length = P.shape[0]
    if partial is None:
        partial = np.full((max(parts, 0) + 1 if slices_alloc is None else slices_alloc, RP, RP), fill, np.float32)
    else:
        partial = np.array(partial, dtype=np.float32, order="C")
    sq = None if sumsq_part is None else np.ascontiguousarray(sumsq_part, dtype=np.float32)
    if sq is not None and (sq.ndim != 2 or sq.shape[1] != RP):
        raise ValueError("sumsq_part: (sq_parts, RP)")
    G = None if route == 3 else np.full((RP, RP), fill, np.float32)
    qx3 = np.full(split_image_bytes(RP // 16, RP) // 2, 0x7FC0, np.uint16) if (with_qx3 and route in (1, 2)) else None
    scale = np.full(RP, fill, np.float32) if sq is not None else None
    plan = (C.c_int * 1)()
    r_prod = product[1].shape[0] if (route == 3 and product is not None) else 0
    prod, plain, rode = _ride_args(product if route == 3 else None, r_prod)
    st = library().nmfamd_op_gram_wide_f32(int(route), _p(P), int(RP), int(length), int(parts), _p(partial), C.c_long(partial.size), _p(G), _p(qx3), _p(sq),
                                           0 if sq is None else int(sq.shape[0]), _p(scale), plan, *prod, int(r_prod), _p(plain), _p(rode), C.c_long(max(r_prod, 1)))
    if st != 0:
        raise EngineError(st, "nmfamd_op_gram_wide_f32")
    return {"partial": partial, "G": G, "qx3": qx3, "scale": scale, "parts": plan[0], "out_plain": plain, "out_ride": rode}


def inverse_padded_rank(r: int, dtype) -> int:
    """The padded rank RP of the r x r inverse's output (csrc/engine.h, padded_rank)."""
    return 64 if r <= 64 else (-(-r // 64) * 64 if np.dtype(dtype) == np.float64 else -(-r // 128) * 128)


def op_inverse(A: np.ndarray, offdiag: float = 0.0, diag: float = 0.0, route: int = 0, full=False, product=None):
    """(A + regulariser)^-1 of a host r x r matrix (float32 or float64) by one launch, regulariser = offdiag everywhere and diag on the diagonal (docs/INVERSE.md).
    route 0: as the engines launch it (Gauss-Jordan up to r = 64, Householder QR above); 1: Householder at any r; 2 / 3 (float32, r <= 64): as the passenger
    workgroup of the fp32 MFMA product / the split-operand product of product = (A_prod X x Y, F_prod 64 x Y[, OUT 64 x X]).
    full=False returns the r x r inverse.  full=True returns a dict: `inv` (the RP x RP output, NaN where the launch wrote nothing), `a_after` (the RP x RP
    input buffer as the launch left it, its padding NaN), `rp`, and on routes 2 / 3 `out` (the product).  full may also be a dict of caller-owned arrays `inv` and
    `a_after` (RP x RP, Fortran order), which a refused call (EngineError, status 1) leaves as they were; so it does an OUT given in `product`."""
    A = _f(A)
    r = A.shape[0]
    dt = A.dtype
    if dt not in (np.float32, np.float64) or A.shape[1] != r:
        raise ValueError("op_inverse takes a square float32 or float64 matrix")
    RP = inverse_padded_rank(r, dt)
    given = full if isinstance(full, dict) else {}
    inv = given.get("inv")
    if inv is None:
        inv = np.full((RP, RP), np.nan, dtype=dt, order="F")
    after = given.get("a_after")
    if after is None and full:
        after = np.full((RP, RP), np.nan, dtype=dt, order="F")
    for a in (inv, after):
        if a is not None and (a.shape != (RP, RP) or a.dtype != dt or not a.flags.f_contiguous):
            raise ValueError(f"op_inverse: the full outputs are {RP} x {RP} Fortran-ordered arrays of A's type")
    null = C.c_void_p(None)
    prod = [null, C.c_long(0), 0, 0, null, C.c_long(0), null, C.c_long(0)]
    out = None
    if product is not None:
        Ap, Fp = _f(product[0]), _f(product[1])
        X, Y = Ap.shape
        if Ap.dtype != np.float32 or Fp.dtype != np.float32 or Fp.shape != (64, Y):
            raise ValueError("op_inverse: product = (A_prod X x Y, F_prod 64 x Y) in float32")
        out = product[2] if len(product) > 2 else np.zeros((64, X), dtype=np.float32, order="F")
        if out.shape != (64, X) or out.dtype != np.float32 or not out.flags.f_contiguous:
            raise ValueError("op_inverse: OUT is a 64 x X Fortran-ordered float32 array")
        prod = [C.c_void_p(Ap.ctypes.data), C.c_long(_ld(Ap)), X, Y, C.c_void_p(Fp.ctypes.data), C.c_long(_ld(Fp)), C.c_void_p(out.ctypes.data), C.c_long(64)]
    rp = C.c_int(0)
    f32 = dt == np.float32
    name = "nmfamd_op_inverse_ex_f32" if f32 else "nmfamd_op_inverse_ex_f64"
    scalar = C.c_float if f32 else C.c_double
    st = getattr(library(), name)(C.c_void_p(A.ctypes.data), C.c_long(_ld(A)), r, scalar(offdiag), scalar(diag), int(route), C.c_void_p(inv.ctypes.data),
                                  C.c_void_p(after.ctypes.data) if after is not None else null, C.byref(rp), *prod)
    if st != 0:
        raise EngineError(st, name)
    assert rp.value == RP, (rp.value, RP)
    if not full:
        return np.asfortranarray(inv[:r, :r])
    return {"inv": inv, "a_after": after, "rp": RP, "out": out}


def op_factor_passes(P: np.ndarray, theta: float = 0.0, colsq: Optional[np.ndarray] = None, reps: int = 0):
    """The passes between the update of a factor panel and the next product at padded rank 256 with bf16 product operands
    (kernels_tri.hip).  P: (len, r) panel rows, 129 <= r <= 256.  Returns a dict: `panel` (after the optional column normalisation
    by the r sums of squares `colsq`), `pack` (the smoothed panel as the bf16 product operand, widened to fp32), `gram` (P^T P of
    the returned panel), `gram_smoothed`, and with reps > 0 `us_finish`, `us_gram` (microseconds per launch group)."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    length, r = P.shape
    out = {"panel": np.zeros_like(P), "pack": np.zeros_like(P), "gram": np.zeros((r, r), np.float32), "gram_smoothed": np.zeros((r, r), np.float32)}
    sq = None if colsq is None else np.ascontiguousarray(colsq, dtype=np.float32)
    if sq is not None and sq.shape != (r,):
        raise ValueError("colsq must hold r values")
    t0, t1 = C.c_double(0.0), C.c_double(0.0)
    st = library().nmfamd_op_factor_passes_f32(C.c_void_p(P.ctypes.data), C.c_long(r), r, length, C.c_void_p(sq.ctypes.data) if sq is not None else None,
                                               C.c_float(theta), C.c_void_p(out["panel"].ctypes.data), C.c_void_p(out["pack"].ctypes.data),
                                               C.c_void_p(out["gram"].ctypes.data), C.c_void_p(out["gram_smoothed"].ctypes.data), int(reps), C.byref(t0), C.byref(t1))
    if st != 0:
        raise EngineError(st, "nmfamd_op_factor_passes_f32")
    if reps > 0:
        out["us_finish"], out["us_gram"] = t0.value, t1.value
    return out


def op_tri_update(P: np.ndarray, num: np.ndarray, Q: np.ndarray, *, old_colsq: Optional[np.ndarray] = None, transform_num: bool = False,
                  num_colsq: Optional[np.ndarray] = None, theta: float = 0.0, frag_theta: float = 0.0, transform_den: bool = False):
    """One multiplicative update of a (len, r) panel the way the rank-256 bf16 path runs it (nmfamd_op_tri_update_f32): pending column scale
    on the old values (given as the sums of squares it comes from), optional scale + smoothing of the numerator rows, the new rows
    unnormalised (`panel`), their bf16 rounding as the product operand (`pack`; smoothed by frag_theta first), the new pending scale
    (`scale`) and the scaled Gram matrix of the rounded rows (`gram`); `gram_raw`, `gram_image` and `diag`: the unscaled matrix, the same matrix read back
    from the split image the reduction writes, its diagonal.  transform_den: the denominator is S D Q D S old instead of old Q (D from num_colsq)."""
    P = np.ascontiguousarray(P, dtype=np.float32); num = np.ascontiguousarray(num, dtype=np.float32); Q = np.ascontiguousarray(Q, dtype=np.float32)
    length, r = P.shape
    if num.shape != P.shape or Q.shape != (r, r):
        raise ValueError("shapes: P, num (len, r); Q (r, r)")
    osc = None if old_colsq is None else np.ascontiguousarray(old_colsq, dtype=np.float32)
    nsc = None if num_colsq is None else np.ascontiguousarray(num_colsq, dtype=np.float32)
    out = {"panel": np.zeros_like(P), "pack": np.zeros_like(P), "scale": np.zeros(r, np.float32), "gram": np.zeros((r, r), np.float32),
           "gram_raw": np.zeros((r, r), np.float32), "gram_image": np.zeros((r, r), np.float32), "diag": np.zeros(r, np.float32)}
    st = library().nmfamd_op_tri_update_f32(C.c_void_p(P.ctypes.data), C.c_void_p(num.ctypes.data), C.c_void_p(Q.ctypes.data), r, length,
                                            C.c_void_p(osc.ctypes.data) if osc is not None else None, int(bool(transform_num)),
                                            C.c_void_p(nsc.ctypes.data) if nsc is not None else None, C.c_float(theta), C.c_float(frag_theta),
                                            int(bool(transform_den)),
                                            C.c_void_p(out["panel"].ctypes.data), C.c_void_p(out["pack"].ctypes.data), C.c_void_p(out["scale"].ctypes.data),
                                            C.c_void_p(out["gram"].ctypes.data), C.c_void_p(out["gram_raw"].ctypes.data), C.c_void_p(out["gram_image"].ctypes.data),
                                            C.c_void_p(out["diag"].ctypes.data))
    if st != 0:
        raise EngineError(st, "nmfamd_op_tri_update_f32")
    return out


def op_hals_sweep(P: np.ndarray, slabs: np.ndarray, G: np.ndarray, r: int, len_valid: int, *, ps: Optional[np.ndarray] = None,
                  sumsq_part: Optional[np.ndarray] = None, penalties: Optional[tuple] = None, _sweeps: Optional[int] = None, _tol: Optional[float] = None,
                  _apg: bool = False):
    """One launch of the HALS sweep (nmfamd_op_hals_sweep_*; with penalties = (l1, l2) through nmfamd_op_hals_sweep_pen_*, zeros included) on padded arrays: P (len_pad, RP) panel columns, slabs (S, slab_stride) with
    slab_stride >= len_pad * RP (slab s is the first len_pad * RP values of row s; the rest of the row is a gap the kernel must not read), G (RP, RP).
    ps (len_pad values) and sumsq_part ((len_pad // 16) * RP values), when given, are copied in before the launch, so entries the kernel leaves
    alone keep the caller's sentinels.  Returns a dict: `P` (the new panel), `ps`, `sumsq_part` (parts x RP) and `parts`."""
    dt = np.dtype(P.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    P = np.array(P, dtype=dt, order="C")
    slabs = np.ascontiguousarray(slabs, dtype=dt); G = np.ascontiguousarray(G, dtype=dt)
    len_pad, RP = P.shape
    S, stride = slabs.shape
    if G.shape != (RP, RP) or stride < len_pad * RP:
        raise ValueError("shapes: P (len_pad, RP); slabs (S, >= len_pad * RP); G (RP, RP)")
    if ps is not None:
        ps = np.array(ps, dtype=dt).reshape(-1)
        if ps.size != len_pad:
            raise ValueError("ps must hold len_pad values")
    if sumsq_part is not None:
        sumsq_part = np.array(sumsq_part, dtype=dt).reshape(-1)
        if sumsq_part.size < (len_pad // 16) * RP:
            raise ValueError("sumsq_part must hold (len_pad // 16) * RP values")
    parts = C.c_int(0)
    lib, real = library(), (C.c_float if dt == np.float32 else C.c_double)
    counts = None
    if _apg and _tol is not None:      # (op_apg_steps_dyn)
        counts = np.full(len_pad, -1, dtype=np.int32)
        fn = lib.nmfamd_op_apg_steps_dyn_f32 if dt == np.float32 else lib.nmfamd_op_apg_steps_dyn_f64
        extra = (real(penalties[0]), real(penalties[1]), C.c_int(_sweeps), real(_tol), C.c_void_p(counts.ctypes.data))
    elif _apg:                   # (op_apg_steps)
        fn, extra = (lib.nmfamd_op_apg_steps_f32 if dt == np.float32 else lib.nmfamd_op_apg_steps_f64), (real(penalties[0]), real(penalties[1]), C.c_int(_sweeps))
    elif _tol is not None:       # (op_hals_sweeps_dyn)
        counts = np.full(len_pad, -1, dtype=np.int32)
        fn = lib.nmfamd_op_hals_sweeps_dyn_f32 if dt == np.float32 else lib.nmfamd_op_hals_sweeps_dyn_f64
        extra = (real(penalties[0]), real(penalties[1]), C.c_int(_sweeps), C.c_double(_tol), C.c_void_p(counts.ctypes.data))
    elif _sweeps is not None:    # (op_hals_sweeps)
        fn, extra = (lib.nmfamd_op_hals_sweeps_f32 if dt == np.float32 else lib.nmfamd_op_hals_sweeps_f64), (real(penalties[0]), real(penalties[1]), C.c_int(_sweeps))
    elif penalties is None:
        fn, extra = (lib.nmfamd_op_hals_sweep_f32 if dt == np.float32 else lib.nmfamd_op_hals_sweep_f64), ()
    else:
        fn, extra = (lib.nmfamd_op_hals_sweep_pen_f32 if dt == np.float32 else lib.nmfamd_op_hals_sweep_pen_f64), (real(penalties[0]), real(penalties[1]))
    st = fn(C.c_void_p(P.ctypes.data), C.c_void_p(slabs.ctypes.data), S, C.c_long(stride), C.c_void_p(G.ctypes.data), RP, int(r), len_pad,
            int(len_valid), C.c_void_p(ps.ctypes.data) if ps is not None else None,
            C.c_void_p(sumsq_part.ctypes.data) if sumsq_part is not None else None, C.byref(parts), *extra)
    if st != 0:
        raise EngineError(st, "nmfamd_op_hals_sweep")
    k = parts.value
    out = {"P": P, "ps": ps, "sumsq_part": None if sumsq_part is None else sumsq_part[:k * RP].reshape(k, RP), "parts": k}
    if counts is not None:
        out["counts"] = counts
    return out


def op_hals_sweeps(P: np.ndarray, slabs: np.ndarray, G: np.ndarray, r: int, len_valid: int, sweeps: int, *, l1=0.0, l2=0.0, ps: Optional[np.ndarray] = None,
                   sumsq_part: Optional[np.ndarray] = None):
    """One launch of `sweeps` HALS sweeps in a row with the penalties (l1, l2) (nmfamd_op_hals_sweeps_*; kernels_hals_multi.hip), on the arrays of op_hals_sweep
    and with its result; ps and sumsq_part describe the final state.  sweeps = 1 is op_hals_sweep's launch; outside 1 ... 64 it is refused."""
    return op_hals_sweep(P, slabs, G, r, len_valid, ps=ps, sumsq_part=sumsq_part, penalties=(l1, l2), _sweeps=_count(sweeps))


def op_hals_sweeps_dyn(P: np.ndarray, slabs: np.ndarray, G: np.ndarray, r: int, len_valid: int, sweeps: int, tol: float, *, l1=0.0, l2=0.0,
                       ps: Optional[np.ndarray] = None, sumsq_part: Optional[np.ndarray] = None):
    """One launch of at most `sweeps` HALS sweeps with per-column dynamic stopping at the tolerance tol (nmfamd_op_hals_sweeps_dyn_*; kernels_hals_dyn.hip,
    docs/HALS.md "Dynamic stopping"), on the arrays of op_hals_sweep.  Returns what op_hals_sweeps returns plus `counts` (len_pad np.int32 values: the sweeps applied
    to each column, 0 on padding).  Always the dynamic kernel, one sweep included; tol outside (0, 1) is refused."""
    return op_hals_sweep(P, slabs, G, r, len_valid, ps=ps, sumsq_part=sumsq_part, penalties=(l1, l2), _sweeps=int(sweeps), _tol=float(tol))


def op_apg_steps(P: np.ndarray, slabs: np.ndarray, G: np.ndarray, r: int, len_valid: int, steps: int, *, l1=0.0, l2=0.0, ps: Optional[np.ndarray] = None,
                 sumsq_part: Optional[np.ndarray] = None):
    """One launch of `steps` accelerated projected-gradient steps of NeNMF with the penalties (l1, l2) (nmfamd_op_apg_steps_*; kernels_nenmf.hip, docs/NENMF.md),
    on the arrays of op_hals_sweep and with its result; ps and sumsq_part describe the final projected iterate, `parts` = len_pad / 32 (float32) or len_pad / 16
    (float64).  Padded ranks 64 and 128; steps outside 1 ... 256 are refused."""
    return op_hals_sweep(P, slabs, G, r, len_valid, ps=ps, sumsq_part=sumsq_part, penalties=(l1, l2), _sweeps=_count(steps), _apg=True)


def op_apg_steps_dyn(P: np.ndarray, slabs: np.ndarray, G: np.ndarray, r: int, len_valid: int, steps: int, tol: float, *, l1=0.0, l2=0.0,
                     ps: Optional[np.ndarray] = None, sumsq_part: Optional[np.ndarray] = None):
    """One launch of at most `steps` steps of NeNMF with per-column dynamic stopping at the tolerance tol (nmfamd_op_apg_steps_dyn_*; kernels_nenmf_dyn.hip,
    docs/NENMF.md "Dynamic stopping"), on the arrays of op_apg_steps.  Returns what op_apg_steps returns plus `counts` (len_pad np.int32 values: the steps applied to
    each column, 0 on padding).  Always the dynamic kernel, one step included; tol outside (0, 1) is refused."""
    return op_hals_sweep(P, slabs, G, r, len_valid, ps=ps, sumsq_part=sumsq_part, penalties=(l1, l2), _sweeps=int(steps), _tol=float(tol), _apg=True)


def op_beta_half_step(A: np.ndarray, B: np.ndarray, X: np.ndarray, r: int, out_valid: int, red_valid: int, beta: int, form: int = 0, *,
                      dsum: Optional[np.ndarray] = None, force_slabs: int = 0):
    """One half-step of the dense beta-divergence update (nmfamd_op_beta_half_step_*) on padded arrays: A (out_pad, RP) the panel that is updated, B (red_pad, RP)
    the other panel, X (out_pad, ldx) the image of V (X[o, k]; zero on the padding).  beta: 1 (KL; dsum = the RP column sums of B) or 0 (Itakura-Saito).
    form: 0 update, 1 update + error terms, 2 error terms only.  Returns a dict: `A` (the new panel), `t_frob`, `t_div` (out_pad values each; None for form 0),
    `sumsq_part`, `sum_part` ((out_pad // 128, RP)) and `slabs`."""
    return _beta_half_step(A, B, X, r, out_valid, red_valid, int(beta), form, dsum, force_slabs, None)


def _beta_half_step(A, B, X, r, out_valid, red_valid, beta, form, dsum, force_slabs, penalties, Omega=None, mixed=False):
    dt = np.dtype(A.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    if mixed and dt != np.dtype(np.float32):
        raise TypeError("the mixed-precision half-step is float32 only")
    A = np.array(A, dtype=dt, order="C"); B = np.ascontiguousarray(B, dtype=dt); X = np.ascontiguousarray(X, dtype=dt)
    out_pad, RP = A.shape
    red_pad = B.shape[0]
    if B.shape[1] != RP or X.shape[0] != out_pad or X.shape[1] < red_pad:
        raise ValueError("shapes: A (out_pad, RP); B (red_pad, RP); X (out_pad, >= red_pad)")
    d = None if dsum is None else np.ascontiguousarray(dsum, dtype=dt)
    if d is not None and d.shape != (RP,):
        raise ValueError("dsum must hold RP values")
    terms = form in (1, 2)
    tf = np.zeros(out_pad, dt) if terms else None
    td = np.zeros(out_pad, dt) if terms else None
    parts = out_pad // 128
    sq, sm = np.zeros((max(parts, 1), RP), dt), np.zeros((max(parts, 1), RP), dt)
    slabs = C.c_int(0)
    lib = library()
    lead = ()
    if Omega is not None:
        Omega = np.ascontiguousarray(Omega, dtype=dt)
        if Omega.shape != X.shape:
            raise ValueError("Omega must have the shape of X")
        lead = (C.c_void_p(Omega.ctypes.data),)
        fn = lib.nmfamd_op_beta_half_step_weighted_f32 if dt == np.float32 else lib.nmfamd_op_beta_half_step_weighted_f64
        how = (C.c_double(beta), C.c_double(penalties[0]), C.c_double(penalties[1]))
    elif mixed:
        fn = lib.nmfamd_op_beta_half_step_mixed_f32
        how = (C.c_double(beta), C.c_double(penalties[0]), C.c_double(penalties[1]))
    elif penalties is None:
        fn, how = (lib.nmfamd_op_beta_half_step_f32 if dt == np.float32 else lib.nmfamd_op_beta_half_step_f64), (int(beta),)
    else:
        fn = lib.nmfamd_op_beta_half_step_general_f32 if dt == np.float32 else lib.nmfamd_op_beta_half_step_general_f64
        how = (C.c_double(beta), C.c_double(penalties[0]), C.c_double(penalties[1]))
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    st = fn(ptr(A), ptr(B), ptr(X), *lead, C.c_long(X.shape[1]), RP, int(r), out_pad, int(out_valid), red_pad, int(red_valid), *how, int(form), int(force_slabs),
            ptr(d), ptr(tf), ptr(td), ptr(sq), ptr(sm), C.byref(slabs))
    if st != 0:
        raise EngineError(st, "nmfamd_op_beta_half_step")
    return {"A": A, "t_frob": tf, "t_div": td, "sumsq_part": sq, "sum_part": sm, "slabs": slabs.value}


def op_beta_half_step_general(A: np.ndarray, B: np.ndarray, X: np.ndarray, r: int, out_valid: int, red_valid: int, beta: float, form: int = 0, *,
                              l1: float = 0.0, l2: float = 0.0, dsum: Optional[np.ndarray] = None, force_slabs: int = 0):
    """op_beta_half_step with any finite beta and penalties l1, l2 >= 0 on the updated panel (nmfamd_op_beta_half_step_general_*): A <- A (num / (den + eps + l1 +
    l2 A))^gamma.  beta = 0 and beta = 1 run the Itakura-Saito and KL launches (dsum: beta = 1 only), every other value the general form, whose `t_div` is the
    beta-divergence of Engine.divergence_value.  The same arguments and the same dict otherwise."""
    return _beta_half_step(A, B, X, r, out_valid, red_valid, float(beta), form, dsum, force_slabs, (float(l1), float(l2)))


def op_beta_half_step_mixed(A: np.ndarray, B: np.ndarray, X: np.ndarray, r: int, out_valid: int, red_valid: int, beta: float, form: int = 0, *,
                            l1: float = 0.0, l2: float = 0.0, dsum: Optional[np.ndarray] = None, force_slabs: int = 0):
    """op_beta_half_step_general (float32 only) with the mixed-precision fused launch (nmfamd_op_beta_half_step_mixed_f32): A, B and the mapped Q, R are rounded to
    bf16 as operands of the two products; X, the map, every sum and the update stay float32 (docs/DIVERGENCE.md, "Mixed precision").  The same arguments and dict."""
    return _beta_half_step(A, B, X, r, out_valid, red_valid, float(beta), form, dsum, force_slabs, (float(l1), float(l2)), mixed=True)


def op_beta_half_step_weighted(A: np.ndarray, B: np.ndarray, X: np.ndarray, Omega: np.ndarray, r: int, out_valid: int, red_valid: int, beta: float, form: int = 0, *,
                               l1: float = 0.0, l2: float = 0.0, force_slabs: int = 0):
    """op_beta_half_step_general with per-entry weights (nmfamd_op_beta_half_step_weighted_*): Omega has the shape of X, weights >= 0 and 0 on the padding.  An entry
    with weight 0 is not there, whatever X holds at it; num, den and the error terms of every other entry are scaled by its weight.  The denominator is a product
    at every beta (no dsum).  The same dict."""
    return _beta_half_step(A, B, X, r, out_valid, red_valid, float(beta), form, None, force_slabs, (float(l1), float(l2)), Omega)


def op_beta_update_rows(P: np.ndarray, num_part: np.ndarray, den: np.ndarray, r: int, out_valid: int, beta: float, *, l1: float = 0.0, l2: float = 0.0,
                        acc=None, rho: float = 0.0, flush: bool = False):
    """The update launch of the minibatch update (nmfamd_op_beta_update_rows_*, kernels_beta_online.hip) on padded arrays: P (out_pad, RP) the panel, num_part
    (slabs, out_pad, RP) the slabs' partial numerators, den either (slabs, out_pad, RP) partial denominators or, at beta = 1, the RP denominators.  acc=None:
    P <- P (num / (den + eps + l1 + l2 P))^gamma.  acc=(A, B), two (out_pad, RP) arrays: the online update A <- rho A + P^(1 / gamma) num, B <- rho B + den + ...,
    P <- (A / B)^gamma.  flush: new values below eps become 0.  Returns a dict: `P`, `A`, `B` (new arrays; None without acc) and `sum_part` ((out_pad // 16, RP):
    the sums of the new values over each 16 rows)."""
    dt = np.dtype(P.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    P = np.array(P, dtype=dt, order="C")
    num_part = np.ascontiguousarray(num_part, dtype=dt)
    den = np.ascontiguousarray(den, dtype=dt)
    out_pad, RP = P.shape
    if num_part.ndim != 3 or num_part.shape[1:] != (out_pad, RP):
        raise ValueError("shapes: P (out_pad, RP); num_part (slabs, out_pad, RP)")
    vec = den.ndim == 1
    if (vec and den.shape != (RP,)) or (not vec and den.shape != num_part.shape):
        raise ValueError("den: (slabs, out_pad, RP) partial denominators, or RP denominators at beta = 1")
    A = B = None
    if acc is not None:
        A = np.array(acc[0], dtype=dt, order="C"); B = np.array(acc[1], dtype=dt, order="C")
        if A.shape != P.shape or B.shape != P.shape:
            raise ValueError("acc: two arrays of the shape of P")
    sm = np.zeros((out_pad // 16, RP), dt)
    fn = library().nmfamd_op_beta_update_rows_f32 if dt == np.float32 else library().nmfamd_op_beta_update_rows_f64
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    st = fn(ptr(P), ptr(A), ptr(B), ptr(num_part), None if vec else ptr(den), int(num_part.shape[0]), ptr(den) if vec else None, RP, int(r), out_pad, int(out_valid),
            C.c_double(beta), C.c_double(l1), C.c_double(l2), int(acc is not None), C.c_double(rho), int(bool(flush)), ptr(sm))
    if st != 0:
        raise EngineError(st, "nmfamd_op_beta_update_rows")
    return {"P": P, "A": A, "B": B, "sum_part": sm}


def op_beta_fused(A: np.ndarray, B: np.ndarray, X: np.ndarray, out_valid: int, red_valid: int, beta: float, *, update: bool = True, terms: bool = False,
                  Omega: Optional[np.ndarray] = None, mixed: bool = False, force_slabs: int = 0, fill=np.nan):
    """The fused launch of a half-step alone (nmfamd_op_beta_fused_*: launch_beta_fused; with Omega launch_beta_fused_weighted; with mixed, float32 only,
    launch_beta_fused_bf16) under the plan of op_beta_half_step*: A (out_pad, RP), B (red_pad, RP), X and Omega (out_pad, ldx >= red_pad).  Every output starts
    as `fill`, so what the launch does not write shows.  Returns a dict: `num_part`, `den_part` (slabs, out_pad, RP), `tf_part`, `td_part` ((slabs, out_pad); None
    without terms) and the plan `slabs`, `tiles`, `tiles_per_slab`, `bo`, `kt`."""
    dt = np.dtype(A.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    A = np.ascontiguousarray(A, dtype=dt); B = np.ascontiguousarray(B, dtype=dt); X = np.ascontiguousarray(X, dtype=dt)
    out_pad, RP = A.shape
    red_pad = B.shape[0]
    if B.shape[1] != RP or X.shape[0] != out_pad or X.shape[1] < red_pad:
        raise ValueError("shapes: A (out_pad, RP); B (red_pad, RP); X (out_pad, >= red_pad)")
    if Omega is not None:
        Omega = np.ascontiguousarray(Omega, dtype=dt)
        if Omega.shape != X.shape:
            raise ValueError("Omega must have the shape of X")
    fn = library().nmfamd_op_beta_fused_f32 if dt == np.float32 else library().nmfamd_op_beta_fused_f64
    plan = (C.c_int * 5)()
    how = (C.c_long(X.shape[1]), RP, out_pad, int(out_valid), red_pad, int(red_valid), C.c_double(beta), int(bool(update)), int(bool(terms)), int(bool(mixed)),
           int(force_slabs))
    st = fn(_p(A), _p(B), _p(X), _p(Omega), *how, None, None, None, None, plan)
    if st != 0:
        raise EngineError(st, "nmfamd_op_beta_fused")
    slabs = plan[0]
    num = np.full((slabs, out_pad, RP), fill, dt); den = np.full((slabs, out_pad, RP), fill, dt)
    tf = np.full((slabs, out_pad), fill, dt) if terms else None
    td = np.full((slabs, out_pad), fill, dt) if terms else None
    st = fn(_p(A), _p(B), _p(X), _p(Omega), *how, _p(num), _p(den), _p(tf), _p(td), plan)
    if st != 0:
        raise EngineError(st, "nmfamd_op_beta_fused")
    return {"num_part": num, "den_part": den, "tf_part": tf, "td_part": td, "slabs": plan[0], "tiles": plan[1], "tiles_per_slab": plan[2], "bo": plan[3], "kt": plan[4]}


def op_beta_update(P: np.ndarray, num_part: Optional[np.ndarray], den: Optional[np.ndarray], r: int, out_valid: int, beta: float, *, l1: float = 0.0, l2: float = 0.0,
                   weighted: bool = False, update: bool = True, terms=None, slabs: Optional[int] = None, fill=np.nan):
    """launch_beta_update alone (nmfamd_op_beta_update_*) on caller-built partial panels, in op_beta_update_rows's convention: P (out_pad, RP), num_part (slabs,
    out_pad, RP), den either (slabs, out_pad, RP) partial denominators or the RP values of dsum (the unweighted beta = 1).  terms = (tf_part, td_part), each (slabs,
    out_pad): the launch also adds them into `t_frob`, `t_div`.  update=False: the terms only.  weighted: the launch of the weighted engines.  slabs: only where
    neither num_part nor terms gives it.  Returns a dict: `P` (a new array), `sumsq_part`, `sum_part` ((out_pad // 128, RP)), `t_frob`, `t_div` (out_pad values; None
    without terms); what the launch does not write is `fill`."""
    dt = np.dtype(P.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    P = np.array(P, dtype=dt, order="C")
    out_pad, RP = P.shape
    num_part = None if num_part is None else np.ascontiguousarray(num_part, dtype=dt)
    den = None if den is None else np.ascontiguousarray(den, dtype=dt)
    tf = td = None
    if terms is not None:
        tf = np.ascontiguousarray(terms[0], dtype=dt); td = np.ascontiguousarray(terms[1], dtype=dt)
        if tf.ndim != 2 or tf.shape[1] != out_pad or td.shape != tf.shape:
            raise ValueError("terms: two (slabs, out_pad) arrays")
    if slabs is None:
        slabs = num_part.shape[0] if num_part is not None else tf.shape[0]
    for a in (num_part, den if den is not None and den.ndim != 1 else None):
        if a is not None and a.shape != (slabs, out_pad, RP):
            raise ValueError("shapes: P (out_pad, RP); num_part and den (slabs, out_pad, RP)")
    if tf is not None and tf.shape[0] != slabs:
        raise ValueError("terms: as many slabs as num_part")
    vec = den is not None and den.ndim == 1
    if vec and den.shape != (RP,):
        raise ValueError("den: (slabs, out_pad, RP) partial denominators, or the RP values of dsum")
    sq = np.full((out_pad // 128, RP), fill, dt); sm = np.full((out_pad // 128, RP), fill, dt)
    of = np.full(out_pad, fill, dt) if terms is not None else None
    od = np.full(out_pad, fill, dt) if terms is not None else None
    fn = library().nmfamd_op_beta_update_f32 if dt == np.float32 else library().nmfamd_op_beta_update_f64
    st = fn(_p(P), _p(num_part), None if vec else _p(den), int(slabs), _p(den) if vec else None, RP, int(r), out_pad, int(out_valid), C.c_double(beta), C.c_double(l1),
            C.c_double(l2), int(bool(weighted)), int(bool(update)), _p(tf), _p(td), _p(sq), _p(sm), _p(of), _p(od))
    if st != 0:
        raise EngineError(st, "nmfamd_op_beta_update")
    return {"P": P, "sumsq_part": sq, "sum_part": sm, "t_frob": of, "t_div": od}


def op_hals_normalize(Wt: np.ndarray, H: np.ndarray, sumsq_part: np.ndarray):
    """The HALS column normalisation (nmfamd_op_hals_normalize_*): Wt (mpad, RP) and H (npad, RP) panels, sumsq_part (parts, RP) partial
    sums of squares.  Returns a dict: `Wt`, `H` (new arrays; the inputs are not changed)."""
    dt = np.dtype(Wt.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    Wt = np.array(Wt, dtype=dt, order="C"); H = np.array(H, dtype=dt, order="C")
    sq = np.ascontiguousarray(sumsq_part, dtype=dt)
    mpad, RP = Wt.shape
    npad = H.shape[0]
    if H.shape[1] != RP or sq.ndim != 2 or sq.shape[1] != RP:
        raise ValueError("shapes: Wt (mpad, RP); H (npad, RP); sumsq_part (parts, RP)")
    fn = library().nmfamd_op_hals_normalize_f32 if dt == np.float32 else library().nmfamd_op_hals_normalize_f64
    st = fn(C.c_void_p(Wt.ctypes.data), RP, mpad, C.c_void_p(H.ctypes.data), npad, C.c_void_p(sq.ctypes.data), sq.shape[0])
    if st != 0:
        raise EngineError(st, "nmfamd_op_hals_normalize")
    return {"Wt": Wt, "H": H}


# The launches of the sparse path (kernels_sparse.hip), one each (nmfamd_op_kl_fused_* ... nmfamd_op_sddmm_quotient_*).  Every output array starts filled with `fill`
# (NaN by default) and is NOT cleared on the device: what the launch did not write is still `fill` in the result.
def _sparse_dtype(a: np.ndarray) -> np.dtype:
    dt = np.dtype(a.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    return dt


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _sparse_fn(name: str, dt: np.dtype):
    return getattr(library(), f"nmfamd_op_{name}_{'f32' if dt == np.float32 else 'f64'}")


def _sparse_image(ptr, idx, val, dt):
    ptr = np.ascontiguousarray(ptr, dtype=np.int32); idx = np.ascontiguousarray(idx, dtype=np.int32); val = np.ascontiguousarray(val, dtype=dt)
    if idx.ndim != 1 or idx.shape != val.shape:
        raise ValueError("idx and val: one value per stored entry")
    return ptr, idx, val


def op_kl_fused(ptr: np.ndarray, idx: np.ndarray, val: np.ndarray, A: np.ndarray, B: np.ndarray, rows: int, rows_pad: int, blocks: int = 1,
                a_scale: Optional[np.ndarray] = None, terms: bool = False, *, fill=np.nan):
    """One launch of the fused KL gather (launch_kl_fused): A (>= rows_pad, RP) holds the output rows' own factor rows, B (b_rows, RP) the gathered panel, ptr / idx /
    val the image (ptr: rows + 1 offsets; with blocks > 1 the (rows, blocks + 1) boundary array).  Returns a dict: `out` (blocks, rows_pad, RP) and, with terms,
    `t_vwh`, `t_kl` (blocks, rows_pad) -- else None."""
    dt = _sparse_dtype(val)
    ptr, idx, val = _sparse_image(ptr, idx, val, dt)
    A = np.ascontiguousarray(A, dtype=dt); B = np.ascontiguousarray(B, dtype=dt)
    rows, rows_pad, blocks = int(rows), int(rows_pad), int(blocks)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.shape[0] < rows_pad:
        raise ValueError("shapes: A (rows_pad, RP); B (b_rows, RP)")
    if ptr.shape != ((rows, blocks + 1) if blocks > 1 else (rows + 1,)):
        raise ValueError("ptr: rows + 1 offsets, or the (rows, blocks + 1) boundary array")
    RP = A.shape[1]
    if a_scale is not None:
        a_scale = np.ascontiguousarray(a_scale, dtype=dt)
        if a_scale.shape != (RP,):
            raise ValueError("a_scale: RP values")
    out = np.full((max(blocks, 1), rows_pad, RP), fill, dt)
    tv = np.full((max(blocks, 1), rows_pad), fill, dt) if terms else None
    tk = np.full((max(blocks, 1), rows_pad), fill, dt) if terms else None
    st = _sparse_fn("kl_fused", dt)(_p(ptr), _p(idx), _p(val), C.c_long(len(val)), _p(A), _p(B), C.c_long(B.shape[0]), RP, rows, rows_pad, blocks, _p(a_scale), _p(out),
                                    _p(tv), _p(tk))
    if st != 0:
        raise EngineError(st, "nmfamd_op_kl_fused")
    return {"out": out, "t_vwh": tv, "t_kl": tk}


def masked_norm_parts(rows: int) -> int:
    """The number of per-workgroup partial vectors a masked half-step over `rows` rows leaves with sums of squares (nmfamd_masked_norm_parts)."""
    return int(library().nmfamd_masked_norm_parts(int(rows)))


def op_masked_beta_half_step(ptr: np.ndarray, idx: np.ndarray, val: np.ndarray, A: np.ndarray, B: np.ndarray, rows: int, divergence: str = "kl", beta: Optional[float] = None,
                             l1: float = 0.0, l2: float = 0.0, update: bool = True, terms: bool = False, sumsq: bool = False, *, fill=np.nan):
    """One launch of the masked beta-divergence half-step (launch_masked_beta_half_step, docs/MISSING.md "Beta-divergence"): A (>= rows, RP) the output rows' own
    factor rows, B (b_rows, RP) the gathered panel, ptr / idx / val the image (rows + 1 offsets); divergence "kl", "is" or "beta" with beta, as Engine's
    missing_divergence / missing_beta.  Returns a dict: `A` (a new array: rows >= `rows` and, with update=False, every row as given), `t_frob`, `t_div` (rows
    values, with terms) and `sumsq_part` ((masked_norm_parts(rows), RP), with sumsq) -- pre-filled with `fill`, else None."""
    dt = _sparse_dtype(val)
    ptr, idx, val = _sparse_image(ptr, idx, val, dt)
    A = np.array(A, dtype=dt, order="C"); B = np.ascontiguousarray(B, dtype=dt)
    rows = int(rows)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.shape[0] < rows:
        raise ValueError("shapes: A (>= rows, RP); B (b_rows, RP)")
    if ptr.shape != (rows + 1,):
        raise ValueError("ptr: rows + 1 offsets")
    if (beta is not None) != (divergence == "beta"):
        raise ValueError('beta goes with divergence="beta"')
    RP = A.shape[1]
    tf = np.full(rows, fill, dt) if terms else None
    td = np.full(rows, fill, dt) if terms else None
    parts = masked_norm_parts(rows) if sumsq else 0
    sq = np.full((parts, RP), fill, dt) if sumsq else None
    st = _sparse_fn("masked_beta_half_step", dt)(_p(ptr), _p(idx), _p(val), C.c_long(len(val)), _p(A), C.c_long(A.shape[0]), _p(B), C.c_long(B.shape[0]), RP, rows,
                                                 {"kl": 1, "is": 2, "beta": 3}[divergence], C.c_double(float(beta or 0.0)), C.c_double(float(l1)), C.c_double(float(l2)),
                                                 int(bool(update)), _p(tf), _p(td), _p(sq), parts)
    if st != 0:
        raise EngineError(st, "nmfamd_op_masked_beta_half_step")
    return {"A": A, "t_frob": tf, "t_div": td, "sumsq_part": sq}


def missing_solver_fault(solver=1, sweeps_h=1, sweeps_w=1, l1_w=0.0, l1_h=0.0, l2_w=0.0, l2_h=0.0, *, dtype=np.float32, missing_values=True, missing_divergence=0, r=1):
    """Why Engine.set_missing_solver (and compute's "missingSolver") would refuse these values on an engine of this dtype, rank and missing-value setting -- the
    library's own rule, asked without an engine or a device (nmfamd_missing_solver_fault) -- or None where it would take them.  solver: 0 / 1 as the C interface
    numbers them; the counts travel as doubles, as compute reads them."""
    fn = library().nmfamd_missing_solver_fault
    fn.restype = C.c_char_p
    why = fn(*(C.c_double(float(v)) for v in (solver, sweeps_h, sweeps_w, l1_w, l1_h, l2_w, l2_h)), int(np.dtype(dtype).itemsize), C.c_double(float(missing_values)),
             C.c_double(float(missing_divergence)), int(r))
    return why.decode() if why else None


def op_masked_cd_half_step(ptr: np.ndarray, idx: np.ndarray, val: np.ndarray, A: np.ndarray, B: np.ndarray, rows: int, r: int, sweeps: int = 1, l1: float = 0.0,
                           l2: float = 0.0, normal: bool = False, *, fill=np.nan):
    """One launch of the coordinate-descent half-step over the observed entries (launch_masked_cd_half_step, docs/MISSING.md "Coordinate descent"): A (>= rows, RP)
    the output rows' own factor rows, B (b_rows, RP) the gathered panel, RP 64 or 128, r the coordinates that count, ptr / idx / val the image (rows + 1 offsets).
    Returns a dict: `A` (a new array; rows >= `rows` as given) and, with normal=True, `G` ((rows, RP, RP)) and `c` ((rows, RP)): the normal equations the launch
    formed, pre-filled with `fill` -- else None."""
    dt = _sparse_dtype(val)
    ptr, idx, val = _sparse_image(ptr, idx, val, dt)
    A = np.array(A, dtype=dt, order="C"); B = np.ascontiguousarray(B, dtype=dt)
    rows = int(rows)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.shape[0] < rows:
        raise ValueError("shapes: A (>= rows, RP); B (b_rows, RP)")
    if ptr.shape != (rows + 1,):
        raise ValueError("ptr: rows + 1 offsets")
    RP = A.shape[1]
    G = np.full((rows, RP, RP), fill, dt) if normal else None
    c = np.full((rows, RP), fill, dt) if normal else None
    st = _sparse_fn("masked_cd_half_step", dt)(_p(ptr), _p(idx), _p(val), C.c_long(len(val)), _p(A), C.c_long(A.shape[0]), _p(B), C.c_long(B.shape[0]), RP, int(r), rows,
                                               _count(sweeps), C.c_double(float(l1)), C.c_double(float(l2)), _p(G), _p(c))
    if st != 0:
        raise EngineError(st, "nmfamd_op_masked_cd_half_step")
    return {"A": A, "G": G, "c": c}


def predict_entry_parts(nnz: int) -> int:
    """Workgroups -- and per-workgroup partial sums -- of a predict / score launch over nnz entries (nmfamd_predict_entry_parts): a function of nnz only."""
    return int(library().nmfamd_predict_entry_parts(C.c_long(int(nnz))))


def op_predict_entries(rows: np.ndarray, cols: np.ndarray, Wt: np.ndarray, H: np.ndarray, r: int, vals: Optional[np.ndarray] = None, beta: Optional[float] = None,
                       base: int = 0, want_out: bool = True, out_len: Optional[int] = None, *, fill=np.nan):
    """One launch of the gather of kernels_predict.hip (launch_predict_entries, docs/PREDICT.md) on caller-built padded panels: Wt (w_rows, RP) and H (h_rows, RP) of
    one dtype, r the coordinates that count; rows / cols the coordinates (index base `base`), vals the values (None: predictions only), beta as Engine.score (None:
    no divergence).  Returns a dict: `out` (out_len >= nnz values pre-filled with `fill`, the first nnz written; None without want_out), `part` ((parts, 3) doubles:
    each workgroup's sums of the squared errors, of d_beta and of its absolute summands; None without vals) and `sq`, `div`, `abs_div`: the parts added in index
    order, as the engine adds them."""
    dt = _sparse_dtype(Wt)
    Wt = np.ascontiguousarray(Wt, dtype=dt); H = np.ascontiguousarray(H, dtype=dt)
    rows = np.ascontiguousarray(rows, dtype=np.int32); cols = np.ascontiguousarray(cols, dtype=np.int32)
    if Wt.ndim != 2 or H.ndim != 2 or Wt.shape[1] != H.shape[1]:
        raise ValueError("shapes: Wt (w_rows, RP); H (h_rows, RP)")
    if rows.ndim != 1 or cols.shape != rows.shape:
        raise ValueError("rows and cols: one coordinate pair per entry")
    nnz = int(rows.shape[0])
    if vals is not None:
        vals = np.ascontiguousarray(vals, dtype=dt)
        if vals.shape != rows.shape:
            raise ValueError("vals: one value per entry")
    out_len = nnz if out_len is None else int(out_len)
    out = np.full(max(out_len, 1), fill, dt) if want_out else None
    parts = predict_entry_parts(nnz) if vals is not None else 0
    part = np.full((parts, 3), fill, np.float64) if vals is not None else None
    st = _sparse_fn("predict_entries", dt)(_p(rows), _p(cols), _p(vals), C.c_long(nnz), int(base), _p(Wt), C.c_long(Wt.shape[0]), _p(H), C.c_long(H.shape[0]),
                                           int(Wt.shape[1]), int(r), C.c_double(float("nan") if beta is None else float(beta)), _p(out), C.c_long(out_len), _p(part), parts)
    if st != 0:
        raise EngineError(st, "nmfamd_op_predict_entries")
    res = {"out": out[:out_len] if out is not None else None, "part": part, "sq": None, "div": None, "abs_div": None}
    if part is not None:
        s = [0.0, 0.0, 0.0]
        for w in range(parts):      # in workgroup order, as Engine<T>::predict_entries
            for k in range(3):
                s[k] += float(part[w, k])
        res.update(sq=s[0], div=s[1] if beta is not None else float("nan"), abs_div=s[2] if beta is not None else float("nan"))
    return res


def split_entries(rows, cols, values, fraction: float, seed: int):
    """Deals the coordinate list (rows[p], cols[p], values[p]) into a training part and a held-out part for Engine.score (docs/PREDICT.md): round(fraction * nnz)
    entries, drawn without replacement by numpy's PCG64 seeded with `seed`, are held out; both parts keep the order of the input.  The same arguments give the same
    split.  Returns ((rows, cols, values) of the training part, (rows, cols, values) of the held-out part); the parts are disjoint as positions of the list and
    their union is the list (a coordinate stored twice may land once in each)."""
    rows, cols, values = np.asarray(rows), np.asarray(cols), np.asarray(values)
    if rows.ndim != 1 or cols.shape != rows.shape or values.shape != rows.shape:
        raise ValueError("rows, cols and values: 1-D arrays of one length")
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("fraction must lie in [0, 1]")
    nnz = rows.shape[0]
    held = np.zeros(nnz, dtype=bool)
    held[np.random.Generator(np.random.PCG64(int(seed))).permutation(nnz)[:int(round(float(fraction) * nnz))]] = True
    return (rows[~held], cols[~held], values[~held]), (rows[held], cols[held], values[held])


def exclusion_lists(queries, rows, cols, axis: int = 0, base: int = 0):
    """The exclusion lists of Engine.top_k (docs/TOPK.md) from a coordinate list (rows[p], cols[p]) -- the training entries: "the items this user has already
    rated".  axis=0: query q is row queries[q] and its list holds the columns of the entries of that row; axis=1: the rows of the entries of that column.  queries,
    rows and cols share the index base `base`, and so does the result.  Returns (excl_ptr, excl_idx): int64 offsets of nq + 1 entries and int32 candidate indices,
    a query's candidates in the order of the coordinate list (duplicates stay); a query listed twice gets its list twice."""
    queries = np.asarray(queries); rows = np.asarray(rows); cols = np.asarray(cols)
    if queries.ndim != 1 or rows.ndim != 1 or cols.shape != rows.shape:
        raise ValueError("queries: a 1-D array; rows and cols: 1-D arrays of one length")
    if axis not in (0, 1):
        raise ValueError("axis must be 0 or 1")
    if base not in (0, 1):
        raise ValueError("base must be 0 or 1")
    key, other = (rows, cols) if axis == 0 else (cols, rows)
    order = np.argsort(key, kind="stable")
    sorted_key = key[order]
    lo = np.searchsorted(sorted_key, queries, side="left"); hi = np.searchsorted(sorted_key, queries, side="right")
    counts = (hi - lo).astype(np.int64)
    ptr = np.zeros(queries.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    within = np.arange(int(ptr[-1]), dtype=np.int64) - np.repeat(ptr[:-1], counts)
    idx = other[order][np.repeat(lo.astype(np.int64), counts) + within].astype(np.int32)
    return ptr, idx


def top_k_slabs(nq: int, count: int) -> int:
    """Slices of the candidate range that one workgroup each walks in a top_k launch of nq queries over `count` candidates (nmfamd_top_k_slabs): a function of the
    two numbers only."""
    return int(library().nmfamd_top_k_slabs(C.c_long(int(nq)), C.c_long(int(count))))


TOPK_MAX_K = 64      # nmfamd_top_k_max(); tests/test_gpu_topk_kernel.py compares the two


def op_top_k(queries: np.ndarray, k: int, A: np.ndarray, B: np.ndarray, count: int, r: int, exclude=None, base: int = 0, slabs: int = 0):
    """The two launches of kernels_topk.hip (launch_topk, docs/TOPK.md) on caller-built padded panels: the query panel A (a_rows, RP) and the candidate panel B
    (b_rows, RP) of one dtype, r the coordinates that count, candidates 0 ... count - 1; queries (index base `base`) name rows of A; exclude: None or (excl_ptr,
    excl_idx) as Engine.top_k; slabs: 0 for the plan's top_k_slabs(nq, count), or 1 ... 256.  Returns (indices (nq, k) int32, scores (nq, k))."""
    dt = _sparse_dtype(A)
    A = np.ascontiguousarray(A, dtype=dt); B = np.ascontiguousarray(B, dtype=dt)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("shapes: A (a_rows, RP); B (b_rows, RP)")
    q = np.ascontiguousarray(queries, dtype=np.int32)
    if q.ndim != 1:
        raise ValueError("queries: a 1-D array")
    nq, k = int(q.shape[0]), int(k)
    ep = ip = None
    if exclude is not None:
        ep = np.ascontiguousarray(exclude[0], dtype=np.int64); ip = np.ascontiguousarray(exclude[1], dtype=np.int32)
        if ep.shape != (nq + 1,) or ip.ndim != 1:
            raise ValueError("exclude: (excl_ptr of nq + 1 offsets, excl_idx)")
        if ep[0] == 0 and (np.diff(ep) >= 0).all() and ep[-1] > ip.shape[0]:
            raise ValueError("exclude: excl_ptr names more entries than excl_idx holds")
    idx = np.empty((nq, max(k, 0)), dtype=np.int32); sc = np.empty((nq, max(k, 0)), dtype=dt)
    st = _sparse_fn("top_k", dt)(_p(q), C.c_long(nq), k, int(base), _p(A), C.c_long(A.shape[0]), _p(B), C.c_long(B.shape[0]), C.c_long(int(count)), int(A.shape[1]),
                                 int(r), _p(ep), _p(ip), int(slabs), _p(idx), _p(sc))
    if st != 0:
        raise EngineError(st, "nmfamd_op_top_k")
    return idx, sc


def op_kl_update(P: np.ndarray, num_parts: np.ndarray, den: np.ndarray, scale: Optional[np.ndarray] = None, want_sumsq: bool = False, want_sum: bool = True,
                 part_stride: Optional[int] = None, *, parts: Optional[int] = None, fill=np.nan):
    """One launch of the KL update (launch_kl_update): P (len_pad, RP); num_parts either (parts, len_pad, RP) or, with part_stride, a flat array that holds `parts`
    panels part_stride values apart (the gaps are uploaded with it); den, scale: RP values.  Returns a dict: `P` (a new array), `sumsq_part`, `sum_part`
    ((len_pad // 128, RP), or None where not asked for)."""
    dt = _sparse_dtype(P)
    P = np.array(P, dtype=dt, order="C")
    num = np.ascontiguousarray(num_parts, dtype=dt)
    den = np.ascontiguousarray(den, dtype=dt)
    if P.ndim != 2 or den.shape != (P.shape[1],):
        raise ValueError("shapes: P (len_pad, RP); den RP values")
    len_pad, RP = P.shape
    if part_stride is None:
        if num.ndim != 3 or num.shape[1:] != (len_pad, RP):
            raise ValueError("num_parts: (parts, len_pad, RP), or a flat array with part_stride")
        parts, part_stride = num.shape[0], len_pad * RP
    else:
        part_stride = int(part_stride)
        if parts is None:
            parts = 1 if part_stride == 0 else (num.size - len_pad * RP) // part_stride + 1
        if num.ndim != 1 or parts < 1 or num.size < (parts - 1) * part_stride + len_pad * RP:
            raise ValueError("num_parts: a flat array of (parts - 1) * part_stride + len_pad * RP values")
    if scale is not None:
        scale = np.ascontiguousarray(scale, dtype=dt)
        if scale.shape != (RP,):
            raise ValueError("scale: RP values")
    sq = np.full((len_pad // 128, RP), fill, dt) if want_sumsq else None
    sm = np.full((len_pad // 128, RP), fill, dt) if want_sum else None
    st = _sparse_fn("kl_update", dt)(_p(P), _p(num), int(parts), C.c_long(part_stride), _p(den), _p(scale), RP, len_pad, _p(sq), _p(sm))
    if st != 0:
        raise EngineError(st, "nmfamd_op_kl_update")
    return {"P": P, "sumsq_part": sq, "sum_part": sm}


def op_kl_sums(sum_part: np.ndarray, sumsq_part: Optional[np.ndarray] = None, want_scale: bool = False, *, fill=np.nan):
    """One launch of launch_kl_sums on (parts, RP) partial sums (and partial sums of squares).  Returns a dict: `sums` (RP) and `scale` (RP, or None)."""
    dt = _sparse_dtype(sum_part)
    sa = np.ascontiguousarray(sum_part, dtype=dt)
    sb = np.ascontiguousarray(sumsq_part, dtype=dt) if sumsq_part is not None else None
    if sa.ndim != 2 or (sb is not None and sb.shape != sa.shape):
        raise ValueError("shapes: sum_part, sumsq_part (parts, RP)")
    parts, RP = sa.shape
    sums = np.full(RP, fill, dt)
    scale = np.full(RP, fill, dt) if want_scale else None
    st = _sparse_fn("kl_sums", dt)(_p(sa), _p(sb), parts, RP, _p(sums), _p(scale))
    if st != 0:
        raise EngineError(st, "nmfamd_op_kl_sums")
    return {"sums": sums, "scale": scale}


def op_panel_rowsum(P: np.ndarray, *, fill=np.nan) -> np.ndarray:
    """One launch_panel_rowsum on P (len_pad, RP): the RP sums over the panel's rows."""
    dt = _sparse_dtype(P)
    P = np.ascontiguousarray(P, dtype=dt)
    if P.ndim != 2:
        raise ValueError("P: (len_pad, RP)")
    sums = np.full(P.shape[1], fill, dt)
    st = _sparse_fn("panel_rowsum", dt)(_p(P), P.shape[1], P.shape[0], _p(sums))
    if st != 0:
        raise EngineError(st, "nmfamd_op_panel_rowsum")
    return sums


def op_spmm_rows(ptr: np.ndarray, idx: np.ndarray, val: np.ndarray, P: np.ndarray, rows: int, rows_pad: int, *, fill=np.nan) -> np.ndarray:
    """One launch_spmm_rows: out (rows_pad, RP) with out(row, :) = sum_p val[p] P(idx[p], :), P (p_rows, RP)."""
    dt = _sparse_dtype(val)
    ptr, idx, val = _sparse_image(ptr, idx, val, dt)
    P = np.ascontiguousarray(P, dtype=dt)
    rows, rows_pad = int(rows), int(rows_pad)
    if P.ndim != 2 or ptr.shape != (rows + 1,):
        raise ValueError("shapes: P (p_rows, RP); ptr rows + 1 offsets")
    out = np.full((rows_pad, P.shape[1]), fill, dt)
    st = _sparse_fn("spmm_rows", dt)(_p(ptr), _p(idx), _p(val), C.c_long(len(val)), _p(P), C.c_long(P.shape[0]), P.shape[1], rows, rows_pad, _p(out))
    if st != 0:
        raise EngineError(st, "nmfamd_op_spmm_rows")
    return out


def op_sddmm_quotient(ptr: np.ndarray, idx: np.ndarray, val: np.ndarray, A: np.ndarray, B: np.ndarray, rows: int, terms: bool = False, *, fill=np.nan):
    """One launch_sddmm_quotient: q[p] = val[p] / (A(row, :) . B(idx[p], :) + eps) per stored entry.  Returns a dict: `q` (nnz) and, with terms, `t_vwh`, `t_kl`
    (rows) -- else None."""
    dt = _sparse_dtype(val)
    ptr, idx, val = _sparse_image(ptr, idx, val, dt)
    A = np.ascontiguousarray(A, dtype=dt); B = np.ascontiguousarray(B, dtype=dt)
    rows = int(rows)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.shape[0] < rows or ptr.shape != (rows + 1,):
        raise ValueError("shapes: A (>= rows, RP); B (b_rows, RP); ptr rows + 1 offsets")
    q = np.full(len(val), fill, dt)
    tv = np.full(rows, fill, dt) if terms else None
    tk = np.full(rows, fill, dt) if terms else None
    st = _sparse_fn("sddmm_quotient", dt)(_p(ptr), _p(idx), _p(val), C.c_long(len(val)), _p(A), _p(B), C.c_long(B.shape[0]), A.shape[1], rows, _p(q), _p(tv), _p(tk))
    if st != 0:
        raise EngineError(st, "nmfamd_op_sddmm_quotient")
    return {"q": q, "t_vwh": tv, "t_kl": tk}


class _PanelFused(C.Structure):
    """nmfamd_panel_fused"""
    _fields_ = [("old_scale", C.c_void_p), ("h_side", C.c_int), ("scale", C.c_void_p), ("smooth", C.c_int), ("off", C.c_double), ("diag", C.c_double),
                ("r", C.c_int), ("smooth_out", C.c_void_p), ("x3_out", C.c_void_p)]


PANEL_MODES = {"mu": 0, "ls": 1, "set": 2}
# nmfamd_op_panel_update_last_form: the kernel of kernels_wide.hip a launch went to ("other": the generic kernel, the fp64 ones, the old rank-64 one)
PANEL_FORMS = ("other", "lds64", "wide32", "wide32_fused", "rows128", "wide64")


def op_panel_update(mode, P: np.ndarray, slabs: np.ndarray, Q: np.ndarray, len_valid: int, *, ps: Optional[np.ndarray] = None,
                    sumsq_part: Optional[np.ndarray] = None, num_out: bool = False, gram_partial: bool = False, x3: bool = False, split_q: bool = False,
                    fused: Optional[dict] = None, tri: bool = False, eps: Optional[float] = None, fill=np.nan):
    """One launch of the Frobenius panel update (nmfamd_op_panel_update_*; docs/PANEL_UPDATE.md) on padded arrays: mode "mu" / "ls" / "set", P (len_pad, RP),
    slabs (S, slab_stride) with slab_stride >= len_pad * RP (the rest of a row is a gap the kernel must not read), Q (RP, RP).  ps (len_pad values) and sumsq_part
    (rows x RP, rows >= parts) are copied in before the launch, so what the kernel leaves alone keeps the caller's sentinels; num_out, gram_partial and x3 (the split
    image of the new rows, decoded to float32) are allocated when asked for and start as `fill`.  split_q: the scratch for the split image of Q is handed over (wide
    fp32 panels).  fused = dict(old_scale, h_side, scale, smooth, off, diag, r, smooth_out, x3), every key optional: the launch of the fused iterations (fp32 with Q as
    its split image; fp64).  eps: the engines' (machine epsilon of the type) unless given.  Returns a dict: `P`, `ps`, `sumsq_part` (rows x RP), `num_out`,
    `gram_partial` (len_pad / 64, 64, 64), `x3`, `smooth_out`, `parts`, `form` (one of PANEL_FORMS).  A combination the launcher refuses raises EngineError (status 1) with nothing launched."""
    dt = np.dtype(P.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64")
    mode = PANEL_MODES[mode] if isinstance(mode, str) else int(mode)
    P = np.array(P, dtype=dt, order="C")
    slabs = np.ascontiguousarray(slabs, dtype=dt); Q = np.ascontiguousarray(Q, dtype=dt)
    len_pad, RP = P.shape
    S, stride = slabs.shape
    if Q.shape != (RP, RP) or stride < len_pad * RP:
        raise ValueError("shapes: P (len_pad, RP); slabs (S, >= len_pad * RP); Q (RP, RP)")
    real = C.c_float if dt == np.float32 else C.c_double
    if ps is not None:
        ps = np.array(ps, dtype=dt).reshape(-1)
        if ps.size != len_pad:
            raise ValueError("ps must hold len_pad values")
    rows = 0
    if sumsq_part is not None:
        sumsq_part = np.array(sumsq_part, dtype=dt, order="C").reshape(-1, RP)
        rows = sumsq_part.shape[0]
    num = np.full((len_pad, RP), fill, dt) if num_out else None
    gram = np.full((len_pad // 64, 64, 64), fill, dt) if gram_partial else None
    image = np.full((len_pad, RP), fill, np.float32) if x3 else None
    fx, smooth_out, keep = None, None, []
    if fused is not None:
        unknown = set(fused) - {"old_scale", "h_side", "scale", "smooth", "off", "diag", "r", "smooth_out", "x3"}
        if unknown:
            raise ValueError(f"fused: unknown keys {sorted(unknown)}")

        def vec(name):
            v = fused.get(name)
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=dt).reshape(-1)
            if v.size != RP:
                raise ValueError(f"fused[{name!r}] must hold RP values")
            keep.append(v)
            return v.ctypes.data
        if fused.get("smooth_out"):
            smooth_out = np.full((len_pad, RP), fill, dt)
        if fused.get("x3"):
            image = np.full((len_pad, RP), fill, np.float32)
        fx = _PanelFused(vec("old_scale"), int(bool(fused.get("h_side", 0))), vec("scale"), int(bool(fused.get("smooth", 0))), float(fused.get("off", 0.0)),
                         float(fused.get("diag", 1.0)), int(fused.get("r", 0)), smooth_out.ctypes.data if smooth_out is not None else None,
                         image.ctypes.data if image is not None else None)
    parts = C.c_int(0)
    lib = library()
    fn = lib.nmfamd_op_panel_update_f32 if dt == np.float32 else lib.nmfamd_op_panel_update_f64
    st = fn(mode, _p(P), _p(slabs), S, C.c_long(stride), _p(Q), RP, len_pad, int(len_valid), real(np.finfo(dt).eps if eps is None else eps), _p(ps), _p(sumsq_part),
            C.c_long(rows), _p(num), _p(gram), _p(image) if fused is None else None, int(bool(split_q)), int(bool(tri)), C.byref(fx) if fx is not None else None,
            C.byref(parts))
    if st != 0:
        raise EngineError(st, "nmfamd_op_panel_update")
    return {"P": P, "ps": ps, "sumsq_part": sumsq_part, "num_out": num, "gram_partial": gram, "x3": image, "smooth_out": smooth_out, "parts": parts.value,
            "form": PANEL_FORMS[lib.nmfamd_op_panel_update_last_form()]}


def op_mu64_update(is_w, P: np.ndarray, slabs: np.ndarray, Q: np.ndarray, scale: np.ndarray, len_valid: int, *, tile: int = 32, Gprev: Optional[np.ndarray] = None,
                   compute_error: bool = False, qsplit: int = 0, ns: Optional[tuple] = None, colsq_part: bool = False, ps: Optional[np.ndarray] = None,
                   gram_partial: bool = True, x3: bool = True, eps: Optional[float] = None, fill=np.nan):
    """One launch of the rank-64 fused multiplicative update (nmfamd_op_mu64_update_f32; kernels_mu64.hip): tile = 64 through launch_mu64_update, tile = 32 through
    launch_mu64_update32.  P (len_pad, 64) float32, slabs (S, slab_stride >= len_pad * 64), scale 64 values, Q (64, 64) -- or, with qsplit in (2, 4, 8), (qsplit, 64, 64)
    unscaled slices, and `q_out` comes back.  ns = (off, diag, r): SmoothAround (H side, tile 32).  ps (len_pad values) is copied in first; compute_error on the W side
    needs Gprev (64, 64).  Returns a dict: `P`, `ps`, `gram_partial` (tile 64; len_pad / 64, 64, 64), `colsq_part` (len_pad / 32, 64), `q_out`, `x3` (the decoded split
    image); what was not asked for is None, what the launch leaves alone is `fill`."""
    P = np.array(P, dtype=np.float32, order="C")
    slabs = np.ascontiguousarray(slabs, dtype=np.float32); Q = np.ascontiguousarray(Q, dtype=np.float32); scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    len_pad, RP = P.shape
    S, stride = slabs.shape
    slices = int(qsplit) if int(qsplit) > 1 else 1
    if RP != 64 or stride < len_pad * 64 or scale.size != 64 or Q.size != slices * 4096:
        raise ValueError("shapes: P (len_pad, 64); slabs (S, >= len_pad * 64); scale 64; Q (64, 64) or (qsplit, 64, 64)")
    if ps is not None:
        ps = np.array(ps, dtype=np.float32).reshape(-1)
        if ps.size != len_pad:
            raise ValueError("ps must hold len_pad values")
    if Gprev is not None:
        Gprev = np.ascontiguousarray(Gprev, dtype=np.float32)
        if Gprev.shape != (64, 64):
            raise ValueError("Gprev (64, 64)")
    gram = np.full((len_pad // 64, 64, 64), fill, np.float32) if gram_partial and tile == 64 else None
    colsq = np.full((len_pad // 32, 64), fill, np.float32) if colsq_part else None
    q_out = np.full((64, 64), fill, np.float32) if slices > 1 else None
    image = np.full((len_pad, 64), fill, np.float32) if x3 else None
    off, diag, r = (0.0, 1.0, 0) if ns is None else ns
    st = library().nmfamd_op_mu64_update_f32(int(bool(is_w)), int(tile), _p(P), _p(slabs), S, C.c_long(stride), _p(Q), _p(scale),
                                             C.c_float(np.finfo(np.float32).eps if eps is None else eps), len_pad, int(len_valid), _p(ps), _p(Gprev), int(bool(compute_error)),
                                             _p(gram), _p(colsq), int(qsplit), _p(q_out), int(ns is not None), C.c_float(off), C.c_float(diag), int(r), _p(image))
    if st != 0:
        raise EngineError(st, "nmfamd_op_mu64_update")
    return {"P": P, "ps": ps, "gram_partial": gram, "colsq_part": colsq, "q_out": q_out, "x3": image}


def host_kmeans(data: np.ndarray, k: int, *, seed: int = 0, iterations: int = 100, threshold: float = 0.005):
    """The host-side Lloyd k-means behind computeKMeans and the KMeans*/EInNMF initialisers, without a
    device or context (nmfamd_host_kmeans_*).  Returns (clusters m x k, membership, passes)."""
    lib = library()
    data = _f(data)
    m, n = data.shape
    clusters = np.zeros((m, k), dtype=data.dtype, order="F")
    membership = np.zeros(n, dtype=np.uint32)
    it = C.c_uint(0)
    fn = getattr(lib, "nmfamd_host_kmeans_f32" if data.dtype == np.float32 else "nmfamd_host_kmeans_f64")
    st = fn(C.c_void_p(data.ctypes.data), C.c_long(_ld(data)), m, n, C.c_void_p(clusters.ctypes.data), C.c_long(m), k,
            C.c_void_p(membership.ctypes.data), C.c_uint(seed), C.c_uint(iterations), C.c_double(threshold), C.byref(it))
    if st != 0:
        raise EngineError(st, "host_kmeans")
    return clusters, membership, int(it.value)


NNDSVD, NNDSVD_A, NNDSVD_AR = 100, 101, 102      # `method` values of host_init for the SVD-based start (Parameter "nndsvd" = 0 / 1 / 2 of nmfgpu::compute)


def host_init(V: np.ndarray, r: int, method: int, *, seed: int = 0, want_h: bool = True):
    """W (m x r) and H (r x n) of the MeanColumns / KMeans* / EInNMF initialisers, or of NNDSVD / NNDSVDa / NNDSVDar (method 100 / 101 / 102) (nmfamd_host_init_*)."""
    lib = library()
    V = _f(V)
    m, n = V.shape
    W = np.zeros((m, r), dtype=V.dtype, order="F")
    H = np.zeros((r, n), dtype=V.dtype, order="F") if want_h else None
    fn = getattr(lib, "nmfamd_host_init_f32" if V.dtype == np.float32 else "nmfamd_host_init_f64")
    st = fn(C.c_void_p(V.ctypes.data), C.c_long(_ld(V)), m, n, r, int(method), C.c_uint(seed), C.c_void_p(W.ctypes.data),
            C.c_void_p(H.ctypes.data) if want_h else None)
    if st != 0:
        raise EngineError(st, "host_init")
    return W, H
