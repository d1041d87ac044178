"""Reference of the r x r inverse tests (tests/test_inverse_cpu.py, tests/test_gpu_inverse.py; docs/INVERSE.md): what the kernels of nmfgpu_amd/csrc/inverse_gj64.h
and k_inverse_small (nmfgpu_amd/csrc/kernels.hip) are asked to return, in extended precision.

  regularised   Areg = A + where(i == j, diag, offdiag) as ONE addition in A's type T: what both kernels invert (k_fill_small adds in place in T, the Gauss-Jordan body
                rounds the sum to T on the way in) -- the rule of the reference's KernelFillMatrix;
  refined       numpy.linalg.inv in double, then four Newton steps X += X (I - Areg X) in extended precision (numpy.longdouble where that is the 80-bit type, mpmath at
                113 bits otherwise); residuals are evaluated in the same arithmetic;
  bounds        (a) max(|X Areg - I|, |Areg X - I|) <= 8 eps(T) cond2(Areg), the factor of tests/test_gpu_boundary_rows.py;
                (b) float32 only: |X - fl32(Xref)| <= ulp32(Xref) + 8 2^-52 cond2 max|Xref| element-wise -- the arithmetic is double on exactly Areg, so only the
                    output rounding (half an ulp, one across a rounding tie) and a double-precision inversion error may show;
  gauss_jordan  a numpy restatement of inverse_gj64_body (same pivot key, same update, the pivot rows divided by their pivots at the write-back, double), with the
                deliberate defects of MUTATIONS: the device-free module shows that each of them leaves a bound or an equality of the GPU tests."""
import numpy as np

EXTENDED = np.finfo(np.longdouble).eps < 2e-19        # x87 80-bit; elsewhere (longdouble = double) the refinement runs in mpmath
if not EXTENDED:
    import mpmath
    mpmath.mp.prec = 113
EPS_X = float(np.finfo(np.longdouble).eps) if EXTENDED else 2.0 ** -112

MUTATIONS = ("difference_pivot_row", "regulariser_in_double", "transposed_write_back", "unpermuted_write_back")


def lift(a):
    """A float array in the extended type."""
    a = np.asarray(a)
    if EXTENDED:
        return a.astype(np.longdouble)
    if a.dtype == object:
        return a
    return np.vectorize(mpmath.mpf, otypes=[object])(a.astype(np.float64))


def lower(a, dtype=np.float64):
    return np.asarray(a).astype(dtype)


def regularised(A, offdiag, diag):
    """A + regulariser as one addition in A's type."""
    A = np.asarray(A)
    T = A.dtype.type
    r = A.shape[0]
    reg = np.where(np.eye(r, dtype=bool), T(diag), T(offdiag)).astype(A.dtype)
    out = A + reg
    assert out.dtype == A.dtype
    return out


def cond2(Areg):
    return float(np.linalg.cond(np.asarray(Areg, dtype=np.float64), 2))


def refined_inverse(Areg, steps=4):
    """Areg^-1 in the extended type."""
    A = lift(Areg)
    eye = lift(np.eye(A.shape[0]))
    X = lift(np.linalg.inv(np.asarray(Areg, dtype=np.float64)))
    for _ in range(steps):
        X = X + X @ (eye - A @ X)
    return X


def residual(X, Areg):
    """max(|X Areg - I|, |Areg X - I|) over all elements, evaluated in the extended type; inf if X holds a non-finite value."""
    if not np.all(np.isfinite(np.asarray(X, dtype=np.float64))):
        return np.inf
    A, Xx = lift(Areg), lift(X)
    eye = lift(np.eye(A.shape[0]))
    return float(max(np.abs(Xx @ A - eye).max(), np.abs(A @ Xx - eye).max()))


def bound_a(dtype, cond):
    return 8 * float(np.finfo(dtype).eps) * cond


def ulp32(x):
    """Spacing of float32 at |x| (x in any type)."""
    return np.spacing(np.abs(lower(x, np.float32))).astype(np.float64)


def bound_b(Xref, cond):
    """Element-wise bound (b) on |X - fl32(Xref)|."""
    return ulp32(Xref) + 8 * 2.0 ** -52 * cond * float(np.abs(lower(Xref)).max())


def excess_b(X, Xref, cond):
    """max |X - fl32(Xref)| / bound (b); at most 1 where the bound holds."""
    err = np.abs(np.asarray(X, dtype=np.float64) - lower(Xref, np.float32).astype(np.float64))
    if not np.all(np.isfinite(err)):
        return np.inf
    return float((err / bound_b(Xref, cond)).max())


def pivot_key(v, lane):
    """gj_search's 32-bit key: the float bits of |v| with the low six bits replaced by 63 - lane (the first of equal maxima wins)."""
    bits = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32).view(np.uint32)
    return (bits & ~np.uint32(63)) | (63 - lane).astype(np.uint32)


def gauss_jordan(A, offdiag, diag, mutation=None):
    """inverse_gj64_body in numpy for r <= 64: the identity-padded 64 x 64 matrix in double, lane = row, no row swaps, the permutation undone on the way out.
    The per-element operations are the kernel's up to the contraction of multiply and add and the last bit of 1 / piv.  Returns the r x r result in A's type."""
    assert mutation is None or mutation in MUTATIONS
    A = np.asarray(A)
    r = A.shape[0]
    assert r <= 64
    if mutation == "regulariser_in_double":
        Areg = A.astype(np.float64) + np.where(np.eye(r, dtype=bool), np.float64(A.dtype.type(diag)), np.float64(A.dtype.type(offdiag)))
    else:
        Areg = regularised(A, offdiag, diag).astype(np.float64)
    M = np.eye(64)
    M[:r, :r] = Areg
    lane = np.arange(64)
    used = np.zeros(64, dtype=bool)
    rowof, pivrow = np.zeros(64, dtype=int), np.zeros(64, dtype=int)
    pending = np.ones(64)                                          # 1 / piv of the step a row was the pivot row of: applied when the result is written
    for k in range(64):
        v = M[:, k].copy()
        key = np.where(used, np.uint32(0), pivot_key(v, lane))
        p = 63 - int(key.max() & 63)
        pivinv = 1.0 / v[p]
        fm = v * pivinv
        rowof[p], pivrow[k] = k, p
        used[p] = True
        prow = M[p, :].copy()
        if mutation == "difference_pivot_row":
            fadj = fm.copy()
            fadj[p] = 1.0 - pivinv
            M = M - fadj[:, None] * prow[None, :]                  # row p: row_p - (1 - 1 / piv) row_p
            M[:, k] = -fm
            M[p, k] = pivinv
        else:
            fadj = fm.copy()
            fadj[p] = 0.0
            M = M - fadj[:, None] * prow[None, :]                  # row p: left as it is, its division by piv deferred to the write-back
            pending[p] = pivinv
            M[:, k] = -fm
            M[p, k] = 1.0
    M = M * pending[:, None]
    out = np.zeros((64, 64))
    for i in range(64):
        for q in range(64):
            kk, j = (i, q) if mutation == "unpermuted_write_back" else (rowof[i], pivrow[q])
            if mutation == "transposed_write_back":
                kk, j = j, kk
            out[kk, j] = M[i, q]
    return out[:r, :r].astype(A.dtype)
