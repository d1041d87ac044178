"""float64 restatements of the two launches of a dense beta-divergence half-step, one launch at a time, with element-wise bounds (docs/DIVERGENCE.md, "Kernel-level
tests"): fused() restates launch_beta_fused / launch_beta_fused_weighted / launch_beta_fused_bf16 slab by slab from the plan the entry returns, update() restates
launch_beta_update on GIVEN partial panels.  tests/test_beta_kernel_cpu.py ties both to the references the project already has and shows that the bounds catch the
defects listed in MUTATIONS; tests/test_gpu_beta_fused.py and tests/test_gpu_beta_update.py hold the kernels to them.

Bounds.  Every quantity is a pair (value, absolute bound) -- class E -- and every operation below is one statement of the kernels: it propagates the operands'
bounds and adds one rounding of the type, u (|value| + propagated).  A sum of n terms adds gamma(n) = n u / (1 - n u) of the sum of the magnitudes, which holds
for any order of summation and with or without fused multiply-adds (docs/PANEL_UPDATE.md).  The counts that result:
    P           RP products and additions, then the eps addition                              gamma(RP + 1) (|A| |B|^T + eps)
    beta = 1    one division;   beta = 0  one reciprocal and two products;   weighted  one more product each
    general     t = exp2((beta - 2) log2 p): the power's bound (below), then one product each for Q and R
    num, den    one rounding per reduction row of the slab on top of Q's and R's bounds       gamma(rows of the slab)
    update      S - 1 for each slab sum, the denominator's additions (one, or three and a product when penalised), the quotient, the root, the product
The error terms are sums with cancellation (x log q - x + p, ratio - log ratio - 1): their bounds are on the sums of the absolute values of the pieces.
The mixed form rounds A, B, Q and R to bf16 as tests/beta_mixed_reference.py does; Q and R are rounded AFTER the fp32 map, so where the fp32 value and the exact
one fall on two sides of a rounding boundary the operands differ by a whole bf16 ulp: the bound carries 2 u_bf16 |q| for that (u_bf16 = 2^-9).

What no count of roundings gives -- the hardware log2 / exp2 of the general map (v_log_f32, v_exp_f32), the device library's log, log2, exp2 and sqrt in the terms and
in the gamma-power -- is bounded as  u (POW_C0 + POW_C1 |y log2 p|)  per power p^y and LIB_ULPS u per library call.  No document shipped with the toolchain states
the accuracy of these, so the constants are MEASURED: the smallest integers with which the worst error / bound ratio of the GPU modules' random cases stays below
1/2 (a margin of 2; the table of docs/DIVERGENCE.md has the ratios).  tests/test_beta_kernel_cpu.py shows that every defect still leaves the bounds with them."""
import numpy as np

from tests import beta_general_reference as gen
from tests.beta_mixed_reference import round_bf16
from tests.panel_update_reference import eps_of, gamma, unit_roundoff      # noqa: F401  (shared definitions)

POW_C0 = 4.0        # ulps of a power p^y at y log2 p = 0: the exp2 itself and the rounding of its argument
POW_C1 = 4.0        # ulps per unit of |y log2 p|: the log2's own error and the product's, magnified by exp2 (ln 2 per unit of absolute error)
LIB_ULPS = 4.0      # ulps of one call of log / sqrt
U_BF16 = 2.0 ** -9

# the defects tests/test_beta_kernel_cpu.py applies (fused: 1-4, 6-9; update: 5, 7, 10-12), numbered as in docs/DIVERGENCE.md
MUTATIONS = ("drop_tile", "drop_rank_term", "swap_row_groups", "no_eps_p", "no_eps_den", "red_valid_off_by_one", "out_valid_off_by_one", "den_from_q",
             "weight_twice", "drop_slab", "l2_new_value", "wrong_gamma")


class E:
    """A value with an absolute bound of its error, in a type of unit roundoff u."""

    def __init__(self, v, b=0.0, u=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.b = np.broadcast_to(np.asarray(b, dtype=np.float64), self.v.shape)
        self.u = u

    def _r(self, v, p):       # one rounding on top of the propagated bound p
        return E(v, p + self.u * (np.abs(v) + p), self.u)

    @staticmethod
    def of(x, u):
        return x if isinstance(x, E) else E(x, 0.0, u)

    def __add__(self, o):
        o = E.of(o, self.u)
        return self._r(self.v + o.v, self.b + o.b)

    def __sub__(self, o):
        o = E.of(o, self.u)
        return self._r(self.v - o.v, self.b + o.b)

    def __mul__(self, o):
        o = E.of(o, self.u)
        return self._r(self.v * o.v, np.abs(self.v) * o.b + np.abs(o.v) * self.b + self.b * o.b)

    def __truediv__(self, o):
        o = E.of(o, self.u)
        room = np.abs(o.v) - o.b
        assert np.all(room[np.isfinite(room)] > 0), "a divisor's bound reaches zero"
        v = self.v / o.v
        return self._r(v, (self.b + np.abs(v) * o.b) / room)

    def rdiv(self, x):
        return E(x * np.ones_like(self.v), 0.0, self.u) / self

    def exact(self, f):       # an operation that does not round (a selection, a product with a power of two, a reshape)
        return E(f(self.v), f(self.b), self.u)

    def sqrt(self):
        v = np.sqrt(self.v)
        p = v - np.sqrt(np.maximum(self.v - self.b, 0.0))
        return E(v, p + LIB_ULPS * self.u * (v + p), self.u)

    def log(self):
        room = self.v - self.b
        assert np.all(room > 0)
        v = np.log(self.v)
        return E(v, self.b / room + LIB_ULPS * self.u * np.abs(v), self.u)

    def power(self, y):
        """p^y as exp2(y log2 p) for p > 0."""
        room = self.v - self.b
        assert np.all(room > 0)
        v = self.v ** y
        p = v * ((self.v / room) ** abs(y) - 1.0)
        return E(v, p + self.u * (POW_C0 + POW_C1 * np.abs(y * np.log2(self.v))) * (v + p), self.u)

    def bf16(self):
        """Rounded to bf16 after a rounding in the type: within the bound plus two half-ulps of bf16 of the exact value's rounding."""
        return E(round_bf16(self.v), self.b + U_BF16 * (2 * np.abs(self.v) + self.b), self.u)

    def where(self, mask, other=0.0):
        return E(np.where(mask, self.v, other), np.where(mask, self.b, 0.0), self.u)

    def sum(self, axis, n=None):
        n = self.v.shape[axis] if n is None else n
        mag = (np.abs(self.v) + self.b).sum(axis=axis)
        return E(self.v.sum(axis=axis), self.b.sum(axis=axis) + (gamma(n, self.u) * mag if n > 0 else 0.0), self.u)

    def dot(self, B, n=None):
        """self (o x k) times an exactly known B (k x c): one rounding per term."""
        n = B.shape[0] if n is None else n
        mag = (np.abs(self.v) + self.b) @ np.abs(B)
        return E(self.v @ B, self.b @ np.abs(B) + (gamma(n, self.u) * mag if n > 0 else 0.0), self.u)


def roundoff_of(dtype):
    """The unit roundoff the bounds are built with.  float32: the kernel's.  float64: twice the kernel's -- the restatement itself runs in float64 there, statement
    for statement, so what is bounded is the distance of two float64 evaluations and each statement counts once for either."""
    return unit_roundoff(dtype) * (2 if np.dtype(dtype) == np.float64 else 1)


def slab_rows(plan, s):
    """The reduction rows [k0, k1) slab s of the plan walks."""
    t0 = s * plan["tiles_per_slab"]
    t1 = min(t0 + plan["tiles_per_slab"], plan["tiles"])
    return t0 * plan["kt"], t1 * plan["kt"]


def host_plan(red_pad, RP, dtype, slabs):
    """The plan plan_beta_half_step returns for a forced slab count (kernels_beta.hip), for the device-free module."""
    if np.dtype(dtype) == np.float32:
        bo, kt = (64, 64) if RP == 256 else (32, 128)
    else:
        bo, kt = 8, 32
    tiles = red_pad // kt
    best = max(1, min(slabs, tiles, 16))
    per = -(-tiles // best)
    return {"bo": bo, "kt": kt, "tiles": tiles, "tiles_per_slab": per, "slabs": -(-tiles // per)}


def entry_map(Xv, W, Pe, beta, *, mixed=False, terms=False, mutate=None):
    """beta_entry / betaw_entry / mixed_entry on the valid block: Xv (exact values), W (weights or None), Pe = P + eps as an E.  Returns Q, R (R None at the
    unweighted beta = 1) and, with terms, the pieces' sums per row as E values (tf, td)."""
    u = Pe.u
    obs = None if W is None else W > 0
    X = np.where(obs, Xv, 1.0) if obs is not None else Xv      # (what lies under a zero weight never enters the arithmetic)
    Xe = E(X, 0.0, u)
    tf = td = None
    if beta == 1:
        Q = Xe / Pe
        R = None
        if terms:
            pos = X > 0
            lg = (Q.where(pos, 1.0)).log()
            d1 = (Xe * lg).where(pos) - Xe + Pe
    elif beta == 0:
        ip = Pe.rdiv(1.0)
        R = ip
        Q = Xe * ip * ip
        if terms:
            ratio = Xe * ip
            d1 = ratio - ratio.log() - 1.0
    else:
        t = Pe.power(beta - 2.0)
        Q = Xe * t
        R = t * Pe
        if terms:
            pos = X > 0
            xb = E(np.where(pos, X, 1.0), 0.0, u).power(beta).where(pos)
            d1 = xb + (R * Pe) * (beta - 1.0) - (Xe * R) * beta
    if terms:
        d = Xe - Pe
        f1 = d * d if W is None else (d * W) * d
        if W is not None:
            d1 = d1 * W
        if obs is not None:
            f1, d1 = f1.where(obs), d1.where(obs)
        tf, td = f1, d1
    if W is not None:
        Ww = W * W if mutate == "weight_twice" else W
        Q = (Q * Ww).where(obs)
        R = E(np.where(obs, Ww, 0.0), 0.0, u) if beta == 1 else (R * Ww).where(obs)
    if mixed:
        Q = Q.bf16()
        R = None if R is None else R.bf16()
    return Q, R, tf, td


def rounded(x, dtype):
    """x with its value rounded to dtype: the exact cases' P + eps, which rounds back to P (or to eps) in the type and not in float64."""
    return E(x.v.astype(dtype).astype(np.float64), x.b, x.u)


def fused(A, B, X, out_valid, red_valid, beta, plan, dtype, *, Omega=None, mixed=False, update=True, terms=False, exact=False, mutate=None):
    """The fused launch, slab by slab.  exact: P + eps is rounded to dtype, as the exact cases need it (every later value is then representable).  A (out_pad, RP), B (red_pad, RP), X / Omega (out_pad, ldx) as the entry takes them; plan: the dict the entry returns (or
    host_plan).  Returns a dict of E values: num, den (slabs, out_pad, RP; den None where the launch writes none: the unweighted beta = 1), tf, td (slabs, out_pad)."""
    u, eps = roundoff_of(dtype), eps_of(dtype)
    out_pad, RP = A.shape
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    ov = out_valid - 1 if mutate == "out_valid_off_by_one" else out_valid
    rv = red_valid - 1 if mutate == "red_valid_off_by_one" else red_valid
    Ao, Bo = (round_bf16(A), round_bf16(B)) if mixed else (A, B)
    S = plan["slabs"]
    has_den = beta != 1 or Omega is not None
    num = np.zeros((2, S, out_pad, RP)); den = np.zeros((2, S, out_pad, RP)); tf = np.zeros((2, S, out_pad)); td = np.zeros((2, S, out_pad))
    for s in range(S):
        k0, k1 = slab_rows(plan, s)
        rows = k1 - k0
        if mutate == "drop_tile":
            k1 -= plan["kt"]
        k1 = min(k1, rv)
        if k1 <= k0 or ov <= 0:
            continue
        a, b = Ao[:ov], Bo[k0:k1]
        a_p = a.copy()
        if mutate == "drop_rank_term":
            a_p[:, np.argmax(np.abs(a).sum(axis=0))] = 0        # one of the RP terms of every P
        P = E(a_p @ b.T, gamma(RP, u) * (np.abs(a_p) @ np.abs(b).T), u)
        Pe = P if mutate == "no_eps_p" else P + eps
        if exact:
            Pe = rounded(Pe, dtype)
        W = None if Omega is None else np.asarray(Omega, dtype=np.float64)[:ov, k0:k1]
        Q, R, f1, d1 = entry_map(np.asarray(X, dtype=np.float64)[:ov, k0:k1], W, Pe, beta, mixed=mixed, terms=terms, mutate=mutate)
        if update:
            b2 = b
            if mutate == "swap_row_groups":
                # rows 0 .. 3 and 4 .. 7 of every 32 of the tile change places in the second product's B operand
                idx = np.arange(k0, k1)
                j = (idx - k0) % 32
                b2 = Bo[np.where(j < 4, idx + 4, np.where(j < 8, idx - 4, idx))]      # (a partner past red_valid is a zero row of B)
            n = Q.dot(b2, rows)
            num[0, s, :ov], num[1, s, :ov] = n.v, n.b
            if has_den:
                d = (Q if mutate == "den_from_q" else R).dot(b2, rows)
                den[0, s, :ov], den[1, s, :ov] = d.v, d.b
        if terms:
            f, d = f1.sum(1, rows), d1.sum(1, rows)
            if beta not in (0, 1):
                # the row sums over beta (beta - 1): a product, a reciprocal and a product in fp32, a product and a division in fp64
                d = (d * (1.0 / (beta * (beta - 1.0)))) * E(1.0, 2 * u, u)
            tf[0, s, :ov], tf[1, s, :ov] = f.v, f.b
            td[0, s, :ov], td[1, s, :ov] = d.v, d.b
    out = {"num": E(num[0], num[1], u) if update else None, "den": E(den[0], den[1], u) if update and has_den else None,
           "tf": E(tf[0], tf[1], u) if terms else None, "td": E(td[0], td[1], u) if terms else None}
    return out


def gamma_of(beta, mutate=None):
    g = gen.gamma_of(beta)
    if mutate == "wrong_gamma":
        # another branch of the rule: the outer ranges take the middle's 1, the middle takes 1/2
        return 0.5 if g == 1.0 else 1.0
    return g


def update(P, num_part, den, r, out_valid, beta, dtype, *, l1=0.0, l2=0.0, weighted=False, terms=None, exact=False, mutate=None):
    """launch_beta_update on given partial panels: P (out_pad, RP), num_part (S, out_pad, RP), den (S, out_pad, RP) or the RP values of dsum (the unweighted beta = 1).
    Whatever the partial panels hold on the padding (rows >= out_valid, columns >= r) is not looked at.  Returns a dict of E values: new, sumsq_part, sum_part
    ((out_pad // 128, RP)), t_frob, t_div."""
    dt = np.dtype(dtype).type
    u, eps = roundoff_of(dtype), eps_of(dtype)
    out_pad, RP = P.shape
    ov = out_valid - 1 if mutate == "out_valid_off_by_one" else out_valid
    l1, l2 = float(dt(l1)), float(dt(l2))
    g = float(dt(gamma_of(float(dt(beta)), mutate)))
    live = (np.arange(out_pad)[:, None] < ov) & (np.arange(RP)[None, :] < r)
    clean = lambda a: np.where(live[None] if a.ndim == 3 else live, np.asarray(a, dtype=np.float64), 1.0)
    parts = clean(num_part)
    if mutate == "drop_slab":
        parts = parts[:-1] if parts.shape[0] > 1 else 0 * parts
    S = parts.shape[0]
    nu = E(parts, 0.0, u).sum(0, max(S - 1, 0))
    den = np.asarray(den)
    if den.ndim == 1:
        assert float(dt(beta)) == 1 and not weighted
        de = E(np.where(live, den.astype(np.float64)[None, :], 1.0), 0.0, u)
    else:
        dparts = clean(den)
        if mutate == "drop_slab":
            dparts = dparts[:-1] if dparts.shape[0] > 1 else 0 * dparts
        de = E(dparts, 0.0, u).sum(0, max(S - 1, 0))
    a = E(np.where(live, np.asarray(P, dtype=np.float64), 1.0), 0.0, u)

    def value(a_in_den):
        # (without its eps a zero denominator divides by zero: 1e-30 stands for that here)
        d = E(np.where(de.v == 0, 1e-30, de.v), de.b, u) if mutate == "no_eps_den" else de + eps
        if exact:
            d = rounded(d, dtype)
        if l1 != 0 or l2 != 0:
            d = d + l1 + a_in_den * l2
        quo = nu / d
        f = quo if g == 1.0 else quo.sqrt() if g == 0.5 else quo.where(quo.v > 0, 1.0).power(g).where(quo.v > 0)
        return a * f

    new = value(a)
    if mutate == "l2_new_value":
        new = value(new)
    new = new.where(live)
    sq = (new * new).exact(lambda x: x.reshape(out_pad // 128, 128, RP)).sum(1)
    sm = new.exact(lambda x: x.reshape(out_pad // 128, 128, RP)).sum(1)
    out = {"new": new, "sumsq_part": sq, "sum_part": sm, "t_frob": None, "t_div": None}
    if terms is not None:
        St = np.asarray(terms[0]).shape[0]
        out["t_frob"] = E(np.asarray(terms[0], dtype=np.float64), 0.0, u).sum(0, St)
        out["t_div"] = E(np.asarray(terms[1], dtype=np.float64), 0.0, u).sum(0, St)
    return out
