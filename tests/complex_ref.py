"""Extended-precision references, derived forward-error bounds and the level-designed generator of the complex geometry tests
(numpy only, no GPU; imported by test_complex_ref_cpu.py and test_gpu_complex_geometry.py).  Everything here works on the CSR
arrays -- no dense matrix is ever formed -- and shares no code with the library or with oracle/.

References.  `z` results are compared against np.clongdouble (x87 extended, eps 1.08e-19), `c` results against np.complex128:
the reference's own error is 2^-11 resp. 2^-29 of the unit roundoff under test and is neglected against a bound that must
hold with ratio < 1.

Bounds.  u is the unit roundoff of the type under test (2^-53 / 2^-24) and c = 4 sqrt(2) u.  In the standard model of complex
arithmetic (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.5) fl(x +- y) = (x +- y)(1 + d),
|d| <= u; fl(x y) = x y (1 + d), |d| <= sqrt(2) gamma_2 ~ 2 sqrt(2) u; fl(x / y) = (x / y)(1 + d), |d| <= sqrt(2) gamma_4 ~
4 sqrt(2) u.  The kernels' c_mac (acc += a b as four fma: every partial product is formed exactly and rounded once with the
sum) commits at most a multiply and an add, (1 + 2 sqrt(2) u)(1 + u); their division (den = |d|^2 by one fma, two fma
numerators, two real divisions) commits 4 real roundings per component and stays within sqrt(2) gamma_4.  So ONE complex
multiply-accumulate or ONE division perturbs its operands by a relative (1 + d), |d| <= c, and k of them in sequence by
(1 + theta_k), |theta_k| <= k c / (1 - k c), written k c below (the bounds carry one spare term for the second order).

  * Product row i with p_i stored entries, y_i = alpha sum_j a_ij x_j + beta y0_i.  A lane group of G lanes sums at most
    ceil(p_i / G) <= p_i entries per lane, adds t = log2 G levels of the shuffle tree, multiplies by alpha (1 op) and applies
    beta as one c_mac (a multiply and an add): every term passes through at most p_i + t + 2 operations, hence
        |y^_i - y_i| <= (p_i + t + 3) c (|alpha| sum_j |a_ij| |x_j| + |beta| |y0_i|).
    csrmm is one chain per output element: t = 0.
  * Triangular solve, row i with p_i off-diagonal entries: s_0 = fl(alpha b_i), s_k = fl(s_{k-1} - t_ik x^_k), x^_i =
    fl(s_p / d_i).  Unrolling, alpha b_i (1 + theta_{p+2}) = d_i x^_i + sum_k t_ik x^_k (1 + theta'_k) with every theta of
    at most p_i + 2 factors, i.e. the residual obeys |alpha b - T x^|_i <= r_i = gamma_i (sum_j |t_ij| |x^_j| + |d_i| |x^_i|),
    gamma_i = (p_i + 3) c (unit diagonal: no division, d_i = 1, gamma_i = (p_i + 2) c).  With T x = alpha b exact,
    T (x^ - x) = -res and |T^-1| <= M(T)^-1 entrywise for a triangular T (M(T): |d_i| on the diagonal, -|t_ij| off it;
    Higham, Theorem 8.12), so |x^ - x| <= w = M(T)^-1 r, one real substitution in float64.
  * Conjugated dot product over n entries on `blocks` = min(1024, ceil(n / 256)) workgroups of 256: a thread chains
    ceil(n / 262144) c_mac, a 64-lane tree (6) and the 4-partial sum (2) follow; the final kernel chains ceil(blocks / 256)
    additions per thread and repeats the 6 + 2 tree: ceil(n / 262144) + ceil(blocks / 256) + 16 operations, bound
        |d^ - d| <= (ceil(n / 262144) + ceil(blocks / 256) + 18) c sum_i |x_i| |y_i|.
"""
import numpy as np

assert np.finfo(np.longdouble).eps < 2.0 ** -60, "the z references need an extended-precision long double"

DESIGN_WIDTHS = (1500, 1, 1300, 5, 70, 1024, 1025, 300)  # every kind of level around TRSV_NARROW = 1024; n = 5225


def real_type(dtype):
    return np.float64 if np.dtype(dtype) == np.complex128 else np.float32


def ext_type(dtype):
    """the type the reference of a `dtype` result is computed in"""
    return np.clongdouble if np.dtype(dtype) == np.complex128 else np.complex128


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else 2.0 ** -24


def cmac_const(dtype):
    """c = 4 sqrt(2) u: one complex multiply-accumulate or one division (module docstring)"""
    return 4.0 * np.sqrt(2.0) * unit_roundoff(dtype)


def ratio(err, bound):
    """largest err / bound over all entries; inf where an entry errs against a zero bound or is not a number"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(np.max(q))


def crand(rng, shape, dtype):
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(dtype)


def product_matrix(dtype, m=131, n=90, seed=17, base=0):
    """rows of 0 .. 19 entries in [-1, 1]^2, sorted; the first and the last row empty (where there are three or more)"""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.integers(0, 20, m), n)
    if m >= 3:
        lens[0] = lens[-1] = 0
    else:
        lens[:] = np.maximum(lens, 2)
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens])
    return (rp + base).astype(np.int32), (ci + base).astype(np.int32), crand(rng, len(ci), dtype)


def rows_of_lengths(dtype, m, n, lengths, seed, base=0):
    """m x n, every row length drawn from `lengths` (each one used), the first and the last row empty, sorted columns"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([lengths, rng.choice(lengths, size=m - 2 - len(lengths))])
    lens = np.concatenate([[0], rng.permutation(lens), [0]]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens])
    return (rp + base).astype(np.int32), (ci + base).astype(np.int32), crand(rng, len(ci), dtype)


# ---- CSR arrays as coordinate triples -------------------------------------------------------------------------------------

def coo(rp, ci, v, base):
    rp0 = np.asarray(rp, np.int64) - base
    r = np.repeat(np.arange(len(rp0) - 1, dtype=np.int64), np.diff(rp0))
    return r, np.asarray(ci, np.int64) - base, np.asarray(v)


def op_coo(r, c, v, shape, op):
    """the triples and shape of op(A), op in 'n', 't', 'h'"""
    if op == "n":
        return r, c, v, tuple(shape)
    return c, r, (np.conj(v) if op == "h" else v), (shape[1], shape[0])


def hermitian_coo(r, c, v, fill):
    """expansion of the stored `fill` triangle: strict part, diagonal as stored, conjugated mirror of the strict part"""
    strict = r > c if fill == "lower" else r < c
    dg = r == c
    return (np.concatenate([r[strict], r[dg], c[strict]]), np.concatenate([c[strict], c[dg], r[strict]]),
            np.concatenate([v[strict], v[dg], np.conj(v[strict])]))


def csr_of(r, c, v, m):
    """triples -> (ptr, ind, val), rows in order, entries of a row in the order given"""
    order = np.argsort(r, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    return ptr, c[order], v[order]


def transpose_csr(rp, ci, v, base, shape):
    """CSR arrays (int32, same base) of the transpose, columns sorted"""
    r, c, a = coo(rp, ci, v, base)
    order = np.lexsort((r, c))
    ptr, ind, val = csr_of(c[order], r[order], a[order], shape[1])
    return (ptr + base).astype(np.int32), (ind + base).astype(np.int32), np.ascontiguousarray(val)


# ---- products -------------------------------------------------------------------------------------------------------------

def row_sums(r, c, v, m, B, acc):
    """sum_j a_ij B[j, :] for every row i, the entries of a row added one after the other in the type `acc`"""
    ptr, ind, val = csr_of(r, c, np.asarray(v).astype(acc), m)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    k = np.arange(len(rows), dtype=np.int64) - ptr[rows]  # position of the entry in its row
    B = np.asarray(B)
    out = np.zeros((m, B.shape[1]), acc)
    for step in range(int(k.max()) + 1 if len(k) else 0):
        sel = np.flatnonzero(k == step)  # at most one entry per row: the indexed += is safe
        out[rows[sel]] += val[sel, None] * B[ind[sel]].astype(acc)
    return out


def product(r, c, v, shape, alpha, B, beta, C0, acc):
    """alpha A B + beta C0 for the triples of A (already op'ed), B (shape[1] x n) and C0 (shape[0] x n), in the type `acc`"""
    s = row_sums(r, c, v, shape[0], B, acc)
    return acc(alpha) * s + acc(beta) * np.asarray(C0).astype(acc)


def product_scale(r, c, v, shape, alpha, B, beta, C0):
    """|alpha| sum_j |a_ij| |B_j| + |beta| |C0_i| (float64) and the stored entries p_i per row"""
    s = row_sums(r, c, np.abs(np.asarray(v).astype(np.complex128)), shape[0], np.abs(np.asarray(B).astype(np.complex128)), np.float64)
    scale = abs(complex(alpha)) * s + abs(complex(beta)) * np.abs(np.asarray(C0).astype(np.complex128))
    return scale, np.bincount(r, minlength=shape[0]).astype(np.float64)


def product_bound(p, t, scale, dtype):
    """(p_i + t + 3) c scale_i; t = log2 of the lane group (0 for csrmm)"""
    return (np.asarray(p, np.float64)[:, None] + t + 3) * cmac_const(dtype) * scale


# ---- triangular solves ----------------------------------------------------------------------------------------------------

class TriOp:
    """op(T) for the stored `fill` triangle T: strict part by rows (ptr, ind, val), diagonal, rows in solve order"""

    def __init__(self, rp, ci, v, base, fill, op, unit):
        r, c, a = coo(rp, ci, v, base)
        n = len(rp) - 1
        strict = r > c if fill == "lower" else r < c
        dg = r == c
        self.n, self.unit = n, unit
        diag = np.ones(n, a.dtype)
        if not unit:
            assert len(np.unique(r[dg])) == n, "a non-unit solve needs a full diagonal"
            diag[r[dg]] = a[dg]
        sr, sc, sv, _ = op_coo(r[strict], c[strict], a[strict], (n, n), op)
        self.diag = np.conj(diag) if op == "h" else diag
        self.ptr, self.ind, self.val = csr_of(sr, sc, sv, n)
        self.lower = (fill == "lower") == (op == "n")  # op(T) is lower triangular: rows ascending
        self.order = np.arange(n) if self.lower else np.arange(n - 1, -1, -1)
        self.p = np.diff(self.ptr).astype(np.float64)

    def levels(self):
        """level[i] = 1 + max level of the rows that row i depends on (0 for none)"""
        level = np.zeros(self.n, np.int64)
        for i in self.order:
            s, e = self.ptr[i], self.ptr[i + 1]
            if e > s:
                level[i] = 1 + level[self.ind[s:e]].max()
        return level

    def solve(self, alpha, B, acc):
        """X = op(T)^-1 alpha B by substitution, B (n x k), in the type `acc`"""
        val, d = self.val.astype(acc), self.diag.astype(acc)
        X = acc(alpha) * np.asarray(B).astype(acc)
        for i in self.order:
            s, e = self.ptr[i], self.ptr[i + 1]
            if e > s:
                X[i] -= val[s:e] @ X[self.ind[s:e]]
            if not self.unit:
                X[i] /= d[i]
        return X

    def bound(self, Xhat, dtype):
        """w = M(T)^-1 r for the computed solution Xhat (n x k), float64 (module docstring)"""
        gamma = (self.p + (2 if self.unit else 3)) * cmac_const(dtype)
        av, ad = np.abs(self.val.astype(np.complex128)), np.abs(self.diag.astype(np.complex128))
        Xa = np.abs(np.asarray(Xhat).astype(np.complex128))
        W = np.zeros(Xa.shape, np.float64)
        for i in self.order:
            s, e = self.ptr[i], self.ptr[i + 1]
            j = self.ind[s:e]
            W[i] = (gamma[i] * (av[s:e] @ Xa[j] + ad[i] * Xa[i]) + av[s:e] @ W[j]) / ad[i]
        return W


def level_widths(rp, ci, base, fill, op):
    """rows per dependency level of op(T), T the `fill` triangle of the CSR arrays"""
    t = TriOp(rp, ci, np.ones(len(ci)), base, fill, op, True)
    return np.bincount(t.levels()).tolist()


def _designed_lower(widths, rng):
    """strict lower dependencies with exactly the levels `widths`: rows 0 .. L-1 are a chain, one seed per level; every other
    row sits at a shuffled index, depends on the seed of the level below and on 0-11 earlier rows of lower level"""
    L, n = len(widths), int(sum(widths))
    assert min(widths) >= 1
    level = np.empty(n, np.int64)
    level[:L] = np.arange(L)
    level[L:] = rng.permutation(np.repeat(np.arange(L), np.asarray(widths) - 1))
    deps = []
    for i in range(n):
        lv = level[i]
        if i < L:
            deps.append(np.arange(i - 1, i) if i else np.zeros(0, np.int64))
        elif lv == 0:
            deps.append(np.zeros(0, np.int64))
        else:
            cand = np.flatnonzero(level[:i] < lv)
            cand = cand[cand != lv - 1]
            k = min(int(rng.integers(0, 12)), len(cand))
            deps.append(np.sort(np.concatenate([[lv - 1], rng.choice(cand, size=k, replace=False)]).astype(np.int64)))
    return deps


def level_triangle(widths, seed, dtype, base):
    """Square complex CSR (sorted rows, full diagonal of modulus in [3, 4] and random phase, off-diagonal entries in the square
    [-0.5, 0.5]^2) whose LOWER triangle has exactly the dependency levels `widths` and whose UPPER triangle is a mirrored
    construction (row i <-> n-1-i, its own draw) with the same widths."""
    rng = np.random.default_rng(seed)
    n = int(sum(widths))
    low, up = _designed_lower(widths, rng), _designed_lower(widths, rng)
    rows = [np.concatenate([low[i], [i], np.sort(n - 1 - up[n - 1 - i])]).astype(np.int64) for i in range(n)]
    lens = np.array([len(c) for c in rows])
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate(rows)
    v = rng.uniform(-0.5, 0.5, len(ci)) + 1j * rng.uniform(-0.5, 0.5, len(ci))
    dg = ci == np.repeat(np.arange(n), lens)
    v[dg] = rng.uniform(3.0, 4.0, n) * np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    return (rp + base).astype(np.int32), (ci + base).astype(np.int32), v.astype(dtype)


# ---- dot product ----------------------------------------------------------------------------------------------------------

DOT_N = 262144 + 300  # one element more than 1024 workgroups of 256 threads hold: the grid-stride loop takes a second turn


def cdot_blocks(n):
    return min(1024, max(1, -(-n // 256)))


def cdot(x, y, acc):
    """sum conj(x_i) y_i, a plain left-to-right sum in the type `acc`"""
    return np.cumsum(np.conj(np.asarray(x).astype(acc)) * np.asarray(y).astype(acc))[-1]


def cdot_bound(x, y, dtype):
    n = len(x)
    s = float(np.sum(np.abs(np.asarray(x).astype(np.complex128)) * np.abs(np.asarray(y).astype(np.complex128))))
    return (-(-n // 262144) + -(-cdot_blocks(n) // 256) + 18) * cmac_const(dtype) * s


def bidiagonal(n, seed, dtype, base):
    """diagonal of modulus in [1, 2] and a subdiagonal in [-0.5, 0.5]^2: the operator of the ?dotmv case"""
    rng = np.random.default_rng(seed)
    lens = np.full(n, 2)
    lens[0] = 1
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.empty(rp[-1], np.int64)
    v = rng.uniform(-0.5, 0.5, rp[-1]) + 1j * rng.uniform(-0.5, 0.5, rp[-1])
    ci[rp[1:] - 1] = np.arange(n)
    ci[rp[1:-1]] = np.arange(n - 1)
    v[rp[1:] - 1] = rng.uniform(1.0, 2.0, n) * np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    return (rp + base).astype(np.int32), (ci + base).astype(np.int32), v.astype(dtype)


def tail_weighted(n, seed, dtype, head=262144, weight=100.0):
    """unit-modulus entries of random phase, the entries past `head` -- the grid-stride loop's second turn -- `weight` times
    larger: one of them weighs ~1e-3 of sum |x_i| |y_i| in x^H (A x), far above the float32 bound of the dot product, so a
    tail that is lost or read at a wrong offset shows in `c` as well as in `z`"""
    rng = np.random.default_rng(seed)
    x = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    x[head:] *= weight
    return x.astype(dtype)
