"""Shared data recipes and CPU references of the energy-distance (csrc/pairwise.hip, K7) and KDE
(csrc/kde.hip) edge tests: test_side_ref_cpu.py, test_gpu_energy_edges.py, test_gpu_kde_edges.py.
No GPU and no package import here.  np.longdouble is the yardstick (dense_ref.longdouble_ok).

Energy distance
---------------
The kernel's pair value is ``ss = 0.0; ss += (a_k - b_k)**2`` for k = 0 .. d-1 in order, then the
IEEE sqrt (compiled -ffp-contract=off): ``dist_model`` is that in NumPy float64 (elementwise,
unfused) and must match bit for bit.  A column sum is compared with ``colsum_ld`` (long double).
Bound, u = 2^-53: a computed squared distance is a sum of d non-negative terms, each with a
rounded difference (squared: 2 roundings' worth) and a rounded square, then d - 1 adds: relative
error <= (d + 2) u; the sqrt halves it and adds its own rounding: (d/2 + 2) u per distance.  A sum of
c non-negative terms in any order adds at most (c - 1) u.  So for every kernel variant, chunked or not,

    |got_i - ref_i| <= (c_i + d + 2) u ref_i            (energy_bound; c_i = 0 must give exactly 0.0)

with c_i the number of pairs of column i.

KDE (at the ABI's level)
------------------------
Inputs as the kernel receives them: whitened p (n, d), q (m, d), logw (n), log_norm, lower L.
``kde_ld`` evaluates in long double  a_ij = logw_i + log_norm - |p_i - q_j|^2 / 2,  log q_j =
logsumexp_i a_ij,  s_ij = exp(a_ij - log q_j),  m_j = sum_i s_ij p_i,  v_j = m_j - q_j,  grad_j =
v_j L^T.  Over the points that matter, P_j = {i: s_ij >= 2^-53}:

    A_j    = max_{i in P_j} |logw_i| + |log_norm| + |p_i - q_j|^2 / 2
    Dev_jl = max_{i in P_j} |p_il - m_jl|

Bound: the float64 a_ij is a d-term sum of squares ((d + 2) u relative on ss / 2), one subtraction
from log_norm and one addition of logw_i (each one rounding of a result no larger than the sum of the
magnitudes), and the shift's subtraction: an absolute error of at most (d + 6) u (1 + A_j), which
enters exp as a relative error of that size.  The sequential sum of n non-negative terms adds n u.
exp and log are budgeted one ulp each (inside the 2^-52 |ref| term together with the final add):

    tau_j = u (n + (d + 6) (1 + A_j))
    |log q_j - ref_j|  <=  tau_j + 2^-52 |ref_j|
    tol_v_jl   = tau_j (Dev_jl + |m_jl|) + 2^-52 |q_jl|
    tol_grad_jk = sum_l |L_kl| tol_v_jl + (d + 1) u sum_l |L_kl| |v_jl|

(the softmax mean's error is the weights' relative error tau_j times the spread of the points that
carry weight, plus the rounding of m and of m - q; the last term is the d-term dot product with L).
``energy_emulate`` and ``kde_emulate`` restate the kernels' operation order in float64 on the CPU (NumPy's
exp / log in place of the device's): test_side_ref_cpu.py keeps them inside these bounds.
"""
import functools

import numpy as np

U = 2.0 ** -53
TILE = 256          # staging tile of the compile-time-d kernels and the column block of both
ENERGY_DIMS = [1, 2, 3, 4, 8, 9, 17]
# (na, nb, b0, b1, tri) of the column-sum tests
COLSUM_SHAPES = [(1, 1, 0, 1, 0), (255, 259, 0, 259, 0), (256, 259, 0, 259, 0), (257, 259, 0, 259, 0),
                 (700, 720, 37, 701, 0), (700, 700, 0, 700, 1), (700, 700, 130, 611, 1), (700, 700, 300, 300, 1)]
# (na, nb, b0, b1, tri, key 14 or None, K, chunk) of the chunked launches (st_distance_colsum_ws)
CHUNK_GEOMETRIES = [(300, 3073, 0, 3073, 0, None, 4, 1024), (3073, 3073, 0, 3073, 1, None, 4, 1024),
                    (257, 2054, 5, 2054, 0, None, 3, 768), (4096, 16485, 100, 16485, 0, 256, 16, 1280)]
KDE_SHAPES = [(1, 5), (2, 1), (255, 257), (256, 256), (257, 255), (513, 300)]
KDE_DIMS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17]
KDE_WIDE = [(257, 65, 33), (257, 65, 64), (257, 65, 128)]    # (n, m, d): the runtime-d kernel's upper range


# ------------------------------------------------------------------------------------------ recipes
@functools.lru_cache(maxsize=None)
def points(n, d, seed):
    """N(0, 1) times per-dimension scales U(0.01, 100); rows [n//3, n//3 + 20) repeat rows [0, 20)
    (zero distances).  Shared: callers must not modify the array."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d)) * rng.uniform(0.01, 100.0, size=d)
    k = min(20, n // 3, n - n // 3)
    x[n // 3:n // 3 + k] = x[:k]
    x.setflags(write=False)
    return x


IN_RANGE = np.array([0.0, -0.0, 2.0 ** -60, -2.0 ** -60, np.nextafter(2.0 ** -60, 1.0), 2.0 ** 60, -2.0 ** 60,
                     1.0, 1.0 + 2.0 ** -52, 3.5])
OUT_OF_RANGE = np.array([2.0 ** -61, 2.0 ** 61, 5e-324, 2.0 ** -1000, 2.0 ** 600])


@functools.lru_cache(maxsize=None)
def boundary_points(d, seed=5):
    """513 rows at the edges of the block-uniform fast range (coordinates 0 or in [2^-60, 2^60]).
    Rows 0-255: the IN_RANGE table only.  Planted: row 0 all 2^-60 and row 1 its neighbour in coordinate 0
    (ss = 2^-224 exactly), row 2 a copy of row 0 and rows 3 / 4 all +0 / -0; row 255 all 2^60, row 254
    all -2^60 (ss = d 2^122), row 253 a copy of row 255.  Rows 256-511: the same rows with some entries
    replaced by OUT_OF_RANGE magnitudes (either sign) -- rows 257-262 kept as they are, so the slow
    path meets the planted pairs too -- and rows 256, 300, 301, 302, 511 out of range in coordinate 0.
    Row 512: ordinary.  All finite."""
    rng = np.random.default_rng(seed)
    x = np.empty((513, d))
    lo = IN_RANGE[rng.integers(0, IN_RANGE.size, size=(256, d))]
    lo[0] = 2.0 ** -60
    lo[1] = lo[0]
    lo[1, 0] = np.nextafter(2.0 ** -60, 1.0)
    lo[2] = lo[0]
    lo[3] = 0.0
    lo[4] = -0.0
    lo[255] = 2.0 ** 60
    lo[254] = -2.0 ** 60
    lo[253] = lo[255]
    x[:256] = lo
    hi = lo.copy()
    swap = rng.random(size=(256, d)) < 0.15
    swap[1:7] = False
    vals = OUT_OF_RANGE[rng.integers(0, OUT_OF_RANGE.size, size=(256, d))] * rng.choice([-1.0, 1.0], size=(256, d))
    hi[swap] = vals[swap]
    for r, v in [(0, 2.0 ** -61), (44, 5e-324), (45, 2.0 ** -1000), (46, 2.0 ** 61), (255, 2.0 ** 600)]:
        hi[r, 0] = v
    x[256:512] = hi
    x[512] = rng.normal(size=d)
    assert np.all(np.isfinite(x))
    x.setflags(write=False)
    return x


def in_fast_range(x):
    a = np.abs(x)
    return (a == 0.0) | ((a >= 2.0 ** -60) & (a <= 2.0 ** 60))


@functools.lru_cache(maxsize=None)
def kde_case(n, m, d, seed=3):
    """Whitened KDE inputs: random SPD cov, x = N(0, 1) chol(cov)' + 3, L = cholesky(inv(cov) / 0.25),
    p = x L (covariance 4 I).  Queries (whitened space): first third data rows (coincident), second
    third data rows + 0.7 N(0, 1), last third additionally shifted by 60 / sqrt(d) in every coordinate:
    a shift of length 60 against differences p_i - q_j of standard deviation 2.9 along it, so
    |p_i - q_j|^2 / 2 > 745 for every i (about 1100 at 4.5 standard deviations, 1800 typically) and every
    exponent underflows without the max-shift (a shift of length 45 leaves pairs near 525).
    Weights U(0, 1)^8 + 1e-300 (300 orders of magnitude), every fifth exactly 0 (i % 5 == 4), and for
    n > 300 all of rows [256, 512): one whole staging tile of the compile-time kernel, eight of the
    runtime-d one.  logw = log(w / sum w), -inf for the zeros."""
    rng = np.random.default_rng([seed, n, m, d])
    a = rng.normal(size=(d, d))
    cov = a @ a.T / d + 0.3 * np.eye(d)
    x = rng.normal(size=(n, d)) @ np.linalg.cholesky(cov).T + 3.0
    L = np.linalg.cholesky(np.linalg.inv(cov) / 0.25)
    p = x @ L
    t1, t2 = m // 3, 2 * m // 3
    q = p[np.arange(m) % n].copy()
    q[t1:] += 0.7 * rng.normal(size=(m - t1, d))
    q[t2:] += 60.0 / np.sqrt(d)
    w = rng.uniform(size=n) ** 8 + 1e-300
    w[4::5] = 0.0
    if n > 300:
        w[256:512] = 0.0
    with np.errstate(divide='ignore'):
        logw = np.log(w / np.sum(w))
    log_norm = float(np.sum(np.log(np.diag(L))) - 0.5 * d * np.log(2 * np.pi))
    out = dict(n=n, m=m, d=d, p=p, q=q, w=w, logw=logw, log_norm=log_norm, L=L, far=t2,
               zero=np.flatnonzero(w == 0.0))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ energy
def ss_model(A, B):
    """The kernel's squared distance in float64: (na, nb), sequential over k from +0.0, unfused."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ss = np.zeros((A.shape[0], B.shape[0]))
    with np.errstate(over='ignore', under='ignore'):
        for k in range(A.shape[1]):
            dk = A[:, k, None] - B[None, :, k]
            ss = ss + dk * dk
    return ss


def dist_model(A, B):
    """The kernel's per-pair bit model: sqrt of the sequential sum (scipy cdist's operation order)."""
    return np.sqrt(ss_model(A, B))


def colsum_ld(A, B, b0, b1, tri, cols=None):
    """(sums, counts) per column i (all of A, or the rows ``cols``): the long-double sum over b in [b0, b1)
    (and b < i when tri) of the long-double distance |A_i - B_b|, and the number of such b."""
    ld = np.longdouble
    cols = np.arange(A.shape[0]) if cols is None else np.asarray(cols, dtype=np.int64)
    Bl = np.asarray(B)[b0:b1].astype(ld)
    nb, d = Bl.shape
    sums = np.zeros(cols.shape[0], dtype=ld)
    counts = np.zeros(cols.shape[0], dtype=np.int64)
    step = max(1, (1 << 22) // max(nb, 1))          # <= 4M pairs (64 MB of long doubles) per temporary
    bidx = np.arange(b0, b1)
    for c0 in range(0, cols.shape[0], step):
        ci = cols[c0:c0 + step]
        Al = np.asarray(A)[ci].astype(ld)
        ss = np.zeros((ci.shape[0], nb), dtype=ld)
        for k in range(d):
            dk = Al[:, k, None] - Bl[None, :, k]
            ss += dk * dk
        dist = np.sqrt(ss)
        if tri:
            keep = bidx[None, :] < ci[:, None]
            dist = np.where(keep, dist, ld(0))
            counts[c0:c0 + step] = np.sum(keep, axis=1)
        else:
            counts[c0:c0 + step] = nb
        sums[c0:c0 + step] = np.sum(dist, axis=1)
    return sums, counts


def energy_bound(ref, counts, d):
    """(c_i + d + 2) 2^-53 ref_i (long double)."""
    return (counts + d + 2).astype(np.longdouble) * np.longdouble(U) * ref


def chunk_split(na, b0, b1, units=32768):
    """(K, chunk) of st_distance_colsum_ws for this launch (csrc/pairwise.hip distance_chunks and
    launch_distance_colsum restated): K chunks of `chunk` B points, whole staging tiles when K > 1."""
    ablocks = (na + TILE - 1) // TILE
    rng_ = b1 - b0
    if ablocks <= 0 or rng_ <= 0:
        return 1, max(rng_, 1)
    K = min((units + ablocks - 1) // ablocks, (rng_ + 4 * TILE - 1) // (4 * TILE), 65535)
    K = max(K, 1)
    if K == 1:
        return 1, rng_
    chunk = (rng_ + K - 1) // K
    return K, (chunk + TILE - 1) // TILE * TILE


def energy_emulate(A, B, b0, b1, tri, unroll=1, K=1, chunk=None, cols=None):
    """Float64 restatement of dist_colsum_kernel's order for the columns ``cols``: per chunk, tiles of 256 B
    points from the chunk's start (cut at the column block's end for the triangle); in a tile wholly
    below the block's first column `unroll` interleaved partial sums added at the tile's end, in other
    tiles one sequential sum with the b < i predicate; the chunk partials added in chunk order."""
    cols = np.arange(A.shape[0]) if cols is None else np.asarray(cols, dtype=np.int64)
    chunk = max(b1 - b0, 1) if chunk is None else chunk
    out = np.zeros(cols.shape[0])
    for blk in np.unique(cols // TILE):
        sel = np.flatnonzero(cols // TILE == blk)
        ci = cols[sel]
        c0 = int(blk) * TILE
        total = None
        for c in range(K):
            lo = b0 + c * chunk
            hi = min(lo + chunk, b1)
            if tri:
                hi = min(hi, c0 + TILE)
            acc = np.zeros(ci.shape[0])
            for bc in range(lo, hi, TILE):
                cnt = min(hi - bc, TILE)
                D = dist_model(A[ci], B[bc:bc + cnt])
                if not tri or bc + cnt <= c0:
                    part = np.zeros((unroll, ci.shape[0]))
                    full = cnt - cnt % unroll
                    for e in range(cnt):
                        part[e % unroll if e < full else 0] += D[:, e]
                    for u in range(1, unroll):
                        part[0] += part[u]
                    acc = acc + part[0]
                else:
                    for e in range(cnt):
                        acc = np.where(bc + e < ci, acc + D[:, e], acc)
            total = acc if total is None else total + acc
        out[sel] = total
    return out


def check_columns(na):
    """The fixed column subset of the chunk-geometry tests: first and last column of each 256-column
    block plus every 16th column."""
    c = set(range(0, na, 16)) | set(range(0, na, TILE)) | {min(b + TILE, na) - 1 for b in range(0, na, TILE)}
    return np.array(sorted(c), dtype=np.int64)


# ------------------------------------------------------------------------------------------ KDE
def kde_ld(p, q, logw, log_norm, L):
    """Long-double log q (m), grad (m, d) and the tolerances of the module docstring: a dict with
    logq, grad, tol_logq, tol_grad (long double), tau, A (float64).  Needs at least one finite logw."""
    ld = np.longdouble
    n, d = p.shape
    m = q.shape[0]
    pl, ql, Ll = p.astype(ld), q.astype(ld), np.asarray(L).astype(ld)
    lw = np.asarray(logw, dtype=np.float64).astype(ld)
    half_ss = np.zeros((m, n), dtype=ld)
    for k in range(d):
        dk = pl[None, :, k] - ql[:, k, None]
        half_ss += dk * dk
    half_ss *= ld(0.5)
    arg = lw[None, :] + (ld(log_norm) - half_ss)
    mx = np.max(arg, axis=1)
    t = np.exp(arg - mx[:, None])
    tot = np.sum(t, axis=1)
    logq = mx + np.log(tot)
    s = t / tot[:, None]
    mean = s @ pl                                    # (m, d)
    carry = s >= ld(2.0 ** -53)
    with np.errstate(invalid='ignore'):
        mag = np.where(carry, np.abs(lw)[None, :] + abs(ld(log_norm)) + half_ss, ld(0))
    A = np.max(mag, axis=1)
    dev = np.empty((m, d), dtype=ld)
    for l in range(d):
        dev[:, l] = np.max(np.where(carry, np.abs(pl[None, :, l] - mean[:, l, None]), ld(0)), axis=1)
    u = ld(U)
    tau = u * (n + (d + 6) * (1 + A))
    v = mean - ql
    absL = np.abs(Ll)
    tol_v = tau[:, None] * (dev + np.abs(mean)) + 2 * u * np.abs(ql)
    return dict(logq=logq, grad=v @ Ll.T, tol_logq=tau + 2 * u * np.abs(logq),
                tol_grad=tol_v @ absL.T + (d + 1) * u * (np.abs(v) @ absL.T),
                tau=tau.astype(np.float64), A=A.astype(np.float64))


def kde_arg_model(p, q, logw, log_norm):
    """The kernel's a_ij in float64, (m, n): ss sequential over k from +0.0, then
    logw_i + (log_norm - 0.5 ss), unfused."""
    ss = np.zeros((q.shape[0], p.shape[0]))
    for k in range(p.shape[1]):
        dk = p[None, :, k] - q[:, k, None]
        ss = ss + dk * dk
    return np.asarray(logw, dtype=np.float64)[None, :] + (log_norm - 0.5 * ss)


def kde_emulate(p, q, logw, log_norm, L):
    """Float64 restatement of kde_kernel's order: the row maximum, then the shifted exponentials
    summed sequentially in i, v = sm / s - q, grad by a sequential dot product with L's rows."""
    m, d = q.shape
    arg = kde_arg_model(p, q, logw, log_norm)
    mx = np.max(arg, axis=1)
    shift = np.where(np.isneginf(mx), 0.0, mx)
    s = np.zeros(m)
    sm = np.zeros((m, d))
    for i in range(p.shape[0]):
        t = np.exp(arg[:, i] - shift)
        s = s + t
        sm = sm + t[:, None] * p[i][None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        logq = np.log(s) + shift
        v = sm / s[:, None] - q
    grad = np.zeros((m, d))
    for l in range(d):
        grad = grad + v[:, l, None] * L[None, :, l]
    return logq, grad
