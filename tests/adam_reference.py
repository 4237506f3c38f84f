"""A plain numpy restatement of the Adam kernels (csrc/okge_adam_device.h: the dense sweep of csrc/okge_adam.hip and the row-sparse
body of csrc/okge_sparse.hip) at float64, with the hard caps an fp32 evaluation of the same chains has to stay inside.  Not a
conftest: the tests import it.

  adam64         torch.optim.Adam (amsgrad False, maximize False, coupled weight decay), step t (after the increment):
                     gj = g + wd p  (wd = 0: gj = g);   m' = m + (gj - m) a;   v' = v beta2 + b gj^2;   a = 1 - beta1, b = 1 - beta2
                     c1 = lr / (1 - beta1^t);  c2 = sqrt(1 - beta2^t);  denom = sqrt(v') / c2 + eps;  delta = c1 m' / denom;  p' = p - delta
  sparse_adam64  torch.optim.SparseAdam on a coalesced row:
                     m' = m + (g - m) a;   v' = v + (g^2 - v) b;   step = lr sqrt(1 - beta2^t) / (1 - beta1^t)
                     denom = sqrt(v') + eps;  delta = step m' / denom;  p' = p - delta
                 The hyper-parameters enter as the C ABI receives them, fp32 (exact=True: as given, for the comparison with torch
                 in float64); everything after that is float64.
  adam_caps      u = 2^-24, one u per rounding of the stated expression, second-order terms covered by rounding the counts up.
                   m'  : gj carries u |gj| (the fma; nothing at wd = 0), the difference u, the factor a (fp32(1 - beta1)) u, the
                         fma u |m'|:        |m - m'| <= u |m'| + u a |gj| + 2u a |gj - m|  <=  2u |m'| + 4u a (|gj| + |m|)
                   v'  dense: b gj^2 carries 5u (b, gj twice, two products), the fma u; every term is >= 0:
                                            |v - v'| <= u v' + 5u b gj^2  <=  8u v'                       (counted 6u)
                       sparse: g^2 u, the difference u, b u, the fma u |v'|:
                                            |v - v'| <= u v' + u b g^2 + 2u b |g^2 - v|  <=  2u v' + 4u b (g^2 + v)
                         which is at most 6u v' too, because v' = (1 - b) v + b g^2 >= b (g^2 + v) for b <= 1/2.
                   p'  : sqrt(v') (1/2 of v's 6u) + u = 4u; / c2 (c2 rounded once: u; the division u) 6u, sparse: none; + eps u;
                         m' / denom u; c1 or step rounded once u, the product u: dense 10u, sparse 8u relative to |delta|, plus m's
                         absolute error carried through c1 / denom, plus u |p'| for the subtraction:
                                            |p - p'| <= 2u |p'| + 14u |delta| + (c1 / denom) 4u a (|gj| + |m|)
                         (the 2u |m'| of m's cap is 2u |delta| of the 14: dense 10 + 2 counted, sparse 8 + 2)
                 The caps hold whether or not the compiler contracts a multiply into the subtraction behind it (one rounding
                 fewer); they assume no underflow (b gj^2 and v' normal fp32 numbers or exactly 0): underflowed() tells.
  adam32, sparse_adam32   the chains in numpy fp32 as okge_adam_device.h spells them, the fmas formed through float64: the
                 yardstick beside the kernel's figures and the CPU self-check of the caps
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126

Step64 = namedtuple("Step64", "p m v delta gj denom scale a b")   # scale: c1 (dense) / step (sparse)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _hyper(exact, *xs):
    return tuple(float(x) if exact else float(np.float32(x)) for x in xs)


def bias_scalars(t, lr, beta1, beta2):
    """(c1, c2, sparse step size) in double from hyper-parameters that already hold the values the kernels see"""
    bc1, bc2 = 1.0 - beta1 ** int(t), 1.0 - beta2 ** int(t)
    return lr / bc1, np.sqrt(bc2), lr * np.sqrt(bc2) / bc1


def adam64(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, exact=False):
    """one dense step in float64 from fp32 inputs; t = the step count after the increment"""
    lr, b1, b2, eps, wd = _hyper(exact, lr, betas[0], betas[1], eps, wd)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    a, b = 1.0 - b1, 1.0 - b2
    c1, c2, _ = bias_scalars(t, lr, b1, b2)
    gj = g + wd * p if wd != 0 else g
    m1 = m + (gj - m) * a
    v1 = v * b2 + b * gj * gj
    denom = np.sqrt(v1) / c2 + eps
    delta = c1 * m1 / denom
    return Step64(p - delta, m1, v1, delta, gj, denom, c1, a, b)


def sparse_adam64(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, exact=False):
    """one step of the rows a coalesced gradient g names, in float64"""
    lr, b1, b2, eps = _hyper(exact, lr, betas[0], betas[1], eps)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    a, b = 1.0 - b1, 1.0 - b2
    _, _, step = bias_scalars(t, lr, b1, b2)
    m1 = m + (g - m) * a
    v1 = v + (g * g - v) * b
    denom = np.sqrt(v1) + eps
    delta = step * m1 / denom
    return Step64(p - delta, m1, v1, delta, g, denom, step, a, b)


def adam_caps(r, m, v, sparse=False):
    """(cap on |p - p'|, on |m - m'|, on |v - v'|) per element for an fp32 evaluation of the chain that gave r = adam64(...) /
    sparse_adam64(...) (sparse=True) from the moments m, v"""
    m, v = _f64(m), _f64(v)
    carried = 4 * U * r.a * (np.abs(r.gj) + np.abs(m))
    cap_m = 2 * U * np.abs(r.m) + carried
    cap_v = 2 * U * r.v + 4 * U * r.b * (r.gj * r.gj + v) if sparse else 8 * U * r.v
    cap_p = 2 * U * np.abs(r.p) + 14 * U * np.abs(r.delta) + (r.scale / r.denom) * carried
    return cap_p, cap_m, cap_v


def underflowed(r):
    """True where b gj^2 or v' is a non-zero number below the smallest normal fp32: the caps do not cover those"""
    t = r.b * r.gj * r.gj
    return ((t > 0) & (t < F32_MIN_NORMAL)) | ((r.v > 0) & (r.v < F32_MIN_NORMAL))


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(x, y, z):
    """fp32 fma: the product of two fp32 numbers is exact in float64; the sum rounds twice only in cases far below the caps"""
    return (_f64(x) * _f64(y) + _f64(z)).astype(np.float32)


def adam32(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """adam1 of okge_adam_device.h in numpy fp32 -> (p', m', v') fp32"""
    lr, b1, b2, eps, wd = _hyper(False, lr, betas[0], betas[1], eps, wd)
    c1, c2, _ = (np.float32(x) for x in bias_scalars(t, lr, b1, b2))
    a, b, b2, eps = np.float32(1.0 - b1), np.float32(1.0 - b2), np.float32(b2), np.float32(eps)
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    gj = _fma32(np.float32(wd), p, g) if wd != 0 else g
    m1 = _fma32(gj - m, a, m)
    v1 = _fma32(v, b2, (b * gj) * gj)
    return p - c1 * (m1 / (np.sqrt(v1) / c2 + eps)), m1, v1


def sparse_adam32(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """adam1_rows of okge_adam_device.h in numpy fp32 -> (p', m', v') fp32"""
    lr, b1, b2, eps = _hyper(False, lr, betas[0], betas[1], eps)
    step = np.float32(bias_scalars(t, lr, b1, b2)[2])
    a, b, eps = np.float32(1.0 - b1), np.float32(1.0 - b2), np.float32(eps)
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    m1 = _fma32(g - m, a, m)
    v1 = _fma32(g * g - v, b, v)
    return p - step * (m1 / (np.sqrt(v1) + eps)), m1, v1


def cap_ratios(got, r, m, v, sparse=False):
    """(largest |p - p'| / cap, the same for m and v) over the elements; an element with cap 0 must be exact (ratio inf if not)"""
    out = []
    for x, want, cap in zip(got, (r.p, r.m, r.v), adam_caps(r, m, v, sparse)):
        err = np.abs(_f64(x) - want)
        if err.size == 0:
            out.append(0.0)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / cap)
        out.append(float(np.nan_to_num(q, nan=np.inf).max()))
    return tuple(out)


def sweep_inputs(n, seed, warm):
    """the inputs of the GPU cases: p ~ 0.1 N(0,1), g ~ N(0,1) 10^U{-4..-1}; the moments cold (0, 0) or warm -- m ~ 0.05 N(0,1),
    v uniform(1e-6, 1e-2); fp32.  The CPU test holds the non-vacuity conditions on exactly these."""
    rng = np.random.default_rng([20261020, seed, n, int(bool(warm))])
    p = (0.1 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    g = (rng.standard_normal(n, dtype=np.float32) * (10.0 ** rng.integers(-4, 0, n)).astype(np.float32)).astype(np.float32)
    if not warm:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (0.05 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    v = rng.uniform(1e-6, 1e-2, n).astype(np.float32)
    return p, g, m, v


def coalesce32(ids, g, table_rows):
    """the host's ascending-position fp32 coalescing of occurrence rows g (n, row_len): -> (distinct in-table ids ascending, their
    summed rows fp32, the number of ids outside the table).  Row by row in position order, sequentially in fp32, as
    okge_adagrad_rows / okge_adam_rows add them."""
    ids = np.asarray(ids, dtype=np.int64)
    g = np.asarray(g, dtype=np.float32)
    ok = (ids >= 0) & (ids < table_rows)
    order = np.argsort(ids[ok], kind="stable")
    sid, rows = ids[ok][order], g[ok][order]
    uniq, first, counts = np.unique(sid, return_index=True, return_counts=True)
    acc = rows[first].copy()
    for k in range(1, int(counts.max()) if counts.size else 0):      # k-th occurrence of every id that has one: position order
        has = counts > k
        acc[has] = acc[has] + rows[first[has] + k]
    return uniq, acc, int((~ok).sum())
