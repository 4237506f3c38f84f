"""A plain numpy restatement of the dense optimizer and clipping kernels of csrc/okge_optim.hip (adagrad_kernel, adagrad2_kernel,
adagrad_multi_kernel, sqnorm_partial_kernel / clip_coef_kernel), of score_triples_kernel (csrc/okge_misc.hip) and of
rank_metrics_kernel (csrc/okge_rank.hip) at
float64, with the hard caps an fp32 evaluation of the same chain has to stay inside.  Not a conftest: the tests import it.

  adagrad64      gj = wd p + g;  s' = s + gj^2;  delta = lr gj / (sqrt(s') + eps);  p' = p - delta      (lr, wd, eps as fp32)
  adagrad_caps   |p - p'| <= 2u |p'| + 8u |delta|,  |s - s'| <= 4u s',  u = 2^-24.  gj takes one rounding (the fma), s' at most
                 3u relative (2u from gj^2, u from the fma), delta at most 6.5u relative (sqrt 1.5u + u, the add u, the division
                 u + gj's u, the multiply u), the final subtraction u of p'.  The caps hold whether or not the compiler contracts
                 the last multiply-subtract into an fma (that only removes a rounding); they assume no underflow (gj^2 and s'
                 normal fp32 numbers or exactly 0): underflowed() says whether a set of inputs meets that.
  adagrad32      the same chain in numpy fp32, the two fmas formed through float64 (the product of two fp32 numbers is exact
                 there): the yardstick beside the kernel's figures and the CPU self-check of the caps
  clip64         float64 norm sqrt(sum g^2); the rest fp32 as clip_coef_kernel does it
  score_triples64, rank_meters   float64 scores with the sum of absolute products; the seven meters
"""
import numpy as np

U = 2.0 ** -24                                         # fp32 unit roundoff
F32_MIN_NORMAL = 2.0 ** -126


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _hyper(lr, wd, eps):
    """the hyper-parameters as the C ABI receives them: fp32"""
    return np.float32(lr), np.float32(wd), np.float32(eps)


def adagrad64(p, g, s, lr, wd, eps):
    """one step in float64 from fp32 inputs -> (p', s', delta)"""
    lr, wd, eps = (float(x) for x in _hyper(lr, wd, eps))
    p, g, s = _f64(p), _f64(g), _f64(s)
    gj = wd * p + g
    s1 = s + gj * gj
    delta = lr * gj / (np.sqrt(s1) + eps)
    return p - delta, s1, delta


def adagrad_caps(p1, s1, delta):
    """(cap on |p - p'|, cap on |s - s'|) per element for an fp32 evaluation of adagrad64's chain"""
    return 2 * U * np.abs(p1) + 8 * U * np.abs(delta), 4 * U * s1


def underflowed(s1):
    """True where the float64 accumulator is a non-zero number below the smallest normal fp32: the caps do not cover those"""
    return (s1 > 0) & (s1 < F32_MIN_NORMAL)


def adagrad32(p, g, s, lr, wd, eps):
    """the chain in fp32, one rounding per operation, the two fmas through float64 -> (p', s') fp32"""
    lr, wd, eps = _hyper(lr, wd, eps)
    p, g, s = (np.asarray(x, dtype=np.float32) for x in (p, g, s))
    gj = (float(wd) * _f64(p) + _f64(g)).astype(np.float32)
    s1 = (_f64(gj) * _f64(gj) + _f64(s)).astype(np.float32)
    q = gj / (np.sqrt(s1) + eps)
    return p - lr * q, s1


def cap_ratios(got_p, got_s, p1, s1, delta):
    """(largest |p - p'| / cap, largest |s - s'| / cap) over the elements; an element with cap 0 must be exact (ratio inf if not)"""
    cap_p, cap_s = adagrad_caps(p1, s1, delta)
    out = []
    for got, want, cap in ((got_p, p1, cap_p), (got_s, s1, cap_s)):
        err = np.abs(_f64(got) - want)
        if err.size == 0:
            out.append(0.0)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / cap)
        out.append(float(np.nan_to_num(r, nan=np.inf).max()))
    return tuple(out)


def sweep_inputs(n, seed, warm):
    """the inputs of the GPU cases that carry a gradient: p ~ 0.1 N(0,1), g ~ N(0,1) 10^U{-4..-1}, the accumulator cold (0) or
    uniform(0.01, 1); fp32.  The CPU test holds the non-vacuity conditions on exactly these."""
    rng = np.random.default_rng([20251019, seed, n, int(bool(warm))])
    p = (0.1 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    g = rng.standard_normal(n, dtype=np.float32) * (10.0 ** rng.integers(-4, 0, n)).astype(np.float32)
    s = rng.uniform(0.01, 1.0, n).astype(np.float32) if warm else np.zeros(n, np.float32)
    return p, g.astype(np.float32), s


def clip64(g0, g1, max_norm):
    """(total, coef) fp32: total = fp32(sqrt(sum g^2)) from float64, coef = min(1, fp32(max_norm / (total + 1e-6f)))"""
    sq = float(np.sum(_f64(g0) ** 2)) + (0.0 if g1 is None else float(np.sum(_f64(g1) ** 2)))
    total = np.float32(np.sqrt(sq))
    return total, clip_coef(total, max_norm)


def clip_coef(total, max_norm):
    """the coefficient clip_coef_kernel forms from an fp32 norm"""
    c = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    return np.float32(c) if c < np.float32(1.0) else np.float32(1.0)


def score_triples64(scorer, s, r, o):
    """(score, A) float64 per row: A = the sum of the absolute three-factor products that enter the score.
    ComplEx (halves 1 | 2): sum s1 o1 r1 + s2 o2 r1 + s1 o2 r2 - s2 o1 r2;  DistMult: sum s o r"""
    s, r, o = _f64(s), _f64(r), _f64(o)
    if scorer == "distmult":
        t = s * o * r
        return t.sum(1), np.abs(t).sum(1)
    h = s.shape[1] // 2
    s1, s2, r1, r2, o1, o2 = s[:, :h], s[:, h:], r[:, :h], r[:, h:], o[:, :h], o[:, h:]
    terms = (s1 * o1 * r1, s2 * o2 * r1, s1 * o2 * r2, -(s2 * o1 * r2))
    return sum(t.sum(1) for t in terms), sum(np.abs(t).sum(1) for t in terms)


def rank_meters(ranks):
    """[#groups, sum 1/(rank+1), sum rank, #rank<1, #rank<3, #rank<10, #rank<50]; the reciprocal is float64(fp32(1) / fp32(rank + 1))
    and is summed in float64; the integer meters are Python ints (exact)"""
    r = np.asarray(ranks, dtype=np.int64)
    rec = (np.float32(1.0) / (r + 1).astype(np.float32)).astype(np.float64)
    return [int(r.size), float(np.sum(rec)), sum(r.tolist()),
            int((r < 1).sum()), int((r < 3).sum()), int((r < 10).sum()), int((r < 50).sum())]
