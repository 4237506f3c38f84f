"""okge_adam_step (adam_prologue_kernel + adam2_kernel, csrc/okge_adam.hip) through the C ABI at the shapes where its branches
change, element by element against the float64 restatement adam64 of tests/adam_reference.py under adam_caps: the n & 3 tail next to
other memory, below and above the launcher's grid cap of 16384 x 256 threads (16 777 216 floats per pass of the grid-stride loop),
two unequal tensors in both orders, every zero_grad mode, weight decay present and absent, and step counts 1, 2 and 1000 through a
preset device state.  test_adam_reference.py holds the conditions that make the caps bite.

Every tensor is a 16-byte-aligned view inside a sentinel-filled buffer (Guarded, test_optim_shapes.py) whose guard words must
survive.  Every capped comparison prints `RATIO <case> <tensor> <max error / cap> | <the same for adam32>`; the table of one run is
in profiles/adam.md."""
import numpy as np
import pytest
import torch

import adam_reference as A
from test_optim_shapes import CAP, CHUNK, SMALL, Guarded, same_bits

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
N_BIG = CAP + 3075                                     # one full pass, a partial second pass, a tail of 3
T0 = (0, 1, 999)                                       # preset steps taken: the call under test is step 1, 2, 1000


@pytest.fixture(scope="module")
def hp(okge_lib):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


class Seg:
    """one tensor of an Adam call: guarded p, g, exp_avg, exp_avg_sq and state on the device, and the host's copy of what they hold"""

    def __init__(self, p, g, m, v, t0=0):
        self.n = int(p.size)
        self.h = [np.array(x, dtype=np.float32) for x in (p, g, m, v)]
        self.p, self.g, self.m, self.v = (Guarded(x) for x in self.h)
        self.t = int(t0)
        self.state = Guarded(np.array([t0, 0, 0, 0], np.int32))

    def intact(self):
        return all(x.intact() for x in (self.p, self.g, self.m, self.v, self.state))


def make_seg(n, seed, warm, t0=0, src=None):
    return Seg(*((x[:n] for x in src) if src is not None else A.sweep_inputs(n, seed, warm)), t0=t0)


def launch(hp, segs, wd, mode, lr=LR, betas=BETAS, eps=EPS):
    from open_knowledge_graph_embeddings_amd import _native as N
    arr = (N.AdamTensor * len(segs))()
    for a, sg in zip(arr, segs):
        a.p, a.g, a.exp_avg, a.exp_avg_sq, a.state, a.n = sg.p.ptr(), sg.g.ptr(), sg.m.ptr(), sg.v.ptr(), sg.state.ptr(), sg.n
    return int(hp.lib.okge_adam_step(arr, len(segs), lr, betas[0], betas[1], eps, wd, mode, hp._stream()))


def check_against_float64(case, tensor, got, p, g, m, v, t, wd):
    """p, m, v against adam64 under adam_caps, element by element, in slices; prints the RATIO lines, then asserts"""
    n = int(p.size)
    worst, yard = [0.0] * 3, [0.0] * 3
    finite = all(bool(np.isfinite(x).all()) for x in got)
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(n, lo + CHUNK))
        r = A.adam64(p[sl], g[sl], m[sl], v[sl], t, LR, BETAS, EPS, wd)
        assert not A.underflowed(r).any(), (case, tensor, "the inputs leave the range the caps are stated for")
        worst = [max(a, b) for a, b in zip(worst, A.cap_ratios([x[sl] for x in got], r, m[sl], v[sl]))]
        if lo == 0:                                    # the yardstick on the first slice (2 M elements at most)
            yard = A.cap_ratios(A.adam32(p[sl], g[sl], m[sl], v[sl], t, LR, BETAS, EPS, wd), r, m[sl], v[sl])
    for name, w, y in zip(("p", "m", "v"), worst, yard):
        print("RATIO %s %s.%s %.3f | %.3f" % (case, tensor, name, w, y))
    assert finite and max(worst) <= 1.0, (case, tensor, worst, finite)


def check_state(case, sg, t):
    """[0] = t exactly; the scratch words hold the fp32 c1, c2 and sparse step size of that t (formed in double on the device: the
    host's double may differ in its last place, which moves the fp32 rounding by at most one unit)"""
    st = sg.state.np()
    assert int(st[0]) == t, (case, "t", int(st[0]), t)
    got = st[1:].view(np.float32).astype(np.float64)
    want = np.array(A.bias_scalars(t, *(float(np.float32(x)) for x in (LR, BETAS[0], BETAS[1]))))
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want), (case, got, want)


def drive(hp, case, segs, wd, modes):
    """one launch per zero_grad mode.  After each: p, m, v against float64 from the state the launch started from (the kernel's
    own after the first), t advanced by exactly one per tensor, the gradient bit for bit untouched or exactly +0, guards intact"""
    for step, mode in enumerate(modes):
        before = [sg.g.v.clone() for sg in segs]
        assert launch(hp, segs, wd, mode) == 0, (case, hp.lib.okge_last_error())
        torch.cuda.synchronize()
        for k, sg in enumerate(segs):
            name = "%s step%d" % (case, step)
            sg.t += 1
            check_state(name, sg, sg.t)
            got = [sg.p.np(), sg.m.np(), sg.v.np()]
            check_against_float64(name, "t%d" % k, got, *sg.h, sg.t, wd)
            if mode == 1 or (mode == 2 and k == 1):
                assert not bool(sg.g.v.any()) and not bool(torch.signbit(sg.g.v).any()), (name, k, "gradient not cleared to +0")
                sg.h[1] = np.zeros(sg.n, np.float32)
            else:
                assert same_bits(sg.g.v, before[k]), (name, k, "gradient touched without zero_grad")
            sg.h[0], sg.h[2], sg.h[3] = got
            assert sg.intact(), (name, k, "guard words overwritten")


@pytest.mark.parametrize("wd", [0.0, 1e-10], ids=["wd0", "wd1e-10"])
@pytest.mark.parametrize("t0", T0)
@pytest.mark.parametrize("n", SMALL)
def test_step_sizes(hp, n, t0, wd):
    """one tensor, warm moments at a preset step count: zero_grad 0, then 1 -- two consecutive steps"""
    drive(hp, "step-n%d-t%d-wd%g" % (n, t0 + 1, wd), [make_seg(n, 10, True, t0)], wd, [0, 1])


@pytest.mark.parametrize("wd", [0.0, 1e-10], ids=["wd0", "wd1e-10"])
@pytest.mark.parametrize("n", [5, 1025])
def test_cold_start(hp, n, wd):
    """zero moments and a zero state, as a fresh optimizer starts: three steps, the gradient kept"""
    drive(hp, "cold-n%d-wd%g" % (n, wd), [make_seg(n, 13, False)], wd, [0, 0, 0])


PAIRS = [(1025, 3), (3, 1025), (262_147, 5), (5, 262_147), (1023, 1023), (1024, 0), (0, 7)]


@pytest.mark.parametrize("wd", [0.0, 1e-10], ids=["wd0", "wd1e-10"])
@pytest.mark.parametrize("n0,n1", PAIRS)
def test_two_tensors_and_modes(hp, n0, n1, wd):
    """unequal lengths in both orders (the longer tensor sizes the grid, the shorter one's tail falls in workgroup 0), an empty
    tensor on either side, different step counts per tensor; zero_grad 0, then 2 (second only), then 1 (both)"""
    segs = [make_seg(n0, 11, True, 4), make_seg(n1, 12, True, 0)]
    drive(hp, "pair-n%d-n%d-wd%g" % (n0, n1, wd), segs, wd, [0, 2, 1])


def test_above_the_grid_cap(hp):
    """16 777 216 + 3075 floats: one full pass of the grid-stride loop, a partial second pass and a tail of 3, next to a short
    second tensor; zero_grad 1"""
    src = A.sweep_inputs(N_BIG, 3, True)
    segs = [make_seg(N_BIG, 0, True, 1, src=src), make_seg(7, 14, True, 1)]
    drive(hp, "big-n%d" % N_BIG, segs, 1e-10, [1])


def test_shared_state_advances_once(hp):
    """two tensors that hand over ONE state: it advances by one per call, and both are updated with that step's scalars"""
    a, b = make_seg(1025, 15, True, 6), make_seg(5, 16, True, 6)
    b.state = a.state
    drive(hp, "shared-state", [a, b], 1e-10, [0, 1])


def test_absent_decay_term_at_wd_zero(hp):
    """wd = 0: the term is absent, not multiplied by zero.  A -0.0 gradient is kept bit for bit and acts as a zero gradient; an
    infinite p leaves its moments finite (fmaf(0, inf, g) would have made them NaN) and stays infinite; its neighbours are untouched
    by it.  With wd = 1e-10 the same infinite p does reach its moments."""
    n = 9
    p, g, m, v = A.sweep_inputs(n, 17, True)
    g[2] = -0.0
    g[6] = -0.0
    p[4] = np.inf
    p[8] = -np.inf                                     # (in the scalar tail)
    sg = Seg(p, g, m, v, 2)
    assert launch(hp, [sg], 0.0, 0) == 0, hp.lib.okge_last_error()
    torch.cuda.synchronize()
    assert same_bits(sg.g.v, torch.from_numpy(g).cuda())
    got = [sg.p.np(), sg.m.np(), sg.v.np()]
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert got[0][4] == np.inf and got[0][8] == -np.inf
    fin = np.isfinite(p)
    check_against_float64("absent-wd0", "t0", [x[fin] for x in got], p[fin], np.where(g == 0, 0.0, g).astype(np.float32)[fin], m[fin], v[fin], 3, 0.0)
    r = A.adam64(p[~fin], g[~fin], m[~fin], v[~fin], 3, LR, BETAS, EPS, 0.0)
    assert np.all(np.abs(got[1][~fin] - r.m) <= A.adam_caps(r, m[~fin], v[~fin])[1])
    assert np.all(np.abs(got[2][~fin] - r.v) <= A.adam_caps(r, m[~fin], v[~fin])[2])
    assert sg.intact()
    sg = Seg(p, g, m, v, 2)
    assert launch(hp, [sg], 1e-10, 0) == 0, hp.lib.okge_last_error()
    torch.cuda.synchronize()
    assert not np.isfinite(sg.m.np()[[4, 8]]).any() and np.isfinite(sg.m.np()[fin]).all()
