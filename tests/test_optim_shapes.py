"""The dense optimizer, clipping and scaling kernels of csrc/okge_optim.hip, the metric kernel of csrc/okge_rank.hip and two
small kernels of csrc/okge_misc.hip through their C-ABI entry points, at the shapes where their branches change, against the
float64 restatement of tests/optim_reference.py.

Every optimizer bit-equality test of the suite (okge_adagrad_rows, okge_adagrad_rows_decay, okge_adagrad_lazy, the touched-row
map) ends at the eager entry points adagrad_kernel, adagrad2_kernel and adagrad_multi_kernel, all three over adagrad_sweep<U, MAP>.
Here those are held, element by element, to adagrad64 under adagrad_caps (|p - p'| <= 2u|p'| + 8u|delta|, |s - s'| <= 4u s'): below and
above the launchers' grid cap of 16384 x 256 threads (16 777 216 floats per pass of the grid-stride loop), with the n & 3 tail
next to other memory, with unequal tensors in both orders, every zero_grad mode, and the touched-row map at row lengths that take
the shift and the division path, 46 float4 above the cap where the unrolled lanes u = 1..3 and the clamp run.  test_optim_reference.py
holds the conditions that make these caps bite: a skipped, doubled or misplaced update is an error of at least 64 caps.
okge_adagrad_lazy, called directly, is held bit-equal to an eager twin driven by okge_adagrad_step (the project's rule for
deferral; the eager side is held to float64 above).  okge_clip_grad_norm, okge_scale_inplace, okge_rescale_gradients,
okge_merge_logsumexp, okge_rank_metrics and okge_score_triples follow, each against its restatement.

Every tensor under test is a 16-byte-aligned view inside a larger sentinel-filled buffer whose words directly before the view and
directly behind element n - 1 must survive.  Every capped comparison prints `RATIO <case> <tensor> <max error / cap>` (Adagrad:
`| <the same for adagrad32>`, the fp32 numpy chain); the table of one run is profiles/optimizer_sweep.md."""
import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

LR, EPS = 0.3, 1e-8
SENTINEL = 12345.678                                   # no result comes near it
GUARD = 64                                             # elements on each side of a view (256 bytes of fp32: the view stays aligned)
ERR_INVALID, ERR_WORKSPACE = -1, -3                    # include/okge.h
CAP = 16384 * 256 * 4                                  # floats per pass of the Adagrad launchers' grid-stride loop
N_BIG = CAP + 3075                                     # one full pass, a partial second pass, a tail of 3
SMALL = (1, 3, 4, 5, 1023, 1024, 1025, 262_147)
CHUNK = 1 << 21                                        # host-side float64 work goes through slices of this many elements
NAN_BITS = 0x7FC01234


@pytest.fixture(scope="module")
def hp(okge_lib):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


@pytest.fixture(scope="module")
def big():
    """the above-the-cap inputs, built once: (p, g, warm accumulator), fp32 numpy, left unchanged by the tests"""
    p, g, s = R.sweep_inputs(N_BIG + 400, 3, True)
    for x in (p, g, s):
        x.setflags(write=False)
    return p, g, s


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
_FILL = {torch.float32: SENTINEL, torch.float64: SENTINEL, torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A}


class Guarded:
    """`n` elements at a 16-byte-aligned offset of a sentinel-filled device buffer: .v the view, .intact() the guard words"""

    def __init__(self, data=None, n=None, dtype=torch.float32):
        if data is not None:
            data = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data
            n, dtype = data.numel(), data.dtype
        self.n = int(n)
        self.whole = torch.full((self.n + 2 * GUARD,), _FILL[dtype], dtype=dtype, device="cuda")
        self.v = self.whole[GUARD:GUARD + self.n]
        assert self.ptr() % 16 == 0
        if data is not None:
            self.v.copy_(data.reshape(-1))

    def ptr(self):
        # (not self.v.data_ptr(): torch gives an empty view a null pointer, and the entry points want an address even for n = 0)
        return self.whole.data_ptr() + GUARD * self.whole.element_size()

    def intact(self):
        fill = torch.full((GUARD,), _FILL[self.whole.dtype], dtype=self.whole.dtype, device="cuda")
        return torch.equal(self.whole[:GUARD], fill) and torch.equal(self.whole[GUARD + self.n:], fill)

    def np(self):
        return self.v.cpu().numpy()


def bits(t):
    """integer view of an fp32 / fp64 tensor (NaN-proof equality)"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Seg:
    """one tensor of an Adagrad call: guarded p, g, state_sum on the device, and the host's copy of what they hold"""

    def __init__(self, p, g, s):
        self.n = int(p.size)
        self.hp_, self.hg, self.hs = (np.array(x, dtype=np.float32) for x in (p, g, s))
        self.p, self.g, self.s = Guarded(self.hp_), Guarded(self.hg), Guarded(self.hs)

    def intact(self):
        return self.p.intact() and self.g.intact() and self.s.intact()


def make_seg(n, seed, warm, src=None, zero_g=False):
    p, g, s = (x[:n] for x in src) if src is not None else R.sweep_inputs(n, seed, warm)
    if src is not None and not warm:
        s = np.zeros(n, np.float32)
    return Seg(p, np.zeros(n, np.float32) if zero_g else g, s)


# ---- the three eager entry points behind one launcher ---------------------------------------------------------------------
def multi_array(segs, zero, maps=None):
    from open_knowledge_graph_embeddings_amd import _native as N
    arr = (N.AdagradTensor * len(segs))()
    for k, (a, sg) in enumerate(zip(arr, segs)):
        a.p, a.g, a.state_sum, a.n, a.zero_grad = sg.p.ptr(), sg.g.ptr(), sg.s.ptr(), sg.n, int(zero[k])
        if maps is not None and maps[k] is not None:
            a.row_touched, a.row_len, a.touched_stamp = maps[k][0].ptr(), int(maps[k][1]), int(maps[k][2])
    return arr


def launch(hp, entry, segs, wd, zero, lr=LR, eps=EPS):
    """zero: per tensor whether its gradient is cleared.  -> the status"""
    L = hp.lib
    if entry == "step":
        (a,) = segs
        return int(L.okge_adagrad_step(a.p.ptr(), a.g.ptr(), a.s.ptr(), a.n, lr, wd, eps, int(zero[0]), hp._stream()))
    if entry == "step2":
        a, b = segs
        mode = {(0, 0): 0, (1, 1): 1, (0, 1): 2}[tuple(int(z) for z in zero)]
        return int(L.okge_adagrad_step2(a.p.ptr(), a.g.ptr(), a.s.ptr(), a.n, b.p.ptr(), b.g.ptr(), b.s.ptr(), b.n, lr, wd, eps, mode,
                                        hp._stream()))
    return int(L.okge_adagrad_multi(multi_array(segs, zero), len(segs), lr, wd, eps, hp._stream()))


def check_against_float64(case, tensor, got_p, got_s, p, g, s, wd):
    """p, s against adagrad64 under adagrad_caps, element by element, in slices; prints the RATIO line, then asserts"""
    n = int(p.size)
    worst, yard = [0.0, 0.0], [0.0, 0.0]
    finite = bool(np.isfinite(got_p).all() and np.isfinite(got_s).all())
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(n, lo + CHUNK))
        p1, s1, delta = R.adagrad64(p[sl], g[sl], s[sl], LR, wd, EPS)
        assert not R.underflowed(s1).any(), (case, tensor, "the inputs leave the range the caps are stated for")
        r = R.cap_ratios(got_p[sl], got_s[sl], p1, s1, delta)
        worst = [max(a, b) for a, b in zip(worst, r)]
        if lo == 0:                                    # the yardstick on the first slice (2 M elements at most)
            yard = R.cap_ratios(*R.adagrad32(p[sl], g[sl], s[sl], LR, wd, EPS), p1, s1, delta)
    print("RATIO %s %s.p %.3f | %.3f" % (case, tensor, worst[0], yard[0]))
    print("RATIO %s %s.s %.3f | %.3f" % (case, tensor, worst[1], yard[1]))
    assert finite and worst[0] <= 1.0 and worst[1] <= 1.0, (case, tensor, worst, finite)


def drive(hp, case, entry, segs, wd, plan):
    """one launch per entry of `plan` (per tensor: clear the gradient or not).  After each: p and s against float64 from the
    state the launch started from (the kernel's own after the first), the gradient bit for bit untouched or exactly zero, the
    guard words intact"""
    for step, zero in enumerate(plan):
        before = [sg.g.v.clone() for sg in segs]
        assert launch(hp, entry, segs, wd, zero) == 0, (case, hp.lib.okge_last_error())
        torch.cuda.synchronize()
        for k, sg in enumerate(segs):
            name = "%s step%d" % (case, step)
            got_p, got_s = sg.p.np(), sg.s.np()
            check_against_float64(name, "t%d" % k, got_p, got_s, sg.hp_, sg.hg, sg.hs, wd)
            if zero[k]:
                assert not bool(sg.g.v.any()) and not bool(torch.signbit(sg.g.v).any()), (name, k, "gradient not cleared to +0")
                sg.hg = np.zeros(sg.n, np.float32)
            else:
                assert same_bits(sg.g.v, before[k]), (name, k, "gradient touched without zero_grad")
            sg.hp_, sg.hs = got_p, got_s
            assert sg.intact(), (name, k, "guard words overwritten")


CONFIGS = [("cold", 1e-10), ("cold", 1e-3), ("warm", 1e-10), ("warm", 1e-3)]


@pytest.mark.parametrize("acc,wd", CONFIGS, ids=["cold-wd1e-10", "cold-wd1e-3", "warm-wd1e-10", "warm-wd1e-3"])
@pytest.mark.parametrize("n", SMALL)
def test_step_sizes(hp, n, acc, wd):
    """okge_adagrad_step: zero_grad 0 then 1, two consecutive steps"""
    drive(hp, "step-n%d-%s-wd%g" % (n, acc, wd), "step", [make_seg(n, 10, acc == "warm")], wd, [(0,), (1,)])


PAIRS = [(1025, 3), (3, 1025), (262_147, 5), (5, 262_147), (1023, 1023), (1024, 0), (0, 7)]


@pytest.mark.parametrize("acc,wd", CONFIGS, ids=["cold-wd1e-10", "cold-wd1e-3", "warm-wd1e-10", "warm-wd1e-3"])
@pytest.mark.parametrize("n0,n1", PAIRS)
def test_step2_sizes_and_modes(hp, n0, n1, acc, wd):
    """okge_adagrad_step2: unequal lengths in both orders (the longer tensor sizes the grid, the shorter one's tail falls in
    workgroup 0), an empty tensor on either side; zero_grad 0, then 2 (second only), then 1 (both)"""
    segs = [make_seg(n0, 11, acc == "warm"), make_seg(n1, 12, acc == "warm")]
    drive(hp, "step2-n%d-n%d-%s-wd%g" % (n0, n1, acc, wd), "step2", segs, wd, [(0, 0), (0, 1), (1, 1)])


QUADS = [(1023, 262_147, 5, 0), (3, 1, 1025, 1024), (0, 4, 0, 262_147)]


@pytest.mark.parametrize("acc,wd", CONFIGS, ids=["cold-wd1e-10", "cold-wd1e-3", "warm-wd1e-10", "warm-wd1e-3"])
@pytest.mark.parametrize("ns", QUADS, ids=lambda q: "-".join(str(x) for x in q))
def test_multi_sizes_and_per_tensor_zero_grad(hp, ns, acc, wd):
    """okge_adagrad_multi without a map: four tensors, zero_grad per tensor"""
    segs = [make_seg(n, 20 + k, acc == "warm") for k, n in enumerate(ns)]
    drive(hp, "multi-%s-%s-wd%g" % ("-".join(map(str, ns)), acc, wd), "multi", segs, wd, [(0, 1, 0, 1), (1, 0, 1, 1)])
    one = [make_seg(ns[1], 24, acc == "warm")]
    drive(hp, "multi-one-n%d-%s-wd%g" % (ns[1], acc, wd), "multi", one, wd, [(0,), (1,)])


@pytest.mark.parametrize("acc,wd", CONFIGS, ids=["cold-wd1e-10", "cold-wd1e-3", "warm-wd1e-10", "warm-wd1e-3"])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 1027, 262_147])
def test_entry_points_agree_bit_for_bit(hp, n, acc, wd):
    """okge_adagrad_step, okge_adagrad_step2 (the tensor in either slot, a one-element dummy in the other) and okge_adagrad_multi
    without a map, on copies of the same p, g and state_sum, under every zero_grad setting: the same bits in p and in state_sum
    from all of them; the gradient +0 wherever the setting clears this tensor, its own bits wherever it does not"""
    src = R.sweep_inputs(n, 170, acc == "warm")
    dummy_src = R.sweep_inputs(1, 171, acc == "warm")
    variants = [("step", None, (z,)) for z in (0, 1)] + [("multi", None, (z,)) for z in (0, 1)] + \
               [("step2", slot, zero) for slot in (0, 1) for zero in ((0, 0), (1, 1), (0, 1))]
    want = None
    for entry, slot, zero in variants:
        sg = Seg(*src)
        segs = [sg] if slot is None else ([sg, Seg(*dummy_src)] if slot == 0 else [Seg(*dummy_src), sg])
        g0 = sg.g.v.clone()
        assert launch(hp, entry, segs, wd, zero) == 0, (entry, slot, zero, hp.lib.okge_last_error())
        torch.cuda.synchronize()
        where = (n, acc, wd, entry, slot, zero)
        if want is None:
            want = (sg.p.v.clone(), sg.s.v.clone())
            assert not same_bits(want[0], torch.from_numpy(np.array(src[0], np.float32)).cuda()), where + ("the step moved nothing",)
        assert same_bits(sg.p.v, want[0]), where + ("p differs from okge_adagrad_step's",)
        assert same_bits(sg.s.v, want[1]), where + ("state_sum differs from okge_adagrad_step's",)
        if zero[slot or 0]:
            assert not bool(bits(sg.g.v).any()), where + ("gradient not cleared to +0",)
        else:
            assert same_bits(sg.g.v, g0), where + ("gradient touched without zero_grad",)
        assert all(x.intact() for x in segs), where + ("guard words overwritten",)


@pytest.mark.parametrize("entry,acc,wd", [("step", "cold", 1e-3), ("step2", "warm", 1e-10), ("multi", "cold", 1e-10)])
def test_above_the_grid_cap(hp, big, entry, acc, wd):
    """16 777 216 + 3075 floats: the second pass of the grid-stride loop and a tail of 3 behind it; the other tensors of a call
    are short, so that their tails fall in workgroup 0 of a grid the long tensor sized"""
    long_ = make_seg(N_BIG, 0, acc == "warm", src=big)
    segs = {"step": [long_], "step2": [long_, make_seg(5, 30, acc == "warm")],
            "multi": [make_seg(1025, 31, acc == "warm"), long_, make_seg(3, 32, acc == "warm"), make_seg(0, 33, False)]}[entry]
    plan = {"step": [(0,), (1,)], "step2": [(0, 1), (1, 1)], "multi": [(0, 0, 1, 0), (1, 1, 1, 1)]}[entry]
    drive(hp, "%s-big-%s-wd%g" % (entry, acc, wd), entry, segs, wd, plan)


@pytest.mark.parametrize("entry", ["step", "step2", "step2-long-second", "multi"])
@pytest.mark.parametrize("n", [5, 1025, 262_147, N_BIG])
def test_decay_only_rows_keep_their_bits(hp, big, entry, n):
    """a warm accumulator, wd = 1e-10, g = 0: the update is below half an ulp of p and of s (test_optim_reference.py), so the
    bits of p and s are unchanged; the gradient stays +0"""
    long_ = make_seg(n, 40, True, src=big if n == N_BIG else None, zero_g=True)
    short = make_seg(7, 41, True, zero_g=True)
    segs = {"step": [long_], "step2": [long_, short], "step2-long-second": [short, long_],
            "multi": [short, long_, make_seg(0, 42, True), make_seg(3, 43, True, zero_g=True)]}[entry]
    kind = "step2" if entry.startswith("step2") else entry
    before = [(sg.p.v.clone(), sg.s.v.clone()) for sg in segs]
    for zero in ([0] * len(segs), [1] * len(segs)):
        assert launch(hp, kind, segs, 1e-10, zero) == 0, hp.lib.okge_last_error()
        torch.cuda.synchronize()
        for k, (sg, (p0, s0)) in enumerate(zip(segs, before)):
            assert same_bits(sg.p.v, p0) and same_bits(sg.s.v, s0), (entry, n, k, "a decay-only element moved")
            assert not bool(bits(sg.g.v).any()) and sg.intact(), (entry, n, k)


def test_misaligned_pointers_are_refused(hp):
    """p, g or state_sum 4 bytes off a 16-byte boundary: OKGE_ERR_INVALID from all three entry points, nothing written"""
    from open_knowledge_graph_embeddings_amd import _native as N
    n = 1024
    sg, other = make_seg(n + 1, 50, True), make_seg(8, 51, True)
    wholes = [x.whole for s_ in (sg, other) for x in (s_.p, s_.g, s_.s)]
    before = [w.clone() for w in wholes]
    L = hp.lib
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        ptrs = [x.ptr() + o for x, o in zip((sg.p, sg.g, sg.s), off)]
        assert L.okge_adagrad_step(*ptrs, n, LR, 1e-3, EPS, 1, hp._stream()) == ERR_INVALID
        assert L.okge_adagrad_step2(*ptrs, n, other.p.ptr(), other.g.ptr(), other.s.ptr(), 8, LR, 1e-3, EPS, 1, hp._stream()) == ERR_INVALID
        assert L.okge_adagrad_step2(other.p.ptr(), other.g.ptr(), other.s.ptr(), 8, *ptrs, n, LR, 1e-3, EPS, 1, hp._stream()) == ERR_INVALID
        arr = (N.AdagradTensor * 2)()
        arr[0].p, arr[0].g, arr[0].state_sum, arr[0].n, arr[0].zero_grad = other.p.ptr(), other.g.ptr(), other.s.ptr(), 8, 1
        arr[1].p, arr[1].g, arr[1].state_sum, arr[1].n, arr[1].zero_grad = ptrs[0], ptrs[1], ptrs[2], n, 1
        assert L.okge_adagrad_multi(arr, 2, LR, 1e-3, EPS, hp._stream()) == ERR_INVALID
    torch.cuda.synchronize()
    for w, b in zip(wholes, before):
        assert same_bits(w, b)


# ---- the touched-row map ---------------------------------------------------------------------------------------------------
STAMP = 7
BIG_ROWS, BIG_LEN = 83_887, 200                        # n4 = 4 194 350: 46 float4 above the cap, the lanes u = 1..3 and the clamp run
assert BIG_ROWS * BIG_LEN // 4 - CAP // 4 == 46


def map_case(hp, case, rows, row_len, acc, wd, stamp_last, src=None):
    """stamped rows carry a gradient, every other row NaN: stamped rows take the step with their gradient and have it cleared,
    the others the decay-only step with their NaNs neither read nor cleared"""
    n = rows * row_len
    sg = make_seg(n, 60, acc == "warm", src=src)
    rng = np.random.default_rng([61, rows, row_len, int(stamp_last)])
    m = rng.choice(np.array([STAMP, STAMP, 0, STAMP - 1, STAMP + 1, 255], np.uint8), rows)
    m[0] = STAMP                                       # the first row; the last row either way (at the big shape it straddles the
    m[-1] = STAMP if stamp_last else STAMP + 1         # pass boundary: floats 16 777 200 .. 16 777 399)
    if rows > 2:
        m[-2] = STAMP + 1 if stamp_last else STAMP
    live = np.repeat(m == STAMP, row_len)
    g_dev = torch.from_numpy(sg.hg).cuda()
    nan = torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    live_dev = torch.from_numpy(live).cuda()
    sg.g.v.copy_(torch.where(live_dev, g_dev, nan))
    before_g = sg.g.v.clone()
    map_dev = Guarded(m)
    arr = multi_array([sg], [1], [(map_dev, row_len, STAMP)])
    assert hp.lib.okge_adagrad_multi(arr, 1, LR, wd, EPS, hp._stream()) == 0, (case, hp.lib.okge_last_error())
    torch.cuda.synchronize()
    check_against_float64(case, "mapped", sg.p.np(), sg.s.np(), sg.hp_, np.where(live, sg.hg, np.float32(0)), sg.hs, wd)
    want_g = torch.where(live_dev, torch.zeros_like(before_g), before_g)
    assert same_bits(sg.g.v, want_g), (case, "stamped gradients must be +0, the NaNs of the other rows untouched")
    assert sg.intact() and map_dev.intact() and np.array_equal(map_dev.np(), m), case
    return sg


@pytest.mark.parametrize("acc,wd", [("cold", 1e-3), ("warm", 1e-10), ("warm", 1e-3)], ids=["cold-wd1e-3", "warm-wd1e-10", "warm-wd1e-3"])
@pytest.mark.parametrize("rows", [1, 17, 5000])
@pytest.mark.parametrize("row_len", [4, 64, 200])
def test_touched_row_map(hp, row_len, rows, acc, wd):
    """row lengths 4 and 64 take the shift, 200 the division"""
    for stamp_last in (True, False):
        map_case(hp, "map-r%d-l%d-%s-wd%g-%s" % (rows, row_len, acc, wd, "last" if stamp_last else "nolast"), rows, row_len, acc, wd,
                 stamp_last)


@pytest.mark.parametrize("stamp_last", [True, False], ids=["last-row-stamped", "last-row-not-stamped"])
def test_touched_row_map_above_the_grid_cap(hp, big, stamp_last):
    """83 887 rows of 200 floats.  The last row holds the float4 the second pass reaches (lane u = 1 of threads 0..45): stamped,
    they take its gradient; not stamped, its NaNs must stay out"""
    map_case(hp, "map-big-%s" % ("last" if stamp_last else "nolast"), BIG_ROWS, BIG_LEN, "warm", 1e-3, stamp_last, src=big)


def test_touched_row_map_refusals(hp):
    """a map with zero_grad = 0, a stamp outside 1..255, a row length that is no multiple of 4, rows that do not tile the tensor:
    refused, nothing written"""
    sg = make_seg(24, 70, True)
    m = Guarded(np.full(6, STAMP, np.uint8))
    wholes = [sg.p.whole, sg.g.whole, sg.s.whole]
    before = [w.clone() for w in wholes]
    for zero, row_len, stamp, what in ((0, 4, STAMP, "zero_grad = 0"), (1, 4, 0, "stamp 0"), (1, 4, 256, "stamp 256"),
                                       (1, 6, STAMP, "row length 6"), (1, 16, STAMP, "24 floats in rows of 16")):
        arr = multi_array([sg], [zero], [(m, row_len, stamp)])
        assert hp.lib.okge_adagrad_multi(arr, 1, LR, 1e-3, EPS, hp._stream()) == ERR_INVALID, what
    torch.cuda.synchronize()
    for w, b in zip(wholes, before):
        assert same_bits(w, b)
    arr = multi_array([sg], [1], [(m, 4, STAMP)])
    assert hp.lib.okge_adagrad_multi(arr, 1, LR, 1e-3, EPS, hp._stream()) == 0


# ---- okge_adagrad_lazy, called directly --------------------------------------------------------------------------------------
def lazy_run(hp, case, specs, window, wd, steps=5, seed=0):
    """specs: (rows, row_len, kind) with kind 'map' (row_steps + touched map), 'steps' (row_steps only) or 'dense' (rows * row_len
    plain floats).  Five STEPs with moving stamps, then FLUSH; the eager twin takes one okge_adagrad_step per STEP with zero
    gradients on the rows that are not stamped.  Everything stays on the device: the comparison is bit for bit."""
    from open_knowledge_graph_embeddings_amd import _native as N
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 + seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)                       # noqa: E731
    T = []
    for rows, row_len, kind in specs:
        n = rows * row_len
        p = 0.1 * rnd(n)
        s = torch.rand(n, device="cuda", generator=gen) * 0.99 + 0.01
        if kind != "dense" and rows > 1:
            s.view(rows, row_len)[::2] = 0.0           # every other row starts cold
        t = dict(rows=rows, row_len=row_len, kind=kind, n=n, p=Guarded(p), s=Guarded(s), g=Guarded(torch.zeros(n, device="cuda")),
                 tp=Guarded(p), ts=Guarded(s), tg=Guarded(torch.zeros(n, device="cuda")))
        if kind != "dense":
            t["steps"] = Guarded(torch.zeros(rows, dtype=torch.int32))
        if kind == "map":
            t["map"] = Guarded(torch.zeros(rows, dtype=torch.uint8))
        T.append(t)
    counters = Guarded(torch.zeros(2, dtype=torch.int32))
    L = hp.lib

    def lazy_call(mode, stamp):
        arr = (N.LazyTensor * len(T))()
        for a, t in zip(arr, T):
            a.p, a.g, a.state_sum = t["p"].ptr(), t["g"].ptr(), t["s"].ptr()
            if t["kind"] == "dense":
                a.rows, a.row_len = 1, t["n"]
            else:
                a.rows, a.row_len, a.row_steps = t["rows"], t["row_len"], t["steps"].ptr()
                if t["kind"] == "map":
                    a.row_touched, a.touched_stamp = t["map"].ptr(), stamp
        assert L.okge_adagrad_lazy(arr, len(T), counters.ptr(), window, mode, LR, wd, EPS, hp._stream()) == 0, (case, L.okge_last_error())

    def twin_step():
        for t in T:
            assert L.okge_adagrad_step(t["tp"].ptr(), t["tg"].ptr(), t["ts"].ptr(), t["n"], LR, wd, EPS, 0, hp._stream()) == 0

    for step in range(steps):
        stamp = (step * 37) % 255 + 1
        others = torch.tensor([0, stamp - 1, stamp + 1 if stamp < 255 else 0, 255 if stamp != 255 else 0], dtype=torch.uint8, device="cuda")
        stamped = {}
        for k, t in enumerate(T):
            grad = rnd(t["n"]) * 10.0 ** torch.randint(-4, 0, (t["n"],), device="cuda", generator=gen).float()
            if t["kind"] == "map":
                rows = t["rows"]
                hit = torch.rand(rows, device="cuda", generator=gen) < 0.3
                hit[0] = step % 2 == 0
                hit[-1] = step % 2 == 1 or rows == 1
                noise = others[torch.randint(0, 4, (rows,), device="cuda", generator=gen)]
                t["map"].v.copy_(torch.where(hit, torch.full_like(noise, stamp), noise))
                stamped[k] = (hit, t["map"].v.clone())
                grad = torch.where(hit[:, None], grad.view(rows, t["row_len"]), torch.zeros((), device="cuda")).reshape(-1)      # (+0, not grad * 0)
            elif t["kind"] == "steps":
                grad = torch.zeros_like(grad)          # no map: only the due slice moves, by decay alone
            t["g"].v.copy_(grad)
            t["tg"].v.copy_(grad)
        lazy_call(0, stamp)
        twin_step()
        torch.cuda.synchronize()
        c = counters.np()
        assert c[0] == step + 1 and c[1] == 0 and counters.intact(), (case, step, c)
        for k, t in enumerate(T):
            where = (case, "step", step, "tensor", k)
            assert not bool(bits(t["g"].v).any()), where + ("gradient not cleared",)
            if t["kind"] == "dense":
                assert same_bits(t["p"].v, t["tp"].v) and same_bits(t["s"].v, t["ts"].v), where + ("dense tensor",)
            else:
                st = t["steps"].v
                assert bool((st <= step + 1).all()) and bool((st >= 0).all()), where
                now = (st == step + 1)[:, None]        # rows that are up to date are the twin's rows already
                for a, b in ((t["p"], t["tp"]), (t["s"], t["ts"])):
                    av, bv = bits(a.v).view(t["rows"], -1), bits(b.v).view(t["rows"], -1)
                    assert torch.equal(torch.where(now, av, bv), bv), where + ("an up-to-date row differs from the twin",)
            if t["kind"] == "map":
                hit, m0 = stamped[k]
                assert bool((t["steps"].v[hit] == step + 1).all()), where
                assert torch.equal(t["map"].v, torch.where(hit, torch.zeros_like(m0), m0)), where + ("map bytes",)
    dense_before = [(t["p"].v.clone(), t["s"].v.clone()) for t in T]
    lazy_call(1, 1)
    torch.cuda.synchronize()
    c = counters.np()
    assert c[0] == steps and c[1] == 0, (case, c)
    for k, t in enumerate(T):
        where = (case, "flush", "tensor", k)
        assert same_bits(t["p"].v, t["tp"].v) and same_bits(t["s"].v, t["ts"].v), where + ("tables differ from the eager twin",)
        if t["kind"] == "dense":
            assert same_bits(t["p"].v, dense_before[k][0]) and same_bits(t["s"].v, dense_before[k][1]), where + ("FLUSH moved a dense tensor",)
        else:
            assert bool((t["steps"].v == steps).all()), where
        for key in ("p", "s", "g", "steps", "map"):
            assert key not in t or t[key].intact(), where + (key, "guard words")
    return [(t["p"].v, t["s"].v) for t in T]


@pytest.mark.parametrize("wd", [1e-3, 1e-10])
@pytest.mark.parametrize("row_len", [4, 200, 256, 260, 1024])
def test_lazy_small_tables(hp, row_len, wd):
    """1, 15, 16, 17 rows (one batch of 16 and its edges) x windows 1, 3, rows + 5; 1024 floats: the row4 > 64 column loop"""
    for rows in (1, 15, 16, 17):
        for window in (1, 3, rows + 5):
            lazy_run(hp, "lazy-r%d-l%d-w%d-wd%g" % (rows, row_len, window, wd), [(rows, row_len, "map")], window, wd, seed=rows + window)


@pytest.mark.parametrize("row_len,window", [(4, 3), (200, 81_942), (256, 1), (260, 3), (1024, 3)])
def test_lazy_second_batch_per_wave(hp, row_len, window):
    """81 937 rows: more than 1280 x 4 x 16, so a wave takes a second batch of rows"""
    lazy_run(hp, "lazy-r81937-l%d-w%d" % (row_len, window), [(81_937, row_len, "map")], window, 1e-3, seed=row_len)


@pytest.mark.parametrize("window", [1, 3, 30])
def test_lazy_mixed_tensors(hp, window):
    """two deferred tables (one with a map, one without) and two plain dense tensors of odd length in one call: the dense ones
    step every STEP with their gradient cleared and are left alone by FLUSH"""
    specs = [(17, 200, "map"), (1023, 1, "dense"), (25, 4, "steps"), (5, 1, "dense")]
    lazy_run(hp, "lazy-mixed-w%d" % window, specs, window, 1e-3, seed=window)


# ---- okge_clip_grad_norm ------------------------------------------------------------------------------------------------------
def clip_call(hp, g0, n0, g1, n1, max_norm, norm_out, ws, ws_len=None):
    return int(hp.lib.okge_clip_grad_norm(g0.ptr(), n0, None if g1 is None else g1.ptr(), n1, max_norm,
                                          None if norm_out is None else norm_out.ptr(), ws.ptr(), ws.n if ws_len is None else ws_len,
                                          hp._stream()))


@pytest.mark.parametrize("n0", [1, 255, 262_144, 262_147, 1_048_576 + 259])
def test_clip_grad_norm(hp, n0):
    """g1 null / empty / shorter / longer x norm below max_norm, above it, all-zero gradients; norm_out given and null"""
    rng = np.random.default_rng([80, n0])
    ws = Guarded(n=8448, dtype=torch.uint8)
    for second in ("null", "empty", "shorter", "longer"):
        n1 = {"null": 0, "empty": 0, "shorter": max(n0 // 3, 1) if n0 > 1 else 0, "longer": 2 * n0 + 1}[second]
        for kind in ("below", "above", "zero"):
            case = "clip-n%d-%s-%s" % (n0, second, kind)
            h0 = (rng.standard_normal(n0) * 10.0 ** rng.integers(-3, 1, n0)).astype(np.float32)
            h1 = (rng.standard_normal(n1) * 10.0 ** rng.integers(-3, 1, n1)).astype(np.float32)
            if kind == "zero":
                h0[:], h1[:] = 0, 0
            want_total, _ = R.clip64(h0, h1, 1.0)
            max_norm = {"below": 2.0 * float(want_total), "above": 0.37 * float(want_total), "zero": 1.0}[kind]
            g0, g1 = Guarded(h0), (None if second == "null" else Guarded(h1))
            norm = Guarded(torch.full((1,), -1.0, dtype=torch.float64))
            assert clip_call(hp, g0, n0, g1, n1, max_norm, norm, ws) == 0, (case, hp.lib.okge_last_error())
            torch.cuda.synchronize()
            got = float(norm.np()[0])
            ulps = abs(got - float(want_total)) / float(np.spacing(want_total)) if want_total > 0 else abs(got)
            print("RATIO %s norm_out %.3f" % (case, ulps))         # (distance from fp32(sqrt(sum g^2)) in fp32 ulps: 0 or 1)
            assert float(np.float32(got)) == got and ulps <= 1.0, (case, got, float(want_total))
            coef = R.clip_coef(np.float32(got), max_norm)
            if kind != "above":
                assert coef == np.float32(1.0), (case, coef)
            else:
                assert coef < np.float32(0.5)
            assert np.array_equal(g0.np().view(np.uint32), (h0 * coef).view(np.uint32)), (case, "g0")
            if g1 is not None:
                assert np.array_equal(g1.np().view(np.uint32), (h1 * coef).view(np.uint32)), (case, "g1")
            assert g0.intact() and norm.intact() and ws.intact() and (g1 is None or g1.intact()), case
            # norm_out null: the same gradients
            f0, f1 = Guarded(h0), (None if second == "null" else Guarded(h1))
            assert clip_call(hp, f0, n0, f1, n1, max_norm, None, ws) == 0
            torch.cuda.synchronize()
            assert same_bits(f0.v, g0.v) and (f1 is None or same_bits(f1.v, g1.v)), (case, "norm_out null")


def test_clip_grad_norm_refusals(hp):
    h = np.arange(1, 9, dtype=np.float32)
    g0, g1 = Guarded(h), Guarded(h)
    norm = Guarded(torch.full((1,), -1.0, dtype=torch.float64))
    ws = Guarded(n=8448, dtype=torch.uint8)
    wholes = [g0.whole, g1.whole, norm.whole, ws.whole]
    before = [w.clone() for w in wholes]
    assert clip_call(hp, g0, 8, g1, 8, 1.0, norm, ws, ws_len=8447) == ERR_WORKSPACE
    assert clip_call(hp, g0, 8, g1, 8, 0.0, norm, ws) == ERR_INVALID
    assert clip_call(hp, g0, 8, g1, 8, -1.0, norm, ws) == ERR_INVALID
    assert clip_call(hp, g0, 8, g1, 8, float("nan"), norm, ws) == ERR_INVALID
    torch.cuda.synchronize()
    for w, b in zip(wholes, before):
        assert torch.equal(w, b)
    assert clip_call(hp, g0, 8, g1, 8, 1.0, norm, ws) == 0


# ---- okge_scale_inplace / okge_rescale_gradients ---------------------------------------------------------------------------
def scalar(x):
    return torch.tensor([x], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("n", [1, 257, 524_288 + 5, 1_048_576 + 5])
def test_scale_inplace(hp, n):
    """1 048 576 elements per pass of scale_kernel's grid: the last size takes a second pass"""
    rng = np.random.default_rng([90, n])
    h = rng.standard_normal(n).astype(np.float32)
    for a in (0.37, -3.0, 1.0):
        x, alpha = Guarded(h), scalar(a)
        assert hp.lib.okge_scale_inplace(x.ptr(), n, alpha.data_ptr(), hp._stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(x.np().view(np.uint32), (h * np.float32(a)).view(np.uint32)), (n, a)
        assert x.intact(), (n, a)


@pytest.mark.parametrize("n0,n1", [(1, 0), (257, 1), (1, 257), (524_288 + 5, 1_048_576 + 5), (1_048_576 + 5, 524_288 + 5), (524_288 + 5, 0)])
def test_rescale_gradients(hp, n0, n1):
    """524 288 elements per pass of rescale2_kernel's grid; g1 null when n1 = 0"""
    rng = np.random.default_rng([91, n0, n1])
    h0, h1 = rng.standard_normal(n0).astype(np.float32), rng.standard_normal(n1).astype(np.float32)
    for alpha, applied in ((0.5, 0.125), (1.0 / 3.0, 7.0), (3.0, 3.0000002)):
        r = np.float32(alpha) / np.float32(applied)
        assert r != np.float32(1.0)
        x0, x1, a = Guarded(h0), (Guarded(h1) if n1 else None), scalar(alpha)
        assert hp.lib.okge_rescale_gradients(x0.ptr(), n0, None if x1 is None else x1.ptr(), n1, a.data_ptr(), applied, hp._stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(x0.np().view(np.uint32), (h0 * r).view(np.uint32)), (n0, n1, alpha, applied, "g0")
        assert x1 is None or np.array_equal(x1.np().view(np.uint32), (h1 * r).view(np.uint32)), (n0, n1, alpha, applied, "g1")
        assert x0.intact() and (x1 is None or x1.intact())
    # alpha == applied: nothing is written -- NaN payloads and -0.0 keep their bits
    for h in (h0, h1):
        if h.size:
            h[-1] = -0.0
            h.view(np.uint32)[0] = NAN_BITS
            if h.size > 2:
                h[h.size // 2] = -0.0
    for value in (0.3, 1.0):
        x0, x1, a = Guarded(h0), (Guarded(h1) if n1 else None), scalar(value)
        applied = float(np.float32(value))
        assert hp.lib.okge_rescale_gradients(x0.ptr(), n0, None if x1 is None else x1.ptr(), n1, a.data_ptr(), applied, hp._stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(x0.np().view(np.uint32), h0.view(np.uint32)) and x0.intact(), (n0, n1, value)
        assert x1 is None or (np.array_equal(x1.np().view(np.uint32), h1.view(np.uint32)) and x1.intact()), (n0, n1, value)


# ---- okge_merge_logsumexp ------------------------------------------------------------------------------------------------
def logsumexp64(x):
    x = np.asarray(x, np.float64)
    m = x.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m + np.log(np.exp(x - np.where(np.isfinite(m), m, 0.0)).sum(0))
    return np.where(np.isfinite(m), out, -np.inf)


@pytest.mark.parametrize("B", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_merge_logsumexp(hp, world, B):
    """magnitudes up to +-80, -inf entries, a column that is -inf on every shard (-> -inf, not NaN), a column one shard dominates by
    more than 100; float64 logsumexp at the tolerance test_dropin_path.py uses for this kernel (rtol 2e-6, atol 2e-6)"""
    rng = np.random.default_rng([100, world, B])
    for special in (False, True):
        x = np.clip(rng.standard_normal((world, B)) * 30, -80, 80).astype(np.float32)
        x[rng.random((world, B)) < 0.1] = -np.inf
        if special:
            if B > 1:
                x[:, B - 1] = -60.0
                x[world // 2, B - 1] = 50.0
            x[:, 0] = -np.inf
        want = logsumexp64(x)
        parts, out = Guarded(x), Guarded(n=B)
        assert hp.lib.okge_merge_logsumexp(parts.ptr(), world, B, out.ptr(), hp._stream()) == 0
        torch.cuda.synchronize()
        got = out.np().astype(np.float64)
        fin = np.isfinite(want)
        assert not np.isnan(got).any() and np.array_equal(got[~fin], want[~fin]), (world, B, special)
        err = np.abs(got[fin] - want[fin])
        tol = 2e-6 + 2e-6 * np.abs(want[fin])
        print("RATIO lse-w%d-B%d-%s out %.3f" % (world, B, "special" if special else "plain", float((err / tol).max()) if err.size else 0.0))
        assert np.all(err <= tol), (world, B, special, float(err.max()))
        if special and B == 1:
            assert got[0] == -np.inf
        assert out.intact() and parts.intact()


# ---- okge_rank_metrics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 255, 256, 257, 100_003])
def test_rank_metrics(hp, n):
    """ranks at the Hits@k edges and above 2^31, a non-zero accumulator on entry, two calls: the five counts exact, the rank sum
    exact (below 2^53), the reciprocal sum within 1e-12 of the restatement (both sum fp32 reciprocals in double: only the order
    differs)"""
    rng = np.random.default_rng([110, n])
    special = np.array([0, 2, 3, 9, 10, 49, 50, 2 ** 31 + 5, 2 ** 33, 2 ** 40 + 7, 1, 48, 51], np.int64)
    ranks = np.concatenate([special, rng.integers(0, 20_000, max(n, 13))])[:n].astype(np.int64)
    rng.shuffle(ranks)
    acc0 = np.array([5.0, 0.25, 1000.0, 1.0, 2.0, 3.0, 4.0])
    m = R.rank_meters(ranks)
    acc = Guarded(acc0)
    r_dev = Guarded(ranks) if n else Guarded(np.zeros(1, np.int64))
    for _ in range(2):
        assert hp.lib.okge_rank_metrics(r_dev.ptr(), n, acc.ptr(), hp._stream()) == 0
    torch.cuda.synchronize()
    got = acc.np()
    assert acc0[2] + 2 * m[2] < 2 ** 53
    for k in (0, 2, 3, 4, 5, 6):
        assert got[k] == acc0[k] + 2 * m[k], (n, k, got[k], m[k])
    want = acc0[1] + 2 * m[1]
    print("RATIO rank-metrics-n%d mrr-sum %.3f" % (n, abs(got[1] - want) / (1e-12 * want)))
    assert abs(got[1] - want) <= 1e-12 * want, (n, got[1], want)
    if n == 0:
        assert np.array_equal(got, acc0)
    assert acc.intact() and r_dev.intact()


# ---- okge_score_triples --------------------------------------------------------------------------------------------------
COMPLEX_D = (2, 6, 126, 128, 130, 200, 512, 516, 4096)
SCORE_CASES = [("complex", d) for d in COMPLEX_D] + [("distmult", d) for d in COMPLEX_D + (1, 3, 63, 65, 129)]


def triple_operands(n, d, seed):
    """three (n, d) operands as views of buffers with different leading dimensions, NaN behind every row"""
    rng = np.random.default_rng([120, n, d, seed])
    host, views = [], []
    for pad in (1, 3, 8):
        x = (rng.standard_normal((n, d)) * 0.5).astype(np.float32)
        buf = torch.full((n, d + pad), float("nan"), device="cuda")
        buf[:, :d] = torch.from_numpy(x).cuda()
        host.append(x)
        views.append(buf[:, :d])
    return host, views


def score_call(hp, scorer, views, n, d, out, lds=None):
    from open_knowledge_graph_embeddings_amd import _native as N
    s, r, o = views
    lds = [v.stride(0) for v in views] if lds is None else lds
    return int(hp.lib.okge_score_triples(N.SCORERS[scorer], s.data_ptr(), lds[0], r.data_ptr(), lds[1], o.data_ptr(), lds[2], n, d, out.ptr(),
                                         hp._stream()))


@pytest.mark.parametrize("scorer,d", SCORE_CASES, ids=lambda x: str(x))
def test_score_triples(hp, scorer, d):
    """every score within (ceil(K / 64) + 12) 2^-24 A of float64: K the length of a lane's chain (d / 2 ComplEx, d DistMult), A the
    sum of absolute products -- the chain, six butterfly levels, at most six roundings inside a term"""
    K = d // 2 if scorer == "complex" else d
    for n in (1, 3, 4, 5, 257):
        host, views = triple_operands(n, d, 0)
        out = Guarded(n=n)
        assert score_call(hp, scorer, views, n, d, out) == 0, hp.lib.okge_last_error()
        torch.cuda.synchronize()
        got = out.np().astype(np.float64)
        want, A = R.score_triples64(scorer, *host)
        cap = (-(-K // 64) + 12) * R.U * A
        err = np.abs(got - want)
        print("RATIO score-%s-d%d-n%d out %.3f" % (scorer, d, n, float((err / cap).max())))
        assert np.isfinite(got).all() and np.all(err <= cap), (scorer, d, n, float((err / cap).max()))
        assert out.intact()


def test_score_triples_refusals(hp):
    """ComplEx with an odd slot size, a leading dimension below d: refused, nothing written"""
    n, d = 5, 9
    _, views = triple_operands(n, d, 1)
    out = Guarded(n=n)
    before = out.whole.clone()
    assert score_call(hp, "complex", views, n, d, out) == ERR_INVALID
    for k in range(3):
        lds = [v.stride(0) for v in views]
        lds[k] = d - 1
        assert score_call(hp, "distmult", views, n, d, out, lds) == ERR_INVALID
        assert score_call(hp, "complex", views, n, d - 1, out, [d - 2 if j == k else x for j, x in enumerate(lds)]) == ERR_INVALID
    torch.cuda.synchronize()
    assert same_bits(out.whole, before)
    assert score_call(hp, "distmult", views, n, d, out) == 0


# ---- the contract, once per entry point: two runs give the same bits, n = 0 is accepted and writes nothing ----------------
def test_contract_eager_adagrad(hp):
    for entry, ns in (("step", (262_147,)), ("step2", (262_147, 1025)), ("multi", (1025, 262_147, 3, 64))):
        runs = []
        for _ in range(2):
            segs = [make_seg(n, 130 + k, False) for k, n in enumerate(ns)]
            for zero in ([0] * len(ns), [1] * len(ns)):
                assert launch(hp, entry, segs, 1e-3, zero) == 0
            torch.cuda.synchronize()
            runs.append([(sg.p.v.clone(), sg.s.v.clone()) for sg in segs])
        for (pa, sa), (pb, sb) in zip(*runs):
            assert same_bits(pa, pb) and same_bits(sa, sb), entry
        empty = [make_seg(8, 140 + k, True) for k in range(len(ns))]
        before = [x.whole.clone() for sg in empty for x in (sg.p, sg.g, sg.s)]
        for sg in empty:
            sg.n = 0
        assert launch(hp, entry, empty, 1e-3, [1] * len(ns)) == 0, (entry, "n = 0")
        torch.cuda.synchronize()
        for w, b in zip([x.whole for sg in empty for x in (sg.p, sg.g, sg.s)], before):
            assert same_bits(w, b), (entry, "n = 0 wrote")


def test_contract_map_and_lazy(hp):
    a = map_case(hp, "contract-map-a", 5000, 200, "warm", 1e-3, True)
    b = map_case(hp, "contract-map-b", 5000, 200, "warm", 1e-3, True)
    assert same_bits(a.p.v, b.p.v) and same_bits(a.s.v, b.s.v)
    # (lazy_run seeds its own generator: two runs of one case start from equal inputs)
    first = lazy_run(hp, "contract-lazy-a", [(17, 200, "map"), (9, 1, "dense")], 3, 1e-3, seed=7)
    again = lazy_run(hp, "contract-lazy-b", [(17, 200, "map"), (9, 1, "dense")], 3, 1e-3, seed=7)
    for (pa, sa), (pb, sb) in zip(first, again):
        assert same_bits(pa, pb) and same_bits(sa, sb)
    # rows = 0: accepted, the counter still advances, nothing else is written
    from open_knowledge_graph_embeddings_amd import _native as N
    sg = make_seg(8, 150, True)
    steps, counters = Guarded(torch.zeros(2, dtype=torch.int32)), Guarded(torch.zeros(2, dtype=torch.int32))
    before = [x.whole.clone() for x in (sg.p, sg.g, sg.s, steps)]
    arr = (N.LazyTensor * 1)()
    arr[0].p, arr[0].g, arr[0].state_sum, arr[0].rows, arr[0].row_len, arr[0].row_steps = sg.p.ptr(), sg.g.ptr(), sg.s.ptr(), 0, 4, steps.ptr()
    for mode in (0, 1):
        assert hp.lib.okge_adagrad_lazy(arr, 1, counters.ptr(), 3, mode, LR, 1e-3, EPS, hp._stream()) == 0
    torch.cuda.synchronize()
    for x, b in zip((sg.p, sg.g, sg.s, steps), before):
        assert same_bits(x.whole, b) if x.whole.dtype == torch.float32 else torch.equal(x.whole, b)
    assert counters.np().tolist() == [1, 0] and counters.intact()


def test_contract_clip_scale_merge_metrics_score(hp):
    rng = np.random.default_rng(160)
    h0, h1 = rng.standard_normal(262_147).astype(np.float32), rng.standard_normal(1025).astype(np.float32)
    ws = Guarded(n=8448, dtype=torch.uint8)
    runs = []
    for _ in range(2):
        g0, g1, norm = Guarded(h0), Guarded(h1), Guarded(torch.zeros(1, dtype=torch.float64))
        assert clip_call(hp, g0, g0.n, g1, g1.n, 1.0, norm, ws) == 0
        a = scalar(0.37)
        assert hp.lib.okge_scale_inplace(g0.ptr(), g0.n, a.data_ptr(), hp._stream()) == 0
        assert hp.lib.okge_rescale_gradients(g0.ptr(), g0.n, g1.ptr(), g1.n, a.data_ptr(), 0.5, hp._stream()) == 0
        torch.cuda.synchronize()
        runs.append((g0.v.clone(), g1.v.clone(), norm.v.clone()))
    for x, y in zip(*runs):
        assert same_bits(x, y)
    # n = 0: accepted, the gradients and their guards untouched (the norm of nothing is 0)
    g0, g1, norm, a = Guarded(h1), Guarded(h1), Guarded(torch.full((1,), -1.0, dtype=torch.float64)), scalar(0.37)
    before = [g0.whole.clone(), g1.whole.clone()]
    assert clip_call(hp, g0, 0, g1, 0, 1.0, norm, ws) == 0
    assert hp.lib.okge_scale_inplace(g0.ptr(), 0, a.data_ptr(), hp._stream()) == 0
    assert hp.lib.okge_rescale_gradients(g0.ptr(), 0, g1.ptr(), 0, a.data_ptr(), 0.5, hp._stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(g0.whole, before[0]) and same_bits(g1.whole, before[1]) and float(norm.np()[0]) == 0.0
    # merge, metrics, score: two runs
    x = Guarded((rng.standard_normal((3, 5000)) * 30).astype(np.float32))
    ranks = Guarded(rng.integers(0, 20_000, 100_003).astype(np.int64))
    host, views = triple_operands(257, 516, 2)
    runs = []
    for _ in range(2):
        out, acc, sc = Guarded(n=5000), Guarded(np.zeros(7)), Guarded(n=257)
        assert hp.lib.okge_merge_logsumexp(x.ptr(), 3, 5000, out.ptr(), hp._stream()) == 0
        assert hp.lib.okge_rank_metrics(ranks.ptr(), ranks.n, acc.ptr(), hp._stream()) == 0
        assert score_call(hp, "complex", views, 257, 516, sc) == 0
        torch.cuda.synchronize()
        runs.append((out.v.clone(), acc.v.clone(), sc.v.clone()))
    for p_, q_ in zip(*runs):
        assert same_bits(p_, q_)
    sc = Guarded(n=4)
    before = sc.whole.clone()
    assert score_call(hp, "complex", views, 0, 516, sc) == 0
    torch.cuda.synchronize()
    assert same_bits(sc.whole, before)
