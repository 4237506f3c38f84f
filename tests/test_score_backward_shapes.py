"""The score backward (okge_prefix_score_backward: gemm_f32_kernel<TA>, splitk_reduce_kernel, fold_rows_kernel,
fold_backward_kernel; csrc/okge_gemm.hip) and the row kernels around it (okge_encode_rows, okge_scatter_rows) through
hotpath.HotPath -- and through the C ABI itself where the wrapper hides an argument (workspace and output placement) -- at the
shapes where their branches change, against the restatement of tests/score_backward_reference.py.

GEMM sweep: b over the 16-row chunk edges of the transposed-A contraction and the 64-row tile edges of the other product, n and d
over the tile edges, one shape for every bound on the split count, three full-size shapes; ComplEx sp / po and DistMult.  d_ent,
d_rel and d_cand are held to lstm_reference.band_check at its default factors (per |want| band: max error <= 3 x, rms <= 1.6 x
the yardstick's error against float64, floor 1e-7 max|want|) with the FP32 CHAIN restatement as the yardstick, and every element
of the two products to the hard cap (K + splits) 2^-24 sum |g| |c| (dC against G^T . q with the fp32 q the kernel multiplies;
dQ read back through a DistMult call against all-one relation rows, whose fold backward is the identity).  Every comparison
prints `RATIO <case> <tensor> <max ratio> <rms ratio> | <the same against torch's CPU fp32 matmul>`; the table of one run is
profiles/score_backward_sweep.md.

Then the contract: a single 1.0 in G copies rows bit for bit; NaN behind every leading dimension, behind the last rows and in the
workspace changes nothing; sentinels around the workspace and the outputs survive; every subset of the outputs gives the same
bits; two runs are bit-identical; bad arguments are refused before anything is written.  encode_rows is bit-equal to its
restatement; scatter_rows is bit-equal without dropout and within (run + 1) 2^-24 sum |row mult| of float64 with it."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import score_backward_reference as R
from lstm_reference import _bands, band_check
from oracle import kge_oracle as ko

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 12345.678                                   # no result comes near it
MODES = {"sp": ("complex", True), "po": ("complex", False), "dm": ("distmult", True)}
ERR_INVALID, ERR_WORKSPACE = -1, -3                    # include/okge.h
SEED = 20250711

B_EDGES = (1, 15, 16, 17, 31, 33, 63, 64, 65, 130, 512)
N_EDGES = (1, 3, 15, 16, 17, 63, 64, 65, 257, 1000, 4099, 14541)
D_EDGES = (1, 3, 17, 2, 6, 62, 64, 66, 128, 200, 258, 512)      # 1, 3, 17: DistMult only (ComplEx needs an even slot size)

DESIGNED = [
    # every edge value of b, n and d at least once
    ("dm", 1, 1, 1), ("sp", 1, 3, 2), ("po", 15, 15, 6), ("dm", 16, 16, 3), ("sp", 17, 17, 62), ("po", 31, 63, 64),
    ("dm", 33, 64, 17), ("sp", 63, 65, 66), ("po", 64, 257, 128), ("sp", 65, 1000, 200), ("dm", 130, 1000, 258),
    ("po", 130, 257, 512), ("sp", 512, 65, 64), ("po", 512, 1000, 200), ("dm", 65, 14541, 6), ("sp", 1, 14541, 2),
    # the bounds on the split count (score_backward_reference.split_plan): one split; capped by n / 64 (5, the last one holds
    # one candidate); capped at 64; capped by 1024 / tiles (16); 64 asked, 52 left by the k_per round-up; a short last split
    ("sp", 64, 64, 64), ("po", 16, 257, 16), ("dm", 64, 4096, 64), ("dm", 512, 4099, 512), ("sp", 64, 4099, 64),
    ("po", 63, 1000, 62),
    # full size: the own-loss batch on FB15k-237's entities, the wide DistMult, Tucker3's relation projection (n = d_e^2)
    ("sp", 512, 14541, 200), ("dm", 512, 14541, 512), ("dm", 512, 40000, 30),
]
FULL_SIZE = DESIGNED[-3:]


def _drawn(count=36):
    """seeded draws from the edge lists; the work of a case is capped so that the float64 side stays cheap"""
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < count:
        mode = ("sp", "po", "dm")[int(rng.integers(3))]
        b, n, d = (int(rng.choice(x)) for x in (B_EDGES, N_EDGES, D_EDGES))
        if (mode != "dm" and d % 2) or b * n * d > 3e8 or (mode, b, n, d) in DESIGNED or (mode, b, n, d) in out:
            continue
        out.append((mode, b, n, d))
    return out


CASES = DESIGNED + _drawn()


def case_id(c):
    return "%s-b%d-n%d-d%d" % c


@pytest.fixture(scope="module")
def hp(okge_lib):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


def inputs(b, n, d, seed):
    """G standard normal, ent / rel / cand normal x 0.3, fp32 numpy"""
    rng = np.random.default_rng([SEED, seed, b, n, d])
    f = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)          # noqa: E731
    return rng.standard_normal((b, n)).astype(np.float32), f(b, d), f(b, d), f(n, d)


def cuda(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def guarded(shape, guard=4096):
    """an fp32 (rows, d) tensor of sentinels inside a larger sentinel-filled buffer -> (view, whole buffer, guard)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * guard,), SENTINEL, device="cuda")
    return whole[guard:guard + n].view(*shape), whole, guard


def guards_intact(whole, guard):
    return bool((whole[:guard] == SENTINEL).all()) and bool((whole[whole.numel() - guard:] == SENTINEL).all())


def ws_bytes(hp, b, n, d):
    return int(hp.lib.okge_prefix_score_backward_workspace_bytes(b, n, d))


def raw_call(hp, mode, g, ent, rel, cand, outs, ws, ws_len=None, ws_ptr=None, ld_g=None, b=None, n=None, d=None):
    """okge_prefix_score_backward itself.  g / ent / rel / cand: 2-d cuda tensors (views allowed: their row stride is the
    leading dimension), outs = (d_ent, d_rel, d_cand) contiguous tensors or None, ws: a uint8 tensor.  Returns the status."""
    from open_knowledge_graph_embeddings_amd import _native as N
    scorer, sp = MODES[mode]
    b = g.shape[0] if b is None else b
    n = g.shape[1] if n is None else n
    d = cand.shape[1] if d is None else d
    for x in (g, ent, rel, cand):
        assert x.dtype == torch.float32 and x.stride(1) == 1
    ptr = lambda t: None if t is None else t.data_ptr()                      # noqa: E731
    return int(hp.lib.okge_prefix_score_backward(N.SCORERS[scorer], 1 if sp else 0, g.data_ptr(), g.stride(0) if ld_g is None else ld_g,
                                                 b, n, ent.data_ptr(), ent.stride(0), rel.data_ptr(), rel.stride(0), cand.data_ptr(),
                                                 cand.stride(0), d, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                                 ws.data_ptr() if ws_ptr is None else ws_ptr, ws.numel() if ws_len is None else ws_len,
                                                 hp._stream()))


def nan_workspace(hp, b, n, d):
    """exactly the bytes the library asks for, every float a NaN"""
    return torch.full((ws_bytes(hp, b, n, d),), 0xFF, dtype=torch.uint8, device="cuda")


def run(hp, mode, g, ent, rel, cand, need=(True, True, True)):
    """one call into fresh NaN-filled outputs with a NaN-filled workspace of exactly the asked size -> [d_ent, d_rel, d_cand]"""
    b, n, d = g.shape[0], g.shape[1], cand.shape[1]
    outs = [torch.full(s, NAN, device="cuda") if k else None for s, k in zip(((b, d), (b, d), (n, d)), need)]
    assert raw_call(hp, mode, g, ent, rel, cand, outs, nan_workspace(hp, b, n, d)) == 0
    return outs


def read_dq(hp, g, cand):
    """dQ = G . C as the library forms it: DistMult against all-one relation rows folds backward to d_ent = dq * 1"""
    b, d = g.shape[0], cand.shape[1]
    ones = torch.ones((b, d), device="cuda")
    return run(hp, "dm", g, ones, ones, cand, need=(True, False, False))[0]


def band_ratios(got, want, want32, min_band=64):
    """band_check's record (worst max-error ratio, worst rms ratio over the |want| bands) without its assertions"""
    x, want, want32 = np.asarray(got, np.float64).reshape(-1), np.asarray(want).reshape(-1), np.asarray(want32).reshape(-1)
    err, err32, mag = np.abs(x - want), np.abs(want32 - want), np.abs(want)
    floor = 1e-7 * max(mag.max(), 1e-30)
    worst = [0.0, 0.0]
    for lo_, hi_ in _bands(mag, min_band):
        band = (mag >= lo_) & (mag <= hi_)
        if band.any():
            worst[0] = max(worst[0], err[band].max() / max(err32[band].max(), floor))
            worst[1] = max(worst[1], np.sqrt((err[band] ** 2).mean()) / max(np.sqrt((err32[band] ** 2).mean()), floor))
    return tuple(worst)


# ---- the GEMM sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sweep_against_float64(hp, case):
    mode, b, n, d = case
    name = case_id(case)
    scorer, sp = MODES[mode]
    G, ent, rel, cand = inputs(b, n, d, 1)
    g_, e_, r_, c_ = cuda(G, ent, rel, cand)
    got = [x.cpu().numpy() for x in hp.prefix_score_backward(scorer, sp, g_, e_, r_, c_)]
    dq = read_dq(hp, g_, c_).cpu().numpy()
    want = R.score_backward(scorer, sp, G, ent, rel, cand, np.float64)
    yard = R.score_backward(scorer, sp, G, ent, rel, cand, np.float32)
    mm = R.score_backward(scorer, sp, G, ent, rel, cand, np.float32, matmul=R.torch_matmul32)
    splits, k_per = R.split_plan(b, n, d)
    failures = []
    for x, key in zip(got, ("d_ent", "d_rel", "d_cand")):
        rm = band_ratios(x, want[key], mm[key])
        rc = band_ratios(x, want[key], yard[key])
        print("RATIO %s splits=%d %s %.3f %.3f | %.3f %.3f" % (name, splits, key, rc[0], rc[1], rm[0], rm[1]))
        try:
            band_check("%s %s" % (name, key), x, want[key], yard[key])
        except AssertionError as e:                      # (every tensor's figures are printed before the case fails)
            failures.append(str(e))
    # the hard cap on every element of the two products
    q32 = yard["q"]
    err_c = np.abs(got[2].astype(np.float64) - R.product_dc(G, q32))
    cap_c = (b + 1) * R.U * R.abs_product_dc(G, q32)
    err_q = np.abs(dq.astype(np.float64) - want["dq"])
    cap_q = (n + splits) * R.U * R.abs_product_dq(G, cand)
    print("CAP %s dC %.3f dQ %.3f of the cap (largest error / cap over the elements)"
          % (name, float((err_c / np.maximum(cap_c, 1e-300)).max()), float((err_q / np.maximum(cap_q, 1e-300)).max())))
    assert np.isfinite(dq).all() and np.all(err_c <= cap_c) and np.all(err_q <= cap_q), (name, "hard cap", splits, k_per)
    assert not failures, (name, failures)


# ---- exact identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sp", "po", "dm"])
@pytest.mark.parametrize("b,n,d", [(66, 4099, 64), (66, 64, 64)], ids=["52-splits", "1-split"])
def test_unit_gradient_copies_rows(hp, mode, b, n, d):
    """G = a single 1.0 at (b0, n0): dC[n0] is the fp32 fold row q[b0], dQ[b0] is C[n0], bit for bit; every other row is 0"""
    scorer, sp = MODES[mode]
    _, ent, rel, cand = inputs(b, n, d, 2)
    q32 = R.fold(scorer, sp, ent, rel, np.float32)
    assert (q32 != 0).all() and (cand != 0).all()
    splits, k_per = R.split_plan(b, n, d)
    assert splits == (52 if n == 4099 else 1)
    e_, r_, c_ = cuda(ent, rel, cand)
    b0s = sorted({0, 15, 16, 63, 64, b - 1})
    n0s = sorted({x for x in (0, 63, 64, k_per - 1, k_per, n - 1) if x < n})
    for b0, n0 in itertools.product(b0s, n0s):
        g_ = torch.zeros((b, n), device="cuda")
        g_[b0, n0] = 1.0
        dc = run(hp, mode, g_, e_, r_, c_, need=(False, False, True))[2].cpu().numpy()
        dq = read_dq(hp, g_, c_).cpu().numpy()
        where = (mode, b, n, d, "b0", b0, "n0", n0)
        assert np.array_equal(dc[n0].view(np.uint32), q32[b0].view(np.uint32)), where
        assert np.array_equal(dq[b0].view(np.uint32), cand[n0].view(np.uint32)), where
        dc[n0] = 0
        dq[b0] = 0
        assert not dc.any() and not dq.any(), where


# ---- guards -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 3, 16])
@pytest.mark.parametrize("mode,b,n,d", [("sp", 65, 333, 64), ("dm", 17, 65, 17), ("po", 130, 257, 66), ("dm", 33, 1000, 30)])
def test_nan_behind_every_edge(hp, mode, b, n, d, pad):
    """G, ent, rel and cand as column slices of buffers `pad` columns wider and 16 rows longer, NaN everywhere outside the
    slice, and a NaN-filled workspace: finite results, bit-equal to the call on contiguous copies"""
    G, ent, rel, cand = inputs(b, n, d, 3)
    views = []
    for x in (G, ent, rel, cand):
        buf = torch.full((x.shape[0] + 16, x.shape[1] + pad), NAN, device="cuda")
        buf[:x.shape[0], :x.shape[1]] = torch.from_numpy(x).cuda()
        views.append(buf[:x.shape[0], :x.shape[1]])
        assert views[-1].stride(0) == x.shape[1] + pad
    plain = run(hp, mode, *cuda(G, ent, rel, cand))
    got = run(hp, mode, *views)
    for x, y, key in zip(got, plain, ("d_ent", "d_rel", "d_cand")):
        assert bool(torch.isfinite(y).all()), (mode, b, n, d, pad, key, "contiguous call")
        assert bool(torch.isfinite(x).all()), (mode, b, n, d, pad, key)
        assert torch.equal(x, y), (mode, b, n, d, pad, key)
    # and the wrapper's zero-initialised-or-not workspace makes no difference either
    scorer, sp = MODES[mode]
    for x, y, key in zip(hp.prefix_score_backward(scorer, sp, *views), plain, ("d_ent", "d_rel", "d_cand")):
        assert torch.equal(x, y), (mode, b, n, d, pad, key, "wrapper")


@pytest.mark.parametrize("case", [("dm", 64, 4096, 64)] + FULL_SIZE, ids=case_id)
def test_stays_inside_workspace_and_outputs(hp, case):
    """the workspace exactly okge_prefix_score_backward_workspace_bytes long at a 16-byte-aligned offset of a larger buffer, every
    output inside a larger buffer: the bytes on both sides survive, and the results are those of the plain call"""
    mode, b, n, d = case
    G, ent, rel, cand = inputs(b, n, d, 4)
    g_, e_, r_, c_ = cuda(G, ent, rel, cand)
    need, guard, off = ws_bytes(hp, b, n, d), 1 << 16, 48
    assert need >= 4 * R.workspace_floats(b, d)
    big = torch.full((off + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = big[off:off + need]
    assert ws.data_ptr() % 16 == 0
    outs, wholes = [], []
    for shape in ((b, d), (b, d), (n, d)):
        v, whole, gd = guarded(shape)
        outs.append(v)
        wholes.append((whole, gd))
    assert raw_call(hp, mode, g_, e_, r_, c_, outs, ws) == 0
    torch.cuda.synchronize()
    assert bool((big[:off] == 0xA5).all()) and bool((big[off + need:] == 0xA5).all()), (case, "workspace overrun")
    for (whole, gd), key in zip(wholes, ("d_ent", "d_rel", "d_cand")):
        assert guards_intact(whole, gd), (case, key, "output overrun")
    for x, y, key in zip(outs, run(hp, mode, g_, e_, r_, c_), ("d_ent", "d_rel", "d_cand")):
        assert torch.equal(x, y), (case, key)


@pytest.mark.parametrize("mode,b,n,d", [("sp", 9, 40, 16), ("po", 65, 333, 64)])
def test_output_subsets(hp, mode, b, n, d):
    """each of the seven non-empty choices of (d_ent, d_rel, d_cand): the bits of the all-three call, and a buffer that was
    not asked for keeps its sentinels"""
    g_, e_, r_, c_ = cuda(*inputs(b, n, d, 5))
    full = run(hp, mode, g_, e_, r_, c_)
    for need in itertools.product((False, True), repeat=3):
        if not any(need):
            continue
        bufs = [torch.full(s, SENTINEL, device="cuda") for s in ((b, d), (b, d), (n, d))]
        outs = [x if k else None for x, k in zip(bufs, need)]
        assert raw_call(hp, mode, g_, e_, r_, c_, outs, nan_workspace(hp, b, n, d)) == 0
        for x, y, k, key in zip(bufs, full, need, ("d_ent", "d_rel", "d_cand")):
            if k:
                assert torch.equal(x, y), (mode, b, n, d, need, key)
            else:
                assert bool((x == SENTINEL).all()), (mode, b, n, d, need, key, "written without being asked for")
        got = hp.prefix_score_backward(MODES[mode][0], MODES[mode][1], g_, e_, r_, c_, *need)
        for x, y, k, key in zip(got, full, need, ("d_ent", "d_rel", "d_cand")):
            assert (x is None) == (not k) and (x is None or torch.equal(x, y)), (mode, b, n, d, need, key, "wrapper")


@pytest.mark.parametrize("mode,b,n,d", [("sp", 512, 14541, 200), ("po", 65, 333, 64)])
def test_bit_reproducible(hp, mode, b, n, d):
    """the same call twice: identical bits (no atomics, the slabs are added in split order)"""
    g_, e_, r_, c_ = cuda(*inputs(b, n, d, 6))
    first = run(hp, mode, g_, e_, r_, c_)
    for x, y, key in zip(run(hp, mode, g_, e_, r_, c_), first, ("d_ent", "d_rel", "d_cand")):
        assert torch.equal(x, y), (mode, b, n, d, key)


def test_refusals_write_nothing(hp):
    """a workspace one byte short, an unaligned workspace, ld_g < n, an odd slot size with ComplEx: the documented status, and
    the outputs keep their sentinels"""
    b, n, d = 33, 130, 32
    g_, e_, r_, c_ = cuda(*inputs(b, n, d, 7))
    need = ws_bytes(hp, b, n, d)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0

    def refused(status, what, **kw):
        outs = [torch.full(s, SENTINEL, device="cuda") for s in ((b, d), (b, d), (n, d))]
        rc = raw_call(hp, kw.pop("mode", "sp"), g_, e_, r_, c_, outs, ws, **kw)
        torch.cuda.synchronize()
        assert rc == status, (what, rc, hp.lib.okge_last_error())
        for x, key in zip(outs, ("d_ent", "d_rel", "d_cand")):
            assert bool((x == SENTINEL).all()), (what, key)
    refused(ERR_WORKSPACE, "workspace one byte short", ws_len=need - 1)
    refused(ERR_WORKSPACE, "unaligned workspace", ws_ptr=ws.data_ptr() + 4, ws_len=need)
    refused(ERR_INVALID, "ld_g < n", ld_g=n - 1)
    refused(ERR_INVALID, "odd d with ComplEx", d=d - 1, mode="po")
    refused(ERR_INVALID, "odd d with ComplEx", d=d - 1, mode="sp")
    assert raw_call(hp, "dm", g_, e_, r_, c_, [torch.empty((b, d - 1), device="cuda"), None, None], ws, d=d - 1) == 0   # DistMult may
    assert raw_call(hp, "sp", g_, e_, r_, c_, [torch.empty((b, d), device="cuda"), None, None], ws, ws_len=need) == 0


# ---- encode_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 1000])
@pytest.mark.parametrize("d", [1, 7, 8, 9, 127, 128, 129, 512])
def test_encode_rows_bit_equal(hp, d, n):
    """id lists with repeats and id 0, and a row range with first_id > 0; no dropout, Philox masks (the oracle's
    dropout_keep_mask) and explicit keep masks; into a buffer 5 columns wider whose padding must stay as it was"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng([SEED, 8, d, n])
    rows = 1500
    table = rng.standard_normal((rows, d)).astype(np.float32)
    t_ = cuda(table)[0]
    ids = rng.integers(0, rows, n)
    if n > 2:
        ids[rng.integers(0, n, n // 10)] = 0
        ids[n // 2:n // 2 + n // 4] = ids[n // 2]
    if n > 1:
        ids[1] = ids[0]
    first = 7
    for p, explicit, use_ids in itertools.product((0.0, 0.3), (False, True), (True, False)):
        where = ("d", d, "n", n, "p", p, "explicit keep" if explicit else "philox", "ids" if use_ids else "range")
        step = 3 + n
        if explicit:
            keep = rng.random((n, d)) >= 0.4
            spec = H.DropoutSpec(p, keep=torch.from_numpy(keep.astype(np.uint8)).cuda())
        else:
            keep = ko.dropout_keep_mask(SEED, H.STREAM_CAND, step, n, d, p)
            spec = H.DropoutSpec(p, SEED, H.STREAM_CAND, step)
        mult = R.drop_mult(keep, p) if p > 0 else None
        want = R.encode_rows(table, ids if use_ids else None, first, n, mult)
        buf = torch.full((n, d + 5), SENTINEL, device="cuda")
        got = hp.encode_rows(t_, torch.from_numpy(ids.astype(np.int32)).cuda() if use_ids else None, first, n, spec, out=buf[:, :d])
        assert got.stride(0) == d + 5
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), where
        assert bool((buf[:, d:] == SENTINEL).all()), where + ("padding written",)
        plain = hp.encode_rows(t_, torch.from_numpy(ids.astype(np.int32)).cuda() if use_ids else None, first, n, spec)
        assert torch.equal(plain, got), where + ("contiguous output",)
        if p > 0:
            assert bool((got == 0).any()) == bool((~keep).any()), where


# ---- scatter_rows -----------------------------------------------------------------------------------------------------
def id_lists(rng, rows):
    zipf = np.minimum(rng.zipf(1.3, 8000), rows - 1)
    with0 = rng.integers(0, 40, 700)
    with0[::9] = 0
    return {
        "distinct": rng.permutation(np.arange(1, rows))[:400],
        "same": np.full(3000, 7),
        "zipf": zipf,                                   # runs of thousands of positions next to runs of one
        "with0": with0,
        "range": None,                                  # ids == NULL: position i names row first_id + i
    }


@pytest.mark.parametrize("d", [1, 127, 128, 129, 512])
def test_scatter_rows(hp, d):
    """without dropout bit-equal to the fp32 sorted-order restatement, added to a table that already holds numbers; with dropout
    (Philox and explicit masks, into a zero table: the cap has no term for what the table held) every element within
    (run + 1) 2^-24 sum |row mult| of float64 -- the multiply-add may contract; rows come from a buffer 3 columns wider with
    NaN padding; id 0's row stays as it was; two runs give the same bits"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng([SEED, 9, d])
    rows_n, first = 600, 5
    base = rng.standard_normal((rows_n, d)).astype(np.float32)
    for name, ids in id_lists(rng, rows_n).items():
        n = 300 if ids is None else len(ids)
        g = rng.standard_normal((n, d)).astype(np.float32)
        buf = torch.full((n, d + 3), NAN, device="cuda")
        buf[:, :d] = torch.from_numpy(g).cuda()
        ids_ = None if ids is None else torch.from_numpy(ids.astype(np.int32)).cuda()
        where = ("d", d, name, "n", n)
        # no dropout: the call ADDS, bit for bit
        want, _, run_len = R.scatter_rows(g, ids, first, base)
        got = hp.scatter_rows(buf[:, :d], ids_, first, torch.from_numpy(base).cuda())
        again = hp.scatter_rows(buf[:, :d], ids_, first, torch.from_numpy(base).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), where
        assert torch.equal(got, again), where + ("second run",)
        assert np.array_equal(got[0].cpu().numpy(), base[0]), where + ("row 0",)
        if name == "same":
            assert run_len[7] == 3000
        if name == "zipf":
            assert run_len.max() > 1000 and (run_len == 1).sum() > 10
        # dropout: float64 within the cap
        for explicit in (False, True):
            p, step = 0.3, 11
            if explicit:
                keep = rng.random((n, d)) >= 0.5
                spec = H.DropoutSpec(p, keep=torch.from_numpy(keep.astype(np.uint8)).cuda())
            else:
                keep = ko.dropout_keep_mask(SEED, H.STREAM_PO_ENT, step, n, d, p)
                spec = H.DropoutSpec(p, SEED, H.STREAM_PO_ENT, step)
            mult = R.drop_mult(keep, p)
            want64, mag, run_len = R.scatter_rows(g, ids, first, np.zeros((rows_n, d)), mult.astype(np.float64), np.float64)
            got = hp.scatter_rows(buf[:, :d], ids_, first, torch.zeros((rows_n, d), device="cuda"), spec)
            again = hp.scatter_rows(buf[:, :d], ids_, first, torch.zeros((rows_n, d), device="cuda"), spec)
            err = np.abs(got.cpu().double().numpy() - want64)
            cap = (run_len[:, None] + 1) * R.U * mag
            w = where + ("explicit keep" if explicit else "philox",)
            assert bool(torch.isfinite(got).all()) and np.all(err <= cap), w + (float(err.max()),)
            assert bool((got[0] == 0).all()), w + ("row 0",)
            assert torch.equal(got, again), w + ("second run",)
            # a dropped element contributes nothing: rows named once are row * mult exactly
            once = np.flatnonzero(run_len == 1)
            if once.size and ids is not None:
                pos = {int(i): j for j, i in enumerate(ids)}
                for i in once[:50]:
                    assert np.array_equal(got[int(i)].cpu().numpy(), g[pos[int(i)]] * mult[pos[int(i)]]), w + ("row", int(i))


def test_scatter_rows_empty_and_single(hp):
    """n = 0 leaves the table alone; n = 1 needs no `order`"""
    from open_knowledge_graph_embeddings_amd import _native as N
    rng = np.random.default_rng([SEED, 10])
    d, rows_n = 9, 20
    base = rng.standard_normal((rows_n, d)).astype(np.float32)
    g = rng.standard_normal((4, d)).astype(np.float32)
    g_ = cuda(g)[0]
    t = torch.from_numpy(base).cuda()
    hp.scatter_rows(g_[:0], torch.zeros(0, dtype=torch.int32, device="cuda"), 0, t)
    hp.scatter_rows(g_[:0], None, 3, t)
    assert np.array_equal(t.cpu().numpy(), base)
    for the_id in (13, 0):
        ids = torch.tensor([the_id], dtype=torch.int32, device="cuda")
        t = torch.from_numpy(base).cuda()
        none = N.Dropout()
        rc = hp.lib.okge_scatter_rows(g_.data_ptr(), g_.stride(0), ids.data_ptr(), None, 0, 1, d, ctypes.byref(none), t.data_ptr(), rows_n,
                                      hp._stream())
        assert rc == 0, hp.lib.okge_last_error()
        want = R.scatter_rows(g[:1], np.array([the_id]), 0, base)[0]
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32)), the_id
    # two positions with ids but no order: refused, nothing written
    ids = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    t = torch.from_numpy(base).cuda()
    assert hp.lib.okge_scatter_rows(g_.data_ptr(), g_.stride(0), ids.data_ptr(), None, 0, 2, d, None, t.data_ptr(), rows_n, hp._stream()) == ERR_INVALID
    assert np.array_equal(t.cpu().numpy(), base)
