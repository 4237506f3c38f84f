"""dQ = G . C from three bf16 planes per operand (csrc/okge_dq_split.{h,hip}; slot sizes up to 208).

CPU: the arithmetic the kernel is meant to implement, restated in numpy -- x = hi + mid + lo exactly, and the six kept
products against float64 at the S-FB dQ shape stay within the error of one fp32 fma chain per slab.

GPU: okge_train_tiles returns dQ directly.  The truth is formed on the CPU from what the library itself returns and is given:
G is RECOMPUTED from the scores okge_score_queries returns for the same queries, candidates and dropout keys
(BCE: G = (sigmoid(x) - y) / normalizer), in float64 for the truth and in float32 for the restatement; the masked candidate
rows Cm = E[cand] * keep * fp32(1 / (1 - p)) are the library's own fp32 numbers (one exact-in-fp32 multiply by the Philox keep
mask of the oracle).  G . Cm in float64 is the truth, G32 . Cm in float32 (torch CPU matmul) the restatement, and dQ is held
to tests/lstm_reference.band_check at its default factors (per magnitude band: max error <= 3 x, rms error <= 1.6 x the
restatement's, floor 1e-7 max|dQ|).  The worst ratios are printed; those of this kernel and of the fp32-MFMA kernel it
replaced, from the same test, are side by side in profiles/dq_split_ablation.md."""
import numpy as np
import pytest
import torch

from lstm_reference import band_check
from oracle import kge_oracle as ko

SEED = 20240607


# ------------------------------------------------------------------------------------------------ the arithmetic, restated
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r1 = x - hi                                        # fp32 subtractions: exact
    mid = bf16_rne(r1)
    lo = bf16_rne(r1 - mid)
    return hi, mid, lo


def six_products(G, C, chunk=32):
    """The kernel's sum: per 32-candidate step every plane product's K = 32 dot exactly (float64 holds it), the five correction
    products in an accumulator of their own (smallest first) and hi.hi in the main one, each add into an accumulator TRUNCATED
    to fp32 -- the harsher of the two accumulate models; the two accumulators are added once, rounded to nearest."""
    def trunc32(v):
        f = v.astype(np.float32)
        over = np.abs(f.astype(np.float64)) > np.abs(v)
        return np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)
    gh, gm, gl = (p.astype(np.float64) for p in split3(G))
    ch, cm, cl = (p.astype(np.float64) for p in split3(C))
    main = np.zeros((G.shape[0], C.shape[1]), np.float32)
    corr = np.zeros_like(main)
    for k0 in range(0, G.shape[1], chunk):
        s = slice(k0, k0 + chunk)
        for a, b in ((gl, ch), (gh, cl), (gm, cm), (gm, ch), (gh, cm)):
            corr = trunc32(corr.astype(np.float64) + a[:, s] @ b[s])
        main = trunc32(main.astype(np.float64) + gh[:, s] @ ch[s])
    return main + corr


def fp32_chain(G, C):
    """one fp32 fma chain over the candidates (what an fp32 MFMA accumulation amounts to)"""
    acc = np.zeros((G.shape[0], C.shape[1]), np.float64)
    for n in range(G.shape[1]):
        acc = (acc + G[:, n:n + 1].astype(np.float64) * C[n:n + 1].astype(np.float64)).astype(np.float32).astype(np.float64)
    return acc.astype(np.float32)                      # (a double-rounded fma: a float64 product of two fp32 is exact)


def test_plane_split_is_exact():
    """hi + mid + lo == x bit for bit for normal fp32 inputs, +-0 included.  Inputs so small that lo would be subnormal
    (|x| < 2^-126 * 2^16 or so) are left out: bf16 has fp32's exponent range and the last plane would lose bits there."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000).astype(np.float32) * np.float32(10.0) ** rng.integers(-25, 25, 200000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0e38, 2.0 ** -100, 1.3e-7, 255.99998], np.float32)])
    x = x[np.isfinite(x) & ((x == 0) | (np.abs(x) > 2.0 ** -100))]
    hi, mid, lo = split3(x)
    back = (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)
    assert np.array_equal(back.view(np.uint32)[x != 0], x.view(np.uint32)[x != 0])
    assert np.all(back[x == 0] == 0)
    for p in (hi, mid, lo):                            # every plane IS a bf16
        assert np.all(p.view(np.uint32) & 0xFFFF == 0)
    # each plane at most 2^-8 of the one before (what ranks the six products)
    nz = hi != 0
    assert np.all(np.abs(mid[nz]) <= np.abs(hi[nz]) * 2.0 ** -8) and np.all(np.abs(lo[nz]) <= np.abs(hi[nz]) * 2.0 ** -16)


def test_six_products_within_fp32_chain_error():
    """The S-FB dQ of one 64-row block, restated: N = 14541 candidates in 32 slabs, d = 200 (a 40-column slice keeps the
    test short), 40 % dropout-masked candidate rows, BCE G scaled by 1 / (B N).  The six-product sum -- with the harsher,
    truncating accumulate -- is no worse than one fp32 chain per slab, in max and in rms error against float64."""
    rng = np.random.default_rng(1)
    B, N, d, nsplit = 64, 14541, 40, 32
    E = (rng.standard_normal((N, d)) * 0.1).astype(np.float32)
    C = (E * (rng.random((N, d)) >= 0.4) * np.float32(1.0 / (1.0 - 0.4))).astype(np.float32)
    x = rng.standard_normal((B, N)) * 0.5
    y = rng.random((B, N)) < 3e-4
    G = ((1.0 / (1.0 + np.exp(-x)) - y) / (512.0 * N)).astype(np.float32)
    want = G.astype(np.float64) @ C.astype(np.float64)
    tiles = (N + 63) // 64
    six = np.zeros((B, d), np.float32)
    chain = np.zeros((B, d), np.float32)
    for s in range(nsplit):                            # slabs as the kernel cuts them, summed in fp32 like slab_reduce
        lo, hi = 64 * (s * tiles // nsplit), min(N, 64 * ((s + 1) * tiles // nsplit))
        six = six + six_products(G[:, lo:hi], C[lo:hi])
        chain = chain + fp32_chain(G[:, lo:hi], C[lo:hi])
    scale = np.abs(want).max()
    e6, ec = np.abs(six - want), np.abs(chain - want)
    rms = lambda e: float(np.sqrt((e ** 2).mean()) / np.sqrt((want ** 2).mean()))     # noqa: E731
    print(f"six products: max {e6.max() / scale:.2e} rms {rms(e6):.2e}   fp32 chain: max {ec.max() / scale:.2e} rms {rms(ec):.2e}")
    assert e6.max() <= ec.max() and rms(e6) <= rms(ec)


# ------------------------------------------------------------------------------------------------------------------ GPU
def dq_case(hp, d, N, B, p, seed, scorer="complex"):
    """-> (dQ as returned [rows][ld], float64 truth [rows][d], fp32 restatement [rows][d], sum |g| |c| [rows][d])"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    n_ent, n_rel, step = N + 2, 12, 3
    E = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    n_po = B // 2
    n_sp = B - n_po
    dev = hp.device
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    # up to three positives per row, (row, col) sorted by column
    y = np.zeros((B, N), bool)
    for r in range(B):
        y[r, rng.choice(N, size=min(N, int(rng.integers(1, 4))), replace=False)] = True
    col, row = np.nonzero(y.T)
    batch = H.PrefixBatch(po_rel=i32(rng.integers(2, n_rel, n_po)) if n_po else None, po_obj=i32(rng.integers(2, n_ent, n_po)) if n_po else None,
                          sp_subj=i32(rng.integers(2, n_ent, n_sp)), sp_rel=i32(rng.integers(2, n_rel, n_sp)),
                          pos_row=i32(row), pos_col=i32(col), cand_first=2, n_cand=N)
    if p > 0:
        batch.drop_cand = H.DropoutSpec(p, SEED, H.STREAM_CAND, step)
    Et, Rt = torch.from_numpy(E).to(dev), torch.from_numpy(R).to(dev)
    sh = H.Shard(0, n_ent, 0)
    q = hp.encode_queries(Et, Rt, scorer, batch, sh)[0]
    x = hp.score_queries(Et, Rt, scorer, q, B, batch, sh)
    dE = torch.zeros_like(Et)
    dq = torch.full_like(q, 7.0)                       # every element must be written
    norm = float(B) * N
    hp.train_tiles(Et, Rt, scorer, q, batch, sh, dE, dq, N, loss="bce", normalizer=norm, grads_zero=True)
    torch.cuda.synchronize()
    # rows B .. rows - 1 of the query block are zero rows: their scores are 0 and they have no positives
    x = np.concatenate([x.cpu().numpy(), np.zeros((q.shape[0] - B, N), np.float32)])
    y = np.concatenate([y, np.zeros((q.shape[0] - B, N), bool)])
    Cm = E[2:]
    if p > 0:
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))                     # the library's fp32 1 / (1 - p)
        Cm = (Cm * scale) * ko.dropout_keep_mask(SEED, H.STREAM_CAND, step, N, d, p)
    Cm = np.ascontiguousarray(Cm, dtype=np.float32)
    G64 = (1.0 / (1.0 + np.exp(-x.astype(np.float64))) - y) / norm
    inv = np.float32(1.0 / norm)
    sig32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)
    G32 = (sig32 * inv - y.astype(np.float32) * inv).astype(np.float32)
    want = G64 @ Cm.astype(np.float64)
    want32 = (torch.from_numpy(G32) @ torch.from_numpy(Cm)).double().numpy()
    return dq, want, want32, np.abs(G64) @ np.abs(Cm.astype(np.float64))


def check_case(hp, name, d, N, B, p, seed):
    dq, want, want32, bound = dq_case(hp, d, N, B, p, seed)
    got = dq.cpu()
    ratios = band_check(name, got[:B, :d], want[:B], want32[:B])
    print(f"{name}: worst max-error ratio {ratios[0]:.3f}, worst rms ratio {ratios[1]:.3f}")
    # The rest of the returned block, as the fp32 kernel left it (recorded on the parent build by this very check): columns
    # >= d are exact zeros (the masked rows are zero-padded), and the rows B .. rows - 1 are neither zero nor untouched but
    # WRITTEN like any other row -- the tile kernel gives the zero query rows behind the batch their G = sigmoid(0) /
    # normalizer, so they hold that times the column sums of Cm; nobody reads them.  All of them carry the SAME G, so their
    # errors are one error repeated and the band statistics mean nothing there; they are held to the classical bound of an
    # fp32 sum instead: |error| <= n u sum |g| |c| with u = 2^-24 and n = the terms of the sum (candidates + slabs).
    pad = got[B:, :d].double().numpy()
    if pad.size:
        err = np.abs(pad - want[B:])
        print(f"{name}: rows behind the batch {pad.shape}: all zero {bool((pad == 0).all())}, untouched {bool((pad == 7.0).all())}, "
              f"max |got - truth| {err.max():.3e} of max |truth| {np.abs(want[B:]).max():.3e}")
        assert np.all(err <= (N + 64) * 2.0 ** -24 * bound[B:]), name
    assert torch.all(got[:, d:] == 0), name
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_dq_flagship_shape(p, seed, okge_lib):
    """S-FB: ComplEx d = 200, B = 512, N = 14541"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    check_case(H.HotPath("cuda:0"), f"S-FB p={p} seed={seed}", 200, 14541, 512, p, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [8, 64, 72, 128, 136, 200, 208])
def test_dq_edge_shapes(d, okge_lib):
    """every kernel instance (slot sizes 64 / 128 / 208), a partial 32-candidate sub-chunk, a partial 64-row block, and (few
    candidate tiles against many workgroups per row block) workgroups whose chunk range is empty; dropout 0.4"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    worst = [0.0, 0.0]
    for N in (1, 31, 33, 64, 65, 14541):
        for B in (1, 63, 64, 65, 512):
            r = check_case(hp, f"d={d} N={N} B={B}", d, N, B, 0.4, 1000 * d + N + B)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"d={d}: worst max-error ratio {worst[0]:.3f}, worst rms ratio {worst[1]:.3f}")


@pytest.mark.gpu
def test_dq_two_candidate_ranges(okge_lib, monkeypatch):
    """G^T budget of 1 MiB at 512 rows = 8 tiles per range: 1000 candidates run as two ranges, the second one ADDS to the
    slabs of the first (DqArgs.accumulate = 1)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    monkeypatch.setenv("OKGE_GT_MBYTES", "1")
    check_case(H.HotPath("cuda:0"), "two ranges d=200 N=1000 B=512", 200, 1000, 512, 0.4, 77)


@pytest.mark.gpu
def test_dq_bit_reproducible(okge_lib):
    """the same call twice: identical bits (no atomics, fixed summation order)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    for d, N, B in ((200, 14541, 512), (64, 333, 65)):
        a = dq_case(hp, d, N, B, 0.4, 5)[0].clone()
        b = dq_case(hp, d, N, B, 0.4, 5)[0]
        assert torch.equal(a, b), (d, N, B)
