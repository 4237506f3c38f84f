"""The train tile's gradient product dC = G^T . Q (fused_tile64_kernel, csrc/okge_train64.hip; slot sizes up to 208), held against
float64 on the candidate rows of dE -- the one output of okge_train_tiles that tests/test_dq_split.py and tests/test_cm_planes.py
(which hold dQ) leave to the end-to-end fixtures.  Written for moving that product from fp32 MFMA to three bf16 planes per operand
(csrc/okge_tile_grad_split.h, profiles/tile_grad_split.md); it tests outputs only and passes on the fp32 product as well.

CPU: the three-plane phase restated in numpy -- per 64-row chunk each 32-row half is ONE K = 32 step of
v_mfma_f32_16x16x32_bf16 per plane product (its dot exact, float64 holds it), every accumulate TRUNCATED to fp32 (the harsher of
the two accumulate models, as in test_dq_split.six_products), the halves' sums added in fp32 as the tile's write-back does --
in both forms of meeting the main sum: the five corrections chained from zero and folded in per chunk by one fp32 add, or kept
in an accumulator of their own that is added once.

GPU: through HotPath.train_tiles, as test_cm_planes.general_case.  Truth: (G64^T . q) * keep * scale in float64, where q is the
library's own fp32 folded queries, G is recomputed from the scores score_queries returns (float64 for the truth, fp32 for the
restatement) and keep * scale is the oracle's Philox mask times the library's fp32 1 / (1 - p).  Restatement: the fp32 torch
matmul G32^T . q, masked in fp32.  Rule: tests/lstm_reference.band_check at its default factors (per magnitude band: max error
<= 3 x, rms error <= 1.6 x the restatement's).  dE is a dense (rows, d) table: it has no padding columns, so what a tile writes
past column d would land in the next row -- which is either a candidate row held to the truth or a row outside the candidate
range, and those are prefilled with a sentinel and must come back untouched."""
import numpy as np
import pytest
import torch

from lstm_reference import band_check
from oracle import kge_oracle as ko
from test_dq_split import SEED, split3

SENTINEL = 7.0


# ------------------------------------------------------------------------------------------------ the arithmetic, restated
def trunc32(v):
    f = v.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)


def three_plane_phase(G, Q, fold):
    """dC[n][k] = sum_b G[b][n] Q[b][k] as the phase forms it: G [rows][n], Q [rows][k] fp32, rows a multiple of 64"""
    gh, gm, gl = (p.astype(np.float64) for p in split3(G))
    qh, qm, ql = (p.astype(np.float64) for p in split3(Q))
    halves = []
    for h in range(2):
        main = np.zeros((G.shape[1], Q.shape[1]), np.float32)
        corr = np.zeros_like(main)
        for b0 in range(0, G.shape[0], 64):
            s = slice(b0 + 32 * h, b0 + 32 * h + 32)
            t = np.zeros_like(main) if fold else corr
            for a, b in ((gl, qh), (gh, ql), (gm, qm), (gm, qh), (gh, qm)):          # smallest first
                t = trunc32(t.astype(np.float64) + a[s].T @ b[s])
            main = trunc32(main.astype(np.float64) + gh[s].T @ qh[s])
            if fold:
                main = main + t                                                      # one fp32 add (round to nearest)
            else:
                corr = t
        halves.append(main if fold else main + corr)
    return halves[0] + halves[1]


def folded_queries(rng, B, d, p):
    """rows like the library's folded ComplEx queries: products of two dropped-out N(0, 0.1) rows"""
    def rows():
        v = (rng.standard_normal((B, d)) * 0.1).astype(np.float32)
        return v * (rng.random((B, d)) >= p) * np.float32(1.0 / (1.0 - p)) if p > 0 else v
    e, r = rows(), rows()
    h = d // 2
    q = np.empty((B, d), np.float32)
    q[:, :h] = e[:, :h] * r[:, :h] - e[:, h:2 * h] * r[:, h:2 * h]
    q[:, h:2 * h] = e[:, :h] * r[:, h:2 * h] + e[:, h:2 * h] * r[:, :h]
    if d & 1:
        q[:, -1] = e[:, -1] * r[:, -1]
    return q


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "own-accumulator"])
@pytest.mark.parametrize("B,n,d,p", [(512, 192, 200, 0.4), (512, 192, 200, 0.0), (65, 130, 70, 0.4), (1, 33, 8, 0.4), (33, 64, 208, 0.4)])
def test_three_plane_phase_within_fp32_restatement(B, n, d, p, fold):
    rng = np.random.default_rng(1000 * B + n + d)
    q = folded_queries(rng, B, d, p)
    x = rng.standard_normal((B, n)) * 0.5
    y = rng.random((B, n)) < max(3e-4, 1.5 / n)
    G = ((1.0 / (1.0 + np.exp(-x)) - y) / (float(B) * n)).astype(np.float32)
    mask = ((rng.random((n, d)) >= p) * np.float32(1.0 / (1.0 - p))).astype(np.float32) if p > 0 else np.ones((n, d), np.float32)
    rows = (B + 63) // 64 * 64
    Gp = np.zeros((rows, n), np.float32)
    Qp = np.zeros((rows, d), np.float32)
    Gp[:B], Qp[:B] = G, q
    Gp[B:] = np.float32(0.5 / (float(B) * n))          # G is not zero on padding rows; their query rows are
    got = three_plane_phase(Gp, Qp, fold) * mask
    want = (G.astype(np.float64).T @ q.astype(np.float64)) * mask
    want32 = ((torch.from_numpy(G).T @ torch.from_numpy(q)) * torch.from_numpy(mask)).double().numpy()
    ratios = band_check(f"B={B} n={n} d={d} p={p} fold={fold}", got, want, want32)
    print(f"B={B} n={n} d={d} p={p} fold={fold}: worst max-error ratio {ratios[0]:.3f}, worst rms ratio {ratios[1]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ GPU
def engine():
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


def tile_case(hp, d, N, B, p, seed, ids=False, loss="bce", prefill=False):
    """one okge_train_tiles call -> (dE as returned (cpu), truth (float64, whole table), fp32 restatement (whole table),
    candidate rows of the table).  prefill: the candidate rows hold random numbers and the call ADDS to them (grads_zero off);
    rows outside the candidate range hold SENTINEL either way."""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    n_ent, n_rel, step = N + 2 + (300 if ids else 0), 12, 3
    E = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    n_po = B // 2
    n_sp = B - n_po
    dev = hp.device
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    y = np.zeros((B, N), bool)
    for r in range(B):
        y[r, rng.choice(N, size=min(N, int(rng.integers(1, 4))), replace=False)] = True
    col, row = np.nonzero(y.T)
    cand = 2 + rng.permutation(n_ent - 2)[:N] if ids else 2 + np.arange(N)
    batch = H.PrefixBatch(po_rel=i32(rng.integers(2, n_rel, n_po)) if n_po else None, po_obj=i32(rng.integers(2, n_ent, n_po)) if n_po else None,
                          sp_subj=i32(rng.integers(2, n_ent, n_sp)), sp_rel=i32(rng.integers(2, n_rel, n_sp)),
                          pos_row=i32(row), pos_col=i32(col), cand_first=2, n_cand=N, cand_ids=i32(cand) if ids else None)
    if p > 0:
        batch.drop_cand = H.DropoutSpec(p, SEED, H.STREAM_CAND, step)
    Et, Rt = torch.from_numpy(E).to(dev), torch.from_numpy(R).to(dev)
    sh = H.Shard(0, n_ent, 0)
    q = hp.encode_queries(Et, Rt, "complex", batch, sh)[0]
    x = hp.score_queries(Et, Rt, "complex", q, B, batch, sh)
    row_lse = hp.row_logsumexp(Et, Rt, "complex", q, B, batch, sh) if loss == "kl" else None
    start = np.full((n_ent, d), SENTINEL, np.float32)
    start[cand] = (rng.standard_normal((N, d)) * 1e-6).astype(np.float32) if prefill else 0.0
    dE = torch.from_numpy(start).to(dev)
    dq = torch.zeros_like(q)
    norm = float(B) * N
    hp.train_tiles(Et, Rt, "complex", q, batch, sh, dE, dq, N, loss=loss, normalizer=norm, grads_zero=not prefill, row_lse=row_lse)
    torch.cuda.synchronize()
    x = x.cpu().numpy()
    q32 = np.ascontiguousarray(q[:B, :d].cpu().numpy())
    mask = np.ones((N, d), np.float32)
    if p > 0:
        mask = (ko.dropout_keep_mask(SEED, H.STREAM_CAND, step, N, d, p) * (np.float32(1.0) / (np.float32(1.0) - np.float32(p)))).astype(np.float32)
    inv = np.float32(1.0 / norm)
    if loss == "kl":
        G64 = ko.loss_and_dscore(x.astype(np.float64), y.astype(np.float64), ko.LOSS_KL)[1] / norm
        G32 = (ko.loss_and_dscore(x, y.astype(np.float32), ko.LOSS_KL)[1] * inv).astype(np.float32)
    else:
        G64 = (1.0 / (1.0 + np.exp(-x.astype(np.float64))) - y) / norm
        sig32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)
        G32 = (sig32 * inv - y.astype(np.float32) * inv).astype(np.float32)
    want = start.astype(np.float64)
    want[cand] += (G64.T @ q32.astype(np.float64)) * mask
    want32 = torch.from_numpy(start.copy())
    want32[torch.from_numpy(cand)] += (torch.from_numpy(np.ascontiguousarray(G32.T)) @ torch.from_numpy(q32)) * torch.from_numpy(mask)
    return dE.cpu(), want, want32.double().numpy(), cand


def check_tile(hp, name, d, N, B, p, seed, **kw):
    got, want, want32, cand = tile_case(hp, d, N, B, p, seed, **kw)
    ratios = band_check(name, got[cand], want[cand], want32[cand])
    print(f"{name}: worst max-error ratio {ratios[0]:.3f}, worst rms ratio {ratios[1]:.3f}")
    outside = np.ones(got.shape[0], bool)
    outside[cand] = False
    assert torch.all(got[torch.from_numpy(outside)] == SENTINEL), (name, "rows outside the candidate range were written")
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 6, 70, 198, 200, 202, 206, 208])
def test_slot_sizes_and_edges(d, okge_lib):
    """every REGC instance -- KB = 4 (2, 6), KB = 8 (70), KB = 13 with the short last round (198, 200) and without (202, 206,
    208) -- partial octets and the full padded width; candidates: one, a ragged 16-block, a ragged second tile, three tiles;
    batch rows around the 32-row half and the 64-row chunk.  The (N, B) cross thinned to a diagonal pattern that keeps every
    N and every B, shifted with d so that the slot sizes together cover the whole cross."""
    hp = engine()
    Ns, Bs = (1, 33, 65, 130), (1, 31, 33, 63, 65, 130)
    shift = [2, 6, 70, 198, 200, 202, 206, 208].index(d)
    worst = [0.0, 0.0]
    for i, N in enumerate(Ns):
        for j, B in enumerate(Bs):
            if (i + j + shift) % 2:
                continue
            r = check_tile(hp, f"d={d} N={N} B={B}", d, N, B, 0.4, 9000 * d + 10 * N + B)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"d={d}: worst max-error ratio {worst[0]:.3f}, worst rms ratio {worst[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,B", [(200, 333, 65), (64, 65, 64)])
def test_explicit_unique_candidate_ids(d, N, B, okge_lib):
    check_tile(engine(), f"ids d={d} N={N} B={B}", d, N, B, 0.4, 17 * d + N, ids=True)


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,B", [(200, 130, 65), (70, 65, 33)])
def test_adds_to_prefilled_gradient(d, N, B, okge_lib):
    """grads_zero off: the candidate rows come back as prefill + gradient (the prefill at the gradient's own magnitude, so that the
    add does not round the gradient's error away)"""
    check_tile(engine(), f"prefill d={d} N={N} B={B}", d, N, B, 0.4, 23 * d + N, prefill=True)


@pytest.mark.gpu
def test_kl_instance(okge_lib):
    check_tile(engine(), "kl d=200 N=333 B=65", 200, 333, 65, 0.4, 13, loss="kl")
    check_tile(engine(), "kl d=208 N=130 B=130", 208, 130, 130, 0.4, 14, loss="kl")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 200])
def test_tail_split_shape(d, okge_lib):
    """275 tiles, the last one ragged, 256 rows: the tail tiles are launched apart with the batch rows split over blockIdx.y
    (chunks that start at multiples of 64 rows) and their partial gradients go through the slabs"""
    check_tile(engine(), f"tail split d={d}", d, 64 * 274 + 37, 256, 0.3, 31 * d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 200])
def test_workspace_reuse(d, okge_lib):
    """a 130-row call, then a 65-row call, in a workspace first filled with NaN patterns: whatever the longer call left behind
    rows 65 .. 127 of the padded batch (G is not zero there) must not reach dE.  Bit-equal to the same call on a fresh engine."""
    N = 130
    used = engine()
    used.workspace(130, N, d).fill_(0xFF)
    tile_case(used, d, N, 130, 0.4, 5)
    after = tile_case(used, d, N, 65, 0.4, 6)[0].clone()
    first = tile_case(engine(), d, N, 65, 0.4, 6)[0]
    assert torch.isfinite(first).all() and torch.isfinite(after).all()
    assert torch.equal(after, first)


@pytest.mark.gpu
def test_bit_reproducible(okge_lib):
    hp = engine()
    for d, N, B in ((200, 333, 130), (70, 130, 65)):
        a = tile_case(hp, d, N, B, 0.4, 5)[0].clone()
        b = tile_case(hp, d, N, B, 0.4, 5)[0]
        assert torch.equal(a, b), (d, N, B)


@pytest.mark.gpu
def test_flagship_shape(okge_lib):
    """S-FB: ComplEx d = 200, B = 512, N = 14541, dropout 0.4"""
    check_tile(engine(), "S-FB p=0.4", 200, 14541, 512, 0.4, 1)


def step_and_tiles(hp_step, hp_tiles, d, N, B, seed):
    """the same batch through the fused step (okge_train_forward_backward: the launch that folds the queries also writes their
    planes) and through encode_queries + train_tiles (the planes come from the caller's query block) -> the candidate rows of dE of
    both.  The prefix entities lie behind the candidate range, so the step adds nothing but the tile's gradient to those rows."""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    n_ent, n_rel = N + 2 + 40, 12
    dev = hp_step.device
    Et = torch.from_numpy((rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)).to(dev)
    Rt = torch.from_numpy((rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)).to(dev)
    n_po = B // 2
    n_sp = B - n_po
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    y = np.zeros((B, N), bool)
    for r in range(B):
        y[r, rng.choice(N, size=min(N, int(rng.integers(1, 4))), replace=False)] = True
    col, row = np.nonzero(y.T)
    batch = H.PrefixBatch(po_rel=i32(rng.integers(2, n_rel, n_po)), po_obj=i32(rng.integers(N + 2, n_ent, n_po)),
                          sp_subj=i32(rng.integers(N + 2, n_ent, n_sp)), sp_rel=i32(rng.integers(2, n_rel, n_sp)),
                          pos_row=i32(row), pos_col=i32(col), cand_first=2, n_cand=N)
    batch.drop_cand = H.DropoutSpec(0.4, SEED, H.STREAM_CAND, 3)
    dE_step, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
    hp_step.forward_backward(Et, Rt, "complex", batch, dE_step, dR, grads_zero=True)
    sh = H.Shard(0, n_ent, 0)
    q = hp_tiles.encode_queries(Et, Rt, "complex", batch, sh)[0]
    dE_tiles = torch.zeros_like(Et)
    hp_tiles.train_tiles(Et, Rt, "complex", q, batch, sh, dE_tiles, torch.zeros_like(q), N, normalizer=float(B) * N, grads_zero=True)
    torch.cuda.synchronize()
    return dE_step[2:N + 2].cpu(), dE_tiles[2:N + 2].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [70, 200])
def test_step_and_tiles_agree_bit_for_bit(d, okge_lib):
    """every producer of the query planes gives the same bits: a 130-row step, then a 65-row step, on an engine whose workspace
    was first filled with NaN patterns (the rows 65 .. 127 of the padded batch must be rewritten as zero planes by the step's
    own launch), against the tiles path on a fresh engine"""
    N = 130
    used = engine()
    used.workspace(130, N, d).fill_(0xFF)
    step_and_tiles(used, engine(), d, N, 130, 8)
    got, want = step_and_tiles(used, engine(), d, N, 65, 9)
    assert torch.isfinite(got).all() and got.abs().max() > 0
    assert torch.equal(got, want)
