"""The KB = 13 train tile's score product X = Q . C^T on the bf16 matrix cores (TileScoreSplit, csrc/okge_tile_grad_split.h;
fused_tile64_kernel<13, ., .>, csrc/okge_train64.hip; slot sizes 193 .. 208): three bf16 planes per operand, the query operand
read TRANSPOSED (ds_read_b64_tr_b16) from the plane image the gradient phase reads by cells.  Record: profiles/tile_score_split.md.

CPU.  (1) The phase restated in numpy: per K step the six plane products, each step's dot exact (float64 holds it), every
accumulate TRUNCATED to fp32 (the harsher of the two accumulate models, as test_tile_grad_split), hi.hi in the main chain, the
five corrections smallest first in a chain of their own through all steps, one fp32 add at the end -- held against float64 by
band_check with the fp32 torch matmul as the restatement.  (2) The address map: the image is built as write_query_row_planes
builds it, with the 16-bit payload (batch row, column) in place of a bf16, and every transposed read of a chunk is replayed
lane by lane: lane i of a group must receive batch row 32h + 16rg + i at the columns col() names, every (row, column) exactly
once per K step, every address a multiple of 8 inside the chunk, and no two lanes of a 32-lane half on one bank ((byte / 4) % 64).
The gradient phase's cell read is replayed on the same image.

GPU: through HotPath.train_tiles and the fused step.  Truth: float64 throughout from the library's own fp32 folded queries and
the masked candidate rows -- scores, loss, G, dQ = G . C, dE rows = G^T . Q (masked).  Restatement: the same chain in fp32 (torch
matmuls, fp32 loss terms).  The KL loss's row log-sum-exp is an INPUT of the call (the library's fp32 tensor, from another
kernel), so truth and restatement both take that tensor, as they take the two smoothed BCE targets.  Rule:
tests/lstm_reference.band_check at its default factors for dQ and for the candidate rows of dE; for the loss, one number, the
same rule written out (check_case).  Every case runs twice on one engine and must give identical bits for the loss, dQ, the
candidate rows and the whole workspace (G^T, the loss partials, both plane regions, the dQ slabs).  Odd slot sizes run DistMult:
ComplEx folds pairs of columns and takes even sizes only, and the tile kernel sees a query block either way."""
import os

import numpy as np
import pytest
import torch

from lstm_reference import band_check
from oracle import kge_oracle as ko
from test_dq_split import SEED, split3
from test_tile_grad_split import folded_queries, trunc32

KB, D16 = 13, 208
STEPS = KB // 2
PLANE_CELLS, HALF_CELLS, CHUNK_CELLS = 4 * D16, 12 * D16, 24 * D16


# ------------------------------------------------------------------------------------------------ the layout, restated
def plane_slot(k):
    return 16 * (4 * (k >> 6) + (k & 3)) + ((k & 63) >> 2) if k < 64 * (KB // 4) else k


def plane_pos(slot, s, swizzled=True):
    return slot ^ ((s >> 1) << 3) if swizzled else slot


def plane_elem(rg, i, s, swizzled=True):
    return 4 * (rg ^ (s & 1)) + i if swizzled else 4 * rg + i


def col(t, g, e):
    if t < STEPS:
        return 32 * t + 16 * (g & 1) + 4 * (e & 3) + 2 * (g >> 1) + (e >> 2)
    return 32 * STEPS + 8 * (g >> 1) + 4 * (g & 1) + (e & 3)


def a_offset(h, lane, t, j, pl, rg, swizzled=True):
    p, q, g = lane & 3, (lane >> 2) & 3, lane >> 4
    cell = h * HALF_CELLS + pl * PLANE_CELLS + p * D16 + plane_pos(plane_slot(col(t, g, 4 * j + q)), p, swizzled)
    return 16 * cell + 8 * ((rg ^ (p & 1)) if swizzled else rg)


def payload_image(swizzled=True):
    """one chunk's image as 16-bit words, element = 256 * row + column + 1 (0: never written); the three planes alike"""
    img = np.zeros(CHUNK_CELLS * 8, np.uint16)
    for r in range(64):
        h, s = r >> 5, (r >> 2) & 3
        e = plane_elem((r >> 4) & 1, r & 3, s, swizzled)
        for k in range(D16):
            for pl in range(3):
                cell = h * HALF_CELLS + pl * PLANE_CELLS + s * D16 + plane_pos(plane_slot(k), s, swizzled)
                assert img[8 * cell + e] == 0
                img[8 * cell + e] = 256 * r + k + 1
    assert (img != 0).all()
    return img


def reads_of_a_chunk():
    for h in range(2):
        for t in range(STEPS + 1):
            for j in range(2 if t < STEPS else 1):
                for pl in range(3):
                    for rg in range(2):
                        yield h, t, j, pl, rg


def worst_bank_conflict(swizzled):
    worst = 0
    for h, t, j, pl, rg in reads_of_a_chunk():
        for half in range(2):
            banks = {}
            for lane in range(32 * half, 32 * half + 32):
                off = a_offset(h, lane, t, j, pl, rg, swizzled)
                for b in ((off // 4) % 64, (off // 4 + 1) % 64):
                    banks[b] = banks.get(b, 0) + 1
            worst = max(worst, max(banks.values()))
    return worst


def test_transposed_read_map_delivers_every_row_and_column_once():
    img = payload_image()
    for h in range(2):
        for pl in range(3):
            for rg in range(2):
                for t in range(STEPS + 1):
                    seen = set()
                    for j in range(2 if t < STEPS else 1):
                        offs = [a_offset(h, lane, t, j, pl, rg) for lane in range(64)]
                        assert all(o % 8 == 0 and 0 <= o and o + 8 <= 16 * CHUNK_CELLS for o in offs)
                        for g in range(4):
                            for i in range(16):                       # lane i of the group: element i % 4 of the pieces of lanes 4q + i / 4
                                for q in range(4):
                                    word = img[offs[16 * g + 4 * q + (i >> 2)] // 2 + (i & 3)]
                                    row, k = (int(word) - 1) >> 8, (int(word) - 1) & 255
                                    assert row == 32 * h + 16 * rg + i, (h, pl, rg, t, j, g, i, q, row)
                                    assert k == col(t, g, 4 * j + q), (h, pl, rg, t, j, g, i, q, k)
                                    seen.add((row, k))
                    lo, n = (32 * t, 32) if t < STEPS else (32 * STEPS, 16)
                    assert seen == {(32 * h + 16 * rg + i, k) for i in range(16) for k in range(lo, lo + n)}


def test_transposed_reads_are_bank_conflict_free():
    assert worst_bank_conflict(swizzled=True) == 1
    unswizzled = worst_bank_conflict(swizzled=False)
    print(f"worst lanes per bank in a 32-lane half: swizzled image 1, unswizzled image {unswizzled}")
    assert unswizzled == 4             # the four cell rows of a column on one bank pair: what the two swizzles are for


def test_gradient_phase_cell_read_on_the_same_image():
    """lane (c, s) of wave (., h) reads position (16 kb + c) ^ 8 (s / 2) of cell row s: element query_plane_elem(rg, i, s) must be
    batch row 32h + 16rg + 4s + i of the column in slot 16 kb + c, and the 16 cells of a lane group (two s of one pair) distinct"""
    img = payload_image()
    for h in range(2):
        for s in range(4):
            for kb in range(KB):
                for c in range(16):
                    cell = h * HALF_CELLS + s * D16 + plane_pos(16 * kb + c, s)
                    for rg in range(2):
                        for i in range(4):
                            word = int(img[8 * cell + plane_elem(rg, i, s)]) - 1
                            assert word >> 8 == 32 * h + 16 * rg + 4 * s + i
                            assert plane_slot(word & 255) == 16 * kb + c
    for s in (0, 2):
        group = [plane_pos(c, s) % 16 for c in (0, 1, 2, 3, 12, 13, 14, 15)] + [plane_pos(c, s + 1) % 16 for c in range(4, 12)]
        assert sorted(group) == list(range(16))


# ------------------------------------------------------------------------------------------------ the arithmetic, restated
def score_phase(Q, C):
    """X[b][n] = sum_k Q[b][k] C[n][k] as the phase forms it: fp32 Q [rows][208], C [n][208] (zeros past d)"""
    qh, qm, ql = (p.astype(np.float64) for p in split3(Q))
    ch, cm, cl = (p.astype(np.float64) for p in split3(C))
    main = np.zeros((Q.shape[0], C.shape[0]), np.float32)
    corr = np.zeros_like(main)
    for t in range(STEPS + 1):
        k = slice(32 * t, min(32 * t + 32, D16))
        for a, b in ((ql, ch), (qh, cl), (qm, cm), (qm, ch), (qh, cm)):              # smallest first
            corr = trunc32(corr.astype(np.float64) + a[:, k] @ b[:, k].T)
        main = trunc32(main.astype(np.float64) + qh[:, k] @ ch[:, k].T)
    return main + corr


@pytest.mark.parametrize("d", [193, 200, 208])
@pytest.mark.parametrize("p", [0.0, 0.4])
def test_score_phase_within_fp32_restatement(d, p):
    rng = np.random.default_rng(7 * d + int(10 * p))
    B, n = 130, 96
    q = folded_queries(rng, B, d, p)
    c = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    if p > 0:
        c = c * ((rng.random((n, d)) >= p) * np.float32(1.0 / (1.0 - p))).astype(np.float32)
    Qp, Cp = np.zeros((B, D16), np.float32), np.zeros((n, D16), np.float32)
    Qp[:, :d], Cp[:, :d] = q, c
    got = score_phase(Qp, Cp)
    want = q.astype(np.float64) @ c.astype(np.float64).T
    want32 = (torch.from_numpy(q) @ torch.from_numpy(c).T).double().numpy()
    ratios = band_check(f"score d={d} p={p}", got, want, want32)
    print(f"score d={d} p={p}: worst max-error ratio {ratios[0]:.3f}, worst rms ratio {ratios[1]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ GPU
def engine():
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


class forced_env:
    """the launch planner reads its overrides per call"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def labels(rng, B, N, many=False):
    y = np.zeros((B, N), bool)
    for r in range(B):
        y[r, rng.choice(N, size=min(N, int(rng.integers(1, 4))), replace=False)] = True
    if many:                                            # 300 positives in the first tile: past the tile's cache of them
        y[:100, :3] = True
    return y


def tiles_case(hp, d, N, B, p, seed, loss="bce", smoothing=0.0, repeats=False, many=False, loss_only=False, b_split="1"):
    """one okge_train_tiles call, made three times -> dict of what it returned (loss, dq [B][d], dE rows of the table; "again": the
    same of the third call; the workspace bytes after the second and the third) and of the float64 truth and the fp32
    restatement of each.  The workspace is compared between the second and third call: the first call of a shape may have
    allocated it, and byte ranges that no kernel of the call writes (the workspace's own query block among them, when the
    caller supplies the queries) were seen to change between the first and the second call on a fresh allocation.  b_split "1":
    one workgroup per tile sweeps all chunks; "2": two workgroups per tile, half the chunks each; None: the planner's own."""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    scorer = "distmult" if d & 1 else "complex"         # ComplEx folds pairs of columns; the tile kernel sees a query block either way
    n_ent, n_rel, step = N + 2 + (40 if repeats else 0), 12, 3
    E = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    n_po = B // 2
    n_sp = B - n_po
    dev = hp.device
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    y = labels(rng, B, N, many)
    colp, rowp = np.nonzero(y.T)
    cand = 2 + rng.integers(0, n_ent - 2, N) if repeats else 2 + np.arange(N)
    batch = H.PrefixBatch(po_rel=i32(rng.integers(2, n_rel, n_po)) if n_po else None, po_obj=i32(rng.integers(2, n_ent, n_po)) if n_po else None,
                          sp_subj=i32(rng.integers(2, n_ent, n_sp)), sp_rel=i32(rng.integers(2, n_rel, n_sp)),
                          pos_row=i32(rowp), pos_col=i32(colp), cand_first=2, n_cand=N, cand_ids=i32(cand) if repeats else None)
    if p > 0:
        batch.drop_cand = H.DropoutSpec(p, SEED, H.STREAM_CAND, step)
    Et, Rt = torch.from_numpy(E).to(dev), torch.from_numpy(R).to(dev)
    sh = H.Shard(0, n_ent, 0)
    q = hp.encode_queries(Et, Rt, scorer, batch, sh)[0]
    row_lse = hp.row_logsumexp(Et, Rt, scorer, q, B, batch, sh) if loss == "kl" else None
    norm = float(B) * N
    runs = []
    for _ in range(3):
        dE = torch.zeros_like(Et)
        dq = torch.full_like(q, 7.0)
        with forced_env(OKGE_B_SPLIT=b_split):
            loss_out = hp.train_tiles(Et, Rt, scorer, q, batch, sh, dE, dq, N, loss=loss, label_smoothing=smoothing, normalizer=norm,
                                      grads_zero=not repeats, row_lse=row_lse, loss_only=loss_only)
        torch.cuda.synchronize()
        ws = hp.workspace(B, N, d)
        runs.append({"loss": float(loss_out.item()), "dq": dq[:B, :d].cpu(), "dE": dE.cpu(), "dq_pad": dq[:, d:].cpu(),
                     "ws": ws.clone()})                     # (on the device: megabytes of slabs)
    out = dict(runs[0])
    out["again"], out["ws_second"], out["cand"] = runs[2], runs[1]["ws"], cand
    q32 = np.ascontiguousarray(q[:B, :d].cpu().numpy())
    Cm = E[cand]
    mask = np.ones((N, d), np.float32)
    if p > 0:
        mask = (ko.dropout_keep_mask(SEED, H.STREAM_CAND, step, N, d, p) * (np.float32(1.0) / (np.float32(1.0) - np.float32(p)))).astype(np.float32)
    Cm = np.ascontiguousarray(Cm * mask, dtype=np.float32)
    x64 = q32.astype(np.float64) @ Cm.astype(np.float64).T
    x32 = (torch.from_numpy(q32) @ torch.from_numpy(Cm).T).numpy()
    inv = np.float32(1.0 / norm)
    out["cancelled"] = False
    if loss == "kl":
        # KLDiv(sum)(log_softmax(x), y), y in {0, 1}: loss = sum over positives of lse - x, d/dx = e^(x - lse) sum_n y - y, with
        # lse the row log-sum-exp tensor the call was handed (an input: both chains take it as it is)
        lse32 = row_lse[:B].cpu().numpy().astype(np.float32)[:, None]
        lse64 = lse32.astype(np.float64)
        ysum = y.sum(axis=1, keepdims=True)
        l64 = ((lse64 - x64) * y).sum()
        g64 = np.exp(x64 - lse64) * ysum - y
        l32 = ((lse32 - x32) * y.astype(np.float32)).astype(np.float32).sum(axis=1, dtype=np.float32).sum(dtype=np.float64)
        g32 = (np.exp(x32 - lse32, dtype=np.float32) * ysum.astype(np.float32) - y.astype(np.float32)).astype(np.float32)
        # N = 1: lse is the log-sum-exp of ONE score, i.e. the other kernel's x itself, and the true loss is 0: what the call
        # returns is the difference of two fp32 dot products' rounding errors, and the fp32 chain's own lse - x can be exactly
        # 0.  There, and only there, the bound is the a-priori error bound of an fp32 dot product of d terms, d u sum_k |q_k c_k|
        # with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1), per positive.
        out["cancelled"] = N == 1
        out["cancel_unit"] = float(d * 2.0 ** -24 * ((np.abs(q32).astype(np.float64) @ np.abs(Cm).astype(np.float64).T) * y).sum())
    else:
        ys64 = np.where(y, 1.0, 0.0)
        ys32 = ys64.astype(np.float32)
        if smoothing > 0:
            invn = np.float32(1.0) / np.float32(N)
            yp, yn = (np.float32(1.0) + invn) * (np.float32(1.0) - np.float32(smoothing)), invn * (np.float32(1.0) - np.float32(smoothing))
            ys32 = np.where(y, yp, yn).astype(np.float32)
            ys64 = ys32.astype(np.float64)                # the targets are inputs: the kernel is handed these two floats
        l64 = (np.maximum(x64, 0) - x64 * ys64 + np.log1p(np.exp(-np.abs(x64)))).sum()
        g64 = 1.0 / (1.0 + np.exp(-x64)) - ys64
        e32 = np.exp(-np.abs(x32), dtype=np.float32)
        l32 = (np.maximum(x32, np.float32(0)) - x32 * ys32 + np.log1p(e32, dtype=np.float32)).astype(np.float32).sum(axis=1, dtype=np.float32).sum(dtype=np.float64)
        g32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x32, dtype=np.float32)) - ys32).astype(np.float32)
    G64 = g64 / norm
    G32 = (g32 * inv).astype(np.float32)
    out["loss64"], out["loss32"] = float(l64), float(l32)
    out["dq64"] = G64 @ Cm.astype(np.float64)
    out["dq32"] = (torch.from_numpy(G32) @ torch.from_numpy(Cm)).double().numpy()
    dE64 = np.zeros((n_ent, d))
    np.add.at(dE64, cand, (G64.T @ q32.astype(np.float64)) * mask)
    dE32 = np.zeros((n_ent, d), np.float32)
    np.add.at(dE32, cand, ((torch.from_numpy(np.ascontiguousarray(G32.T)) @ torch.from_numpy(q32)) * torch.from_numpy(mask)).numpy())
    out["dE64"], out["dE32"] = dE64, dE32.astype(np.float64)
    return out


def check_case(hp, name, *args, **kw):
    o = tiles_case(hp, *args, **kw)
    rows = np.unique(o["cand"])
    # repeated runs, identical bits: the loss, dQ, the whole workspace (G^T among it) and the candidate rows -- those not where a
    # candidate list with repeats has several tiles add to one row with float atomics, in whatever order they arrive
    again = o["again"]
    assert o["loss"] == again["loss"], (name, "loss differs between two runs", o["loss"], again["loss"])
    assert torch.equal(o["dq"], again["dq"]), (name, "dQ differs between two runs")
    assert torch.equal(o["ws_second"], again["ws"]), (name, "workspace (G^T, partials, planes, slabs) differs between two runs")
    if not kw.get("repeats"):
        assert torch.equal(o["dE"], again["dE"]), (name, "dE differs between two runs")
    # band_check's rule for one number: error <= 3 x the fp32 chain's + 1e-7 |truth|; only at N = 1 with the KL loss, where
    # the truth is 0 (tiles_case), the dot product's a-priori bound on top.
    err, err32 = abs(o["loss"] - o["loss64"]), abs(o["loss32"] - o["loss64"])
    bound = 3.0 * err32 + 1e-7 * abs(o["loss64"]) + (o["cancel_unit"] if o["cancelled"] else 0.0)
    print(f"{name}: loss {o['loss']!r} float64 {o['loss64']!r} fp32 chain {o['loss32']!r} (error {err:.3e}, bound {bound:.3e})")
    assert np.isfinite(o["loss"]) and err <= bound, (name, "loss", err, bound)
    if kw.get("loss_only"):
        assert torch.all(o["dE"] == 0) and torch.all(o["dq"] == 7.0), (name, "loss_only wrote gradients")
        return o
    r_dq = band_check(name + " dQ", o["dq"], o["dq64"], o["dq32"])
    r_de = band_check(name + " dE", o["dE"][rows], o["dE64"][rows], o["dE32"][rows])
    print(f"{name}: worst max-error / rms ratios  dQ {r_dq[0]:.3f} / {r_dq[1]:.3f}   dE {r_de[0]:.3f} / {r_de[1]:.3f}")
    assert torch.all(o["dq_pad"] == 0), (name, "dQ padding columns")
    outside = np.ones(o["dE"].shape[0], bool)
    outside[rows] = False
    assert torch.all(o["dE"][torch.from_numpy(outside)] == 0), (name, "rows outside the candidate list were written")
    return o


DS, NS, BS = (193, 194, 200, 202, 208), (1, 63, 64, 65, 130), (1, 63, 64, 65, 130, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["bce", "kl"])
@pytest.mark.parametrize("d", DS)
def test_shapes_against_float64(d, loss, okge_lib):
    """the whole (N, B, dropout) cross at every slot size and loss; BCE with label smoothing 0.1.  One workgroup per tile sweeps
    all chunks (B = 130: three, B = 200: four -- both plane buffers are reused)."""
    hp = engine()
    for N in NS:
        for B in BS:
            for p in (0.0, 0.4):
                check_case(hp, f"{loss} d={d} N={N} B={B} p={p}", d, N, B, p, 9000 * d + 10 * N + B, loss=loss,
                           smoothing=0.1 if loss == "bce" else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["bce", "kl"])
def test_further_cases(loss, okge_lib):
    hp = engine()
    check_case(hp, f"{loss} repeats", 200, 130, 130, 0.4, 21, loss=loss, repeats=True)
    check_case(hp, f"{loss} rows split over blockIdx.y, one chunk each", 200, 130, 200, 0.4, 22, loss=loss, b_split=None)
    check_case(hp, f"{loss} rows split in two, four chunks each", 200, 130, 512, 0.4, 26, loss=loss, b_split="2")
    check_case(hp, f"{loss} rows split in two, partial last chunk", 194, 65, 300, 0.0, 27, loss=loss, b_split="2")
    check_case(hp, f"{loss} loss_only", 202, 65, 130, 0.4, 23, loss=loss, loss_only=True)
    check_case(hp, f"{loss} 300 positives in a tile", 200, 65, 130, 0.0, 24, loss=loss, many=True)
    check_case(hp, f"{loss} 300 positives, rows split", 200, 65, 130, 0.4, 28, loss=loss, many=True, b_split=None)
    check_case(hp, f"{loss} no smoothing", 193, 65, 65, 0.0, 25, loss=loss)


def step_and_tiles_with_loss(hp_step, hp_tiles, d, N, B, seed):
    """the same batch through the fused step (the launch that folds the queries writes their planes) and through encode_queries +
    train_tiles (the planes come from the caller's query block) -> (loss, candidate rows of dE) of both.  The prefix entities
    lie behind the candidate range, so the step adds nothing but the tile's gradient to those rows."""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    n_ent, n_rel = N + 2 + 40, 12
    dev = hp_step.device
    Et = torch.from_numpy((rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)).to(dev)
    Rt = torch.from_numpy((rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)).to(dev)
    n_po = B // 2
    n_sp = B - n_po
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    y = labels(rng, B, N)
    col_, row_ = np.nonzero(y.T)
    batch = H.PrefixBatch(po_rel=i32(rng.integers(2, n_rel, n_po)), po_obj=i32(rng.integers(N + 2, n_ent, n_po)),
                          sp_subj=i32(rng.integers(N + 2, n_ent, n_sp)), sp_rel=i32(rng.integers(2, n_rel, n_sp)),
                          pos_row=i32(row_), pos_col=i32(col_), cand_first=2, n_cand=N)
    batch.drop_cand = H.DropoutSpec(0.4, SEED, H.STREAM_CAND, 3)
    dE_step, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
    l_step = hp_step.forward_backward(Et, Rt, "complex", batch, dE_step, dR, grads_zero=True)
    sh = H.Shard(0, n_ent, 0)
    q = hp_tiles.encode_queries(Et, Rt, "complex", batch, sh)[0]
    dE_tiles = torch.zeros_like(Et)
    l_tiles = hp_tiles.train_tiles(Et, Rt, "complex", q, batch, sh, dE_tiles, torch.zeros_like(q), N, normalizer=float(B) * N, grads_zero=True)
    torch.cuda.synchronize()
    return (float(l_step.item()), dE_step[2:N + 2].cpu()), (float(l_tiles.item()), dE_tiles[2:N + 2].cpu())


@pytest.mark.gpu
def test_step_then_shorter_step_in_a_nan_workspace(okge_lib):
    """a 130-row step, then a 65-row step, on an engine whose workspace was first filled with NaN patterns, against the tiles path
    on a fresh engine: the candidate rows bit for bit and the loss to the order of a double sum (both producers of the query
    planes; nothing stale behind row 65 reaches the scores, which the loss would show)"""
    d, N = 200, 130
    used = engine()
    used.workspace(130, N, d).fill_(0xFF)
    step_and_tiles_with_loss(used, engine(), d, N, 130, 8)
    (l_got, got), (l_want, want) = step_and_tiles_with_loss(used, engine(), d, N, 65, 9)
    assert torch.isfinite(got).all() and got.abs().max() > 0
    assert torch.equal(got, want)
    assert np.isfinite(l_got) and abs(l_got - l_want) <= 1e-12 * abs(l_want), (l_got, l_want)
