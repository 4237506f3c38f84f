"""The masked candidate rows reach the dQ kernel as three bf16 planes written once by the tile kernel (csrc/okge_train64.hip,
DqSplit::write_planes in csrc/okge_dq_split.h) instead of as fp32 rows that every row-block workgroup of dq8s_kernel split again.

What tests/test_dq_split.py leaves out of that hand-over: slot sizes that end in a partial octet and take the scalar gather, an
explicit candidate id list, the tail-split launch (whose tiles address the planes through tile_window), two candidate ranges at
the smaller instances, the KL tile instances, a workspace that held a longer range before, and reproducibility with an id
list.  Truth, restatement and bounds are test_dq_split's: dQ against G . Cm in float64, held by band_check at its default
factors to the fp32 restatement G32 . Cm."""
import numpy as np
import pytest
import torch

from lstm_reference import band_check
from oracle import kge_oracle as ko
from test_dq_split import SEED, check_case, dq_case

pytestmark = pytest.mark.gpu


def engine():
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


def general_case(hp, d, N, B, p, seed, ids=False, loss="bce"):
    """dq_case with an explicit candidate id list (a unique random subset of a larger table; the dropout key of a candidate is
    its POSITION in the list) and / or the KL loss -> (dQ as returned [rows][ld], float64 truth [B][d], fp32 restatement)"""
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
    dE = torch.zeros_like(Et)
    dq = torch.full_like(q, 7.0)
    norm = float(B) * N
    hp.train_tiles(Et, Rt, "complex", q, batch, sh, dE, dq, N, loss=loss, normalizer=norm, grads_zero=not ids, row_lse=row_lse)
    torch.cuda.synchronize()
    x = x.cpu().numpy()
    Cm = E[cand]
    if p > 0:
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        Cm = (Cm * scale) * ko.dropout_keep_mask(SEED, H.STREAM_CAND, step, N, d, p)
    Cm = np.ascontiguousarray(Cm, dtype=np.float32)
    inv = np.float32(1.0 / norm)
    if loss == "kl":
        G64 = ko.loss_and_dscore(x.astype(np.float64), y.astype(np.float64), ko.LOSS_KL)[1] / norm
        G32 = (ko.loss_and_dscore(x, y.astype(np.float32), ko.LOSS_KL)[1] * inv).astype(np.float32)
    else:
        G64 = (1.0 / (1.0 + np.exp(-x.astype(np.float64))) - y) / norm
        sig32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)
        G32 = (sig32 * inv - y.astype(np.float32) * inv).astype(np.float32)
    want = G64 @ Cm.astype(np.float64)
    want32 = (torch.from_numpy(G32) @ torch.from_numpy(Cm)).double().numpy()
    return dq, want, want32


def check_general(hp, name, d, N, B, p, seed, **kw):
    dq, want, want32 = general_case(hp, d, N, B, p, seed, **kw)
    got = dq.cpu()
    ratios = band_check(name, got[:B, :d], want, want32)
    print(f"{name}: worst max-error ratio {ratios[0]:.3f}, worst rms ratio {ratios[1]:.3f}")
    assert torch.all(got[:, d:] == 0), name
    return dq


@pytest.mark.parametrize("d", [2, 6, 70, 198, 202, 206])
def test_partial_octet_slot_sizes(d, okge_lib):
    """slot sizes that are no multiple of 4 (scalar gather) and end in a partial octet, at every instance: KB = 4 (2, 6), KB = 8
    (70), KB = 13 with the short last round (198) and without (202, 206); one tile, a ragged sub-chunk, a ragged second tile,
    three tiles; one row and a partial second row block"""
    hp = engine()
    for N in (1, 33, 65, 130):
        for B in (1, 65):
            check_case(hp, f"d={d} N={N} B={B}", d, N, B, 0.4, 7000 * d + N + B)


@pytest.mark.parametrize("d,N,B", [(200, 333, 65), (64, 65, 64)])
def test_explicit_candidate_ids(d, N, B, okge_lib):
    check_general(engine(), f"ids d={d} N={N} B={B}", d, N, B, 0.4, 11 * d + N, ids=True)


@pytest.mark.parametrize("mbytes", [None, "16"])
@pytest.mark.parametrize("d", [64, 200])
def test_tail_split_shape(d, mbytes, okge_lib, monkeypatch):
    """275 tiles, the last one ragged, 256 rows: 19 tiles are launched apart with the rows split over workgroups, and only the
    blockIdx.y == 0 workgroups of that launch write planes, at the tail's offset (tile_window).  16 MiB of G^T: two ranges of 256
    and 19 tiles; the second is no more than one round, so it runs as ONE plain launch (no tail split) that writes its planes
    over the head of the first range's and adds to its slabs."""
    if mbytes is None:
        monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    else:
        monkeypatch.setenv("OKGE_GT_MBYTES", mbytes)
    check_case(engine(), f"tail split d={d} GT={mbytes}", d, 64 * 274 + 37, 256, 0.3, 31 * d)


@pytest.mark.parametrize("d", [64, 128])
def test_two_ranges_small_instances(d, okge_lib, monkeypatch):
    monkeypatch.setenv("OKGE_GT_MBYTES", "1")
    check_case(engine(), f"two ranges d={d} N=1000 B=512", d, 1000, 512, 0.4, 77 + d)


def test_kl_instance(okge_lib):
    """the KL tile kernels are instantiations of their own; G = (softmax(x) sum_n y - y) / normalizer from the oracle"""
    check_general(engine(), "kl d=200 N=333 B=65", 200, 333, 65, 0.4, 13, loss="kl")


@pytest.mark.parametrize("d", [64, 200])
def test_workspace_reuse(d, okge_lib):
    """a call with 130 candidates, then one with 65 on the same engine: the planes of the longer call's third tile are still in
    the workspace behind the range.  Bit-equal to the same call on a fresh engine whose workspace was filled with NaN patterns."""
    B = 65
    used = engine()
    dq_case(used, d, 130, B, 0.4, 5)
    after = dq_case(used, d, 65, B, 0.4, 6)[0].clone()
    fresh = engine()
    fresh.workspace(B, 65, d).fill_(0xFF)
    first = dq_case(fresh, d, 65, B, 0.4, 6)[0]
    assert torch.equal(after, first)
    assert torch.isfinite(first).all()


def test_bit_reproducible_with_ids(okge_lib):
    hp = engine()
    a = general_case(hp, 200, 333, 65, 0.4, 5, ids=True)[0].clone()
    b = general_case(hp, 200, 333, 65, 0.4, 5, ids=True)[0]
    assert torch.equal(a, b)
