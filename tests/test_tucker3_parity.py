"""Tucker3 lookup model (csrc/okge_tucker3.hip: fold and backward on the exact-fp32 MFMA) on the GPU against the reference's own
LookupTucker3RelationModel (tests/golden/g18_tucker3_*.npz), against the float64 restatement (tests/tucker3_reference.py) at
full size and at edge shapes, and for the properties the kernels promise: bit-reproducible runs, the drop-in route equal to the
fused step, fused ranks equal to the materialised ones, refused sizes leave the outputs alone."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from lstm_reference import band_check
import tucker3_reference as TR
from test_tucker3_reference import KEYS, construct, state_before

pytestmark = pytest.mark.gpu

CASES = [n for n in golden_names("g18_tucker3_") if n != "g18_tucker3_adagrad"]
F64, F32 = torch.float64, torch.float32


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def close_to_largest(got, want, frac, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    np.testing.assert_allclose(got, want, rtol=0, atol=frac * max(np.abs(want).max(), 1e-30), err_msg=what)


def batch_of(z, pre="", masks=True):
    """fixture batch -> PrefixBatch; a 1-vs-all case takes the contiguous range, a shared list its ids; captured keep-masks replay"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    b = H.PrefixBatch()
    if pre + "po_rel" in z.files:
        b.po_rel, b.po_obj = dev(z[pre + "po_rel"].reshape(-1)), dev(z[pre + "po_obj"].reshape(-1))
    if pre + "sp_subj" in z.files:
        b.sp_subj, b.sp_rel = dev(z[pre + "sp_subj"].reshape(-1)), dev(z[pre + "sp_rel"].reshape(-1))
    cand = z[pre + "cand"].reshape(-1).astype(np.int32)
    if "shared" in z.files and not int(z["shared"]):
        b.cand_first, b.n_cand = int(cand[0]), int(cand.size)
    else:
        b.cand_ids = dev(cand)
    b.pos_row, b.pos_col = H.positives_from_dense(dev(z[pre + "labels"]))
    if masks and "mask_cand" in z.files:
        p_in, p_rel = float(z["input_dropout"]), float(z["relation_input_dropout"])
        spec = lambda key, p: H.DropoutSpec(p=p, keep=dev(z[key])) if key in z.files else H.DropoutSpec()      # noqa: E731
        b.drop_cand, b.drop_po_ent, b.drop_sp_ent = spec("mask_cand", p_in), spec("mask_po_ent", p_in), spec("mask_sp_ent", p_in)
        b.drop_po_rel, b.drop_sp_rel = spec("mask_po_rel", p_rel), spec("mask_sp_rel", p_rel)
    return b


def step_of(z, prefix="init/", sums=None, **kw):
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep
    E, R, W = (dev(z[prefix + k]).clone() for k in KEYS)
    st = Tucker3TrainStep(E, R, W, **kw)
    if sums is not None:
        for t, k in zip((st.sumE, st.sumR, st.sumW), KEYS):
            t.copy_(dev(z[sums + k]))
    return st


def case_step(z):
    return step_of(z, loss=str(z["loss_kind"]), label_smoothing=float(z["smoothing"]))


@pytest.mark.parametrize("name", CASES)
def test_train_step_matches_reference(okge_lib, name):
    """Tucker3TrainStep.forward_backward: loss, outputs, the three parameters' gradients"""
    z = golden(name)
    st = case_step(z)
    B, N = z["labels"].shape
    scores = torch.empty((B, (N + 3) // 4 * 4), device="cuda:0")[:, :N]
    loss = st.forward_backward(batch_of(z), normalizer=float(z["normalizer"]), scores=scores)
    torch.cuda.synchronize()
    np.testing.assert_allclose(scores.cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
    assert abs(float(loss[0]) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    for k, g in zip(KEYS, (st.dE, st.dR, st.dW)):
        close_to_largest(g, z["grad/" + k], 1e-4, k)
    assert not st.dE[0].any() and not st.dR[0].any()               # padding_idx rows: no gradient


@pytest.mark.parametrize("name", CASES)
def test_module_addloss_and_eval_match_reference(okge_lib, name):
    """the reference Trainer's statements on the seeded module: AddLossModule forward + backward (gradients in .grad), then
    eval mode: prefix scores and triple scores.  (The dropout case draws its own Philox masks here: only loss finiteness.)"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden(name)
    dropout = float(z["input_dropout"]) > 0
    m = construct(z, input_dropout=float(z["input_dropout"]), relation_input_dropout=float(z["relation_input_dropout"]))
    m.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in KEYS})
    m = m.cuda()
    m.train()
    lossf = torch.nn.BCEWithLogitsLoss(reduction="sum") if str(z["loss_kind"]) == "bce" else torch.nn.KLDivLoss(reduction="sum")
    mod = AddLossModule(m, lossf, float(z["smoothing"]))
    po = (dev(z["po_rel"]), dev(z["po_obj"])) if "po_rel" in z.files else None
    sp = (dev(z["sp_subj"]), dev(z["sp_rel"])) if "sp_subj" in z.files else None
    loss, hook, outs = mod(inputs=[po, sp], labels=dev(z["labels"]), use_batch_shared_entities=bool(z["shared"]),
                           batch_shared_entities=dev(z["cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    (loss.sum() / float(z["normalizer"])).backward()
    assert hook is None and np.isfinite(float(loss.detach()))
    if not dropout:
        assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
        np.testing.assert_allclose(outs.detach().cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
        for k, p in m.named_parameters():
            close_to_largest(p.grad, z["grad/" + k], 1e-4, k)
    m.eval()
    with torch.no_grad():
        if not dropout:                                            # validation loss (trainer.py:363-369): no gradients, no masks
            vloss, _, vouts = mod(inputs=[po, sp], labels=dev(z["labels"]), use_batch_shared_entities=bool(z["shared"]),
                                  batch_shared_entities=dev(z["cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
            assert abs(float(vloss) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
            np.testing.assert_allclose(vouts.cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
        if sp is not None:
            x = m.sp_prefix_score(*sp)
            np.testing.assert_allclose(x.cpu().numpy(), z["sp_all_eval"], rtol=1e-5, atol=1e-5)
        if po is not None:
            x = m.po_prefix_score(*po)
            np.testing.assert_allclose(x.cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)
            many = m.precompute_batch_shared_inputs(torch.arange(2, int(z["n_ent"]), dtype=torch.int32, device="cuda"))
            np.testing.assert_allclose(m.po_prefix_score(*po, many).cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)
        tri = m(dev(z["t_subj"]), dev(z["t_rel"]), dev(z["t_obj"]))
        assert tuple(tri.shape) == tuple(z["triple_eval"].shape)
        np.testing.assert_allclose(tri.cpu().numpy(), z["triple_eval"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("step", [0, 1, 2])
def test_adagrad_steps_restarted_from_reference_state(okge_lib, step):
    """each of the reference's three OptimRegime Adagrad steps, restarted from the reference's state before it"""
    z = golden("g18_tucker3_adagrad")
    pre, post = state_before(step), f"s{step}_after/"
    lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
    st = step_of(z, pre + "param/", sums=pre + "sum/", lr=lr, weight_decay=float(z["opt_weight_decay"]), eps=eps)
    B, N = z[f"s{step}_labels"].shape
    loss = st.step(batch_of(z, f"s{step}_"), normalizer=float(B * N))
    assert abs(float(loss[0]) - float(z[f"s{step}_loss"])) <= 1e-5 * abs(float(z[f"s{step}_loss"]))
    for k, p, s in zip(KEYS, (st.E, st.R, st.W), (st.sumE, st.sumR, st.sumW)):
        want_p, want_s = z[post + "param/" + k], z[post + "sum/" + k]
        # (tests/test_lstm_parity.py's rule: 2e-4 of lr, plus what a gradient error of 1e-4 of the tensor's largest gradient -- the
        #  bar of the gradient tests -- does to lr g / (sqrt(sum) + eps) where the accumulator holds little more than g^2)
        g = np.sqrt(np.maximum(want_s - z[pre + "sum/" + k], 0))
        tol = 2e-4 * lr + lr * (1e-4 * g.max()) * (np.sqrt(z[pre + "sum/" + k]) + eps) / (np.sqrt(want_s) + eps) ** 2
        bad = np.abs(p.cpu().numpy() - want_p) > tol
        assert not bad.any(), (k, int(bad.sum()), float(np.abs(p.cpu().numpy() - want_p).max()))
        close_to_largest(s, want_s, 2e-4, k + " accumulator")
        assert not st.dE.any() and not st.dR.any() and not st.dW.any()          # the sweep cleared the gradients


def test_dropin_route_gives_the_fused_steps_gradients(okge_lib):
    """AddLossModule + loss.backward() (any torch optimizer then steps the module) against Tucker3TrainStep.forward_backward"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden("g18_tucker3_adagrad")
    m = construct(z)
    m.load_state_dict({k: torch.from_numpy(z["s0_before/param/" + k]) for k in KEYS})
    m = m.cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    st = step_of(z, "s0_before/param/")
    B, N = z["s0_labels"].shape
    loss, _, outs = mod(inputs=[(dev(z["s0_po_rel"]), dev(z["s0_po_obj"])), (dev(z["s0_sp_subj"]), dev(z["s0_sp_rel"]))],
                        labels=dev(z["s0_labels"]), use_batch_shared_entities=True, batch_shared_entities=dev(z["s0_cand"]), epoch=1,
                        input_style_triple_or_prefix="right_and_left_prefix")
    (loss.sum() / float(B * N)).backward()
    l2 = st.forward_backward(batch_of(z, "s0_"), normalizer=float(B * N))
    assert abs(float(loss.detach()) - float(l2[0])) <= 1e-6 * abs(float(l2[0]))
    assert tuple(outs.shape) == (B, N)
    for (k, p), g in zip(m.named_parameters(), (st.dE, st.dR, st.dW)):
        np.testing.assert_allclose(p.grad.cpu().numpy(), g.cpu().numpy(), rtol=0, atol=1e-5, err_msg=k)
    opt = torch.optim.Adagrad(m.parameters(), lr=0.1)              # any torch optimizer trains the module as a drop-in
    before = [p.detach().clone() for p in m.parameters()]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))


def test_prefix_scores_carry_gradients_for_a_callers_loss(okge_lib):
    """sp_prefix_score / po_prefix_score with gradients enabled: a caller's own loss on the scores reaches all three parameters
    (float64 restatement through torch autograd as the yardstick)"""
    z = golden("g18_tucker3_bce_all")
    m = construct(z)
    m.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in KEYS})
    m = m.cuda()
    m.eval()
    sp, po = (dev(z["sp_subj"]), dev(z["sp_rel"])), (dev(z["po_rel"]), dev(z["po_obj"]))
    (m.sp_prefix_score(*sp).pow(2).sum() + m.po_prefix_score(*po).sin().sum()).backward()
    P = [torch.from_numpy(z["init/" + k]).double().requires_grad_() for k in KEYS]
    po_rel, po_obj, sp_subj, sp_rel, _ = TR.ids_of(z)
    q, _ = TR.fold(P[2], P[0][torch.cat([po_obj, sp_subj])], P[1][torch.cat([po_rel, sp_rel])], po_rel.numel())
    x = q @ P[0][2:].t()
    (x[po_rel.numel():].pow(2).sum() + x[:po_rel.numel()].sin().sum()).backward()
    for (k, p), want in zip(m.named_parameters(), P):
        close_to_largest(p.grad, want.grad.numpy(), 1e-4, k)


def seeded_module(z):
    m = construct(z)
    m.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in KEYS})
    m = m.cuda()
    m.eval()
    return m


def ids(z, k):
    return torch.as_tensor(np.asarray(z[k]).reshape(-1).astype(np.int64))


@pytest.mark.parametrize("name", CASES)
def test_encoded_row_surface_has_the_reference_shapes(okge_lib, name):
    """encode_rel / get_rel / get_all_rel return the (., d^2) projected rows (Linear of the relation rows, float64 restatement),
    and the reference's idioms on ENCODED rows run: triple_score(encode_subj, encode_rel, encode_obj) (model.py:36-41) and
    _score(..., prefix=True) in both directions (model.py:52-74) reproduce the reference's recorded scores"""
    z = golden(name)
    m = seeded_module(z)
    d, r, n_rel = int(z["d"]), int(z["r_e"]), int(z["n_rel"])
    R, W = torch.from_numpy(z["init/" + KEYS[1]]).double(), torch.from_numpy(z["init/" + KEYS[2]]).double()
    with torch.no_grad():
        M = m.encode_rel(dev(z["t_rel"]))
        assert tuple(M.shape) == (z["t_rel"].shape[0], d * d)
        np.testing.assert_allclose(M.cpu().numpy(), (R[ids(z, "t_rel")] @ W.t()).numpy(), rtol=1e-5, atol=1e-5)
        one = m.get_rel(3)
        assert tuple(one.shape) == (1, d * d)
        np.testing.assert_allclose(one.cpu().numpy(), (R[3:4] @ W.t()).numpy(), rtol=1e-5, atol=1e-5)
        every = m.get_all_rel()
        assert tuple(every.shape) == (n_rel - 2, d * d)
        np.testing.assert_allclose(every.cpu().numpy(), (R[2:] @ W.t()).numpy(), rtol=1e-5, atol=1e-5)
        rows = m.encode_rel(m.relation_embedding.weight[2:5].contiguous(), lookup=False)      # model.py:459-460: rows in hand
        np.testing.assert_allclose(rows.cpu().numpy(), every[:3].cpu().numpy(), rtol=0, atol=0)
        tri = m.triple_score(m.encode_subj(dev(z["t_subj"])), M, m.encode_obj(dev(z["t_obj"])))
        assert tuple(tri.shape) == tuple(z["triple_eval"].shape)
        np.testing.assert_allclose(tri.cpu().numpy(), z["triple_eval"], rtol=1e-5, atol=1e-5)
        tri = m._score(m.encode_subj(dev(z["t_subj"])), M, m.encode_obj(dev(z["t_obj"])))
        np.testing.assert_allclose(tri.cpu().numpy(), z["triple_eval"], rtol=1e-5, atol=1e-5)
        if "sp_subj" in z.files:
            x = m._score(m.encode_subj(dev(z["sp_subj"])), m.encode_rel(dev(z["sp_rel"])), m.get_all_obj(), prefix=True, sp=True, po=False)
            np.testing.assert_allclose(x.cpu().numpy(), z["sp_all_eval"], rtol=1e-5, atol=1e-5)
        x = m._score(m.get_all_subj(), m.encode_rel(dev(z["po_rel"])), m.encode_obj(dev(z["po_obj"])), prefix=True, sp=False, po=True)
        np.testing.assert_allclose(x.cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)
        with pytest.raises(ValueError):
            m.triple_score(m.encode_subj(dev(z["t_subj"])), M[:, :-1], m.encode_obj(dev(z["t_obj"])))


@pytest.mark.parametrize("route", ["forward_ids", "triple_idiom", "score_prefix_sp", "score_prefix_po", "encode_rel"])
def test_triple_and_encoded_row_paths_carry_gradients(okge_lib, route):
    """a caller's own loss on forward(subj, rel, obj), on triple_score / _score of encoded rows and on encode_rel itself reaches
    entity table, relation table and projection: float64 torch autograd through the restatement as the yardstick, each gradient
    within 1e-4 of that tensor's largest entry (the bar of the other gradient tests)"""
    z = golden("g18_tucker3_bce_all")
    m = seeded_module(z)
    s, r, o = dev(z["t_subj"]), dev(z["t_rel"]), dev(z["t_obj"])
    P = [torch.from_numpy(z["init/" + k]).double().requires_grad_() for k in KEYS]
    E, R, W = P
    si, ri, oi = ids(z, "t_subj"), ids(z, "t_rel"), ids(z, "t_obj")
    d = E.shape[1]
    if route == "forward_ids":
        got, want = m(s, r, o), TR.triple_scores(W, E[si], R[ri], E[oi])
    elif route == "triple_idiom":
        got, want = m.triple_score(m.encode_subj(s), m.encode_rel(r), m.encode_obj(o)), TR.triple_scores(W, E[si], R[ri], E[oi])
    elif route == "score_prefix_sp":
        got = m._score(m.encode_subj(s), m.encode_rel(r), m.get_all_obj(), prefix=True, sp=True, po=False)
        want = torch.bmm(E[si][:, None, :], TR.project(W, R[ri], d)).reshape(-1, d) @ E[2:].t()
    elif route == "score_prefix_po":
        got = m._score(m.get_all_subj(), m.encode_rel(r), m.encode_obj(o), prefix=True, sp=False, po=True)
        want = torch.bmm(TR.project(W, R[ri], d), E[oi][:, :, None]).reshape(-1, d) @ E[2:].t()
    else:
        got, want = m.encode_rel(r), R[ri] @ W.t()
    assert got.requires_grad
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-5)
    (got.sin().sum() + got.pow(2).sum()).backward()
    (want.sin().sum() + want.pow(2).sum()).backward()
    for (k, p), w in zip(m.named_parameters(), P):
        if w.grad is None:                                         # encode_rel alone does not touch the entity table
            assert p.grad is None or not p.grad.any(), k
            continue
        assert p.grad is not None, k
        close_to_largest(p.grad, w.grad.numpy(), 1e-4, f"{route} {k}")


def test_gradient_accumulation_treats_the_three_tensors_alike(okge_lib):
    """forward_backward(accumulate=True) on a second batch adds to dE, dR AND dW"""
    z = golden("g18_tucker3_adagrad")
    st = step_of(z, "s0_before/param/")
    B, N = z["s0_labels"].shape
    st.forward_backward(batch_of(z, "s0_"), normalizer=float(B * N))
    one = [g.clone() for g in (st.dE, st.dR, st.dW)]
    st.forward_backward(batch_of(z, "s0_"), normalizer=float(B * N), accumulate=True)
    for a, g, k in zip(one, (st.dE, st.dR, st.dW), KEYS):
        close_to_largest(g, 2 * a.cpu().numpy(), 1e-6, k)


# ---- full size and edge shapes against float64 -------------------------------------------------------------------------------
def random_problem(rng, B, n_po, d, r):
    ent = (rng.standard_normal((B, d)) * 0.5).astype(np.float32)
    rho = (rng.standard_normal((B, r)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((d * d, r)) * (2.0 / np.sqrt(d * r))).astype(np.float32)
    dq = (rng.standard_normal((B, d)) * 1e-3).astype(np.float32)
    return ent, rho, W, dq


def run_kernels(kern, ent, rho, W, dq, n_po):
    """fold + backward through the C ABI on given rows -> (Q block, d_ent, d_rel, dW)"""
    B, d = ent.shape
    r = rho.shape[1]
    e, p, w = dev(ent), dev(rho), dev(W)
    Q = kern.fold(w, e, p, n_po, B - n_po)
    dQ = torch.zeros_like(Q)
    dQ[:B, :d] = dev(dq)
    d_ent, d_rel = torch.full((B, d), float("nan"), device="cuda"), torch.full((B, r), float("nan"), device="cuda")
    dW = torch.full((d * d, r), float("nan"), device="cuda")
    kern.backward(w, e, p, dQ, n_po, B - n_po, d_ent, d_rel, dW, fresh=True)
    torch.cuda.synchronize()
    return Q, d_ent, d_rel, dW


def restate(ent, rho, W, dq, n_po, dtype):
    e, p, w, g = (TR.T(x, dtype) for x in (ent, rho, W, dq))
    q, M = TR.fold(w, e, p, n_po)
    d_ent, d_rel, dW = TR.fold_backward(w, e, p, g, n_po, M)
    return [x.double().numpy() for x in (q, d_ent, d_rel, dW)]


@pytest.mark.parametrize("d,r", [(200, 200), (200, 30), (61, 17)])
def test_full_size_against_float64(okge_lib, d, r):
    """B = 512 (256 po + 256 sp rows), |E| = 14 543: one fused step; its Q, and dW / d_rel_rows / d_ent_rows from the step's own dQ,
    against the float64 restatement, per magnitude band no further off than 3x (max) / 1.6x (rms) the fp32 restatement's own error"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep
    rng = np.random.default_rng(1860 + d + r)
    n_ent, n_rel, B, n_po = 14543, 239, 512, 256
    E = (rng.standard_normal((n_ent, d)) * 0.5).astype(np.float32)
    R = (rng.standard_normal((n_rel, r)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((d * d, r)) * (2.0 / np.sqrt(d * r))).astype(np.float32)
    st = Tucker3TrainStep(dev(E), dev(R), dev(W))
    b = H.PrefixBatch(po_rel=dev(rng.integers(2, n_rel, n_po).astype(np.int32)), po_obj=dev(rng.integers(2, n_ent, n_po).astype(np.int32)),
                      sp_subj=dev(rng.integers(2, n_ent, B - n_po).astype(np.int32)), sp_rel=dev(rng.integers(2, n_rel, B - n_po).astype(np.int32)),
                      cand_first=2, n_cand=n_ent - 2)
    y = torch.zeros((B, n_ent - 2), device="cuda")
    y[torch.arange(B, device="cuda").repeat_interleave(3), dev(rng.integers(0, n_ent - 2, 3 * B))] = 1.0
    b.pos_row, b.pos_col = H.positives_from_dense(y)
    loss = st.forward_backward(b)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss[0]))
    ent, rho, dq = st.ent_rows.cpu().numpy(), st.rel_rows.cpu().numpy(), st.dQ[:B, :d].cpu().numpy()
    assert np.abs(dq).max() > 0
    want, want32 = restate(ent, rho, W, dq, n_po, F64), restate(ent, rho, W, dq, n_po, F32)
    got = (st.Q[:B, :d], st.d_ent, st.d_rel, st.dW)
    for name, g, w, w32 in zip(("Q", "d_ent_rows", "d_rel_rows", "dW"), got, want, want32):
        print(f"d={d} r={r} {name}: (max, rms) error ratio to the fp32 restatement", band_check(name, g, w, w32))
    assert not st.Q[B:].any() and not st.Q[:, d:].any()            # the query block's padding is zero


EDGE = [(1, 1), (1, 17), (2, 2), (15, 16), (16, 15), (16, 16), (17, 1), (17, 64), (64, 17), (64, 255), (255, 2), (256, 256)]


def test_edge_shapes_against_float64(okge_lib):
    """(d, r_e) off and on the 16 / 64 tiles x B in {1, 63, 64, 65} x {both directions, po only, sp only}: every output under the
    rule of the full-size test (lstm_reference.band_check at its defaults: per |x| band, max error <= 3x and rms <= 1.6x the fp32
    restatement's own, each plus 1e-7 of the largest entry); the query block's padding is zero"""
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3Kernels
    kern = Tucker3Kernels(HotPath("cuda:0"))
    rng = np.random.default_rng(1870)
    for i, (d, r) in enumerate(EDGE):
        for B in (1, 63, 64, 65):
            splits = {0: B // 2, 1: B, 2: 0}
            n_po = splits[(i + B) % 3] if (d, r) != (256, 256) else B // 2
            ent, rho, W, dq = random_problem(rng, B, n_po, d, r)
            Q, d_ent, d_rel, dW = run_kernels(kern, ent, rho, W, dq, n_po)
            want, want32 = restate(ent, rho, W, dq, n_po, F64), restate(ent, rho, W, dq, n_po, F32)
            for name, g, w, w32 in zip(("Q", "d_ent_rows", "d_rel_rows", "dW"), (Q[:B, :d], d_ent, d_rel, dW), want, want32):
                band_check(f"{name} d={d} r={r} B={B} n_po={n_po}", g, w, w32)
            assert not Q[B:].any() and not Q[:, d:].any(), (d, r, B)


def test_dw_accumulates_without_the_fresh_flag(okge_lib):
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3Kernels
    kern = Tucker3Kernels(HotPath("cuda:0"))
    ent, rho, W, dq = random_problem(np.random.default_rng(1871), 70, 30, 17, 9)
    Q, _, _, dW = run_kernels(kern, ent, rho, W, dq, 30)
    dQ = torch.zeros_like(Q)
    dQ[:70, :17] = dev(dq)
    acc = dW.clone()
    kern.backward(dev(W), dev(ent), dev(rho), dQ, 30, 40, None, None, acc, fresh=False)
    assert torch.equal(acc, dW + dW)


def test_two_runs_are_bit_identical(okge_lib):
    """no float atomics on the Tucker3 path: loss and all gradients of two runs on identical inputs are equal bit for bit"""
    z = golden("g18_tucker3_bce_all")
    runs = []
    for _ in range(2):
        st = case_step(z)
        loss = st.forward_backward(batch_of(z), normalizer=float(z["normalizer"]))
        torch.cuda.synchronize()
        runs.append((loss.clone(), st.dE.clone(), st.dR.clone(), st.dW.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    rng = np.random.default_rng(1872)
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3Kernels
    kern = Tucker3Kernels(HotPath("cuda:0"))
    prob = random_problem(rng, 300, 140, 200, 30)
    a, b = run_kernels(kern, *prob, 140), run_kernels(kern, *prob, 140)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fused_ranks_equal_materialised_ranks(okge_lib):
    """evaluation: filtered ranks through the fused evaluator fed with the folded query block == the ranks computed from the
    materialised okge_score_queries block, exactly"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep
    rng = np.random.default_rng(1873)
    for d, r, n_ent, n_po, n_sp, ties in [(24, 9, 500, 20, 23, False), (16, 16, 300, 0, 31, True), (200, 30, 3000, 40, 37, False)]:
        n_rel, N, B = 12, n_ent - 2, n_po + n_sp
        if ties:                                                   # a tiny alphabet: many scores are exactly equal
            E, R = rng.integers(-1, 2, (n_ent, d)).astype(np.float32) * 0.5, rng.integers(-1, 2, (n_rel, r)).astype(np.float32) * 0.5
            W = rng.integers(-1, 2, (d * d, r)).astype(np.float32) * 0.25
        else:
            E, R = (rng.standard_normal((n_ent, d)) * 0.5).astype(np.float32), (rng.standard_normal((n_rel, r)) * 0.5).astype(np.float32)
            W = (rng.standard_normal((d * d, r)) * (2.0 / np.sqrt(d * r))).astype(np.float32)
        b = H.PrefixBatch(cand_first=2, n_cand=N)
        if n_po:
            b.po_rel, b.po_obj = dev(rng.integers(2, n_rel, n_po).astype(np.int32)), dev(rng.integers(2, n_ent, n_po).astype(np.int32))
        b.sp_subj, b.sp_rel = dev(rng.integers(2, n_ent, n_sp).astype(np.int32)), dev(rng.integers(2, n_rel, n_sp).astype(np.int32))
        row_ptr, grp_ptr, ids, filt_ptr, filt_col = [0], [0], [], [0], []
        for _ in range(B):
            row_ids = []
            for _ in range(int(rng.integers(0, 4))):
                g = rng.integers(0, N, int(rng.integers(1, 4))).tolist()
                ids.extend(g)
                row_ids.extend(g)
                grp_ptr.append(len(ids))
            row_ptr.append(len(grp_ptr) - 1)
            f = np.unique(np.concatenate([rng.integers(0, N, 9), np.asarray(row_ids, np.int64)])).astype(np.int64)
            filt_col.extend(f.tolist())
            filt_ptr.append(len(filt_col))
        csr = [dev(np.asarray(a, t)) for a, t in ((filt_ptr, np.int64), (filt_col, np.int32), (row_ptr, np.int64), (grp_ptr, np.int64),
                                                   (ids, np.int32))]
        st = Tucker3TrainStep(dev(E), dev(R), dev(W))
        ranks = st.ranks(b, *csr)
        x = st.scores(b)
        ref = st.engine.filtered_ranks(x.contiguous(), *csr)
        torch.cuda.synchronize()
        assert ranks.numel() == len(grp_ptr) - 1 > 0
        np.testing.assert_array_equal(ranks.cpu().numpy(), ref.cpu().numpy())


def test_refused_sizes_leave_the_outputs_alone(okge_lib):
    L = okge_lib
    B, d = 8, 16
    ent, rho = torch.randn(B, 300, device="cuda"), torch.randn(B, 300, device="cuda")
    W = torch.randn(d * d, 300, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((64, 512), 7.0, device="cuda")
    ld = int(L.okge_query_ld(d))
    # r_e = 300: unsupported
    rc = L.okge_tucker3_fold(W.data_ptr(), d, 300, ent.data_ptr(), 300, rho.data_ptr(), 300, 4, 4, out.data_ptr(), ld, ws.data_ptr(),
                             ws.numel(), None)
    assert rc == -2 and b"256" in L.okge_last_error()
    rc = L.okge_tucker3_backward(W.data_ptr(), 300, d, ent.data_ptr(), 300, rho.data_ptr(), 300, out.data_ptr(), 512, 4, 4, 0, out.data_ptr(),
                                 out.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -2
    # a query block with the wrong leading dimension, a workspace that is too small, empty batch, unknown flag: invalid
    rc = L.okge_tucker3_fold(W.data_ptr(), d, 16, ent.data_ptr(), 300, rho.data_ptr(), 300, 4, 4, out.data_ptr(), ld + 4, ws.data_ptr(),
                             ws.numel(), None)
    assert rc == -1
    rc = L.okge_tucker3_fold(W.data_ptr(), d, 16, ent.data_ptr(), 300, rho.data_ptr(), 300, 4, 4, out.data_ptr(), ld, ws.data_ptr(), 16, None)
    assert rc == -3
    rc = L.okge_tucker3_fold(W.data_ptr(), d, 16, ent.data_ptr(), 300, rho.data_ptr(), 300, 0, 0, out.data_ptr(), ld, ws.data_ptr(),
                             ws.numel(), None)
    assert rc == -1
    rc = L.okge_tucker3_backward(W.data_ptr(), d, 16, ent.data_ptr(), 300, rho.data_ptr(), 300, out.data_ptr(), 512, 4, 4, 2, out.data_ptr(),
                                 out.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -1
    rc = L.okge_tucker3_score_triples(W.data_ptr(), d, 16, ent.data_ptr(), 8, rho.data_ptr(), 300, ent.data_ptr(), 300, 4, out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), None)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
