"""LSTM-encoded models (csrc/okge_lstm.hip: forward and backward through time on the exact-fp32 MFMA) on the GPU against the
reference's own LSTMComplexRelationModel / LSTMDistmultRelationModel (tests/golden/g17_lstm_*.npz), against a float64
restatement of the reference's op sequence at d = 512, and for the properties the kernels promise: bit-reproducible runs,
no gradient for the padding row, chunk-independent precompute, no torch LSTM on the product path."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from lstm_reference import GRAD_NAMES, band_check, lstm_pass
from test_lstm_api import build

pytestmark = pytest.mark.gpu

CASES = [n for n in golden_names("g17_lstm_") if n != "g17_lstm_adagrad"]
SIDES = ("entity", "relation")
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def slots(z, params, bufs=None, sums=None):
    """LSTMSlot pair from name -> array maps (fixture layout); sums: Adagrad accumulators by parameter name"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot
    out = []
    for side, tok in zip(SIDES, ("ent_tokens", "rel_tokens")):
        lst = [dev(params[f"{side}_encoder_in.{k}"]) for k in LSTM_KEYS]
        flat = torch.cat([x.reshape(-1) for x in lst])
        views, o = [], 0
        for x in lst:
            views.append(flat[o:o + x.numel()].view_as(x))
            o += x.numel()
        bn = running = None
        if f"{side}_batchnorm.weight" in params:
            bn = (dev(params[f"{side}_batchnorm.weight"]), dev(params[f"{side}_batchnorm.bias"]))
            d = bn[0].numel()
            running = (dev(bufs[f"{side}_batchnorm.running_mean"]).clone(), dev(bufs[f"{side}_batchnorm.running_var"]).clone()) if bufs \
                else (torch.zeros(d, device="cuda"), torch.ones(d, device="cuda"))
        s = LSTMSlot(dev(params[f"{side}_embedding.weight"]).clone(), dev(z[tok]), views, bn, running, flat=flat)
        if sums is not None:
            s.sumW.copy_(dev(sums[f"{side}_embedding.weight"]))
            s.sum_flat.copy_(torch.cat([dev(sums[f"{side}_encoder_in.{k}"]).reshape(-1) for k in LSTM_KEYS]))
            if bn is not None:
                s.sum_bn.copy_(torch.cat([dev(sums[f"{side}_batchnorm.weight"]), dev(sums[f"{side}_batchnorm.bias"])]))
        out.append(s)
    return out


def sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def batch_of(z, pre=""):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    b = PrefixBatch()
    b.po_rel, b.po_obj = dev(z[pre + "po_rel"].reshape(-1)), dev(z[pre + "po_obj"].reshape(-1))
    b.sp_subj, b.sp_rel = dev(z[pre + "sp_subj"].reshape(-1)), dev(z[pre + "sp_rel"].reshape(-1))
    b.cand_ids = dev(z[pre + "cand"].reshape(-1).astype(np.int32))
    b.pos_row, b.pos_col = positives_from_dense(dev(z[pre + "labels"]))
    return b


def grads_of(st):
    """fixture names -> this step's gradients"""
    g = {}
    for side, sl in zip(SIDES, (st.entity, st.relation)):
        g[f"{side}_embedding.weight"] = sl.dW
        for k, t in zip(LSTM_KEYS, sl.dlstm):
            g[f"{side}_encoder_in.{k}"] = t
        if sl.bn is not None:
            g[f"{side}_batchnorm.weight"], g[f"{side}_batchnorm.bias"] = sl.d_bn[:sl.d], sl.d_bn[sl.d:]
    return g


def close_to_largest(got, want, frac, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    np.testing.assert_allclose(got, want, rtol=0, atol=frac * max(np.abs(want).max(), 1e-30), err_msg=what)


def scorer_of(z):
    return "complex" if "Complex" in str(z["model"]) else "distmult"


@pytest.mark.parametrize("name", CASES)
def test_train_step_matches_reference(okge_lib, name):
    """LSTMTrainStep.forward_backward: loss, outputs, every parameter's gradient, running statistics"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden(name)
    e, r = slots(z, sub(z, "init/"))
    st = LSTMTrainStep(e, r, scorer_of(z), lr=0.1)
    B, N = z["labels"].shape
    scores = torch.empty((B, (N + 3) // 4 * 4), device="cuda:0")[:, :N]
    loss = st.forward_backward(batch_of(z), scores=scores)
    torch.cuda.synchronize()
    np.testing.assert_allclose(scores.cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
    assert abs(float(loss[0]) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    mine = grads_of(st)
    for k in (str(x) for x in z["param_names"]):
        close_to_largest(mine[k], z["grad/" + k], 1e-4, k)
    assert not e.dW[0].any() and not r.dW[0].any()                 # padding_idx row: no gradient
    for side, sl in zip(SIDES, (e, r)):
        if sl.bn is not None:
            np.testing.assert_allclose(sl.running_mean.cpu().numpy(), z[f"buf/{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(sl.running_var.cpu().numpy(), z[f"buf/{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_module_addloss_and_eval_match_reference(okge_lib, name):
    """the reference Trainer's statements on the seeded module: AddLossModule forward + backward (gradients in .grad), then
    eval mode: precompute_embeddings_from_tokens tables (running statistics) and the prefix scores"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden(name)
    m = build(z).cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    inputs = [(dev(z["po_rel"]), dev(z["po_obj"])), (dev(z["sp_subj"]), dev(z["sp_rel"]))]
    loss, _, outs = mod(inputs=inputs, labels=dev(z["labels"]), use_batch_shared_entities=bool(z["shared"]),
                        batch_shared_entities=dev(z["cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    (loss.sum() / float(z["normalizer"])).backward()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    np.testing.assert_allclose(outs.detach().cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
    for k, p in m.named_parameters():
        close_to_largest(p.grad, z["grad/" + k], 1e-4, k)
    for k, b in m.named_buffers():
        if "running" in k:
            np.testing.assert_allclose(b.cpu().numpy(), z["buf/" + k], rtol=1e-5, atol=1e-6)
    m.eval()
    with torch.no_grad():
        m.precompute_embeddings_from_tokens()
        np.testing.assert_allclose(m.entity_embedding_from_tokens.cpu().numpy(), z["E_eval"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(m.relations_embedding_from_tokens.cpu().numpy(), z["R_eval"], rtol=1e-5, atol=1e-5)
        assert m.get_all_rel().shape[0] == int(z["n_rel"]) - 2          # the reference's slice by min_entities_size
        sp = m.sp_prefix_score(dev(z["sp_subj"]), dev(z["sp_rel"]))
        po = m.po_prefix_score(dev(z["po_rel"]), dev(z["po_obj"]))
    np.testing.assert_allclose(sp.cpu().numpy(), z["sp_all_eval"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(po.cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("step", [0, 1, 2])
def test_adagrad_steps_restarted_from_reference_state(okge_lib, step):
    """each of the reference's three OptimRegime Adagrad steps, restarted from the reference's state before it: parameters,
    accumulators and running statistics after it"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden("g17_lstm_adagrad")
    pre = f"s{step}_before/"
    e, r = slots(z, sub(z, pre + "param/"), bufs=sub(z, pre + "buf/"), sums=sub(z, pre + "sum/"))
    st = LSTMTrainStep(e, r, "complex", lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]), eps=float(z["opt_eps"]))
    B, N = z[f"s{step}_labels"].shape
    loss = st.step(batch_of(z, f"s{step}_"), normalizer=float(B * N))
    assert abs(float(loss[0]) - float(z[f"s{step}_loss"])) <= 1e-5 * abs(float(z[f"s{step}_loss"]))
    post = f"s{step}_after/"
    for side, sl in zip(SIDES, (e, r)):
        got = {f"{side}_embedding.weight": (sl.W, sl.sumW)}
        n, o = {}, 0
        for k, t in zip(LSTM_KEYS, sl.lstm):
            n[k] = (t, sl.sum_flat[o:o + t.numel()].view_as(t))
            o += t.numel()
        got.update({f"{side}_encoder_in.{k}": v for k, v in n.items()})
        if sl.bn is not None:
            got[f"{side}_batchnorm.weight"] = (sl.bn[:sl.d], sl.sum_bn[:sl.d])
            got[f"{side}_batchnorm.bias"] = (sl.bn[sl.d:], sl.sum_bn[sl.d:])
            np.testing.assert_allclose(sl.running_mean.cpu().numpy(), z[post + f"buf/{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(sl.running_var.cpu().numpy(), z[post + f"buf/{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6)
        lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
        for k, (p, s) in got.items():
            want_p, want_s = z[post + "param/" + k], z[post + "sum/" + k]
            # an Adagrad step moves a parameter by lr g / (sqrt(sum) + eps), at most lr: 2e-4 of lr, plus what a gradient error
            # of 1e-4 of the tensor's largest gradient (the bar of the gradient tests) does to that quotient -- it matters only
            # where g is tiny and the accumulator holds little more than g^2 (step 0: sum = g^2, the update ~ lr sign(g))
            g = np.sqrt(want_s - z[pre + "sum/" + k])
            tol = 2e-4 * lr + lr * (1e-4 * g.max()) * (np.sqrt(z[pre + "sum/" + k]) + eps) / (np.sqrt(want_s) + eps) ** 2
            bad = np.abs(p.cpu().numpy() - want_p) > tol
            assert not bad.any(), (k, int(bad.sum()), float(np.abs(p.cpu().numpy() - want_p).max()))
            close_to_largest(s, want_s, 2e-4, k + " accumulator")


def _run_step(z, steps=2, loss="bce"):
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    e, r = slots(z, sub(z, "init/"))
    st = LSTMTrainStep(e, r, scorer_of(z), lr=0.1, loss=loss)
    out = []
    for _ in range(steps):
        out.append(float(st.step(batch_of(z))[0]))
    torch.cuda.synchronize()
    return st, out


def test_bit_reproducible(okge_lib):
    """two runs on the same inputs: identical losses, tables, LSTM tensors, accumulators, running statistics"""
    z = golden("g17_lstm_distmult_bn_shared")
    a, la = _run_step(z)
    b, lb = _run_step(z)
    assert la == lb
    for x, y in zip(a.state_tensors(), b.state_tensors()):
        assert torch.equal(x, y)


def test_padding_row_gets_no_gradient(okge_lib):
    """token row 0 is read as stored (padding positions step through the LSTM) but never receives a gradient"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden("g17_lstm_complex_bn_all")
    e, r = slots(z, sub(z, "init/"))
    assert (dev(z["ent_tokens"]) == 0).any()
    st = LSTMTrainStep(e, r, "complex")
    st.forward_backward(batch_of(z))
    torch.cuda.synchronize()
    assert not e.dW[0].any() and not r.dW[0].any()
    assert e.dW[1:].abs().sum() > 0


def test_precompute_is_chunk_independent(okge_lib, monkeypatch):
    from open_knowledge_graph_embeddings_amd import lstm as LM
    z = golden("g17_lstm_distmult_bn_shared")
    m = build(z).cuda()
    m.eval()
    m.precompute_embeddings_from_tokens()
    E1, R1 = m.entity_embedding_from_tokens.clone(), m.relations_embedding_from_tokens.clone()
    monkeypatch.setattr(LM, "PRECOMPUTE_CHUNK", 7)
    m.train()
    m.eval()
    m.precompute_embeddings_from_tokens()
    assert torch.equal(E1, m.entity_embedding_from_tokens) and torch.equal(R1, m.relations_embedding_from_tokens)


def test_addloss_with_torch_optimizer_equals_own_optimizer(okge_lib):
    """three steps: AddLossModule + a torch optimizer over model.parameters() (the reference Trainer's statements) and
    LSTMTrainStep's own dense Adagrad land on the same parameters"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden("g17_lstm_adagrad")
    m1, m2 = build(z).cuda(), build(z).cuda()
    m1.train()
    m2.train()
    mod = AddLossModule(m1, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    opt = OkgeAdagrad(torch.optim.Adam(m1.parameters(), lr=0).param_groups)          # as OptimRegime.adjust does
    for grp in opt.param_groups:
        grp["lr"], grp["weight_decay"] = 0.1, 1e-10
    st = m2.train_step(lr=0.1, weight_decay=1e-10, eps=float(opt.param_groups[0]["eps"]))
    for s in range(3):
        B, N = z[f"s{s}_labels"].shape
        inputs = [(dev(z[f"s{s}_po_rel"]), dev(z[f"s{s}_po_obj"])), (dev(z[f"s{s}_sp_subj"]), dev(z[f"s{s}_sp_rel"]))]
        opt.zero_grad()
        loss, _, _ = mod(inputs=inputs, labels=dev(z[f"s{s}_labels"]), use_batch_shared_entities=True,
                         batch_shared_entities=dev(z[f"s{s}_cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (loss.sum() / float(B * N)).backward()
        opt.step()
        l2 = st.step(batch_of(z, f"s{s}_"), normalizer=float(B * N))
        assert abs(float(loss.detach()) - float(l2[0])) <= 1e-6 * abs(float(l2[0]))
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        np.testing.assert_allclose(p1.detach().cpu().numpy(), p2.detach().cpu().numpy(), rtol=0, atol=1e-5, err_msg=k)


def test_kl_loss_runs(okge_lib):
    z = golden("g17_lstm_complex_none_shared")
    st, losses = _run_step(z, steps=2, loss="kl")
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert torch.isfinite(st.entity.W).all() and torch.isfinite(st.entity.flat).all()


def test_no_torch_lstm_on_the_product_path(okge_lib, monkeypatch):
    """with torch's LSTM (MIOpen) made to raise: a training step, an AddLossModule call, a grad-enabled encode_subj with its
    backward, and the precompute all run"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule

    def no_lstm(*a, **k):
        raise AssertionError("torch LSTM called on the product path")
    monkeypatch.setattr(torch._VF, "lstm", no_lstm)
    z = golden("g17_lstm_complex_bn_all")
    _run_step(z, steps=1)
    m = build(z).cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    inputs = [(dev(z["po_rel"]), dev(z["po_obj"])), (dev(z["sp_subj"]), dev(z["sp_rel"]))]
    loss, _, _ = mod(inputs=inputs, labels=dev(z["labels"]), use_batch_shared_entities=False, batch_shared_entities=dev(z["cand"]),
                     epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    loss.sum().backward()
    m.zero_grad()
    enc = m.encode_subj(dev(z["sp_subj"]))
    assert enc.requires_grad
    enc.square().sum().backward()
    assert m.entity_encoder_in.weight_hh_l0.grad.abs().sum() > 0 and m.entity_embedding.weight.grad.abs().sum() > 0
    assert not m.entity_embedding.weight.grad[0].any()
    m.eval()
    with torch.no_grad():
        m.precompute_embeddings_from_tokens()
    torch.cuda.synchronize()


def test_grad_enabled_encode_matches_autograd_of_the_reference_sequence(okge_lib):
    """encode_subj with gradients enabled (LSTMEncodeFn) against torch autograd through the reference's op sequence on the CPU"""
    z = golden("g17_lstm_distmult_bn_shared")
    m = build(z)
    ref = build(z)
    ids = torch.from_numpy(z["sp_subj"].reshape(-1).astype(np.int64))
    ref.train()
    tokens = ref.entity_token_ids[ids].long()
    last = (tokens > 0).long().sum(1) - 1
    h, _ = ref.entity_encoder_in(ref.entity_embedding(tokens))
    enc = ref.entity_batchnorm(h[torch.arange(len(ids)), last])
    w = torch.linspace(-1, 1, enc.numel()).reshape(enc.shape)
    (enc * w).sum().backward()
    m = m.cuda()
    m.train()
    mine = m.encode_subj(dev(ids.numpy().astype(np.int32))).squeeze(1)
    (mine * w.cuda()).sum().backward()
    np.testing.assert_allclose(mine.detach().cpu().numpy(), enc.detach().numpy(), rtol=1e-5, atol=1e-5)
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            assert p.grad is None or not p.grad.any(), k
            continue
        close_to_largest(p.grad, q.grad.numpy(), 1e-4, k)


# ---- at size: d = 512, max_len 10, a few thousand rows, against a float64 restatement of the reference's op sequence ----------
def _reference_sequence(W, tok, w_ih, w_hh, b_ih, b_hh, bn_w, bn_b, d_out, dtype):
    """LSTMRelationEmbedder._encode in torch-CPU at `dtype` (model.py:966-986): embedding -> LSTM -> h at last -> BatchNorm1d
    (training statistics); gradients of sum(out * d_out) -- one call over every row of `tok` (tests/lstm_reference.py)"""
    r = lstm_pass(W, tok, (w_ih, w_hh, b_ih, b_hh), [(None, 0, tok.shape[0])], bn=(bn_w, bn_b), training=True, d_out=d_out,
                  dtype=dtype)
    return [r["out"]] + [r[k] for k in GRAD_NAMES]


def test_full_size_against_float64(okge_lib):
    from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot, LstmPass
    g = torch.Generator().manual_seed(1717)
    d, L, R, vocab = 512, 10, 2048, 6000
    lens = torch.randint(1, L + 4, (R,), generator=g)
    tok = torch.zeros((R, L), dtype=torch.int32)
    for i in range(R):
        k = min(int(lens[i]), L)
        tok[i, :k] = torch.randint(1, vocab, (k,), generator=g)
    tok[5] = 0                                                   # all padding: last wraps to L - 1
    W = torch.randn(vocab, d, generator=g) * 0.3
    bound = 1.0 / np.sqrt(d)
    w_ih, w_hh = [(torch.rand(4 * d, d, generator=g) * 2 - 1) * bound for _ in range(2)]
    b_ih, b_hh = [(torch.rand(4 * d, generator=g) * 2 - 1) * bound for _ in range(2)]
    bn_w, bn_b = torch.rand(d, generator=g), torch.randn(d, generator=g) * 0.1
    d_out = torch.randn(R, d, generator=g)
    ref = _reference_sequence(W, tok, w_ih, w_hh, b_ih, b_hh, bn_w, bn_b, d_out, torch.float64)
    r32 = _reference_sequence(W, tok, w_ih, w_hh, b_ih, b_hh, bn_w, bn_b, d_out, torch.float32)
    sl = LSTMSlot(W.cuda(), tok.cuda(), [x.cuda() for x in (w_ih, w_hh, b_ih, b_hh)], (bn_w.cuda(), bn_b.cuda()),
                  (torch.zeros(d, device="cuda"), torch.ones(d, device="cuda")))
    ps = LstmPass("cuda")
    ids = torch.arange(R, dtype=torch.int32, device="cuda")
    raw, out = torch.empty((R, d), device="cuda"), torch.empty((R, d), device="cuda")
    ps.encode(sl, [(ids, 0, R)], True, raw, out)
    dW, dl, d_bn = torch.zeros_like(sl.W), [torch.empty_like(x) for x in sl.lstm], torch.empty(2 * d, device="cuda")
    ps.backward(sl, [(ids, 0, R)], raw, d_out.cuda(), dW, dl, d_bn)
    torch.cuda.synchronize()
    mine = [out, dW] + dl + [d_bn[:d], d_bn[d:]]
    names = ["out", "dW", "dW_ih", "dW_hh", "db_ih", "db_hh", "d_bn_weight", "d_bn_bias"]
    for name, x, want, w32 in zip(names, mine, ref, r32):
        band_check(name, x, want, w32, min_band=None)          # the plain quantile bands, factors 3 (max) and 1.6 (rms)
    assert not dW[0].any()
