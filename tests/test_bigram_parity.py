"""Bigram-pooling models (csrc/okge_bigram.hip: the pair product on the exact-fp32 MFMA, forward and backward) on the GPU
against the reference's own BigramPooling models run through the id -> token shim (tests/golden/g19_bigram_*.npz; the shim
is described in tests/golden/make_golden_bigram.py), at the tolerances test_lstm_parity.py uses for g17, and for the
properties the kernels promise: bit-reproducible runs, no gradient for the padding row, chunk-independent precompute, no
torch convolution or batch-norm on the product path."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from test_bigram_api import build

pytestmark = pytest.mark.gpu

CASES = [n for n in golden_names("g19_bigram_") if n != "g19_bigram_adagrad"]
SIDES = ("entity", "relation")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def slots(z, params, bufs=None, sums=None):
    """BigramSlot pair from name -> array maps (fixture layout); sums: Adagrad accumulators by parameter name"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramSlot
    out = []
    for side, tok in zip(SIDES, ("ent_tokens", "rel_tokens")):
        bn = running = nbt = None
        if f"{side}_batchnorm.weight" in params:
            bn = (dev(params[f"{side}_batchnorm.weight"]), dev(params[f"{side}_batchnorm.bias"]))
            if bufs:
                running = (dev(bufs[f"{side}_batchnorm.running_mean"]).clone(), dev(bufs[f"{side}_batchnorm.running_var"]).clone())
                nbt = dev(bufs[f"{side}_batchnorm.num_batches_tracked"]).to(torch.int64).clone()
        s = BigramSlot(dev(params[f"{side}_embedding.weight"]).clone(), dev(z[tok]), dev(params[f"{side}_encoder_in.0.weight"]),
                       str(z["pool"]), str(z["normalize"]), bn, running, nbt)
        if sums is not None:
            s.sumW.copy_(dev(sums[f"{side}_embedding.weight"]))
            parts = [dev(sums[f"{side}_encoder_in.0.weight"]).reshape(-1)]
            if bn is not None:
                parts += [dev(sums[f"{side}_batchnorm.weight"]), dev(sums[f"{side}_batchnorm.bias"])]
            s.sum_flat.copy_(torch.cat(parts))
        out.append(s)
    return out


def sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def batch_of(z, pre=""):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    b = PrefixBatch()
    b.po_rel, b.po_obj = dev(z[pre + "po_rel"].reshape(-1)), dev(z[pre + "po_obj"].reshape(-1))
    if pre + "sp_subj" in z.files:
        b.sp_subj, b.sp_rel = dev(z[pre + "sp_subj"].reshape(-1)), dev(z[pre + "sp_rel"].reshape(-1))
    b.cand_ids = dev(z[pre + "cand"].reshape(-1).astype(np.int32))
    b.pos_row, b.pos_col = positives_from_dense(dev(z[pre + "labels"]))
    return b


def grads_of(st):
    """fixture names -> this step's gradients"""
    g = {}
    for side, sl in zip(SIDES, (st.entity, st.relation)):
        g[f"{side}_embedding.weight"] = sl.dW
        g[f"{side}_encoder_in.0.weight"] = sl.d_conv
        if sl.bn is not None:
            g[f"{side}_batchnorm.weight"], g[f"{side}_batchnorm.bias"] = sl.d_bn[:sl.d], sl.d_bn[sl.d:]
    return g


def close_to_largest(got, want, frac, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    np.testing.assert_allclose(got, want, rtol=0, atol=frac * max(np.abs(want).max(), 1e-30), err_msg=what)


def scorer_of(z):
    return "complex" if "Complex" in str(z["model"]) else "distmult"


def check_running(z, side, sl, prefix="buf/"):
    np.testing.assert_allclose(sl.running_mean.cpu().numpy(), z[f"{prefix}{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sl.running_var.cpu().numpy(), z[f"{prefix}{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6)
    assert int(sl.num_batches_tracked) == int(z[f"{prefix}{side}_batchnorm.num_batches_tracked"])


@pytest.mark.parametrize("name", CASES)
def test_train_step_matches_reference(okge_lib, name):
    """BigramTrainStep.forward_backward: loss, outputs, every parameter's gradient, running statistics and counters"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    z = golden(name)
    e, r = slots(z, sub(z, "init/"))
    st = BigramTrainStep(e, r, scorer_of(z), lr=0.1)
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
            check_running(z, side, sl)


@pytest.mark.parametrize("name", CASES)
def test_module_addloss_and_eval_match_reference(okge_lib, name):
    """the reference Trainer's statements on the seeded module: AddLossModule forward + backward (gradients in .grad), then
    eval mode: precompute_embeddings_from_tokens tables (running statistics) and the prefix scores"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden(name)
    m = build(z).cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    has_sp = "sp_subj" in z.files
    inputs = [(dev(z["po_rel"]), dev(z["po_obj"])), (dev(z["sp_subj"]), dev(z["sp_rel"])) if has_sp else None]
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
        if "num_batches_tracked" in k:
            assert int(b) == int(z["buf/" + k])
    m.eval()
    with torch.no_grad():
        m.precompute_embeddings_from_tokens()
        np.testing.assert_allclose(m.entity_embedding_from_tokens.cpu().numpy(), z["E_eval"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(m.relations_embedding_from_tokens.cpu().numpy(), z["R_eval"], rtol=1e-5, atol=1e-5)
        assert m.get_all_rel().shape[0] == int(z["n_rel"]) - 2          # the reference's slice by min_entities_size
        po = m.po_prefix_score(dev(z["po_rel"]), dev(z["po_obj"]))
        np.testing.assert_allclose(po.cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)
        if has_sp:
            sp = m.sp_prefix_score(dev(z["sp_subj"]), dev(z["sp_rel"]))
            np.testing.assert_allclose(sp.cpu().numpy(), z["sp_all_eval"], rtol=1e-5, atol=1e-5)
    for k, b in m.named_buffers():                                      # eval mode leaves the statistics alone
        if "num_batches_tracked" in k:
            assert int(b) == int(z["buf/" + k])


def _state(sl, side):
    got = {f"{side}_embedding.weight": (sl.W, sl.sumW)}
    dd = 2 * sl.d * sl.d
    got[f"{side}_encoder_in.0.weight"] = (sl.conv, sl.sum_flat[:dd].view_as(sl.conv))
    if sl.bn is not None:
        got[f"{side}_batchnorm.weight"] = (sl.bn[:sl.d], sl.sum_flat[dd:dd + sl.d])
        got[f"{side}_batchnorm.bias"] = (sl.bn[sl.d:], sl.sum_flat[dd + sl.d:])
    return got


@pytest.mark.parametrize("step", [0, 1, 2])
def test_adagrad_steps_restarted_from_reference_state(okge_lib, step):
    """each of the reference's three OptimRegime Adagrad steps, restarted from the reference's state before it: parameters,
    accumulators, running statistics and counters after it"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    z = golden("g19_bigram_adagrad")
    pre = f"s{step}_before/"
    e, r = slots(z, sub(z, pre + "param/"), bufs=sub(z, pre + "buf/"), sums=sub(z, pre + "sum/"))
    st = BigramTrainStep(e, r, "complex", lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]), eps=float(z["opt_eps"]))
    B, N = z[f"s{step}_labels"].shape
    loss = st.step(batch_of(z, f"s{step}_"), normalizer=float(B * N))
    assert abs(float(loss[0]) - float(z[f"s{step}_loss"])) <= 1e-5 * abs(float(z[f"s{step}_loss"]))
    post = f"s{step}_after/"
    for side, sl in zip(SIDES, (e, r)):
        check_running(z, side, sl, post + "buf/")
        lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
        for k, (p, s) in _state(sl, side).items():
            want_p, want_s = z[post + "param/" + k], z[post + "sum/" + k]
            # test_lstm_parity.py's accumulator rule: an Adagrad step moves a parameter by lr g / (sqrt(sum) + eps), at most lr:
            # 2e-4 of lr, plus what a gradient error of 1e-4 of the tensor's largest gradient (the bar of the gradient tests)
            # does to that quotient -- it matters only where g is tiny and the accumulator holds little more than g^2
            g = np.sqrt(want_s - z[pre + "sum/" + k])
            tol = 2e-4 * lr + lr * (1e-4 * g.max()) * (np.sqrt(z[pre + "sum/" + k]) + eps) / (np.sqrt(want_s) + eps) ** 2
            bad = np.abs(p.cpu().numpy() - want_p) > tol
            assert not bad.any(), (k, int(bad.sum()), float(np.abs(p.cpu().numpy() - want_p).max()))
            close_to_largest(s, want_s, 2e-4, k + " accumulator")


def _run_step(z, steps=2, loss="bce"):
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    e, r = slots(z, sub(z, "init/"))
    st = BigramTrainStep(e, r, scorer_of(z), lr=0.1, loss=loss)
    out = []
    for _ in range(steps):
        out.append(float(st.step(batch_of(z))[0]))
    torch.cuda.synchronize()
    return st, out


@pytest.mark.parametrize("name", ["g19_bigram_complex_bn_sum_all", "g19_bigram_complex_mean_max_shared"])
def test_bit_reproducible(okge_lib, name):
    """two runs on the same inputs: identical losses, tables, conv weights, accumulators, running statistics"""
    z = golden(name)
    a, la = _run_step(z)
    b, lb = _run_step(z)
    assert la == lb
    for x, y in zip(a.state_tensors(), b.state_tensors()):
        assert torch.equal(x, y)


def test_padding_row_gets_no_gradient_but_decays(okge_lib):
    """token row 0 is read as stored and never receives a gradient; Adagrad's weight decay still moves it"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    z = golden("g19_bigram_complex_bn_sum_all")
    e, r = slots(z, sub(z, "init/"))
    assert (dev(z["ent_tokens"]) == 0).any()
    st = BigramTrainStep(e, r, "complex", weight_decay=0.1)
    row0 = e.W[0].clone()
    st.forward_backward(batch_of(z))
    torch.cuda.synchronize()
    assert not e.dW[0].any() and not r.dW[0].any()
    assert e.dW[1:].abs().sum() > 0
    st.optimizer_step()                                            # (the sweep clears the gradients it has applied)
    torch.cuda.synchronize()
    assert not torch.equal(e.W[0], row0)


def test_precompute_is_chunk_independent(okge_lib, monkeypatch):
    from open_knowledge_graph_embeddings_amd import bigram as BG
    z = golden("g19_bigram_complex_bn_sum_all")
    m = build(z).cuda()
    with torch.no_grad():
        m.entity_batchnorm.running_mean.normal_(std=0.1)
        m.entity_batchnorm.running_var.uniform_(0.5, 1.5)
    m.eval()
    m.precompute_embeddings_from_tokens()
    E1, R1 = m.entity_embedding_from_tokens.clone(), m.relations_embedding_from_tokens.clone()
    monkeypatch.setattr(BG, "PRECOMPUTE_CHUNK", 7)
    m.train()
    m.eval()
    m.precompute_embeddings_from_tokens()
    assert torch.equal(E1, m.entity_embedding_from_tokens) and torch.equal(R1, m.relations_embedding_from_tokens)


def test_addloss_with_torch_optimizer_equals_own_optimizer(okge_lib):
    """three steps: AddLossModule + a torch optimizer over model.parameters() (the reference Trainer's statements) and
    BigramTrainStep's own dense Adagrad land on the same parameters; train_step() moves the module's parameters in place"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden("g19_bigram_adagrad")
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
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        np.testing.assert_allclose(b1.cpu().numpy(), b2.cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
    assert int(m2.entity_batchnorm.num_batches_tracked) == 9 and int(m2.relation_batchnorm.num_batches_tracked) == 6


def test_kl_loss_and_dropout_run(okge_lib):
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    z = golden("g19_bigram_distmult_none_sum_shared")
    st, losses = _run_step(z, steps=2, loss="kl")
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert torch.isfinite(st.entity.W).all() and torch.isfinite(st.entity.flat).all()
    e, r = slots(z, sub(z, "init/"))
    st = BigramTrainStep(e, r, "distmult", dropout=0.3, seed=5)
    l0 = float(st.step(batch_of(z))[0])
    assert np.isfinite(l0) and abs(l0 - float(z["loss"])) > 1e-3 * abs(float(z["loss"]))       # the masks changed the rows


def test_no_torch_conv_or_batchnorm_on_the_product_path(okge_lib, monkeypatch):
    """with torch's conv1d and batch_norm made to raise: a training step, an AddLossModule call, a grad-enabled encode_subj
    with its backward, and the precompute all run"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule

    def boom(*a, **k):
        raise AssertionError("torch convolution / batch-norm called on the product path")
    monkeypatch.setattr(torch.nn.functional, "conv1d", boom)
    monkeypatch.setattr(torch.nn.functional, "batch_norm", boom)
    monkeypatch.setattr(torch.nn.Conv1d, "forward", boom)
    monkeypatch.setattr(torch.nn.BatchNorm1d, "forward", boom)
    z = golden("g19_bigram_complex_bn_sum_all")
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
    assert m.entity_encoder_in[0].weight.grad.abs().sum() > 0 and m.entity_embedding.weight.grad.abs().sum() > 0
    assert not m.entity_embedding.weight.grad[0].any()
    m.eval()
    with torch.no_grad():
        m.precompute_embeddings_from_tokens()
    torch.cuda.synchronize()


def test_grad_enabled_encode_matches_autograd_of_the_reference_sequence(okge_lib):
    """encode_subj with gradients enabled (BigramEncodeFn) against torch autograd through the reference's op sequence on the
    CPU (float64 restatement, tests/bigram_reference.py)"""
    from bigram_reference import bigram_pass
    z = golden("g19_bigram_complex_bn_max_po_only")
    m = build(z)
    ids = torch.from_numpy(z["po_obj"].reshape(-1).astype(np.int32))
    w = torch.linspace(-1, 1, ids.numel() * int(z["d"])).reshape(ids.numel(), -1)
    ref = bigram_pass(m.entity_embedding.weight, m.entity_token_ids, m.entity_encoder_in[0].weight, [(ids, 0, ids.numel())],
                      "max", "batchnorm", (m.entity_batchnorm.weight, m.entity_batchnorm.bias), d_out=w)
    m = m.cuda()
    m.train()
    mine = m.encode_subj(ids.cuda()).squeeze(1)
    (mine * w.cuda()).sum().backward()
    np.testing.assert_allclose(mine.detach().cpu().numpy(), ref["out"], rtol=1e-5, atol=1e-5)
    for p, k in ((m.entity_embedding.weight, "dW"), (m.entity_encoder_in[0].weight, "d_conv"), (m.entity_batchnorm.weight, "d_bn_weight"),
                 (m.entity_batchnorm.bias, "d_bn_bias")):
        close_to_largest(p.grad, ref[k], 1e-4, k)
    assert m.relation_embedding.weight.grad is None
    assert int(m.entity_batchnorm.num_batches_tracked) == 1
