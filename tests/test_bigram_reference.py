"""tests/bigram_reference.py pinned on the CPU: to torch autograd through the reference's module composition
(nn.Embedding -> nn.Conv1d(d, d, 2, bias=False) -> nn.BatchNorm1d(d, momentum=None) -> residual, mask, pool), and to the
reference's own BigramPooling models run through the id -> token shim (tests/golden/g19_bigram_*.npz)."""
import numpy as np
import pytest
import torch

from bigram_reference import bigram_pass, encode
from conftest import golden, golden_names

CASES = [n for n in golden_names("g19_bigram_") if n != "g19_bigram_adagrad"]
SIDES = ("entity", "relation")


def _module_sequence(emb, conv, bn, tokens, pool, normalize):
    """BigramPoolingRelationEmbedder._encode (model.py:874-897, gates False) on a token matrix, statement by statement"""
    mask = (tokens > 0).unsqueeze(1).to(emb.weight.dtype)[:, :, 1:]
    embedded = emb(tokens).transpose(1, 2)
    encoded = conv(embedded)
    if bn is not None:
        encoded = bn(encoded)
    encoded = encoded + embedded[:, :, 1:]
    if pool == 'max':
        encoded, _ = (encoded * mask).max(dim=2)
    else:
        encoded = (encoded * mask).sum(dim=2)
    if normalize == 'mean':
        encoded = encoded / (mask.sum(2) + 1e-12)
    return encoded


@pytest.mark.parametrize("pool,normalize", [("sum", "batchnorm"), ("max", "batchnorm"), ("max", "mean"), ("sum", ""), ("max", "")])
def test_restatement_equals_autograd_through_the_module_composition(pool, normalize):
    g = torch.Generator().manual_seed(19)
    d, L, vocab, n_ids = 12, 6, 30, 50
    tok = torch.randint(1, vocab, (n_ids, L), generator=g, dtype=torch.int32)
    lens = torch.randint(0, L + 2, (n_ids,), generator=g)
    tok[torch.arange(L)[None, :] >= lens[:, None]] = 0
    tok[7, 2] = 0                                                     # a 0 token inside a row
    emb = torch.nn.Embedding(vocab, d, padding_idx=0).double()
    conv = torch.nn.Conv1d(d, d, kernel_size=2, bias=False).double()
    bn = torch.nn.BatchNorm1d(d, momentum=None).double() if normalize == "batchnorm" else None
    with torch.no_grad():
        emb.weight.copy_(torch.randn(vocab, d, generator=g) * 0.3)      # row 0 non-zero, as after normal_
        if bn is not None:
            bn.weight.copy_(torch.rand(d, generator=g))
            bn.bias.copy_(torch.randn(d, generator=g) * 0.1)
    calls = [(torch.randint(0, n_ids, (9,), generator=g, dtype=torch.int32), 0, 9), (None, 3, 20), (None, 30, 4)]
    d_out = torch.randn(33, d, generator=g).double()
    outs = []
    for ids, first, n in calls:
        rows = torch.arange(first, first + n) if ids is None else ids.long()
        outs.append(_module_sequence(emb, conv, bn, tok[rows].long(), pool, normalize))
    want = torch.cat(outs)
    (want * d_out).sum().backward()
    got = bigram_pass(emb.weight, tok, conv.weight, calls, pool, normalize, None if bn is None else (bn.weight, bn.bias),
                      d_out=d_out)
    np.testing.assert_allclose(got["out"], want.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["dW"], emb.weight.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["d_conv"], conv.weight.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert not got["dW"][0].any()
    if bn is not None:
        np.testing.assert_allclose(got["d_bn_weight"], bn.weight.grad.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(got["d_bn_bias"], bn.bias.grad.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(got["running_mean"], bn.running_mean.numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["running_var"], bn.running_var.numpy(), rtol=1e-12, atol=1e-14)
        assert got["num_batches_tracked"] == int(bn.num_batches_tracked) == 3
        # eval mode on the statistics the training pass left, counter and statistics unchanged
        bn.eval()
        with torch.no_grad():
            want_eval = _module_sequence(emb, conv, bn, tok[3:23].long(), pool, normalize)
        ev = bigram_pass(emb.weight, tok, conv.weight, [(None, 3, 20)], pool, normalize, (bn.weight, bn.bias),
                         running=(bn.running_mean, bn.running_var), counter=3, training=False)
        np.testing.assert_allclose(ev["out"], want_eval.numpy(), rtol=1e-12, atol=1e-12)
        assert ev["num_batches_tracked"] == 3
        np.testing.assert_array_equal(ev["running_mean"], bn.running_mean.numpy())


def test_dead_rows_encode_to_zero_and_padding_pairs_enter_the_statistics():
    """a row with no live bigram encodes to exact 0 under every pool; under batch-norm the (pad, pad) positions of a call are
    part of its statistics: dropping them changes the running mean"""
    g = torch.Generator().manual_seed(3)
    d, L, vocab = 8, 5, 20
    tok = torch.zeros((6, L), dtype=torch.int32)
    tok[0, :1] = 5                                                    # length 1
    tok[2, :4] = torch.tensor([3, 4, 5, 6], dtype=torch.int32)
    tok[3, :3] = torch.tensor([7, 8, 9], dtype=torch.int32)
    W, conv = torch.randn(vocab, d, generator=g), torch.randn(d, d, 2, generator=g) * 0.3
    for pool in ("sum", "max"):
        for normalize in ("", "mean", "batchnorm"):
            r = bigram_pass(W, tok, conv, [(None, 0, 6)], pool, normalize, (torch.ones(d), torch.zeros(d)))
            assert not r["out"][[0, 1, 4, 5]].any() and r["out"][[2, 3]].any()
    r = bigram_pass(W, tok, conv, [(None, 0, 6)], "sum", "batchnorm", (torch.ones(d), torch.zeros(d)))
    live = (tok[:, 1:] > 0).numpy()
    assert not np.allclose(r["running_mean"], r["Y"][live].mean(0))
    np.testing.assert_allclose(r["running_mean"], r["Y"].reshape(-1, d).mean(0), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["running_var"], r["Y"].reshape(-1, d).var(0, ddof=1), rtol=1e-12, atol=1e-14)


# ---- the g19 fixtures: the restatement + the scorer and loss in torch ---------------------------------------------------
def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _leaves(z, prefix="init/"):
    """side -> [W, conv, (bn weight, bn bias)] float64 leaves, in named_parameters order per side"""
    out = {}
    for side in SIDES:
        ps = [_t(z[f"{prefix}{side}_embedding.weight"]), _t(z[f"{prefix}{side}_encoder_in.0.weight"])]
        if f"{prefix}{side}_batchnorm.weight" in z.files:
            ps += [_t(z[f"{prefix}{side}_batchnorm.weight"]), _t(z[f"{prefix}{side}_batchnorm.bias"])]
        out[side] = [p.requires_grad_(True) for p in ps]
    return out


def _scores(scorer, ent, rel, cand, sp):
    if scorer == "distmult":
        return (ent * rel) @ cand.t()
    h = ent.shape[1] // 2
    e1, e2, r1, r2 = ent[:, :h], ent[:, h:], rel[:, :h], rel[:, h:]
    q = torch.cat([e1 * r1 - e2 * r2, e2 * r1 + e1 * r2], 1) if sp else torch.cat([e1 * r1 + e2 * r2, e2 * r1 - e1 * r2], 1)
    return q @ cand.t()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_training_step_and_eval_tables(name):
    """float64 restatement of the five encode calls in the reference's order + scorer + summed BCE: loss, outputs, every
    parameter gradient, running statistics and counters of the fixture; then the eval-mode tables"""
    z = golden(name)
    pool, normalize = str(z["pool"]), str(z["normalize"])
    scorer = "complex" if "Complex" in str(z["model"]) else "distmult"
    lv = _leaves(z)
    tok = {"entity": torch.from_numpy(z["ent_tokens"]), "relation": torch.from_numpy(z["rel_tokens"])}
    d = int(z["d"])
    run = {s: [torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)] for s in SIDES}
    counter = {s: 0 for s in SIDES}

    def enc(side, ids):
        p = lv[side]
        out, _, counter[side] = encode(p[0], tok[side], p[1], [(torch.from_numpy(ids.reshape(-1)), 0, ids.size)], pool, normalize,
                                       p[2:] or None, run[side], counter[side], True)
        return out
    has_sp = "sp_subj" in z.files
    C = enc("entity", z["cand"])
    r_po, o = enc("relation", z["po_rel"]), enc("entity", z["po_obj"])
    outs = [_scores(scorer, o, r_po, C, sp=False)]
    if has_sp:
        s, r_sp = enc("entity", z["sp_subj"]), enc("relation", z["sp_rel"])
        outs.append(_scores(scorer, s, r_sp, C, sp=True))
    outputs = torch.cat(outs)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(outputs, _t(z["labels"]), reduction="sum")
    (loss / float(z["normalizer"])).backward()
    err = np.abs(outputs.detach().numpy() - z["outputs"]) / (1e-5 + 1e-5 * np.abs(z["outputs"]))
    print(f"FIXTURE {name} reference fp32 error of the outputs / (atol 1e-5 + rtol 1e-5): {err.max():.3f}")
    assert err.max() <= 0.5            # the fixture leaves the GPU parity test half of its tolerance (make_golden_bigram.py)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    for side in SIDES:
        names = [f"{side}_embedding.weight", f"{side}_encoder_in.0.weight", f"{side}_batchnorm.weight", f"{side}_batchnorm.bias"]
        for k, p in zip(names, lv[side]):
            g = p.grad.clone()
            if k.endswith("embedding.weight"):
                g[0] = 0
            want = z["grad/" + k]
            np.testing.assert_allclose(g.numpy(), want, rtol=0, atol=1e-4 * max(np.abs(want).max(), 1e-30), err_msg=k)
        if normalize == "batchnorm":
            np.testing.assert_allclose(run[side][0].numpy(), z[f"buf/{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(run[side][1].numpy(), z[f"buf/{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6)
            assert counter[side] == int(z[f"buf/{side}_batchnorm.num_batches_tracked"])
    # eval: every row of the token matrices on the running statistics
    for side, key in (("entity", "E_eval"), ("relation", "R_eval")):
        p = [x.detach() for x in lv[side]]
        r = bigram_pass(p[0], tok[side], p[1], [(None, 0, tok[side].shape[0])], pool, normalize, p[2:] or None,
                        running=run[side] if normalize == "batchnorm" else None, counter=counter[side], training=False)
        np.testing.assert_allclose(r["out"], z[key], rtol=1e-5, atol=1e-5)


def test_fixture_counters_advance_three_and_two_per_step():
    """one count per _encode call: a training step moves the entity counter by 3 and the relation counter by 2"""
    z = golden("g19_bigram_adagrad")
    for step in range(3):
        assert int(z[f"s{step}_after/buf/entity_batchnorm.num_batches_tracked"]) == 3 * (step + 1)
        assert int(z[f"s{step}_after/buf/relation_batchnorm.num_batches_tracked"]) == 2 * (step + 1)
    z = golden("g19_bigram_complex_bn_max_po_only")
    assert int(z["buf/entity_batchnorm.num_batches_tracked"]) == 2 and int(z["buf/relation_batchnorm.num_batches_tracked"]) == 1
