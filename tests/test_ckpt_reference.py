"""Checkpoints of the token-encoded and Tucker3 models against the reference's own (tests/golden/g22_ckpt_*.npz): the dict its
`Trainer.save` held after two steps is loaded and step three run on the GPU; and a checkpoint this package wrote is handed to
torch's optimizers and compared, key for key, with the reference's layout.

THE BOUNDS of step three are those the models' golden tests put on one training step restarted from the reference's state --
test_lstm_parity.test_adagrad_steps_restarted_from_reference_state (G17), which test_tucker3_parity (G18), test_bigram_parity
(G19) and test_databias_parity repeat word for word:
    loss               1e-5 relative
    parameters         2e-4 of lr, plus what a gradient error of `bar` x the tensor's largest gradient does to the update
                       lr g / (sqrt(sum) + eps):  lr (bar g_max) (sqrt(sum_before) + eps) / (sqrt(sum_after) + eps)^2
    accumulators       2e-4 of the tensor's largest (close_to_largest, imported from test_lstm_parity)
    running statistics rtol 1e-5, atol 1e-6;  counters, `step` entries, parameters no gradient reaches: exact
with bar = 1e-4, the bar of those files' gradient tests.  The rule is written inline there, so `adagrad_tolerance` restates it.
The token-pooled model's golden step test (test_token_pooled.test_train_forward_backward_matches_reference, G9) sets the loss
at 3e-5 and the gradients at bar = 5e-5: the same rule with that bar, and 2 bar = 1e-4 of the largest for the accumulators (sum
grows by g^2; an error e in g changes it by 2 g e <= 2 bar g_max^2).
Under Adam no golden test exists; the same reasoning on torch.optim.Adam's update u = lr m^ / (sqrt(v^) + eps) gives
    |du/dg| <= lr [ c1 / (sqrt(v^) + eps)  +  |m^| c2 |g| / (sqrt(v^) (sqrt(v^) + eps)^2) ],  c1 = (1-b1)/(1-b1^t), c2 = (1-b2)/(1-b2^t)
    parameters 2e-4 lr + |du/dg| bar g_max;   exp_avg (1-b1) bar g_max;   exp_avg_sq 2 (1-b2) bar g_max^2  (+ 4 fp32 ulps of the largest)
with g read back from the fixture's moments, g = (m_after - b1 m_before) / (1 - b1)."""
import numpy as np
import pytest
import torch

from ckpt_cases import KINDS, build, fixture, fixture_batch, fixture_checkpoint, fixture_layout, flat, layout
from test_lstm_parity import close_to_largest

pytestmark = pytest.mark.gpu

RUNS = [(k, "") for k in KINDS] + [("unigram", "adam_"), ("lstm", "adam_")]
BAR = {"unigram": (5e-5, 3e-5, 1e-4)}          # kind -> (gradient bar, loss, accumulators); every other kind: G17's
G17 = (1e-4, 1e-5, 2e-4)
ULP = float(np.finfo(np.float32).eps)


def adagrad_tolerance(lr, eps, bar, sum_before, sum_after):
    g = np.sqrt(np.maximum(sum_after - sum_before, 0))
    return 2e-4 * lr + lr * (bar * g.max()) * (np.sqrt(sum_before) + eps) / (np.sqrt(sum_after) + eps) ** 2


def adam_tolerances(lr, eps, betas, t, bar, m0, m1, v1):
    """-> (parameters, exp_avg, exp_avg_sq): see the module docstring"""
    b1, b2 = betas
    g = (m1.astype(np.float64) - b1 * m0) / (1 - b1)
    g_max = np.abs(g).max()
    c1, c2 = (1 - b1) / (1 - b1 ** t), (1 - b2) / (1 - b2 ** t)
    m_hat, rv = m1 / (1 - b1 ** t), np.sqrt(v1 / (1 - b2 ** t))
    second = np.where(rv > 0, np.abs(m_hat) * c2 * np.abs(g) / (np.maximum(rv, 1e-300) * (rv + eps) ** 2), 0.0)
    slope = lr * (c1 / (rv + eps) + second)
    return (2e-4 * lr + slope * bar * g_max, (1 - b1) * bar * g_max + 4 * ULP * np.abs(m1).max(),
            2 * (1 - b2) * bar * g_max ** 2 + 4 * ULP * np.abs(v1).max())


def module_at(kind, z, prefix="sd0/"):
    m = build(kind)
    m.load_state_dict({k: torch.tensor(z[prefix + k]) for k in m.state_dict()})
    m = m.cuda()
    m.train()
    return m


@pytest.mark.parametrize("kind,run", RUNS)
def test_step_three_from_the_references_checkpoint(okge_lib, kind, run):
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, model_checkpoint
    z = fixture(kind)
    bar, loss_tol, acc_tol = BAR.get(kind, G17)
    before = fixture_checkpoint(z, run)
    group = before["optimizer_state_dict"][0]["optimizer_state"]["param_groups"][0]
    adam = run == "adam_"
    m = module_at(kind, z)
    st = m.train_step(optimizer="adam" if adam else "adagrad")                  # (lr, weight decay, eps, betas: the file's)
    load_model_checkpoint(m, st, before)
    lr, eps = float(group["lr"]), float(group["eps"])
    assert (st.lr, st.weight_decay, st.eps, st.steps) == (lr, float(group["weight_decay"]), eps, 2)
    assert lr == (0.01 if adam else 0.3) and "okge" not in before
    B, N = z["s2_labels"].shape
    loss = float(st.step(fixture_batch(z, 2), normalizer=float(B * N))[0])
    want_loss = float(z[run + "s2_loss"])
    print(kind, run, "loss", loss, want_loss)
    assert abs(loss - want_loss) <= loss_tol * abs(want_loss)
    got = dict(flat(model_checkpoint(m, st)))
    want = dict(flat(fixture_checkpoint(z, run, "end")))
    old = dict(flat(before))
    assert list(got) == list(want)
    moved = {i for i, (_, _, mv) in enumerate(m.optimizer_params_and_state(st)[0]) if mv}
    names = list(m.state_dict())
    number = {id(p): i for i, p in enumerate(m.parameters())}
    # state_dict key -> index of its parameter (the bigram model lists its batch-norm's parameters under two keys)
    params = {k: number[id(v)] for k, v in m.state_dict(keep_vars=True).items() if id(v) in number}
    for path, w in want.items():
        x, w = got[path].numpy(), w.numpy()
        head, _, key = path.partition("/")
        if head == "optimizer":
            i, _, name = key.partition("/")
            i = int(i)
            if name == "step" or i not in moved:
                assert np.array_equal(x, w), path
            elif name == "sum":
                close_to_largest(x, w, acc_tol, path)
            else:
                m0, m1, v1 = (s[f"optimizer/{i}/{n}"].numpy() for s, n in ((old, "exp_avg"), (want, "exp_avg"), (want, "exp_avg_sq")))
                tol = adam_tolerances(lr, eps, group["betas"], 3, bar, m0, m1, v1)[1 if name == "exp_avg" else 2]
                assert np.abs(x - w).max() <= tol, (path, float(np.abs(x - w).max()), float(tol))
        elif key in params:
            i = params[key]
            if i not in moved:
                assert np.array_equal(x, w) and np.array_equal(w, old[path].numpy()), path
                continue
            if adam:
                m0, m1, v1 = (s[f"optimizer/{i}/{n}"].numpy() for s, n in ((old, "exp_avg"), (want, "exp_avg"), (want, "exp_avg_sq")))
                tol = adam_tolerances(lr, eps, group["betas"], 3, bar, m0, m1, v1)[0]
            else:
                tol = adagrad_tolerance(lr, eps, bar, old[f"optimizer/{i}/sum"].numpy(), want[f"optimizer/{i}/sum"].numpy())
            err = np.abs(x - w)
            print(path, "max error", float(err.max()), "largest share of its bound", float((err / tol).max()))
            assert not (err > tol).any(), (path, int((err > tol).sum()), float(err.max()))
        elif "running" in key:
            np.testing.assert_allclose(x, w, rtol=1e-5, atol=1e-6, err_msg=path)
        else:                                                      # token ids, num_batches_tracked
            assert key in names and np.array_equal(x, w), path


@pytest.mark.parametrize("kind,run", RUNS)
def test_written_checkpoint_has_the_references_layout_and_loads_into_torch(okge_lib, kind, run):
    from open_knowledge_graph_embeddings_amd.checkpoint import model_checkpoint
    z = fixture(kind)
    ref = fixture_checkpoint(z, run)
    group = ref["optimizer_state_dict"][0]["optimizer_state"]["param_groups"][0]
    adam = run == "adam_"
    m = module_at(kind, z)
    st = m.train_step(lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], optimizer="adam" if adam else "adagrad")
    for s in range(2):
        B, N = z[f"s{s}_labels"].shape
        st.step(fixture_batch(z, s), normalizer=float(B * N))
    ckpt = model_checkpoint(m, st, epoch=1)
    assert list(ckpt) == list(ref) + ["okge"]
    assert layout(flat(ckpt)) == fixture_layout(z, run)
    mine = ckpt["optimizer_state_dict"][0]
    assert list(mine["optimizer_state"]["param_groups"][0].items()) == [(k, tuple(v) if k == "betas" else v) for k, v in group.items()]
    assert mine["regime"] == ref["optimizer_state_dict"][0]["regime"] and len(ckpt["optimizer_state_dict"]) == 1
    assert (ckpt["epoch"], ckpt["training_steps"]) == (ref["epoch"], ref["training_steps"])
    for path, w in flat(ref):                                       # counters and steps: the reference's after the same batches
        if path.endswith(("num_batches_tracked", "/step", "token_ids")):
            assert torch.equal(dict(flat(ckpt))[path], w), path
    opt = (torch.optim.Adam if adam else torch.optim.Adagrad)(m.parameters(), lr=1.0)
    opt.load_state_dict(mine["optimizer_state"])
    assert opt.param_groups[0]["lr"] == group["lr"]
    entries, word = m.optimizer_params_and_state(st)
    for p, views, moved in entries:
        held = opt.state.get(p, {})
        if adam and not moved:
            assert not held
            continue
        assert float(held["step"]) == (2.0 if moved else 0.0)
        for name, v in zip(("exp_avg", "exp_avg_sq") if adam else ("sum",), views):
            assert held[name].shape == p.shape and torch.equal(held[name], v), name
            assert held[name].data_ptr() != v.data_ptr()           # a copy: torch's optimizer never steps the driver's buffers
    assert (int(word[0]) == 2) if adam else (word is None)
