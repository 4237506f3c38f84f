"""optimizer="adam" and grad_clip on the token-encoded and Tucker3 steps (step_optim.py over okge_adam_multi and
okge_clip_grad_norm_multi), at the smallest shapes that carry every tensor kind: |E| = 40, |R| = 7, vocabularies 30 / 12, L = 4,
d = 16, B = 6 + 5, 20 candidates; Tucker3 with d = r_e = 8.

The checks are ONE STEP AHEAD, as in test_adam_step.py: after forward_backward the state the optimizer starts from -- parameters,
the gradients the device itself left, moments or accumulators, t -- is read back; the clip (clip64 / clip_coef of
tests/optim_reference.py, the coefficient formed from the step's own grad_norm) and the update (adam64 of tests/adam_reference.py,
adagrad64 of tests/optim_reference.py) are restated on exactly that, and the tensors after optimizer_step() are held to the
restatements' caps.  Errors do not compound, so no trajectory tolerance is guessed."""
import numpy as np
import pytest
import torch

import adam_reference as A
import optim_reference as R
from test_adam_step import X_BETAS, X_EPS, X_LR, X_WD, _hold

pytestmark = pytest.mark.gpu

N_ENT, N_REL, V_ENT, V_REL, L_TOK, D, N_PO, N_SP, N_CAND, D_T3 = 40, 7, 30, 12, 4, 16, 6, 5, 20, 8
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
KINDS = ("pooled-sum-bn", "pooled-max", "lstm-bn", "bigram-bn", "tucker3", "lstm-bias-entity")
REPRODUCIBLE = tuple(k for k in KINDS if k != "pooled-max")       # (max pooling scatters with float atomics)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _tokens(rng, n, vocab):
    m = np.zeros((n, L_TOK), np.int32)
    for r in range(n):
        k = int(rng.integers(1, L_TOK + 1))
        m[r, :k] = rng.integers(1, vocab, k)
    return m


def _f32(rng, *shape, scale=0.3):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def batches(n=3, seed=5):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        y = np.zeros((N_PO + N_SP, N_CAND), np.float32)
        y[np.arange(N_PO + N_SP), rng.integers(0, N_CAND, N_PO + N_SP)] = 1
        b = PrefixBatch(cand_ids=dev(rng.choice(np.arange(2, N_ENT), N_CAND, replace=False).astype(np.int32)),
                        po_rel=dev(rng.integers(1, N_REL, N_PO).astype(np.int32)), po_obj=dev(rng.integers(2, N_ENT, N_PO).astype(np.int32)),
                        sp_subj=dev(rng.integers(2, N_ENT, N_SP).astype(np.int32)), sp_rel=dev(rng.integers(1, N_REL, N_SP).astype(np.int32)))
        b.pos_row, b.pos_col = positives_from_dense(dev(y))
        out.append(b)
    return out


def make(kind, **kw):
    """a fresh step of `kind` from fixed parameters (the same bits every call)"""
    rng = np.random.default_rng(len(kind))
    kw.setdefault("lr", LR)
    sides = ((N_ENT, V_ENT), (N_REL, V_REL))
    bn = lambda: (dev(rng.random(D).astype(np.float32) + 0.5), dev(_f32(rng, D, scale=0.1)))      # noqa: E731
    if kind.startswith("pooled"):
        from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
        pool, norm = ("sum", True) if kind == "pooled-sum-bn" else ("max", False)
        slots = [TokenSlot(dev(_f32(rng, v, D)), dev(_tokens(rng, n, v)), pool, norm, *(bn() if norm else ())) for n, v in sides]
        return TokenPooledTrainStep(slots[0], slots[1], "complex", **kw)
    if kind.startswith("lstm"):
        from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot, LSTMTrainStep
        slots = []
        for n, v in sides:
            flat = dev(_f32(rng, 8 * D * D + 8 * D))
            views = [x.view(s) for x, s in zip(flat.split([4 * D * D, 4 * D * D, 4 * D, 4 * D]), ((4 * D, D), (4 * D, D), (4 * D,), (4 * D,)))]
            slots.append(LSTMSlot(dev(_f32(rng, v, D)), dev(_tokens(rng, n, v)), views, bn(),
                                  (torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")), flat=flat))
        return LSTMTrainStep(slots[0], slots[1], "bias_entity" if kind == "lstm-bias-entity" else "complex", **kw)
    if kind == "bigram-bn":
        from open_knowledge_graph_embeddings_amd.bigram import BigramSlot, BigramTrainStep
        slots = [BigramSlot(dev(_f32(rng, v, D)), dev(_tokens(rng, n, v)), dev(_f32(rng, D, D, 2)), "", "batchnorm", bn()) for n, v in sides]
        return BigramTrainStep(slots[0], slots[1], "complex", **kw)
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep
    return Tucker3TrainStep(dev(_f32(rng, N_ENT, D_T3)), dev(_f32(rng, N_REL, D_T3)), dev(_f32(rng, D_T3 * D_T3, D_T3)), **kw)


def snapshot(step):
    """host copies of every optimizer tensor (an unused slot's included): p, g, state_sum and, under Adam, exp_avg, exp_avg_sq, t"""
    torch.cuda.synchronize()
    live = {t[0].data_ptr() for t in step._param_groups()}
    out = []
    for t in step._param_groups(every=True):
        rec = dict(p=_np(t[0]), g=_np(t[1]), s=_np(t[2]), live=t[0].data_ptr() in live)
        if step.optimizer == "adam":
            m, v, st = step._adam[t[0].data_ptr()]
            rec.update(m=_np(m), v=_np(v), t=int(st[0].item()))
        out.append(rec)
    return out


def grad_norm64(pre):
    return float(np.sqrt(sum(float((r["g"].astype(np.float64) ** 2).sum()) for r in pre if r["live"])))


def binding_clip(kind):
    """a max_norm a fifth of the first batch's gradient norm (read from a probe step's own gradients): three Adam or Adagrad
    steps at these learning rates do not shrink the norm that far, and every step asserts that its coefficient is below 1"""
    probe = make(kind)
    probe.forward_backward(batches()[0])
    return 0.2 * grad_norm64(snapshot(probe))


def clipped(case, step, pre, binding):
    """the clip restated on the snapshot: grad_norm is an fp32 value within 1 fp32 ulp of fp32(sqrt(sum g^2)) at float64, the
    coefficient is clip_coef of it; -> the gradients the optimizer reads (g * coef in fp32)"""
    if step.grad_clip <= 0:
        return [r["g"] for r in pre]
    total, _ = R.clip64(np.concatenate([r["g"].ravel() for r in pre if r["live"]]), None, step.grad_clip)
    got = float(step.grad_norm.item())
    ulps = abs(got - float(total)) / float(np.spacing(total))
    print("RATIO %s grad_norm %.3f" % (case, ulps))
    assert float(np.float32(got)) == got and ulps <= 1.0, (case, got, float(total))
    coef = R.clip_coef(np.float32(got), step.grad_clip)
    print("COEF %s %.6f" % (case, coef))
    assert (coef < np.float32(1.0)) if binding else (coef == np.float32(1.0)), (case, coef)     # binding: the clip does scale
    return [(r["g"] * coef).astype(np.float32) if r["live"] else r["g"] for r in pre]


def untouched(case, pre, post, names):
    for name in names:
        assert np.array_equal(pre[name].view(np.uint32), post[name].view(np.uint32)), (case, name, "an unused slot's tensor moved")


def adam_step_ahead(case, step, batch, binding, hyper=None):
    """one forward_backward + optimizer_step with the Adam update restated on the state in between; -> (pre, clipped gradients)"""
    lr, betas, eps, wd = hyper or (step.lr, step.betas, step.eps, step.weight_decay)
    step.forward_backward(batch)
    pre = snapshot(step)
    step.optimizer_step()
    post = snapshot(step)
    gs = clipped(case, step, pre, binding)
    assert any(np.abs(r["g"]).max() > 0 for r in pre if r["live"])
    for k, (a, b, g) in enumerate(zip(pre, post, gs)):
        if not a["live"]:
            untouched(case, a, b, ("p", "m", "v", "g"))
            assert b["t"] == a["t"] == 0, (case, k, "an unused slot's t advanced")
            continue
        assert b["t"] == a["t"] + 1, (case, k, "t counts optimizer steps")
        r = A.adam64(a["p"], g, a["m"], a["v"], b["t"], lr, betas, eps, wd, exact=hyper is not None)
        _hold("%s t%d" % (case, k), [b["p"], b["m"], b["v"]], r, a["m"], a["v"])
        assert not b["g"].any(), (case, k, "gradient not cleared")
        untouched(case, a, b, ("s",))                          # the Adagrad accumulators are left alone
    return pre, gs


@pytest.mark.parametrize("clip", ["clip", "noclip"])
@pytest.mark.parametrize("kind", KINDS)
def test_adam_one_step_ahead(okge_lib, kind, clip):
    grad_clip = binding_clip(kind) if clip == "clip" else 0.0
    step = make(kind, optimizer="adam", betas=BETAS, eps=EPS, weight_decay=1e-2 if kind != "pooled-max" else 0.0, grad_clip=grad_clip)
    for k, b in enumerate(batches()):
        adam_step_ahead("%s-%s step%d" % (kind, clip, k), step, b, clip == "clip")
    assert step.adam_t == 3
    if kind == "lstm-bias-entity":
        assert all(int(st[0].item()) == 0 for *_, st in step.adam_tensors(every=True)[3:])


def adagrad_step_ahead(case, step, batch, binding):
    step.forward_backward(batch)
    pre = snapshot(step)
    step.optimizer_step()
    post = snapshot(step)
    gs = clipped(case, step, pre, binding)
    for k, (a, b, g) in enumerate(zip(pre, post, gs)):
        if not a["live"]:
            untouched(case, a, b, ("p", "s", "g"))
            continue
        p1, s1, delta = R.adagrad64(a["p"], g, a["s"], step.lr, step.weight_decay, step.eps)
        ok = ~R.underflowed(s1)
        assert (~ok).sum() <= 8, (case, k, int((~ok).sum()))
        ratios = R.cap_ratios(b["p"][ok], b["s"][ok], p1[ok], s1[ok], delta[ok])
        print("RATIO %s t%d p %.3f s %.3f" % (case, k, *ratios))
        assert np.isfinite(b["p"]).all() and max(ratios) <= 1.0, (case, k, ratios)
        assert not b["g"].any(), (case, k, "gradient not cleared")


@pytest.mark.parametrize("kind", KINDS)
def test_adagrad_with_clip_one_step_ahead(okge_lib, kind):
    step = make(kind, optimizer="adagrad", grad_clip=binding_clip(kind), weight_decay=1e-10)
    for k, b in enumerate(batches()):
        adagrad_step_ahead("%s-adagrad-clip step%d" % (kind, k), step, b, True)


def params_and_state(step):
    step.flush()
    torch.cuda.synchronize()
    out = []
    for t in step._param_groups(every=True):
        out += [t[0], t[2]]
        if step.optimizer == "adam":
            out += list(step._adam[t[0].data_ptr()])
    return out


def same_after_three_steps(a, b):
    for batch in batches():
        la, lb = a.step(batch).clone(), b.step(batch).clone()
        assert torch.equal(la.view(torch.int64), lb.view(torch.int64))
    for k, (x, y) in enumerate(zip(params_and_state(a), params_and_state(b))):
        assert torch.equal(_bits(x), _bits(y)), k


def test_deferred_decay_with_clip_equals_the_eager_sweep(okge_lib):
    """decay_window = 4 under a binding clip: after flush() bit-equal to decay_window = 1 with the same clip"""
    clip = binding_clip("pooled-sum-bn")
    a = make("pooled-sum-bn", grad_clip=clip, decay_window=4, weight_decay=1e-3)
    b = make("pooled-sum-bn", grad_clip=clip, decay_window=1, weight_decay=1e-3)
    assert a.decay_window == 4 and b.decay_window == 1
    same_after_three_steps(a, b)
    assert torch.equal(a.grad_norm.view(torch.int64), b.grad_norm.view(torch.int64))


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
@pytest.mark.parametrize("kind", REPRODUCIBLE)
def test_a_clip_far_above_the_norm_changes_nothing(okge_lib, kind, optimizer):
    same_after_three_steps(make(kind, optimizer=optimizer, grad_clip=1e6), make(kind, optimizer=optimizer))


@pytest.mark.parametrize("kind", REPRODUCIBLE)
def test_adagrad_keyword_is_the_default_object(okge_lib, kind):
    a, b = make(kind), make(kind, optimizer="adagrad", betas=(0.5, 0.5), grad_clip=0.0)
    assert not hasattr(b, "_adam") and b.grad_norm is None
    assert [t.shape for t in a.state_tensors()] == [t.shape for t in b.state_tensors()]
    same_after_three_steps(a, b)


def test_graphed_step_replays_equal_eager_steps(okge_lib):
    """three replays of a captured token-pooled Adam step with a binding clip = three eager steps, bit for bit: parameters,
    moments, t and the clipped norm; the capture's warm-up steps leave t where it was"""
    from open_knowledge_graph_embeddings_amd.train_step import GraphedTrainStep
    clip = binding_clip("pooled-sum-bn")
    kw = dict(optimizer="adam", grad_clip=clip, weight_decay=1e-4)
    eager, graphed = make("pooled-sum-bn", **kw), make("pooled-sum-bn", **kw)
    bs = batches()
    for s in (eager, graphed):                                 # both start from one eager step: t = 1 at capture
        s.step(bs[0])
    gs = GraphedTrainStep(graphed, bs[0], pos_capacity=max(b.nnz for b in bs) + 3)
    torch.cuda.synchronize()
    assert graphed.adam_t == 1
    for b in bs:
        le, lg = eager.step(b).clone(), gs.step(b).clone()
        assert torch.equal(le.view(torch.int64), lg.view(torch.int64))
    torch.cuda.synchronize()
    assert eager.adam_t == graphed.adam_t == 4
    for k, (x, y) in enumerate(zip(params_and_state(eager), params_and_state(graphed))):
        assert torch.equal(_bits(x), _bits(y)), k
    assert torch.equal(eager.grad_norm.view(torch.int64), graphed.grad_norm.view(torch.int64))


@pytest.mark.parametrize("clip", ["clip", "noclip"])
@pytest.mark.parametrize("kind", ["pooled-sum-bn", "lstm-bn", "bigram-bn", "tucker3"])
def test_against_torch_adam_on_identical_gradients(okge_lib, kind, clip):
    """three steps from the same state: before each optimizer_step the snapshot's parameters, moments and t go into a
    torch.optim.Adam over CPU clones, the snapshot's gradients behind torch.nn.utils.clip_grad_norm_; both must land within
    adam_caps of adam64 of the common starting point (test_adam_step.py::test_okge_adam_against_torch_adam's bound, with its
    hyper-parameters, which fp32 holds exactly).  adam_caps count the roundings of the UPDATE from an exact gradient, so under a
    clip each side's adam64 takes the gradient that side's own clip handed to its optimizer (g * coef, fp32): torch sums the
    squares in fp32, this library in double, the two norms differ in their last places and the clipped gradients by a few u
    (2.7 u on random tensors of these sizes), for which the caps leave no room (held to OUR clipped gradients torch's
    exp_avg_sq stood at up to 4.3 caps at these shapes; the library's own side passes either way).  What ties the two clips together is the norm: an fp32 sum of n squares in any order is within n u of the
    exact one, its root within n u / 2 + u, the norm over K <= 8 such roots within another (K + 1) u; so torch's total norm
    lies within (n / 2 + 12) u of the float64 norm, n = the gradients' element count, and ours within 1 ulp of it (clipped())."""
    grad_clip = binding_clip(kind) if clip == "clip" else 0.0
    step = make(kind, optimizer="adam", lr=X_LR, betas=X_BETAS, eps=X_EPS, weight_decay=X_WD, grad_clip=grad_clip)
    hyper = (X_LR, X_BETAS, X_EPS, X_WD)
    for k, b in enumerate(batches()):
        case = "%s-%s-torch step%d" % (kind, clip, k)
        step.forward_backward(b)
        pre = snapshot(step)
        twins = [torch.nn.Parameter(torch.from_numpy(r["p"].copy())) for r in pre]
        ref = torch.optim.Adam(twins, lr=X_LR, betas=X_BETAS, eps=X_EPS, weight_decay=X_WD)
        for q, r in zip(twins, pre):
            q.grad = torch.from_numpy(r["g"].copy())
            if r["t"]:
                ref.state[q] = dict(step=torch.tensor(float(r["t"])), exp_avg=torch.from_numpy(r["m"].copy()),
                                    exp_avg_sq=torch.from_numpy(r["v"].copy()))
        if grad_clip > 0:
            theirs, exact = float(torch.nn.utils.clip_grad_norm_(twins, grad_clip)), grad_norm64(pre)
            n = sum(r["g"].size for r in pre)
            print("NORM %s torch %.9g float64 %.9g: %.1f u of %.1f allowed" % (case, theirs, exact, abs(theirs - exact) / exact / A.U, n / 2 + 12))
            assert abs(theirs - exact) <= (n / 2 + 12) * A.U * exact, (case, theirs, exact)
        torch_gs = [q.grad.numpy().copy() for q in twins]       # (what torch's optimizer reads)
        ref.step()
        step.optimizer_step()
        post = snapshot(step)
        gs = clipped(case, step, pre, clip == "clip")
        for i, (a, c, g, tg, q) in enumerate(zip(pre, post, gs, torch_gs, twins)):
            st = ref.state[q]
            assert float(st["step"]) == c["t"] == a["t"] + 1
            r = A.adam64(a["p"], g, a["m"], a["v"], a["t"] + 1, *hyper, exact=True)
            _hold("%s okge t%d" % (case, i), [c["p"], c["m"], c["v"]], r, a["m"], a["v"])
            r = A.adam64(a["p"], tg, a["m"], a["v"], a["t"] + 1, *hyper, exact=True)
            _hold("%s torch t%d" % (case, i), [q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()], r, a["m"], a["v"])
