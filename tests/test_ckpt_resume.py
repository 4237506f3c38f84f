"""Stop and continue the token-encoded and Tucker3 training steps (checkpoint.model_checkpoint / save_model_checkpoint /
load_model_checkpoint): a run resumed from a file is BIT-identical to the uninterrupted run -- every state_dict tensor, every
optimizer-state tensor, every loss -- with dropout on, on 1-vs-all batches and batches with a candidate list, under Adagrad and
Adam.  pool='sum' and slot sizes that are multiples of 4: every step is on its atomics-free (bit-reproducible) path, which the
control test shows case by case before the resume test relies on it."""
import functools

import pytest
import torch

from ckpt_cases import KINDS, OPTIMIZERS, P_DROP, build, flat, random_batches

pytestmark = pytest.mark.gpu

LR = {"adagrad": 0.05, "adam": 0.01}
CASES = [(k, o) for k in KINDS for o in OPTIMIZERS]


def start(kind, optimizer, seed=3, **kw):
    """a module of `kind` with every parameter drawn from `seed`, in training mode, and its driver"""
    m = build(kind, dropout=P_DROP, seed=seed).cuda()
    m.train()
    return m, m.train_step(lr=LR[optimizer], weight_decay=1e-10, optimizer=optimizer, **kw)


def advance(st, batches):
    return [float(st.step(b)[0]) for b in batches]


def state_of(m, st):
    """(path, tensor) of everything a checkpoint carries, and its plain numbers"""
    from open_knowledge_graph_embeddings_amd.checkpoint import model_checkpoint
    ckpt = model_checkpoint(m, st)
    return flat(ckpt), ckpt["okge"]


def assert_same(a, b):
    assert [p for p, _ in a] == [p for p, _ in b]
    for (path, x), (_, y) in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), path


@functools.lru_cache(maxsize=None)
def uninterrupted(kind, optimizer):
    """four steps in one go: (losses, state, numbers, the step's own list of its tensors)"""
    m, st = start(kind, optimizer)
    losses = advance(st, random_batches(kind))
    tensors = [t.detach().cpu().clone() for t in st.state_tensors()]
    return (losses,) + state_of(m, st) + (tensors,)


@pytest.mark.parametrize("kind,optimizer", CASES)
def test_control_two_uninterrupted_runs_are_bit_equal(okge_lib, kind, optimizer):
    losses, state, numbers, tensors = uninterrupted(kind, optimizer)
    m, st = start(kind, optimizer)
    again = advance(st, random_batches(kind))
    assert again == losses and all(x == x and x > 0 for x in losses)
    for x, y in zip(tensors, st.state_tensors()):
        assert torch.equal(x, y.cpu())
    mine, mine_numbers = state_of(m, st)
    assert_same(state, mine)
    assert numbers == mine_numbers and numbers["steps"] == 4
    moved = [p for p, t in state if p.startswith("optimizer/") and not p.endswith("/step") and t.any()]
    assert moved                                                   # (the optimizer state is not all zeros: there is something to carry)


@pytest.mark.parametrize("kind,optimizer", CASES)
def test_resumed_run_is_bit_equal_to_the_uninterrupted_one(okge_lib, tmp_path, kind, optimizer):
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, save_model_checkpoint
    losses, state, numbers, _ = uninterrupted(kind, optimizer)
    batches = random_batches(kind)
    m, st = start(kind, optimizer)
    first = advance(st, batches[:2])
    path = str(tmp_path / "two_steps.pt")
    save_model_checkpoint(path, m, st, epoch=1)
    m2, st2 = start(kind, optimizer, seed=77)                      # other parameters, fresh buffers
    loaded = load_model_checkpoint(m2, st2, path)
    assert loaded["epoch"] == 1 and loaded["training_steps"] == 2 and st2.steps == 2
    second = advance(st2, batches[2:])
    assert first + second == losses
    mine, mine_numbers = state_of(m2, st2)
    assert_same(state, mine)
    assert mine_numbers == numbers


def test_resume_with_gradient_clipping(okge_lib, tmp_path):
    """grad_clip > 0 (binding: every norm is above it): the clipped run resumes bit-equal, the norm of step three included; the
    resuming driver is built WITHOUT clipping and takes it from the file"""
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, save_model_checkpoint
    kind, optimizer, clip = "lstm", "adagrad", 1e-3
    batches = random_batches(kind)
    m, st = start(kind, optimizer, grad_clip=clip)
    losses, norms = [], []
    for b in batches:
        losses.append(float(st.step(b)[0]))
        norms.append(float(st.grad_norm[0]))
    print("gradient norms", norms)
    assert all(n > clip for n in norms)
    want, _ = state_of(m, st)
    m1, st1 = start(kind, optimizer, grad_clip=clip)
    assert advance(st1, batches[:2]) == losses[:2]
    path = str(tmp_path / "clipped.pt")
    save_model_checkpoint(path, m1, st1)
    m2, st2 = start(kind, optimizer, seed=77)
    load_model_checkpoint(m2, st2, path)
    assert st2.grad_clip == clip
    assert float(st2.step(batches[2])[0]) == losses[2] and float(st2.grad_norm[0]) == norms[2]
    assert float(st2.step(batches[3])[0]) == losses[3]
    assert_same(want, state_of(m2, st2)[0])
    plain = uninterrupted(kind, optimizer)[1]                     # (and clipping did change the run)
    assert any(not torch.equal(x, y) for (_, x), (_, y) in zip(want, plain))


def test_deferred_decay_is_settled_in_the_file_and_resumes(okge_lib, tmp_path, monkeypatch):
    """token-pooled step with decay_window = 4, saved after step two -- mid-window, with rows that still owe decay-only steps:
    the file is the one a decay_window = 1 run writes, tensor for tensor, and the run resumed at window 4 equals the uninterrupted
    window-4 run once both are flushed"""
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, save_model_checkpoint
    kind, optimizer = "unigram", "adagrad"
    batches = random_batches(kind, pattern="llal")
    files = {}
    for window in (1, 4):
        monkeypatch.setenv("OKGE_LAZY_DECAY", str(window))
        m, st = start(kind, optimizer)
        assert st.decay_window == window
        advance(st, batches[:2])
        if window == 4:
            lag = sum(int((sl.row_steps < st._counters[0]).sum()) for sl in (st.entity, st.relation))
            print("rows that owe decay-only steps at the save:", lag)
            assert lag > 0 and st._pending is not None
        files[window] = str(tmp_path / f"window{window}.pt")
        save_model_checkpoint(files[window], m, st)
        if window == 4:
            assert st._pending is None
            want_losses = advance(st, batches[2:])
            want, _ = state_of(m, st)                              # (flushes)
    a, b = (torch.load(files[w], weights_only=True) for w in (1, 4))
    assert_same(flat(a), flat(b))
    assert a["okge"] == b["okge"]
    m2, st2 = start(kind, optimizer, seed=77)
    assert st2.decay_window == 4
    load_model_checkpoint(m2, st2, files[4])
    assert advance(st2, batches[2:]) == want_losses
    assert_same(want, state_of(m2, st2)[0])


def two_steps(kind, optimizer):
    m, st = start(kind, optimizer)
    advance(st, random_batches(kind)[:2])
    return m, st


@pytest.mark.parametrize("kind,optimizer", CASES)
def test_reset_optimizer_takes_the_state_dict_alone(okge_lib, kind, optimizer):
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, model_checkpoint
    m, st = two_steps(kind, optimizer)
    ckpt = model_checkpoint(m, st)
    m2, st2 = start(kind, optimizer, seed=77)
    advance(st2, random_batches(kind, seed=12)[:1])                # (so that there is optimizer state to reset)
    load_model_checkpoint(m2, st2, ckpt, reset_optimizer=True)
    for (k, x), (_, y) in zip(ckpt["state_dict"].items(), m2.state_dict().items()):
        assert torch.equal(x, y.cpu().to(x.dtype)), k
    entries, word = m2.optimizer_params_and_state(st2)
    for p, views, moved in entries:
        assert len(views) == (2 if optimizer == "adam" else 1)
        for v in views:
            assert v.shape == p.shape and not v.any()
    assert st2.steps == 0 and st2.lr == LR[optimizer]
    if optimizer == "adam":
        assert int(word[0]) == 0 and st2.adam_t == 0
    else:
        assert word is None
    assert all(not t[1].any() for t in st2._param_groups(every=True))          # gradient buffers: the head of a step
    assert float(st2.step(random_batches(kind)[2])[0]) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_other_optimizers_state_is_refused(okge_lib, kind):
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, model_checkpoint
    for have, want in (("adagrad", "adam"), ("adam", "adagrad")):
        ckpt = model_checkpoint(*two_steps(kind, have))
        m2, st2 = start(kind, want, seed=77)
        before, _ = state_of(m2, st2)
        with pytest.raises(ValueError, match=f"the checkpoint holds {have} optimizer state and this step trains with {want}: its "
                                             f"accumulators do not carry over -- load with reset_optimizer=True"):
            load_model_checkpoint(m2, st2, ckpt)
        assert_same(before, state_of(m2, st2)[0])


@pytest.mark.parametrize("kind,optimizer", [("bigram", "adagrad"), ("lstm", "adam"), ("tucker3", "adagrad")])
def test_a_tensor_of_the_wrong_shape_is_refused_before_anything_is_written(okge_lib, kind, optimizer):
    from open_knowledge_graph_embeddings_amd.checkpoint import load_model_checkpoint, model_checkpoint
    good = model_checkpoint(*two_steps(kind, optimizer))
    m2, st2 = start(kind, optimizer, seed=77)
    before, numbers = state_of(m2, st2)
    last = list(good["state_dict"])[-1]                            # (every tensor in front of it would fit)
    bad = dict(good, state_dict=dict(good["state_dict"]))
    bad["state_dict"][last] = torch.zeros(tuple(n + 1 for n in good["state_dict"][last].shape) or (2,))
    with pytest.raises(ValueError, match=last.replace(".", r"\.")):
        load_model_checkpoint(m2, st2, bad)
    ost = good["optimizer_state_dict"][0]["optimizer_state"]
    n = len(ost["state"]) - 1
    name = "exp_avg_sq" if optimizer == "adam" else "sum"
    state = dict(ost["state"])
    state[n] = dict(state[n], **{name: torch.zeros(3, 5, 7)})
    bad = dict(good, optimizer_state_dict=[dict(good["optimizer_state_dict"][0], optimizer_state=dict(ost, state=state))])
    with pytest.raises(ValueError, match=f"'{name}' of parameter {n}"):
        load_model_checkpoint(m2, st2, bad)
    after, after_numbers = state_of(m2, st2)
    assert_same(before, after)
    assert numbers == after_numbers and st2.steps == 0


def test_file_loads_with_weights_only(okge_lib, tmp_path):
    from open_knowledge_graph_embeddings_amd.checkpoint import save_model_checkpoint
    m, st = two_steps("bigram", "adam")
    path = str(tmp_path / "ckpt.pt")
    written = save_model_checkpoint(path, m, st, epoch=3, training_steps=17)
    back = torch.load(path, weights_only=True)
    assert back["epoch"] == 3 and back["training_steps"] == 17 and back["okge"] == written["okge"] and back["okge"]["steps"] == 2
    assert all(t.device.type == "cpu" for _, t in flat(back))
    assert_same(flat(written), flat(back))
