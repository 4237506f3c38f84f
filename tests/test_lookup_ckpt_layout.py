"""The lookup step's checkpoint against torch's own optimizers (no GPU): what to_reference_checkpoint writes for a FusedTrainStep
-- Adagrad or Adam, nothing / the entity table / the relation table frozen -- holds the state entries, keys, shapes, dtypes and
`step` values torch.optim.Adagrad / torch.optim.Adam hold after the same three steps (the frozen parameter has .grad None),
torch's load_state_dict takes it, and load_reference_checkpoint brings every tensor back bit for bit."""
import copy

import pytest
import torch

from open_knowledge_graph_embeddings_amd import checkpoint as C
from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep

STEPS = 3
TENSORS = ("E", "R", "dE", "dR", "sumE", "sumR", "mE", "vE", "mR", "vR", "adam_stateE", "adam_stateR")
CASES = [(o, f) for o in ("adagrad", "adam") for f in (None, "entities", "relations")]


def _held(st, names=TENSORS, clone=True):
    """{name: the tensor the step holds under it, or None}"""
    held = {name: getattr(st, name, None) for name in names}
    return {k: v.clone() if clone and v is not None else v for k, v in held.items()}


def _step(optimizer, freeze, fill=True):
    g = torch.Generator().manual_seed(5)
    E, R = torch.randn(6, 8, generator=g), torch.randn(3, 8, generator=g)
    if not fill:
        return FusedTrainStep(torch.zeros_like(E), torch.zeros_like(R), "complex", optimizer=optimizer, freeze=freeze, engine=object())
    st = FusedTrainStep(E, R, "complex", lr=0.05, weight_decay=1e-6, eps=1e-9, optimizer=optimizer, betas=(0.8, 0.99), freeze=freeze,
                        engine=object())
    for t in _held(st, TENSORS[4:10], clone=False).values():
        if t is not None:
            t.copy_(torch.rand(t.shape, generator=g))
    st.steps = STEPS
    if optimizer == "adam":
        st.set_adam_t(STEPS)
    return st


def _torch_twin(optimizer, freeze):
    p = [torch.nn.Parameter(torch.zeros(6, 8)), torch.nn.Parameter(torch.zeros(3, 8))]
    opt = (torch.optim.Adam if optimizer == "adam" else torch.optim.Adagrad)(p, lr=0.05)
    for _ in range(STEPS):
        for q, name in zip(p, ("entities", "relations")):
            q.grad = None if name == freeze else torch.ones_like(q)
        opt.step()
    return opt


def _same(a, b):
    return a.keys() == b.keys() and all((a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])) for k in a)


@pytest.mark.parametrize("optimizer,freeze", CASES)
def test_optimizer_state_is_what_torch_holds(optimizer, freeze):
    opt = _torch_twin(optimizer, freeze)
    want = opt.state_dict()
    got = C.to_reference_checkpoint(_step(optimizer, freeze))["optimizer_state_dict"][0]["optimizer_state"]
    assert sorted(got["state"]) == sorted(want["state"])
    for i, entry in want["state"].items():
        assert sorted(got["state"][i]) == sorted(entry)
        for k, v in entry.items():
            assert got["state"][i][k].shape == v.shape and got["state"][i][k].dtype == v.dtype, (i, k)
        assert float(got["state"][i]["step"]) == float(entry["step"])
    assert got["param_groups"][0]["params"] == want["param_groups"][0]["params"]
    assert set(got["param_groups"][0]) >= set(want["param_groups"][0])
    opt.load_state_dict(copy.deepcopy(got))
    assert opt.param_groups[0]["lr"] == 0.05 and opt.param_groups[0]["eps"] == 1e-9


@pytest.mark.parametrize("optimizer,freeze", CASES)
def test_round_trip_is_bit_exact(optimizer, freeze):
    src = _step(optimizer, freeze)
    ckpt = C.to_reference_checkpoint(src, training_steps=STEPS)
    dst = _step(optimizer, freeze, fill=False)
    C.load_reference_checkpoint(dst, ckpt)
    a, b = _held(src), _held(dst)
    if optimizer == "adagrad" and freeze is not None:         # the frozen table's `sum` travels as zeros where the step held none
        frozen = "sumE" if freeze == "entities" else "sumR"
        assert a[frozen] is None and not b.pop(frozen).any()
        del a[frozen]
    assert _same(a, b)
    assert dst.steps == STEPS and (dst.lr, dst.weight_decay, dst.eps) == (src.lr, src.weight_decay, src.eps) == (0.05, 1e-6, 1e-9)
    assert optimizer != "adam" or (dst.adam_t == STEPS and dst.betas == src.betas == (0.8, 0.99))      # (Adagrad reads no betas)


@pytest.mark.parametrize("optimizer,freeze", [c for c in CASES if c[1] is not None])
def test_freeze_param_freezes_an_unfrozen_step_and_keeps_the_count(optimizer, freeze):
    ckpt = C.to_reference_checkpoint(_step(optimizer, freeze), training_steps=STEPS)
    dst = _step(optimizer, None, fill=False)
    C.load_reference_checkpoint(dst, ckpt, freeze_param=[C.ENTITY_KEY if freeze == "entities" else C.RELATION_KEY])
    assert dst.freeze == freeze and dst.steps == STEPS
    assert (dst.dE is None) == (freeze == "entities") and (dst.dR is None) == (freeze == "relations")
    again = C.to_reference_checkpoint(dst, training_steps=STEPS)["optimizer_state_dict"][0]["optimizer_state"]["state"]
    want = ckpt["optimizer_state_dict"][0]["optimizer_state"]["state"]
    assert sorted(again) == sorted(want)
    assert all(torch.equal(again[i][k], want[i][k]) for i in want for k in want[i])


@pytest.mark.parametrize("optimizer,key,value", [("adagrad", "lr_decay", 0.1), ("adagrad", "initial_accumulator_value", 0.5),
                                                 ("adam", "amsgrad", True)])
def test_refused_hyper_parameters_leave_the_step_as_it_was(optimizer, key, value):
    ckpt = C.to_reference_checkpoint(_step(optimizer, None), training_steps=STEPS)
    ckpt["optimizer_state_dict"][0]["optimizer_state"]["param_groups"][0][key] = value
    dst = _step(optimizer, None, fill=False)
    dst.steps = 7
    before = _held(dst)
    with pytest.raises(NotImplementedError):
        C.load_reference_checkpoint(dst, ckpt, freeze_param=[C.ENTITY_KEY])
    assert _same(before, _held(dst)) and dst.steps == 7 and dst.freeze is None and dst.lr == 0.3
