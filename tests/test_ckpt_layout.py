"""Checkpoints of the token-encoded and Tucker3 models, the part that needs no device: the reference's `Trainer.save` layout
(tests/golden/g22_ckpt_*.npz) against what torch's own optimizers hold over a CPU instance of this package's modules -- which
pins parameters() order, shapes and dtypes of the optimizer state against the reference -- and the refusal of the lookup steps."""
import pytest
import torch

from ckpt_cases import KINDS, build, fixture, fixture_checkpoint, fixture_layout, flat, layout

RUNS = [(k, "") for k in KINDS] + [("unigram", "adam_"), ("lstm", "adam_")]


def test_fixture_set():
    for kind in KINDS:
        z = fixture(kind)
        assert [str(r) for r in z["runs"]] == (["", "adam_"] if kind in ("unigram", "lstm") else [""])
        ckpt = fixture_checkpoint(z)
        assert ckpt["training_steps"] == 2 and ckpt["optimizer_state_dict"][0]["regime"][0]["lr"] == 0.3
        assert layout(flat(ckpt)) == fixture_layout(z)                     # (the helper rebuilds the dict in the stored order)


@pytest.mark.parametrize("kind,run", RUNS)
def test_optimizer_state_layout_is_torchs_over_this_packages_module(kind, run):
    """key list, order, shapes and dtypes of the reference's optimizer state = torch.optim.Adagrad / Adam over model.parameters()"""
    z = fixture(kind)
    m = build(kind)
    ref = [e for e in fixture_layout(z, run) if e[0].startswith("optimizer/")]
    if run == "adam_":
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        for p in m.parameters():                                           # (Adam creates a parameter's state at its first step)
            p.grad = torch.zeros_like(p)
        opt.step()
    else:
        opt = torch.optim.Adagrad(m.parameters(), lr=0.3)
    mine = [(f"optimizer/{i}/{k}", v) for i, st in opt.state_dict()["state"].items() for k, v in st.items()]
    assert layout(mine) == ref
    group = fixture_checkpoint(z, run)["optimizer_state_dict"][0]["optimizer_state"]["param_groups"][0]
    assert group["params"] == list(range(len(list(m.parameters())))) == opt.state_dict()["param_groups"][0]["params"]


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_shapes_are_the_references(kind):
    z = fixture(kind)
    m = build(kind)
    ref = [e[:2] for e in fixture_layout(z) if e[0].startswith("state_dict/")]
    assert [e[:2] for e in layout(("state_dict/" + k, v) for k, v in m.state_dict().items())] == ref
    m.load_state_dict(fixture_checkpoint(z)["state_dict"])                 # a reference-written state_dict loads


@pytest.mark.parametrize("cls", ["FusedTrainStep", "ShardedTrainStep"])
def test_lookup_steps_are_sent_to_the_two_table_functions(cls, tmp_path):
    from open_knowledge_graph_embeddings_amd import checkpoint as C
    from open_knowledge_graph_embeddings_amd import sharded, train_step
    kind = getattr(train_step, cls, None) or getattr(sharded, cls)
    step = kind.__new__(kind)                                              # (refused by its class: nothing of it is read)
    m = build("unigram")
    for call in (lambda: C.model_checkpoint(m, step), lambda: C.save_model_checkpoint(str(tmp_path / "x.pt"), m, step),
                 lambda: C.load_model_checkpoint(m, step, fixture_checkpoint(fixture("unigram")))):
        with pytest.raises(TypeError, match="to_reference_checkpoint"):
            call()
    assert not (tmp_path / "x.pt").exists()
