"""The float64 restatement of the data-bias scorers and their training step (tests/databias_reference.py over
tests/lstm_reference.py) pinned to the reference's own DataBiasOnlyEntityModel / DataBiasOnlyRelationModel on the CPU
(tests/golden/g20_databias_*.npz).  The GPU tests hold the HIP kernels to the same fixtures.

Bounds (a float64 restatement against fp32 fixtures): running statistics and eval tables as in test_lstm_reference.py
(rtol 1e-5 / atol 1e-6, rtol = atol = 1e-5); scores, loss and gradients as the fixtures are held everywhere else (rtol = atol =
1e-5, 1e-5 relative, 1e-4 of the tensor's largest element); Adagrad steps under test_lstm_parity.py's conditioning-aware bound."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from databias_reference import SCORER_OF, adagrad, chain, fold, scores, slot_params, step
from lstm_reference import lstm_pass

CASES = [n for n in golden_names("g20_databias_") if "adagrad" not in n]
ADAGRAD = [n for n in golden_names("g20_databias_") if "adagrad" in n]


def sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def batch_of(z, pre=""):
    keys = ("cand", "po_rel", "po_obj") + (("sp_subj", "sp_rel") if pre + "sp_subj" in z.files else ())
    return {k: z[pre + k] for k in keys}


def test_fixture_set_is_complete():
    assert sorted(CASES) == ["g20_databias_entity_bn_all", "g20_databias_entity_none_shared", "g20_databias_relation_bn_shared",
                             "g20_databias_relation_none_po_only"]
    assert sorted(ADAGRAD) == ["g20_databias_adagrad_entity", "g20_databias_adagrad_relation"]
    assert not int(golden("g20_databias_relation_none_po_only")["has_sp"])
    for n in CASES + ADAGRAD:
        assert int(golden(n)["d"]) <= 32


def test_scorer_restatement_is_a_copy_and_a_product():
    g = torch.Generator().manual_seed(20)
    ent, rel, cand = (torch.randn(5, 6, generator=g, dtype=torch.float64).numpy() for _ in range(3))
    assert fold("bias_relation", ent, rel) is rel and fold("bias_entity", ent, rel) is ent
    np.testing.assert_array_equal(scores("bias_relation", ent, rel, cand), rel @ cand.T)
    np.testing.assert_array_equal(scores("bias_entity", ent, rel, cand), ent @ cand.T)
    dq = np.ones((5, 6))
    assert chain("bias_relation", dq)[0] is None and chain("bias_relation", dq)[1] is dq
    assert chain("bias_entity", dq)[1] is None and chain("bias_entity", dq)[0] is dq


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_step(name):
    z = golden(name)
    scorer = SCORER_OF[str(z["model"])]
    r = step(scorer, sub(z, "init/"), None, (z["ent_tokens"], z["rel_tokens"]), batch_of(z), z["labels"], float(z["normalizer"]))
    np.testing.assert_allclose(r["outputs"], z["outputs"], rtol=1e-5, atol=1e-5)
    assert abs(r["loss"] - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    names = [str(x) for x in z["param_names"]]
    assert [k for k in names if k in set(r["grad_none"])] == [str(x) for x in z["grad_none"]]
    assert len(set(r["grad_none"])) == len(z["grad_none"])
    assert sorted(r["grads"]) == sorted(k for k in names if k not in set(r["grad_none"]))
    for k, g in r["grads"].items():
        want = z["grad/" + k]
        np.testing.assert_allclose(g, want, rtol=0, atol=1e-4 * max(np.abs(want).max(), 1e-30), err_msg=k)
    bufs = sub(z, "buf/")
    assert sorted(r["running"]) == sorted(bufs)                    # the unused relation slot's statistics move too
    for k, v in r["running"].items():
        np.testing.assert_allclose(v, bufs[k], rtol=1e-5, atol=1e-6, err_msg=k)
        assert np.abs(v - (0.0 if k.endswith("mean") else 1.0)).max() > 1e-3, k


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_eval_tables_and_prefix_scores(name):
    z = golden(name)
    scorer = SCORER_OF[str(z["model"])]
    params, bufs, tables = sub(z, "init/"), sub(z, "buf/"), {}
    for side, tok, key in (("entity", "ent_tokens", "E_eval"), ("relation", "rel_tokens", "R_eval")):
        W, lstm, bn = slot_params(params, side)
        running = None if bn is None else tuple(torch.from_numpy(bufs[f"{side}_batchnorm.running_{k}"]) for k in ("mean", "var"))
        tables[side] = lstm_pass(W, torch.from_numpy(z[tok]), lstm, [(None, 0, z[tok].shape[0])], bn=bn, running=running,
                                 training=False)["out"]
        np.testing.assert_allclose(tables[side], z[key], rtol=1e-5, atol=1e-5, err_msg=side)
    E, R = tables["entity"], tables["relation"]
    ids = lambda k: z[k].reshape(-1).astype(np.int64)              # noqa: E731
    po = scores(scorer, E[ids("po_obj")], R[ids("po_rel")], E[2:])
    np.testing.assert_allclose(po, z["po_all_eval"], rtol=1e-5, atol=1e-5)
    if int(z["has_sp"]):
        sp = scores(scorer, E[ids("sp_subj")], R[ids("sp_rel")], E[2:])
        np.testing.assert_allclose(sp, z["sp_all_eval"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ADAGRAD)
@pytest.mark.parametrize("s", [0, 1, 2])
def test_restatement_reproduces_the_adagrad_steps(name, s):
    """each OptimRegime step restarted from the reference's state before it; parameters without a gradient are not stepped:
    bit-unchanged, no accumulator -- the `no_state` list"""
    z = golden(name)
    scorer = SCORER_OF[str(z["model"])]
    pre, post = f"s{s}_before/", f"s{s}_after/"
    B, N = z[f"s{s}_labels"].shape
    r = step(scorer, sub(z, pre + "param/"), sub(z, pre + "buf/"), (z["ent_tokens"], z["rel_tokens"]), batch_of(z, f"s{s}_"),
             z[f"s{s}_labels"], float(B * N))
    assert abs(r["loss"] - float(z[f"s{s}_loss"])) <= 1e-5 * abs(float(z[f"s{s}_loss"]))
    names = [str(x) for x in z["param_names"]]
    assert [k for k in names if k in set(r["grad_none"])] == [str(x) for x in z["no_state"]] == [str(x) for x in z["grad_none"]]
    lr, eps, wd = float(z["opt_lr"]), float(z["opt_eps"]), float(z["opt_weight_decay"])
    for k in names:
        p0, s0 = z[pre + "param/" + k], z[pre + "sum/" + k]
        want_p, want_s = z[post + "param/" + k], z[post + "sum/" + k]
        if k in r["grad_none"]:
            np.testing.assert_array_equal(want_p, p0, err_msg=k)
            assert not want_s.any() and not s0.any(), k
            continue
        p1, s1 = adagrad(p0, r["grads"][k], s0, lr, wd, eps)
        g = np.sqrt(np.maximum(want_s - s0, 0))
        tol = 2e-4 * lr + lr * (1e-4 * g.max()) * (np.sqrt(s0) + eps) / (np.sqrt(want_s) + eps) ** 2
        assert (np.abs(p1 - want_p) <= tol).all(), (k, float(np.abs(p1 - want_p).max()))
        np.testing.assert_allclose(s1, want_s, rtol=0, atol=2e-4 * max(np.abs(want_s).max(), 1e-30), err_msg=k)
    for k, v in r["running"].items():
        np.testing.assert_allclose(v, z[post + "buf/" + k], rtol=1e-5, atol=1e-6, err_msg=k)

