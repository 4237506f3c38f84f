"""CPU: the restatement of the Tucker3 model (tests/tucker3_reference.py) reproduces every fixture the reference itself
produced (tests/golden/g18_tucker3_*.npz), the scores are the Tucker3 contraction sum_ijk T[i,j,k] e_s[i] e_o[j] rho_r[k], and the
package's model class has the reference's constructor surface: parameter names, shapes and -- same seed -- values; every keyword
outside the HIP path raises; the registry and the C ABI know the new names.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, golden_names
import tucker3_reference as TR

CASES = [n for n in golden_names("g18_tucker3_") if n != "g18_tucker3_adagrad"]
KEYS = ("entity_embedding.weight", "relation_embedding.weight", "relation_projection.0.weight")
F64 = torch.float64


def params(z, prefix="init/"):
    return [z[prefix + k] for k in KEYS]


def close(got, want, tol, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= tol * max(1.0, np.abs(want).max()), (name, err)


def run_case(z, dtype):
    return TR.step(*params(z), z, dtype, loss_kind=str(z["loss_kind"]), smoothing=float(z["smoothing"]), p_in=float(z["input_dropout"]),
                   p_rel=float(z["relation_input_dropout"]), normalizer=float(z["normalizer"]))


def test_fixture_set():
    assert CASES == ["g18_tucker3_" + n for n in ("bce_all", "bce_dropout", "bce_smooth_po_only", "kl_shared")]
    z = golden("g18_tucker3_kl_shared")
    c = z["cand"].reshape(-1)
    assert len(set(c.tolist())) < c.size                          # the batch-shared list names an id twice
    assert "sp_subj" not in golden("g18_tucker3_bce_smooth_po_only").files
    for n in CASES:
        assert 1.0 <= np.abs(golden(n)["outputs"]).max() <= 8.0    # scores large enough for an absolute tolerance to bite


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    """float64 restatement vs the reference's fp32 run: loss, outputs, the three gradients, eval scores (fp32 rounding apart)"""
    z = golden(name)
    assert list(z["state_keys"]) == list(KEYS) and list(z["param_names"]) == list(KEYS)
    out = run_case(z, F64)
    assert abs(out["loss"] - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    close(out["outputs"], z["outputs"], 2e-6, "outputs")
    for k, g in zip(KEYS, (out["dE"], out["dR"], out["dW"])):
        close(g, z["grad/" + k], 2e-6, k)
    sp, po, tri = TR.eval_scores(*params(z), z, F64)
    if "sp_all_eval" in z.files:
        close(sp, z["sp_all_eval"], 2e-6, "sp")
    close(po, z["po_all_eval"], 2e-6, "po")
    close(tri, z["triple_eval"], 2e-6, "triple")


@pytest.mark.parametrize("name", CASES)
def test_fp32_restatement_close_to_float64(name):
    z = golden(name)
    a, b = run_case(z, torch.float32), run_case(z, F64)
    for k in ("outputs", "dE", "dR", "dW"):
        close(a[k], b[k], 1e-5, k)


@pytest.mark.parametrize("name", CASES)
def test_scores_are_the_tucker3_contraction(name):
    """score(s, r, o) = sum_ijk T[i,j,k] e_s[i] e_o[j] rho_r[k], T[i,j,k] = W[i d + j, k], for both directions"""
    z = golden(name)
    E, R, W = (torch.from_numpy(p).double() for p in params(z))
    d, r = E.shape[1], R.shape[1]
    T3 = W.view(d, d, r)
    po_rel, po_obj, sp_subj, sp_rel, _ = TR.ids_of(z)
    cand = E[2:]
    if sp_subj.numel():
        x = torch.einsum("ijk,bi,nj,bk->bn", T3, E[sp_subj], cand, R[sp_rel])
        close(x, z["sp_all_eval"], 2e-6, "sp einsum")
    x = torch.einsum("ijk,ni,bj,bk->bn", T3, cand, E[po_obj], R[po_rel])
    close(x, z["po_all_eval"], 2e-6, "po einsum")


def state_before(step):
    """key prefix of the Adagrad fixture's state in front of `step` (stored once per step boundary)"""
    return "s0_before/" if step == 0 else f"s{step - 1}_after/"


def test_adagrad_restatement_reproduces_the_reference():
    z = golden("g18_tucker3_adagrad")
    lr, wd, eps = float(z["opt_lr"]), float(z["opt_weight_decay"]), float(z["opt_eps"])
    assert int(z["n_opt_params"]) == 3 and lr == pytest.approx(0.3) and wd == pytest.approx(1e-10)
    assert not any(k.startswith(("s1_before", "s2_before")) for k in z.files)     # one run: a step starts where the last ended
    for s in range(3):
        pre = state_before(s)
        P = [z[f"{pre}param/{k}"] for k in KEYS]
        out = TR.step(*P, z, F64, prefix=f"s{s}_")
        assert abs(out["loss"] - float(z[f"s{s}_loss"])) <= 1e-5 * abs(float(z[f"s{s}_loss"]))
        for k, g in zip(KEYS, (out["dE"], out["dR"], out["dW"])):
            p, acc = TR.adagrad(TR.T(z[f"{pre}param/{k}"], F64), g, TR.T(z[f"{pre}sum/{k}"], F64), lr, wd, eps)
            close(acc, z[f"s{s}_after/sum/{k}"], 1e-5, f"sum {k}")
            close(p, z[f"s{s}_after/param/{k}"], 1e-5, f"param {k}")


# ---- the package's model class (construction is CPU work; every compute method needs the GPU) ----------------------------
class Meta:
    def __init__(self, n_ent, n_rel):
        self.entities_size, self.relations_size, self.min_entities_size, self.min_relations_size = n_ent, n_rel, 2, 2


def construct(z, **kw):
    from open_knowledge_graph_embeddings_amd.model import Models
    torch.manual_seed(int(z["seed"]))
    args = dict(entity_slot_size=int(z["d"]), relation_slot_size=int(z["r_e"]), train_data=Meta(int(z["n_ent"]), int(z["n_rel"])),
                init_std=float(z["init_std"]), sparse=False)
    args.update(kw)
    return Models.LookupTucker3RelationModel(**args)


@pytest.mark.parametrize("name", CASES)
def test_model_constructs_with_the_reference_parameters(name):
    z = golden(name)
    m = construct(z, input_dropout=float(z["input_dropout"]), relation_input_dropout=float(z["relation_input_dropout"]))
    assert [k for k, _ in m.named_parameters()] == list(z["param_names"])
    assert list(m.state_dict().keys()) == list(z["state_keys"])
    d, r = int(z["d"]), int(z["r_e"])
    assert tuple(m.state_dict()[KEYS[2]].shape) == (d * d, r) and tuple(m.state_dict()[KEYS[1]].shape) == (int(z["n_rel"]), r)
    for k, p in m.named_parameters():                              # same seed, same construction order: the same values
        assert np.array_equal(p.detach().numpy(), z["ctor/" + k]), k
    assert m.project_relation is True and m.scorer_name == "rescal" and m.get_slot_size() == d
    m.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in KEYS})        # a reference-written state dict loads


def test_project_relation_is_forced():
    z = golden(CASES[0])
    assert construct(z, project_relation=False).project_relation is True        # model.py:1001-1004


@pytest.mark.parametrize("kw", [dict(relation_dropout=0.1), dict(project_relation_activation="ReLU"), dict(project_entity=True),
                                dict(batch_norm=True), dict(normalize="norm"), dict(l2_reg=0.01), dict(sparse=True),
                                dict(entity_embedding_size=5), dict(entity_slot_size=257), dict(relation_slot_size=300),
                                dict(dropout=0.2, relation_dropout=None)])
def test_unsupported_keywords_raise(kw):
    with pytest.raises(NotImplementedError):
        construct(golden(CASES[0]), **kw)


def test_existing_embedder_still_refuses_the_projection():
    from open_knowledge_graph_embeddings_amd.model import LookupBaseRelationEmbedder
    with pytest.raises(NotImplementedError):
        LookupBaseRelationEmbedder(8, 8, Meta(10, 5), project_relation=True)


def test_names_in_registry_header_and_exports():
    from open_knowledge_graph_embeddings_amd import _native, tucker3
    from open_knowledge_graph_embeddings_amd.model import Models
    assert Models.LookupTucker3RelationModel is tucker3.LookupTucker3RelationModel
    assert issubclass(tucker3.LookupTucker3RelationModel, tucker3.RescalRelationScorer)
    header = open(os.path.join(ROOT, "include", "okge.h")).read()
    declared = set(re.findall(r"\b(okge_[a-z0-9_]+)\s*\(", header))
    new = {"okge_tucker3_workspace_bytes", "okge_tucker3_fold", "okge_tucker3_backward", "okge_tucker3_score_triples",
           "okge_tucker3_apply", "okge_tucker3_outer"}
    assert new <= declared and new <= set(_native.EXPORTS)
    assert "okge_tucker3.hip" in _native.SOURCES
    assert re.search(r"#define OKGE_ABI_VERSION 2\b", header)


def test_argument_errors_before_any_device_work():
    from open_knowledge_graph_embeddings_amd import _native
    L = _native.lib()
    assert L.okge_tucker3_workspace_bytes(512, 200, 200) > 0
    assert L.okge_tucker3_workspace_bytes(512, 257, 16) == 0 and L.okge_tucker3_workspace_bytes(512, 16, 257) == 0
    assert L.okge_tucker3_workspace_bytes(0, 16, 16) == 0
    assert L.okge_tucker3_fold(None, 16, 16, None, 16, None, 16, 4, 4, None, 64, None, 0, None) == -1
    assert b"tucker3" in L.okge_last_error()
    assert L.okge_tucker3_fold(1, 300, 16, 1, 300, 1, 16, 4, 4, 1, 512, 1, 1 << 30, None) == -2      # OKGE_ERR_UNSUPPORTED, nothing touched
    assert L.okge_tucker3_backward(1, 16, 300, 1, 16, 1, 300, 1, 64, 4, 4, 0, None, None, None, 1, 1 << 30, None) == -2
    assert L.okge_tucker3_score_triples(1, 16, 16, 1, 16, 1, 16, 1, 16, 0, 1, 1, 1 << 30, None) == -1
