"""The NumPy restatement of the lookup embedder's variants (tests/lookup_variants_reference.py) against G12 = the reference's
LookupComplexRelationModel + AddLossModule (tests/golden/g12_variant_*.npz), at the tolerances of tests/test_embedder_variants.py:
loss 3e-5 relative, hook 1e-5 relative, outputs 1e-4, every parameter's gradient 5e-5 max|ref| + 1e-10, running statistics
rtol 1e-5 / atol 1e-6, eval outputs 1e-4.  CPU only: this pins the yardstick the HIP encode is held to."""
import numpy as np
import pytest

from conftest import golden
from lookup_variants_reference import default_cfg, full_step
from oracle import kge_oracle as ko

CASES = ["g12_variant_bn", "g12_variant_proj", "g12_variant_norm", "g12_variant_l2", "g12_variant_all"]
PARAMS = {"entity_embedding.weight": "E", "relation_embedding.weight": "R", "subj_projection.0.weight": "W_subj",
          "obj_projection.0.weight": "W_obj", "bn_e.weight": "bn_e_w", "bn_e.bias": "bn_e_b", "bn_r.weight": "bn_r_w",
          "bn_r.bias": "bn_r_b", "bn_e.running_mean": "bn_e_mean", "bn_e.running_var": "bn_e_var", "bn_r.running_mean": "bn_r_mean",
          "bn_r.running_var": "bn_r_var"}


def fixture_problem(z):
    """-> (P, cfg, batch) of a G12 fixture; the candidates are all entities from id 2 on"""
    P = {PARAMS[k[3:]]: z[k] for k in z.files if k.startswith("p0_") and k[3:] in PARAMS}
    cfg = default_cfg(batch_norm=bool(z["batch_norm"]), project=bool(z["project_entity"]), normalize=str(z["normalize"]),
                      l2_reg=float(z["l2_reg"]))
    batch = {k: z[k].reshape(-1) for k in ("cand", "po_rel", "po_obj", "sp_subj", "sp_rel")}
    return P, cfg, batch


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(name, dt):
    z = golden(name)
    P, cfg, batch = fixture_problem(z)
    got = full_step(ko.COMPLEX, P, cfg, batch, z["labels"], dt, normalizer=float(z["normalizer"]))
    np.testing.assert_allclose(got["outputs"], z["outputs"], rtol=0, atol=1e-4)
    assert abs(got["loss"] - float(z["loss"])) <= 3e-5 * abs(float(z["loss"]))
    if bool(z["has_hook"]):
        assert abs(got["hook"] - float(z["hook"])) <= 1e-5 * abs(float(z["hook"]))
    else:
        assert got["hook"] == 0.0
    for key, mine in PARAMS.items():
        if "g_" + key in z.files:
            ref = z["g_" + key]
            np.testing.assert_allclose(got["grads"][mine], ref, rtol=0, atol=5e-5 * np.abs(ref).max() + 1e-10, err_msg=key)
    for k in z.files:
        if k.startswith("after_"):
            np.testing.assert_allclose(got["running"][PARAMS[k[6:]]], z[k], rtol=1e-5, atol=1e-6, err_msg=k)
    # eval mode with the statistics the training pass left: sp rows against get_all_obj(); the po rows of eval_outputs come from
    # po_prefix_score = get_all_subj() (subj_projection on the candidates), so they compare only without a projection
    P_after = dict(P)
    P_after.update(got["running"])
    ev = full_step(ko.COMPLEX, P_after, cfg, batch, z["labels"], dt, training=False)
    n_po = z["po_rel"].shape[0]
    np.testing.assert_allclose(ev["outputs"][n_po:], z["eval_outputs"][n_po:], rtol=0, atol=1e-4)
    if not cfg["project"]:
        np.testing.assert_allclose(ev["outputs"][:n_po], z["eval_outputs"][:n_po], rtol=0, atol=1e-4)
