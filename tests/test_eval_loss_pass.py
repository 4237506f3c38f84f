"""The FB15k-237 validation pass (tests/golden/g13_valid_pass_fb15k237.npz, as tests/test_validation_pass.py runs it) through
both evaluators with loss="bce": the sum of the 40 per-batch losses against the float64 restatement of the pass computed
here on the CPU from the same tables (3e-5 relative, the bound of tests/test_eval_loss_shapes.py) and against the
reference's own eval_loss_sum (1e-4 relative: tests/test_eval_loss_reference.py measures the restatement 2.36e-5 from it,
the reference's fp32 reduction); the meter's count is sum B N = 292 419 510; ranks equal those of a loss=None run."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_eval_loss_reference import pass_loss
from test_validation_pass import _producer, _tables


@pytest.mark.gpu
@pytest.mark.usefixtures("production_config")
def test_validation_pass_loss(okge_lib, tmp_path):
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    z = golden("g13_valid_pass_fb15k237")
    E, R = _tables(z)
    Et, Rt = torch.from_numpy(E).cuda(), torch.from_numpy(R).cuda()
    batches = list(_producer(tmp_path, z, "cuda:0"))
    assert len(batches) == 40
    want64, elems = pass_loss(z, tmp_path)
    want_ref = float(z["eval_loss_sum"])
    assert elems == 292419510
    base = FusedEvaluator(Et, Rt, "complex", collect_ranks=True)
    res0, n0 = base.run(iter(batches))
    assert res0["loss"].count == 0
    sums = {}
    for name, ev in (("fused", FusedEvaluator(Et, Rt, "complex", collect_ranks=True, loss="bce")),
                     ("pipelined", PipelinedEvaluator(Et, Rt, "complex", collect_ranks=True, loss="bce"))):
        res, n = ev.run(iter(batches))
        losses = ev.batch_losses.cpu().tolist()
        assert n == n0 == 35068 and len(losses) == 40
        total = 0.0
        for v in losses:
            total += v
        print(f"{name}: sum L {total!r}  float64 {want64!r} ({abs(total - want64) / want64:.2e})  "
              f"reference {want_ref!r} ({abs(total - want_ref) / want_ref:.2e})  meter {res['loss'].avg!r}")
        assert abs(total - want64) <= 3e-5 * want64, (name, total, want64)
        assert abs(total - want_ref) <= 1e-4 * want_ref, (name, total, want_ref)
        assert res["loss"].count == 292419510 and res["loss"].avg == total / 292419510
        assert torch.equal(ev.ranks, base.ranks), name
        for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
            assert res[k].count == res0[k].count and abs(res[k].avg - res0[k].avg) <= 1e-12 * max(1.0, abs(res0[k].avg)), (name, k)
        sums[name] = total
    assert abs(sums["fused"] - sums["pipelined"]) <= 3e-5 * want64
