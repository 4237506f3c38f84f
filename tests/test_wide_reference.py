"""Pins tests/wide_reference.py -- the float64 truth and the fp32 yardstick the GPU tests of the wide path (test_wide_shapes.py)
are judged against -- to the oracle, to the planner (okge_plan.h through tests/wide_plan_driver.cpp) and to fixtures generated
from the reference at slot sizes 516 (ComplEx) and 513 (DistMult): tests/golden/g22_wide_* (make_golden_wide.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_reference as wr  # noqa: E402
from conftest import golden  # noqa: E402
from oracle import kge_oracle as ko  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = [("g22_wide_complex_d516", "complex", 516), ("g22_wide_distmult_d513", "distmult", 513)]
U = 2.0 ** -24


def _z(g):
    return {k: g[k].reshape(-1) for k in ("po_rel", "po_obj", "sp_subj", "sp_rel")}


@pytest.mark.parametrize("name,scorer,d", FIXTURES)
@pytest.mark.parametrize("loss,smoothing", [("bce", 0.1), ("kl", 0.0)])
def test_restatements_against_the_reference(name, scorer, d, loss, smoothing):
    """the reference's own fp32 numbers (torch CPU: blocked matmuls) against the float64 truth and the fp32 yardstick"""
    g = golden(name)
    assert g["E"].shape == (40, d) and g["R"].shape == (6, d) and g["labels"].shape == (11, 38)
    assert os.path.getsize(os.path.join(HERE, "golden", name + ".npz")) < 400_000
    cand = g["cand"].reshape(-1)
    t = wr.truth(scorer, g["E"], g["R"], _z(g), cand, g["labels"], loss, smoothing)
    y = wr.yardstick(scorer, g["E"], g["R"], _z(g), cand, g["labels"], loss, smoothing)
    for got in (y, {k: g[f"{loss}_{k}"] for k in ("outputs", "dE", "dR")} | {"loss": float(g[f"{loss}_loss"])}):
        # a d-term fp32 dot product: error <= d u sum|q c|, far above what either fp32 computation shows; 64 u max is ample
        for k in ("outputs", "dE", "dR"):
            scale = np.abs(t[k]).max()
            assert np.abs(got[k] - t[k]).max() <= 64 * U * scale, (k, np.abs(got[k] - t[k]).max() / scale)
        assert abs(got["loss"] - t["loss"]) <= 3e-5 * abs(t["loss"])


def test_truth_is_the_oracle_with_philox_masks():
    """truth() only forwards to the oracle: with dropout its masks are dropout_keep_mask's, position-keyed, stream per list"""
    rng = np.random.default_rng(5)
    n_ent, n_rel, d, n_po, n_sp = 30, 5, 520, 3, 2
    E, R = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.3).astype(np.float32)
    z = dict(po_rel=rng.integers(2, n_rel, n_po), po_obj=rng.integers(2, n_ent, n_po), sp_subj=rng.integers(2, n_ent, n_sp),
             sp_rel=rng.integers(2, n_rel, n_sp))
    cand = np.arange(2, n_ent)
    y = (rng.random((n_po + n_sp, len(cand))) < 0.1).astype(np.float32)
    m = wr.philox_masks(99, 3, n_po, n_sp, len(cand), d, 0.4, 0.25)
    assert m["keep_cand"].shape == (len(cand), d) and m["keep_po_rel"].shape == (n_po, d)
    assert np.array_equal(m["keep_sp_ent"], ko.dropout_keep_mask(99, 3, 3, n_sp, d, 0.4))
    t = wr.truth("complex", E, R, z, cand, y, p_ent=0.4, p_rel=0.25, masks=m)
    yd = wr.yardstick("complex", E, R, z, cand, y, p_ent=0.4, p_rel=0.25, masks=m)
    for k in ("outputs", "dE", "dR"):
        assert np.abs(yd[k] - t[k]).max() <= 64 * U * np.abs(t[k]).max(), k
    # dropped candidate columns receive no gradient through the candidate path, whatever G holds
    dead = ~m["keep_cand"]
    only_cand = np.setdiff1d(cand, np.concatenate([z["po_obj"], z["sp_subj"]]))
    assert not yd["dE"][only_cand][dead[only_cand - 2]].any()


def test_range_and_split_cut_changes_the_yardstick_only_in_the_last_bits():
    """several candidate ranges (OKGE_GT_MBYTES = 1): same scores bit for bit, dQ-borne gradients within fp32 noise"""
    rng = np.random.default_rng(6)
    n_ent, n_rel, d, n_po, n_sp = 302, 5, 4096, 2, 2
    E, R = (rng.standard_normal((n_ent, d)) * 0.05).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.05).astype(np.float32)
    z = dict(po_rel=rng.integers(2, n_rel, n_po), po_obj=rng.integers(2, n_ent, n_po), sp_subj=rng.integers(2, n_ent, n_sp),
             sp_rel=rng.integers(2, n_rel, n_sp))
    cand = np.arange(2, n_ent)
    y = (rng.random((4, 300)) < 0.05).astype(np.float32)
    assert wr.plan(4, 300, d)["n_ranges"] == 1 and wr.plan(4, 300, d, 1)["n_ranges"] == 3
    a, b = wr.yardstick("distmult", E, R, z, cand, y), wr.yardstick("distmult", E, R, z, cand, y, gt_mbytes=1)
    assert np.array_equal(a["outputs"], b["outputs"]) and a["loss"] == b["loss"]
    assert np.abs(a["dR"] - b["dR"]).max() <= 16 * U * np.abs(a["dR"]).max()


def test_plan_restates_the_planner(tmp_path):
    cc = next((p for p in map(shutil.which, ("c++", "g++", "hipcc")) if p), None)
    assert cc, "no C++ compiler on the path"
    exe = str(tmp_path / "wide_plan_driver")
    built = subprocess.run([cc, "-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "wide_plan_driver.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    import json
    cases = [(B, N, d, gt) for B in (1, 64, 65, 131, 512, 4096) for N in (1, 65, 129, 700, 14541, 312500) for d in (513, 528, 1000, 4096)
             for gt in (-1, 1)]
    out = subprocess.run([exe], input="\n".join("%d %d %d %d" % c for c in cases) + "\n", capture_output=True, text=True, check=True).stdout
    for (B, N, d, gt), line in zip(cases, out.splitlines()):
        p, mine = json.loads(line), wr.plan(B, N, d, None if gt < 0 else gt)
        assert {k: p[k] for k in mine} == mine, (B, N, d, gt)
