"""The wide path's planner (okge_plan.h: plan_wide, wide_train_layout, wide_score_layout), driven on the CPU through
tests/wide_plan_driver.cpp: shapes, candidate ranges, the workspace layout, and that the built library sizes its workspaces with
the same functions.  Slot sizes 513 .. 4096 are wide; 512 and 4097 are not."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "wide_plan_driver.cpp")

BS = [1, 64, 65, 512, 4096]
NS = [1, 64, 65, 14541, 312500]
DS = [513, 528, 1000, 4096]
GTS = [-1, 1]                      # OKGE_GT_MBYTES: default (1024), 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cc = next((p for p in map(shutil.which, ("c++", "g++", "hipcc")) if p), None)
    assert cc, "no C++ compiler on the path"
    exe = str(tmp_path_factory.mktemp("wide_plan") / "wide_plan_driver")
    built = subprocess.run([cc, "-std=c++17", "-O1", "-o", exe, DRIVER], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        lines = ["%d %d %d %d" % c for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [json.loads(o) for o in out]
    return run


@pytest.fixture(scope="module")
def grid(plan):
    cases = list(itertools.product(BS, NS, DS, GTS))
    return cases, plan(cases)


def test_shapes(grid):
    for (B, N, d, gt), p in zip(*grid):
        assert p["ok"] == 1 and p["tile_n"] == 128
        assert p["Bpad"] % 128 == 0 and 0 <= p["Bpad"] - B < 128 and p["row_blocks"] == p["Bpad"] // 128
        assert p["ldq"] % 16 == 0 and 0 <= p["ldq"] - d < 16
        assert p["tiles"] == -(-N // 128)
        assert p["n_loss_partials"] == p["tiles"] * p["row_blocks"]


def test_ranges_cover_the_candidates_once_within_budget(grid):
    for (B, N, d, gt), p in zip(*grid):
        w = p["tile_n"]
        assert p["range_n"] == p["range_tiles"] * w and p["ldg"] == p["range_n"]           # whole tiles
        assert p["range_tiles"] >= 1
        # ranges [r * range_n, min(N, (r + 1) * range_n)) cover [0, N) exactly once, none empty
        assert (p["n_ranges"] - 1) * p["range_n"] < N <= p["n_ranges"] * p["range_n"]
        # G + Cm + dC of one range within the budget, except the unavoidable one-tile minimum
        budget = (1024 if gt < 0 else gt) << 20
        assert p["tile_bytes"] == w * (p["Bpad"] + 2 * p["ldq"]) * 4
        range_bytes = p["range_tiles"] * p["tile_bytes"]
        assert range_bytes <= budget or p["range_tiles"] == 1
        # ... and not needlessly short: one more range could not have been saved
        if p["n_ranges"] > 1 and p["range_tiles"] > 1:
            assert (p["n_ranges"] - 1) * (budget // p["tile_bytes"]) < p["tiles"]
        # the dQ product's split of a range's candidates
        kn = min(p["range_n"], N)
        assert 1 <= p["dq_splits"] <= 64 and p["dq_k_per"] % 16 == 0
        assert (p["dq_splits"] - 1) * p["dq_k_per"] < kn <= p["dq_splits"] * p["dq_k_per"]


def test_layout_regions_are_disjoint_aligned_and_add_up(grid):
    for (B, N, d, gt), p in zip(*grid):
        end = 0
        for off, size in p["regions"]:
            assert off % 256 == 0 and off >= end, (B, N, d, gt)
            end = off + size
        assert p["total"] >= end and p["total"] - end < 256
        assert p["regions"][0][0] == 0 == p["score_off_Q"]
        assert p["score_total"] == p["score_bytes"] == p["regions"][1][0]                  # the query block alone
        assert p["lse_bytes"] == p["regions"][6][0]                                        # ... + the row log-sum-exp part
        assert p["regions"][7][1] == p["Bpad"] * p["range_n"] * 4


def test_512_and_4097_are_not_wide(plan):
    got = plan([(64, 100, 512, -1), (64, 100, 4097, -1), (64, 100, 513, -1), (64, 100, 4096, -1), (0, 100, 600, -1), (64, 0, 600, -1)])
    assert [(g["ok"], g["is_wide"]) for g in got] == [(0, 0), (0, 0), (1, 1), (1, 1), (0, 1), (0, 1)]


@pytest.mark.parametrize("gt", GTS, ids=["default", "gt_mbytes_1"])
def test_library_answers_the_planner_sizes(plan, monkeypatch, gt):
    """the built library sizes the wide workspaces as the driver does, and answers 0 above 4096"""
    from open_knowledge_graph_embeddings_amd import _native
    if _native.needs_build():
        _native.build_native()
    L = _native.lib()
    monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    if gt >= 0:
        monkeypatch.setenv("OKGE_GT_MBYTES", str(gt))
    shapes = list(itertools.product(BS, NS, DS))
    for (B, N, d), p in zip(shapes, plan([(B, N, d, gt) for B, N, d in shapes])):
        assert L.okge_train_workspace_bytes(B, N, d) == p["total"]
        assert L.okge_lse_workspace_bytes(B, N, d) == p["lse_bytes"]
        assert L.okge_score_workspace_bytes(B, d) == p["score_total"]
        assert L.okge_train_row_grads_workspace_bytes(B, N, d) == 0        # the row-sparse step stops at 512
    assert L.okge_train_workspace_bytes(64, 100, 4097) == 0
    assert L.okge_score_workspace_bytes(64, 4097) == 0
    assert L.okge_lse_workspace_bytes(64, 100, 4097) == 0
