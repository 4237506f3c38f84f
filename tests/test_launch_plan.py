"""CPU-only: the launch planner (csrc/okge_plan.h) -- shapes, launch plans and workspace layouts as plain integer arithmetic
on (B, N, d, CU count, the five OKGE_* overrides).  tests/plan_driver.cpp includes nothing but that header, is compiled here with
the host compiler, and prints every plan field as JSON; the tests check the invariants the launches rely on, a table of plans
pinned from the code before the planner was cut out of the C ABI's host layer (now csrc/okge_api_*.hip), and that the built library
answers the same sizes."""
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "open_knowledge_graph_embeddings_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "plan_driver.cpp")

BS = [1, 63, 64, 65, 77, 128, 192, 512, 4096]
NS = [1, 64, 65, 900, 2000, 4500, 10000, 14541, 16384, 16448, 17600, 19200, 312500, 2500000]
DS = [16, 17, 64, 128, 200, 208, 209, 256, 257, 512]
CUS = [64, 256, 304]
KNOB_NAMES = ("TAIL_SPLIT", "GT_MBYTES", "B_SPLIT", "STREAMK", "DQ_SPLIT")
KNOB_SETS = [{}, {"GT_MBYTES": 1}, {"TAIL_SPLIT": 0}, {"B_SPLIT": 2}, {"STREAMK": 0}, {"STREAMK": 0, "B_SPLIT": 2}, {"DQ_SPLIT": 3}]
TOPK_K = 10


def case_line(B, N, d, cus, knobs, k=TOPK_K, range_n=0, n_groups=None, n_filter=None):
    n_groups = 3 * B if n_groups is None else n_groups
    n_filter = 5 * B if n_filter is None else n_filter
    return " ".join(str(x) for x in (B, N, d, cus, k, range_n, n_groups, n_filter, *(knobs.get(n, "-") for n in KNOB_NAMES)))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """-> run(lines): the driver's JSON answers.  A compile failure fails the tests: no ROCm include path, no HIP flag."""
    cc = next((p for p in map(shutil.which, ("c++", "g++", "hipcc")) if p), None)
    assert cc, "no C++ compiler on the path"
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    built = subprocess.run([cc, "-std=c++17", "-O1", "-o", exe, DRIVER], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [json.loads(o) for o in out]
    return run


@pytest.fixture(scope="module")
def grid(plan):
    cases = list(itertools.product(BS, NS, DS, CUS, KNOB_SETS))
    return cases, plan([case_line(*c) for c in cases])


def test_planner_headers_are_gpu_free():
    """the driver and the headers it pulls in name no HIP header: standard headers and okge_consts.h only"""
    seen = {}
    for path in (DRIVER, os.path.join(CSRC, "okge_plan.h"), os.path.join(CSRC, "okge_consts.h")):
        seen[os.path.basename(path)] = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(path).read(), re.M)
    assert seen["okge_consts.h"] == []
    assert [i for i in seen["okge_plan.h"] if "." in i] == ["okge_consts.h"]
    assert [i for i in seen["plan_driver.cpp"] if "." in i] == ["../open_knowledge_graph_embeddings_amd/csrc/okge_plan.h"]
    assert not any("hip" in i for incs in seen.values() for i in incs)


def ordered_regions(offsets, total):
    assert all(o % 256 == 0 for o in offsets) and total % 256 == 0
    assert all(a <= b for a, b in zip(offsets, offsets[1:])) and offsets[-1] <= total


def check_sweep(sw, tiles, Bpad, B, KB, cus):
    assert sw["tiles"] == tiles and sw["main_tiles"] + sw["tail_tiles"] == tiles and sw["main_tiles"] >= 0
    if KB > 16:
        assert sw["sk_wgs"] == min(cus, 511, tiles * ((B + 31) // 32)) and sw["tail_tiles"] == 0
    else:
        assert sw["sk_wgs"] == 0
    if sw["tail_tiles"]:
        assert sw["tail_split"] > 1 and sw["tail_split"] * sw["tail_b_per_block"] >= Bpad > (sw["tail_split"] - 1) * sw["tail_b_per_block"]


def test_plan_invariants(grid):
    for (B, N, d, cus, knobs), p in zip(*grid):
        assert p["ok"] == 1
        Bpad, KB, D16, tiles = p["Bpad"], p["KB"], p["D16"], p["tiles"]
        assert Bpad % 64 == 0 and 0 <= Bpad - B < 64 and D16 == 16 * KB >= d and p["ldq"] == D16 and tiles == -(-N // 64)
        # ranges: tiles 0 .. tiles-1 exactly once, all but the last of range_tiles tiles
        rt, nr = p["range_tiles"], p["n_ranges"]
        last = tiles - (nr - 1) * rt
        assert 1 <= last <= rt and p["range_n"] == p["ldg"] == rt * 64
        assert p["lse_ranges"] == [rt, nr, rt * 64]
        # ranges of whole rounds when the rule of the code this was cut from asks for them
        budget_tiles = max(1, min((max(1, knobs.get("GT_MBYTES", 1024)) << 20) // (Bpad * 64 * 4), tiles))
        if -(-tiles // budget_tiles) > 1 and KB <= 16 and budget_tiles >= cus:
            assert rt % cus == 0
        # batch split, tail split of the last train range, stream-K
        assert p["b_split"] * p["b_per_block"] >= Bpad > (p["b_split"] - 1) * p["b_per_block"]
        if p["tail_tiles"]:
            assert p["tail_split"] > 1 and p["tail_tiles"] <= last and p["b_split"] == 1 and p["sk_wgs"] == 0
            assert p["tail_split"] * p["tail_b_per_block"] >= Bpad > (p["tail_split"] - 1) * p["tail_b_per_block"]
        else:
            assert p["tail_split"] == 0
        if p["sk_wgs"]:
            assert KB == 32 and nr == 1 and p["sk_chunks"] == (B + 31) // 32
            assert p["sk_wgs"] == min(cus, 511, tiles * p["sk_chunks"]) and p["b_split"] == 1
        check_sweep(p["sweep"], tiles, Bpad, B, KB, cus)
        check_sweep(p["sweep_last"], last, Bpad, B, KB, cus)
        assert 1 <= p["nsplit"] <= rt
        # what the launches write: one loss partial per workgroup; partial candidate gradients per stream-K workgroup (two
        # slabs of a tile), per batch split (all tiles) or per row split of the tail tiles
        tile_floats = 64 * D16
        if p["sk_wgs"]:
            partials, slab_floats = p["sk_wgs"], 2 * p["sk_wgs"] * tile_floats
        elif p["b_split"] > 1:
            partials, slab_floats = tiles * p["b_split"], p["b_split"] * tiles * tile_floats
        else:
            partials = tiles + p["tail_tiles"] * max(0, p["tail_split"] - 1)
            slab_floats = p["tail_split"] * p["tail_tiles"] * tile_floats
        assert p["n_loss_partials"] == partials and p["dc_slabs"] * p["dc_slab_rows"] * D16 == slab_floats
        assert partials * 8 <= p["loss_bytes"] <= p["off_GT"] - p["off_loss"]
        assert slab_floats * 4 == p["dcs_bytes"] <= p["off_Qp"] - p["off_dcs"]
        # layouts
        names = ("off_Q", "off_tptr", "off_stats", "off_lse", "off_ysum", "off_run", "off_loss", "off_GT", "off_Cm", "off_slab",
                 "off_dcs", "off_Qp")
        ordered_regions([p[n] for n in names], p["total"])
        assert p["off_tptr"] - p["off_Q"] >= Bpad * D16 * 4 and p["off_lse"] - p["off_stats"] >= (4 if KB > 16 else 1) * rt * Bpad * 8
        assert p["off_stats"] - p["off_tptr"] >= (tiles + 1) * 4 and p["off_Cm"] - p["off_GT"] >= Bpad * p["ldg"] * 4
        assert p["off_slab"] - p["off_Cm"] >= rt * 64 * D16 * (4 if KB > 13 else 6)
        assert p["off_dcs"] - p["off_slab"] >= p["nsplit"] * Bpad * D16 * 4
        assert p["total"] - p["off_Qp"] >= (Bpad * D16 * 6 if KB == 13 else 0)
        assert p["score_total"] == p["score_bytes"] <= p["lse_bytes"] <= p["total"] and p["lse_bytes"] == p["off_loss"]
        ordered_regions(p["rows"][:3], p["rows"][3])
        assert p["rows"][0] >= p["total"] and p["rows"][3] - p["rows"][2] >= 2 * B * 4
        t_rt, t_nr, t_rn, *t_off = p["topk"]
        ordered_regions(t_off[:3], t_off[3])
        assert 1 <= tiles - (t_nr - 1) * t_rt <= t_rt and t_rn == t_rt * 64
        assert t_off[0] == 0 and t_off[2] - t_off[1] >= t_rt * Bpad * TOPK_K * 8 and t_off[3] - t_off[2] >= (Bpad * t_rn * 4 if KB > 16 else 0)
        ordered_regions(p["eval"][:7], p["eval"][7])
        assert p["eval"][0] == 0 and p["eval"][1] == p["score_bytes"]     # one query block in the score, top-k and eval layouts


def test_invalid_shapes_and_calls_fail(plan):
    bad = plan([case_line(0, 10, 16, 256, {}), case_line(10, 0, 16, 256, {}), case_line(10, 10, 0, 256, {}), case_line(-1, 10, 16, 256, {})])
    assert [b["ok"] for b in bad] == [0, 0, 0, 0]
    calls = plan([case_line(64, 1000, 64, 256, {}, k=0), case_line(64, 1000, 64, 256, {}, k=65), case_line(64, 1000, 64, 256, {}, range_n=-1),
                  case_line(64, 1000, 64, 256, {}, n_groups=-1), case_line(64, 1000, 64, 256, {}, n_filter=-1)])
    assert [c["topk"] is None for c in calls] == [True, True, True, False, False]
    assert [c["eval"] is None for c in calls] == [False, False, False, True, True]


# B, N, d -> KB, tiles, ranges x tiles, b_split / rows, stream-K wgs / chunks, tail tiles x split (rows), nsplit, train bytes:
# the answers at 256 CUs with no override of the code the planner was cut from
PINNED = [
    ((512, 14541, 200), (13, 228, 1, 228, 1, 512, 0, 0, 0, 0, 512, 32, 66541312)),
    ((512, 10000, 512), (32, 157, 1, 157, 1, 512, 256, 16, 0, 0, 512, 32, 145452800)),
    ((4096, 8192, 256), (16, 128, 1, 128, 2, 2048, 0, 0, 0, 0, 4096, 4, 197203200)),
    ((4096, 312500, 256), (16, 4883, 5, 1024, 1, 4096, 0, 0, 19, 13, 320, 4, 1312412160)),
    ((192, 17600, 64), (4, 275, 1, 275, 1, 192, 0, 0, 19, 3, 64, 80, 26890240)),
    ((256, 16448, 128), (8, 257, 1, 257, 2, 128, 0, 0, 0, 0, 256, 64, 56957440)),
    ((77, 900, 64), (4, 15, 1, 15, 2, 64, 0, 0, 0, 0, 128, 15, 1940224)),
    ((1, 1, 16), (4, 1, 1, 1, 1, 64, 0, 0, 0, 0, 64, 1, 77312)),
]
PINNED_FIELDS = ("KB", "tiles", "n_ranges", "range_tiles", "b_split", "b_per_block", "sk_wgs", "sk_chunks", "tail_tiles", "tail_split",
                 "tail_b_per_block", "nsplit", "total")


def test_pinned_plans(plan):
    got = plan([case_line(*shape, 256, {}) for shape, _ in PINNED])
    for (shape, want), p in zip(PINNED, got):
        assert tuple(p[f] for f in PINNED_FIELDS) == want, shape
    p, = plan([case_line(512, 14541, 200, 256, {"GT_MBYTES": 1})])
    assert (p["n_ranges"], p["range_tiles"], p["nsplit"], p["total"]) == (29, 8, 8, 6305536)


@pytest.mark.parametrize("knobs", [{}, {"GT_MBYTES": 1}], ids=["default", "gt_mbytes_1"])
def test_library_answers_the_planner_sizes(plan, monkeypatch, knobs):
    """the built library (no device here: it plans for 256 CUs) sizes every workspace as the driver does"""
    from open_knowledge_graph_embeddings_amd import _native
    if _native.needs_build():
        _native.build_native()
    L = _native.lib()
    for name in KNOB_NAMES:
        monkeypatch.delenv("OKGE_" + name, raising=False)
    for name, v in knobs.items():
        monkeypatch.setenv("OKGE_" + name, str(v))
    shapes = list(itertools.product(BS, NS, DS))
    for (B, N, d), p in zip(shapes, plan([case_line(B, N, d, 256, knobs) for B, N, d in shapes])):
        assert L.okge_train_workspace_bytes(B, N, d) == p["total"]
        assert L.okge_lse_workspace_bytes(B, N, d) == p["lse_bytes"]
        assert L.okge_score_workspace_bytes(B, d) == p["score_total"]
        assert L.okge_train_row_grads_workspace_bytes(B, N, d) == p["rows"][3]
        assert L.okge_topk_workspace_bytes(B, N, d, TOPK_K, 0) == p["topk"][6]
        assert L.okge_eval_workspace_bytes(B, N, d, 3 * B, 5 * B) == p["eval"][7]
