"""tests/adam_reference.py pinned on the CPU: the float64 restatements are torch.optim.Adam's and torch.optim.SparseAdam's, the fp32
restatement stays inside the caps the GPU sweeps (test_adam_shapes.py, test_adam_rows_shapes.py) assert, the sweep's inputs make
a skipped, doubled or misplaced update an error of at least 64 caps, and the two new entry points refuse what they document --
return code and exact okge_last_error() text, with host pointers, before any launch (the table style of test_abi_refusals.py)."""
import ctypes
import os
import re
from ctypes import addressof

import numpy as np
import pytest
import torch

import adam_reference as A
from open_knowledge_graph_embeddings_amd import _native as nv

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the float64 restatements are torch's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
def test_adam64_is_torch_adam(wd):
    """5 steps of torch.optim.Adam in float64 on the CPU against adam64 with the hyper-parameters as given (exact=True)"""
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal((7, 5))
    par = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([par], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, 6):
        g = rng.standard_normal(p0.shape) * 10.0 ** rng.integers(-3, 1, p0.shape)
        par.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        r = A.adam64(p, g, m, v, t, LR, BETAS, EPS, wd, exact=True)
        p, m, v = r.p, r.m, r.v
        st = opt.state[par]
        np.testing.assert_allclose(p, par.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        assert float(st["step"]) == t


def test_sparse_adam64_is_torch_sparse_adam():
    """5 steps of torch.optim.SparseAdam in float64 with duplicate ids: sparse_adam64 on torch's own coalesced sum (float64, where
    the order of the additions does not matter); rows no id names do not move.  One of the steps has an empty gradient: the
    tables stand still and the step count still advances."""
    rng = np.random.default_rng(2)
    rows, d = 11, 4
    p0 = rng.standard_normal((rows, d))
    par = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.SparseAdam([par], lr=LR, betas=BETAS, eps=EPS)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, 6):
        ids = rng.integers(0, rows - 3, 9) if t != 3 else np.zeros(0, np.int64)
        vals = rng.standard_normal((ids.size, d))
        par.grad = torch.sparse_coo_tensor(torch.tensor(ids[None, :], dtype=torch.int64), torch.tensor(vals, dtype=torch.float64), (rows, d))
        opt.step()
        dense = np.zeros((rows, d))
        np.add.at(dense, ids, vals)
        named = np.unique(ids)
        assert ids.size == 0 or named.size < ids.size           # (duplicates are present)
        r = A.sparse_adam64(p[named], dense[named], m[named], v[named], t, LR, BETAS, EPS, exact=True)
        p[named], m[named], v[named] = r.p, r.m, r.v
        st = opt.state[par]
        np.testing.assert_allclose(p, par.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)
        assert float(st["step"]) == t


def test_coalesce32_adds_in_ascending_position():
    ids = np.array([3, 1, 3, 9, 3, -1, 1], np.int32)
    g = np.array([[1e8], [1.0], [1.0], [5.0], [-1e8], [7.0], [2.0]], np.float32)
    uniq, acc, bad = A.coalesce32(ids, g, 9)
    assert uniq.tolist() == [1, 3] and bad == 2
    assert acc[:, 0].tolist() == [3.0, float(np.float32(np.float32(np.float32(1e8) + np.float32(1.0)) - np.float32(1e8)))]
    assert acc[1, 0] == 0.0                                      # (1e8 + 1 rounds back to 1e8 in fp32: the order is visible)


# ---- the fp32 chains stay inside the caps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-10, 1e-2])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_fp32_restatement_stays_inside_its_caps(warm, t, wd):
    p, g, m, v = A.sweep_inputs(500_003, 5, warm)
    g = g.copy()
    g[::5] = 0.0
    r = A.adam64(p, g, m, v, t, LR, BETAS, EPS, wd)
    ok = ~A.underflowed(r)
    assert ok.all()
    ratios = A.cap_ratios(A.adam32(p, g, m, v, t, LR, BETAS, EPS, wd), r, m, v)
    print("RATIO self-dense-%s-t%d-wd%g p %.3f m %.3f v %.3f" % ("warm" if warm else "cold", t, wd, *ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_fp32_sparse_restatement_stays_inside_its_caps(warm, t):
    p, g, m, v = A.sweep_inputs(500_003, 6, warm)
    r = A.sparse_adam64(p, g, m, v, t, LR, BETAS, EPS)
    assert not A.underflowed(r).any()
    ratios = A.cap_ratios(A.sparse_adam32(p, g, m, v, t, LR, BETAS, EPS), r, m, v, sparse=True)
    print("RATIO self-sparse-%s-t%d p %.3f m %.3f v %.3f" % ("warm" if warm else "cold", t, *ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("n", [1025, 262_147])
def test_gradient_cases_are_not_vacuous(n, warm, sparse):
    """on the GPU cases' inputs every one of the three updates is more than 64 caps on at least 99 % of the elements (float64
    alone): skipping or doubling an update, or applying it to the neighbouring element, cannot hide inside the tolerance"""
    p, g, m, v = A.sweep_inputs(n, 1, warm)
    for t in (1, 2, 1000):
        r = A.sparse_adam64(p, g, m, v, t, LR, BETAS, EPS) if sparse else A.adam64(p, g, m, v, t, LR, BETAS, EPS, 1e-10)
        assert not A.underflowed(r).any()
        caps = A.adam_caps(r, m, v, sparse)
        moves = (np.abs(r.delta), np.abs(r.m - m), np.abs(r.v - v))
        for name, move, cap in zip("pmv", moves, caps):
            share = float(np.mean(move > 64 * cap))
            print("SHARE n=%d %s t=%d %s: move > 64 caps on %.4f of the elements" % (n, "warm" if warm else "cold", t, name, share))
            assert share >= 0.99, (n, warm, sparse, t, name, share)
        # misplaced: the neighbour's update instead of the element's own
        for name, got, want, cap in zip("pmv", (np.roll(r.p, 1), np.roll(r.m, 1), np.roll(r.v, 1)), (r.p, r.m, r.v), caps):
            share = float(np.mean(np.abs(got - want) > 64 * cap))
            assert share >= 0.99, (n, warm, sparse, t, name, "misplaced", share)


# ---- the header and the bindings --------------------------------------------------------------------------------------------
def test_header_declares_the_adam_entry_points():
    text = open(os.path.join(ROOT, "include", "okge.h")).read()
    assert re.search(r"#define OKGE_ABI_VERSION 2\b", text)
    for sym in ("okge_adam_step", "okge_adam_rows_workspace_bytes", "okge_adam_rows"):
        assert re.search(r"\b%s\(" % sym, text), sym
        assert sym in nv.EXPORTS
    for struct in ("okge_adam_tensor", "okge_adam_rows_tensor"):
        assert re.search(r"typedef struct %s \{" % struct, text), struct
    assert ctypes.sizeof(nv.AdamTensor) == 48 and ctypes.sizeof(nv.AdamRowsTensor) == 72
    assert nv.lib().okge_abi_version() == 2


# ---- refusals: host pointers, never reaching a launch -------------------------------------------------------------------------
INV, UNS, WS = -1, -2, -3
_RAW = (ctypes.c_char * 4096)()
P = (addressof(_RAW) + 255) & ~255
P4 = P + 4
HUGE = 1 << 40
ALIGN = "adam buffers must be 16-byte aligned"
HYPER = "adam needs 0 <= beta1, beta2 < 1, eps >= 0 and lr >= 0"
ADAM_WS = "workspace too small (okge_adam_rows_workspace_bytes)"


def adam_t(p=P, g=P, m=P, v=P, state=P, n=16):
    return nv.AdamTensor(p, g, m, v, state, n)


def rows_t(p=P, m=P, v=P, state=P, ids=P, g=P, ld_g=4, n=3, table_rows=10, row_len=4):
    return nv.AdamRowsTensor(p, m, v, state, ids, g, ld_g, n, table_rows, row_len)


def arr(kind, *items):
    return (kind * len(items))(*items)


def step(tensors, n=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, zero=0):
    a = arr(nv.AdamTensor, *tensors) if tensors is not None else None
    return "okge_adam_step", (a, len(tensors) if n is None else n, lr, b1, b2, eps, wd, zero, None)


def rows(tensors, n=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, ws=P, ws_bytes=HUGE):
    a = arr(nv.AdamRowsTensor, *tensors) if tensors is not None else None
    return "okge_adam_rows", (a, len(tensors) if n is None else n, lr, b1, b2, eps, ws, ws_bytes, None)


NAN = float("nan")
REFUSALS = [
    ("step-null-array", step(None, n=1), INV, "one or two tensors"),
    ("step-zero-tensors", step([adam_t()], n=0), INV, "one or two tensors"),
    ("step-three-tensors", step([adam_t(), adam_t(), adam_t()]), INV, "one or two tensors"),
    ("step-null-p", step([adam_t(p=None)]), INV, "bad adam arguments"),
    ("step-null-g", step([adam_t(g=None)]), INV, "bad adam arguments"),
    ("step-null-exp-avg", step([adam_t(), adam_t(m=None)]), INV, "bad adam arguments"),
    ("step-null-exp-avg-sq", step([adam_t(v=None)]), INV, "bad adam arguments"),
    ("step-null-state", step([adam_t(state=None)]), INV, "bad adam arguments"),
    ("step-negative-n", step([adam_t(n=-1)]), INV, "bad adam arguments"),
    ("step-unaligned-p", step([adam_t(p=P4)]), INV, ALIGN),
    ("step-unaligned-g", step([adam_t(g=P4)]), INV, ALIGN),
    ("step-unaligned-exp-avg", step([adam_t(m=P4)]), INV, ALIGN),
    ("step-unaligned-exp-avg-sq", step([adam_t(), adam_t(v=P4)]), INV, ALIGN),
    ("step-beta1-one", step([adam_t()], b1=1.0), INV, HYPER),
    ("step-beta1-negative", step([adam_t()], b1=-0.1), INV, HYPER),
    ("step-beta2-one", step([adam_t()], b2=1.0), INV, HYPER),
    ("step-beta2-nan", step([adam_t()], b2=NAN), INV, HYPER),
    ("step-eps-negative", step([adam_t()], eps=-1e-8), INV, HYPER),
    ("step-lr-negative", step([adam_t()], lr=-1e-3), INV, HYPER),
    ("step-wd-negative", step([adam_t()], wd=-1e-3), INV, "adam needs weight_decay >= 0"),
    ("step-zero-grad-3", step([adam_t()], zero=3), INV, "zero_grad is 0 (none), 1 (both) or 2 (second tensor only)"),
    ("rows-null-array", rows(None, n=1), INV, "one or two tensors"),
    ("rows-zero-tensors", rows([rows_t()], n=0), INV, "one or two tensors"),
    ("rows-three-tensors", rows([rows_t(), rows_t(), rows_t()]), INV, "one or two tensors"),
    ("rows-negative-n", rows([rows_t(n=-1)]), INV, "negative occurrence count"),
    ("rows-too-many", rows([rows_t(n=(1 << 20) + 1)]), UNS, "okge_adam_rows takes up to 2^20 occurrence rows per tensor"),
    ("rows-null-state-empty", rows([rows_t(n=0, state=None)]), INV, "null tensor"),
    ("rows-null-p", rows([rows_t(p=None)]), INV, "null tensor"),
    ("rows-null-exp-avg", rows([rows_t(m=None)]), INV, "null tensor"),
    ("rows-null-exp-avg-sq", rows([rows_t(), rows_t(v=None)]), INV, "null tensor"),
    ("rows-null-ids", rows([rows_t(ids=None)]), INV, "null tensor"),
    ("rows-null-g", rows([rows_t(g=None)]), INV, "null tensor"),
    ("rows-ld-below-row", rows([rows_t(ld_g=3)]), INV, "bad table shape / leading dimension"),
    ("rows-no-table", rows([rows_t(table_rows=0)]), INV, "bad table shape / leading dimension"),
    ("rows-beta1-one", rows([rows_t()], b1=1.0), INV, HYPER),
    ("rows-beta2-negative", rows([rows_t()], b2=-1.0), INV, HYPER),
    ("rows-eps-negative", rows([rows_t()], eps=-1.0), INV, HYPER),
    ("rows-lr-nan", rows([rows_t()], lr=NAN), INV, HYPER),
    ("rows-null-workspace", rows([rows_t()], ws=None), WS, ADAM_WS),
    ("rows-small-workspace", rows([rows_t(n=1000)], ws_bytes=1000 * 16 - 1), WS, ADAM_WS),
]


@pytest.mark.parametrize("call,rc,msg", [pytest.param(c, rc, msg, id=name) for name, c, rc, msg in REFUSALS])
def test_refusals(call, rc, msg):
    L = nv.lib()
    fn, args = call
    assert getattr(L, fn)(*args) == rc
    assert L.okge_last_error().decode() == msg


def test_rows_workspace_is_the_adagrad_one():
    L = nv.lib()
    for n0, n1 in ((0, 0), (1, 0), (1000, 7), (1 << 20, 1 << 20)):
        assert L.okge_adam_rows_workspace_bytes(n0, n1) == L.okge_adagrad_rows_workspace_bytes(n0, n1)
    assert L.okge_adam_rows_workspace_bytes((1 << 20) + 1, 0) == 0
