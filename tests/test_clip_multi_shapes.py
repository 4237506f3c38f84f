"""okge_clip_grad_norm_multi (sqnorm_multi_kernel, clip_coef_kernel, scale_multi_kernel; csrc/okge_optim.hip) through the C ABI:
1, 2, 5 and 8 tensors of mixed sizes, the norm below max_norm / above it / all-zero gradients, with and without touched-row maps
(NaN in the gradient rows a map does not stamp: they must survive bit for bit, and must not reach the norm).  The bounds are
test_optim_shapes.py::test_clip_grad_norm's: norm_out is an fp32 value within 1 fp32 ulp of fp32(sqrt(sum g^2)) at float64,
coef == clip_coef(fp32(norm_out), max_norm), every gradient bit-equal to g * coef in fp32 (to g when coef == 1).  Two runs are
bit-identical, norm_out = NULL gives the same gradients, and the workspace of exactly the asked size keeps its guard words."""
import numpy as np
import pytest
import torch

import optim_reference as R
from test_optim_shapes import NAN_BITS, Guarded, same_bits

pytestmark = pytest.mark.gpu

STAMP = 9
SIZES = (0, 1, 3, 255, 1027, 262_147)
# per case: (n,) a dense tensor, (rows, row_len) a mapped one
DENSE = {
    "1": [(1027,)],
    "1-empty": [(0,)],
    "2": [(3,), (262_147,)],
    "5": [(255,), (0,), (1027,), (1,), (262_147,)],
    "8": [(1,), (262_147,), (3,), (0,), (255,), (1027,), (3,), (255,)],
}
MAPPED = {
    "1-map": [(65, 200)],
    "2-map": [(1000, 8), (1027,)],
    "5-map": [(63, 512), (255,), (1, 4), (64, 8), (0,)],
    "8-map": [(1000, 200), (3,), (65, 4), (262_147,), (1, 512), (1,), (64, 200), (1027,)],
}


@pytest.fixture(scope="module")
def hp(okge_lib):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


@pytest.fixture(scope="module")
def ws(hp):
    """guard words around a workspace of exactly the asked size"""
    return Guarded(n=int(hp.lib.okge_clip_grad_norm_multi_workspace_bytes()), dtype=torch.uint8)


class Case:
    def __init__(self, shapes, kind, seed):
        rng = np.random.default_rng([90, seed, len(shapes)])
        self.host, self.live, self.maps = [], [], []
        for sh in shapes:
            n = int(np.prod(sh))
            h = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 1, n)).astype(np.float32)
            if kind == "zero":
                h[:] = 0
            live, m = np.ones(n, bool), None
            if len(sh) == 2:
                m = rng.choice(np.array([STAMP, STAMP, 0, STAMP - 1, STAMP + 1, 255], np.uint8), sh[0])
                m[0] = STAMP
                live = np.repeat(m == STAMP, sh[1])
            self.host.append(h)
            self.live.append(live)
            self.maps.append(m)
        self.shapes = shapes
        sq = sum(float(np.sum(h[lv].astype(np.float64) ** 2)) for h, lv in zip(self.host, self.live))
        self.total = np.float32(np.sqrt(sq))
        if self.total == 0:                                    # (only empty tensors: any max_norm is "below")
            kind = "zero"
        self.max_norm = {"below": 2.0 * float(self.total), "above": 0.37 * float(self.total), "zero": 1.0}[kind]
        self.kind = kind

    def device(self):
        """fresh device copies: gradients with NaN in the rows a map does not stamp, the maps"""
        gs, maps = [], []
        for h, lv, m in zip(self.host, self.live, self.maps):
            x = h.copy().view(np.uint32)
            x[~lv] = NAN_BITS
            gs.append(Guarded(x.view(np.float32)))
            maps.append(None if m is None else Guarded(m))
        return gs, maps


def call(hp, case, gs, maps, norm, ws, ws_len=None):
    from open_knowledge_graph_embeddings_amd import _native as N
    arr = (N.GradTensor * len(gs))()
    for a, g, m, sh in zip(arr, gs, maps, case.shapes):
        a.g, a.n = g.ptr(), g.n
        if m is not None:
            a.row_touched, a.row_len, a.touched_stamp = m.ptr(), sh[1], STAMP
    return int(hp.lib.okge_clip_grad_norm_multi(arr, len(gs), case.max_norm, None if norm is None else norm.ptr(), ws.ptr(),
                                                ws.n if ws_len is None else ws_len, hp._stream()))


@pytest.mark.parametrize("kind", ["below", "above", "zero"])
@pytest.mark.parametrize("name", list(DENSE) + list(MAPPED))
def test_clip_grad_norm_multi(hp, ws, name, kind):
    assert set(sh[0] for shapes in DENSE.values() for sh in shapes) == set(SIZES)
    shapes = (DENSE.get(name) or MAPPED[name])
    c = Case(shapes, kind, len(name))
    case = "clipm-%s-%s" % (name, kind)
    gs, maps = c.device()
    norm = Guarded(torch.full((1,), -1.0, dtype=torch.float64))
    assert call(hp, c, gs, maps, norm, ws) == 0, (case, hp.lib.okge_last_error())
    torch.cuda.synchronize()
    got = float(norm.np()[0])
    ulps = abs(got - float(c.total)) / float(np.spacing(c.total)) if c.total > 0 else abs(got)
    print("RATIO %s norm_out %.3f" % (case, ulps))             # (distance from fp32(sqrt(sum g^2)) in fp32 ulps: 0 or 1)
    assert float(np.float32(got)) == got and ulps <= 1.0, (case, got, float(c.total))
    coef = R.clip_coef(np.float32(got), c.max_norm)
    if c.kind != "above":
        assert coef == np.float32(1.0), (case, coef)
    else:
        assert coef < np.float32(0.5)
    for k, (g, h, lv, m) in enumerate(zip(gs, c.host, c.live, maps)):
        want = (h * coef).view(np.uint32)
        want[~lv] = NAN_BITS                                   # rows the map does not stamp: neither read nor written
        assert np.array_equal(g.np().view(np.uint32), want), (case, "g%d" % k)
        assert g.intact() and (m is None or (m.intact() and np.array_equal(m.np(), c.maps[k]))), (case, k)
    assert norm.intact() and ws.intact(), case
    # a second run from the same inputs: bit-identical norm and gradients; norm_out null: the same gradients
    gs2, maps2 = c.device()
    norm2 = Guarded(torch.full((1,), -1.0, dtype=torch.float64))
    assert call(hp, c, gs2, maps2, norm2, ws) == 0
    gs3, maps3 = c.device()
    assert call(hp, c, gs3, maps3, None, ws) == 0
    torch.cuda.synchronize()
    assert same_bits(norm.v, norm2.v), (case, "the norm differs between two runs")
    for k, (a, b, d) in enumerate(zip(gs, gs2, gs3)):
        assert same_bits(a.v, b.v), (case, k, "second run")
        assert same_bits(a.v, d.v), (case, k, "norm_out null")
    assert ws.intact(), case


def test_refusals_write_nothing(hp, ws):
    c = Case([(6, 4), (8,)], "below", 1)
    gs, maps = c.device()
    norm = Guarded(torch.full((1,), -1.0, dtype=torch.float64))
    wholes = [g.whole for g in gs] + [norm.whole, ws.whole, maps[0].whole]
    before = [w.clone() for w in wholes]
    assert call(hp, c, gs, maps, norm, ws, ws_len=ws.n - 1) == -3
    c.max_norm = 0.0
    assert call(hp, c, gs, maps, norm, ws) == -1
    c.max_norm = float("nan")
    assert call(hp, c, gs, maps, norm, ws) == -1
    torch.cuda.synchronize()
    for w, b in zip(wholes, before):
        assert same_bits(w, b) if w.is_floating_point() else torch.equal(w, b)
