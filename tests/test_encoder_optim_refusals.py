"""CPU-only: every refusal of okge_adam_multi and okge_clip_grad_norm_multi that is reached before the first HIP call, by return
code and exact okge_last_error() text (in the manner of test_abi_refusals.py: pointers a refusal path only compares against NULL
or tests for alignment point at a small host buffer), and the Python-side refusals of the keywords optimizer / betas / grad_clip
on the token-encoded and Tucker3 steps.  Default keywords construct the object the steps have always been."""
import ctypes
import types
from ctypes import addressof

import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd import _native as nv

INV, WS = -1, -3
_RAW = (ctypes.c_char * 4096)()
P = (addressof(_RAW) + 255) & ~255          # a 256-byte aligned host address: compared against NULL / tested for alignment only
P4 = P + 4                                  # 4-byte aligned only
HUGE = 1 << 40

ADAM_COUNT = "1 to 4 tensors per adam launch"
ADAM_ARGS = "bad adam arguments"
ADAM_ALIGN = "adam buffers must be 16-byte aligned"
ADAM_HYPER = "adam needs 0 <= beta1, beta2 < 1, eps >= 0 and lr >= 0"
ADAM_WD = "adam needs weight_decay >= 0"
MAP_ROWS = "a touched-row map needs rows of a multiple of 4 floats that tile the tensor"
MAP_STAMP = "touched_stamp must lie in 1..255"
CLIP_COUNT = "1 to 8 tensors per clip_grad_norm launch"
CLIP_ARGS = "bad clip_grad_norm arguments"
CLIP_NORM = "clip_grad_norm needs max_norm > 0"
CLIP_ALIGN = "gradient rows under a touched-row map must be 16-byte aligned"
CLIP_WS = "workspace too small (okge_clip_grad_norm_multi_workspace_bytes)"


def adam_t(p=P, g=P, m=P, v=P, state=P, n=24, touched=None, row_len=0, stamp=0):
    return nv.AdamMultiTensor(p, g, m, v, state, n, touched, row_len, stamp)


def adam(tensors, n=None, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    arr = (nv.AdamMultiTensor * max(len(tensors), 1))(*tensors) if tensors is not None else None
    return (arr, len(tensors) if n is None else n, lr, b1, b2, eps, wd, None)


def grad_t(g=P, n=24, touched=None, row_len=0, stamp=0):
    return nv.GradTensor(g, n, touched, row_len, stamp)


def clip(tensors, n=None, max_norm=1.0, norm=P, ws=P, ws_bytes=HUGE):
    arr = (nv.GradTensor * max(len(tensors), 1))(*tensors) if tensors is not None else None
    return (arr, len(tensors) if n is None else n, max_norm, norm, ws, ws_bytes, None)


NAN = float("nan")
ROWS = [
    ("adam-null-descriptor", "okge_adam_multi", adam(None, n=1), INV, ADAM_COUNT),
    ("adam-0-tensors", "okge_adam_multi", adam([adam_t()], n=0), INV, ADAM_COUNT),
    ("adam-5-tensors", "okge_adam_multi", adam([adam_t()] * 5), INV, ADAM_COUNT),
    ("adam-null-p", "okge_adam_multi", adam([adam_t(p=None)]), INV, ADAM_ARGS),
    ("adam-null-g", "okge_adam_multi", adam([adam_t(), adam_t(g=None)]), INV, ADAM_ARGS),
    ("adam-null-exp-avg", "okge_adam_multi", adam([adam_t(m=None)]), INV, ADAM_ARGS),
    ("adam-null-exp-avg-sq", "okge_adam_multi", adam([adam_t(v=None)]), INV, ADAM_ARGS),
    ("adam-null-state", "okge_adam_multi", adam([adam_t(), adam_t(), adam_t(), adam_t(state=None)]), INV, ADAM_ARGS),
    ("adam-negative-n", "okge_adam_multi", adam([adam_t(n=-1)]), INV, ADAM_ARGS),
    ("adam-alignment-p", "okge_adam_multi", adam([adam_t(p=P4)]), INV, ADAM_ALIGN),
    ("adam-alignment-exp-avg-sq", "okge_adam_multi", adam([adam_t(v=P4)]), INV, ADAM_ALIGN),
    ("adam-map-row-len-6", "okge_adam_multi", adam([adam_t(touched=P, row_len=6, stamp=1)]), INV, MAP_ROWS),
    ("adam-map-row-len-0", "okge_adam_multi", adam([adam_t(touched=P, row_len=0, stamp=1)]), INV, MAP_ROWS),
    ("adam-map-rows-do-not-tile", "okge_adam_multi", adam([adam_t(touched=P, row_len=16, stamp=1)]), INV, MAP_ROWS),
    ("adam-map-stamp-0", "okge_adam_multi", adam([adam_t(touched=P, row_len=8, stamp=0)]), INV, MAP_STAMP),
    ("adam-map-stamp-256", "okge_adam_multi", adam([adam_t(touched=P, row_len=8, stamp=256)]), INV, MAP_STAMP),
    ("adam-beta1-1", "okge_adam_multi", adam([adam_t()], b1=1.0), INV, ADAM_HYPER),
    ("adam-beta2-negative", "okge_adam_multi", adam([adam_t()], b2=-0.1), INV, ADAM_HYPER),
    ("adam-beta1-nan", "okge_adam_multi", adam([adam_t()], b1=NAN), INV, ADAM_HYPER),
    ("adam-eps-negative", "okge_adam_multi", adam([adam_t()], eps=-1e-8), INV, ADAM_HYPER),
    ("adam-lr-negative", "okge_adam_multi", adam([adam_t()], lr=-0.1), INV, ADAM_HYPER),
    ("adam-wd-negative", "okge_adam_multi", adam([adam_t()], wd=-1e-3), INV, ADAM_WD),
    ("adam-wd-nan", "okge_adam_multi", adam([adam_t()], wd=NAN), INV, ADAM_WD),
    ("clip-null-descriptor", "okge_clip_grad_norm_multi", clip(None, n=1), INV, CLIP_COUNT),
    ("clip-0-tensors", "okge_clip_grad_norm_multi", clip([grad_t()], n=0), INV, CLIP_COUNT),
    ("clip-9-tensors", "okge_clip_grad_norm_multi", clip([grad_t()] * 9), INV, CLIP_COUNT),
    ("clip-null-g", "okge_clip_grad_norm_multi", clip([grad_t(), grad_t(g=None)]), INV, CLIP_ARGS),
    ("clip-negative-n", "okge_clip_grad_norm_multi", clip([grad_t(n=-3)]), INV, CLIP_ARGS),
    ("clip-map-row-len-6", "okge_clip_grad_norm_multi", clip([grad_t(touched=P, row_len=6, stamp=1)]), INV, MAP_ROWS),
    ("clip-map-rows-do-not-tile", "okge_clip_grad_norm_multi", clip([grad_t(touched=P, row_len=16, stamp=1)]), INV, MAP_ROWS),
    ("clip-map-stamp-0", "okge_clip_grad_norm_multi", clip([grad_t(touched=P, row_len=8, stamp=0)]), INV, MAP_STAMP),
    ("clip-map-stamp-256", "okge_clip_grad_norm_multi", clip([grad_t(touched=P, row_len=8, stamp=256)]), INV, MAP_STAMP),
    ("clip-map-alignment", "okge_clip_grad_norm_multi", clip([grad_t(g=P4, touched=P, row_len=8, stamp=1)]), INV, CLIP_ALIGN),
    ("clip-max-norm-0", "okge_clip_grad_norm_multi", clip([grad_t()], max_norm=0.0), INV, CLIP_NORM),
    ("clip-max-norm-negative", "okge_clip_grad_norm_multi", clip([grad_t()], max_norm=-1.0), INV, CLIP_NORM),
    ("clip-max-norm-nan", "okge_clip_grad_norm_multi", clip([grad_t()], max_norm=NAN), INV, CLIP_NORM),
    ("clip-null-workspace", "okge_clip_grad_norm_multi", clip([grad_t()], ws=None), WS, CLIP_WS),
    ("clip-workspace-one-byte-short", "okge_clip_grad_norm_multi", clip([grad_t()], ws_bytes=8447), WS, CLIP_WS),
]


@pytest.fixture(scope="module")
def L():
    if nv.needs_build():
        nv.build_native()
    return nv.lib()


@pytest.mark.parametrize("fn,args,rc,msg", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusal(L, fn, args, rc, msg):
    assert getattr(L, fn)(*args) == rc
    assert L.okge_last_error().decode() == msg


def test_workspace_size_and_abi_version(L):
    assert int(L.okge_clip_grad_norm_multi_workspace_bytes()) == 8448        # 1024 partial sums (double) + the coefficient's 256 bytes
    assert int(L.okge_abi_version()) == 2                                    # additions only


# ---- the step classes, on the CPU: construction validates before anything touches a device ------------------------------------
D, L_TOK = 8, 3


def _tok(n, vocab, rng):
    return torch.from_numpy(rng.integers(1, vocab, (n, L_TOK)).astype(np.int32))


def pooled(**kw):
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    rng = np.random.default_rng(1)
    e = TokenSlot(torch.randn(30, D), _tok(40, 30, rng), "sum", True)
    r = TokenSlot(torch.randn(12, D), _tok(7, 12, rng), "sum", True)
    return TokenPooledTrainStep(e, r, "complex", engine=object(), **kw)


def lstm(scorer="complex", **kw):
    from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot, LSTMTrainStep
    rng = np.random.default_rng(2)
    slots = []
    for n, vocab in ((40, 30), (7, 12)):
        flat = torch.randn(8 * D * D + 8 * D)
        views = [v.view(s) for v, s in zip(flat.split([4 * D * D, 4 * D * D, 4 * D, 4 * D]), ((4 * D, D), (4 * D, D), (4 * D,), (4 * D,)))]
        slots.append(LSTMSlot(torch.randn(vocab, D), _tok(n, vocab, rng), views, (torch.rand(D), torch.zeros(D)),
                              (torch.zeros(D), torch.ones(D)), flat=flat))
    return LSTMTrainStep(slots[0], slots[1], scorer, engine=object(), **kw)


def bigram(**kw):
    from open_knowledge_graph_embeddings_amd.bigram import BigramSlot, BigramTrainStep
    rng = np.random.default_rng(3)
    slots = [BigramSlot(torch.randn(vocab, D), _tok(n, vocab, rng), torch.randn(D, D, 2), "", "batchnorm", (torch.rand(D), torch.zeros(D)))
             for n, vocab in ((40, 30), (7, 12))]
    return BigramTrainStep(slots[0], slots[1], "complex", engine=object(), **kw)


def tucker3(**kw):
    from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep
    eng = types.SimpleNamespace(lib=None, device=torch.device("cpu"))
    return Tucker3TrainStep(torch.randn(40, D), torch.randn(7, D), torch.randn(D * D, D), engine=eng, **kw)


MAKERS = {"token-pooled": pooled, "lstm": lstm, "bigram": bigram, "tucker3": tucker3}


@pytest.mark.parametrize("make", list(MAKERS.values()), ids=list(MAKERS))
def test_keyword_refusals(make):
    with pytest.raises(ValueError, match="optimizer 'sgd': 'adagrad' or 'adam'"):
        make(optimizer="sgd")
    with pytest.raises(ValueError, match="Invalid beta parameters"):
        make(optimizer="adam", betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="Invalid beta parameters"):
        make(optimizer="adam", betas=(0.9, -0.1))
    make(optimizer="adagrad", betas=(1.0, 7.0))                # (betas are read by Adam only, as on FusedTrainStep)


def test_decay_window_belongs_to_adagrad(monkeypatch):
    with pytest.raises(ValueError, match="decay_window"):
        pooled(optimizer="adam", decay_window=4)
    assert pooled(optimizer="adam", decay_window=1).decay_window == 1
    assert pooled(optimizer="adam", decay_window=None).decay_window == 1
    monkeypatch.setenv("OKGE_LAZY_DECAY", "8")                 # the default resolves to 1 under Adam whatever the environment says
    assert pooled(optimizer="adam").decay_window == 1
    assert pooled().decay_window == 8


@pytest.mark.parametrize("kw", [dict(optimizer="adam"), dict(grad_clip=1.0), dict(optimizer="adam", grad_clip=0.5)],
                         ids=["adam", "grad_clip", "both"])
def test_replica_step_refuses_the_new_keywords(kw):
    from open_knowledge_graph_embeddings_amd.sharded import ReplicaStep
    with pytest.raises(NotImplementedError, match="optimizer='adam' and grad_clip are built for the single-device steps"):
        ReplicaStep(pooled(**kw))


@pytest.mark.parametrize("name", list(MAKERS))
def test_defaults_construct_the_same_object(name, monkeypatch):
    """no moment buffers, no norm buffer, the same state_tensors(); decay_window resolved as before"""
    monkeypatch.delenv("OKGE_LAZY_DECAY", raising=False)
    a, b = MAKERS[name](), MAKERS[name](optimizer="adagrad", betas=(0.5, 0.5), grad_clip=0.0)
    for s in (a, b):
        assert s.optimizer == "adagrad" and s.grad_clip == 0.0 and s.grad_norm is None and not hasattr(s, "_adam")
        assert s._optimizer_state() == []
    assert [t.shape for t in a.state_tensors()] == [t.shape for t in b.state_tensors()]
    n_state = {"token-pooled": 16, "lstm": 22, "bigram": 18, "tucker3": 9}[name]
    assert len(a.state_tensors()) == n_state
    if name == "token-pooled":
        assert a.decay_window == 1                             # (small tables: the eager sweep)
        monkeypatch.setenv("OKGE_LAZY_DECAY", "4")
        assert pooled().decay_window == 4 and pooled(decay_window=2).decay_window == 2


@pytest.mark.parametrize("name", list(MAKERS))
def test_adam_allocates_moments_and_states(name):
    s = MAKERS[name](optimizer="adam", grad_clip=0.25)
    groups = s._param_groups(every=True)
    assert len(s._adam) == len(groups) and s.grad_norm.dtype == torch.float64 and s.grad_norm.shape == (1,)
    for (p, g, m, v, st) in s.adam_tensors(every=True):
        assert m.shape == v.shape == p.shape and not bool(m.any()) and not bool(v.any())
        assert st.dtype == torch.int32 and st.tolist() == [0, 0, 0, 0]
    assert len(s.state_tensors()) == len(MAKERS[name]().state_tensors()) + 3 * len(groups)
    assert s.adam_t == 0
    s.set_adam_t(7)
    assert s.adam_t == 7 and all(st.tolist() == [7, 0, 0, 0] for *_, st in s.adam_tensors(every=True))


def test_bias_entity_keeps_the_relation_slot_out():
    s = lstm("bias_entity", optimizer="adam")
    assert len(s._param_groups()) == 3 and len(s._param_groups(every=True)) == 6
    assert all(t[0] is not x for t in s._param_groups() for x in (s.relation.W, s.relation.flat, s.relation.bn))
