"""The bigram encoder kernels (csrc/okge_bigram.hip) through bigram.BigramPass, the product's ctypes path, at the shapes where
their branches change -- one channel and one position, partial row / column tiles, d = 512, max_len 64 full and with no live
bigram anywhere, 0 tokens inside rows, exact ties under max, eight calls, id lists mixed with ranges, strided rows, split-K
slabs nearly all zero -- against the float64 restatement of tests/bigram_reference.py.  Every pooled row and parameter gradient
is held to lstm_reference.band_check (max error <= 3x, rms <= 1.6x the fp32 restatement's, bands of >= 64 elements).  Then the
ABI's contract: dW is added to, the other gradients are written, two runs are bit-identical, a workspace left by a larger
pass gives bit-identical results, an out-of-vocabulary token is counted and read as row 0, and bad arguments are refused
before anything is launched.

Conditioning.  Training batch-norm maps an error e of Y to w e / sqrt(var + eps) of the normalised value; where a channel's
variance over the call's positions nears eps = 1e-5 the band rule would compare two implementations' amplified rounding noise.
Here a call's statistics run over n (L-1) positions, so even a 2-row call has several samples -- but identical (pad, pad)
positions carry no variance, so the calls under TINY_CALL rows draw their ids from full-length rows, and `compare` ASSERTS on
the float64 restatement's own Y that every channel variance of every call is at least MIN_VAR = 100 eps.  With that no call
needs the LSTM sweep's separate judgement of tiny calls.  (The no-live-bigram case is exempt: nothing passes through its
normalisation, rows and gradients are exact zeros.)

Each comparison prints `RATIO <case> <tensor> <max-error ratio> <rms ratio>` (against the fp32 restatement, worst band)."""
import ctypes

import numpy as np
import pytest
import torch

from bigram_reference import BN_EPS, bigram_pass
from lstm_reference import band_check

pytestmark = pytest.mark.gpu

NAN = float("nan")
TINY_CALL = 8
MIN_VAR = 100 * BN_EPS
TENSORS = ("out", "running_mean", "running_var", "dW", "d_conv", "d_bn_weight", "d_bn_bias")


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def slot_data(d, L, n_ids, vocab, kind, seed):
    """token rows of the given kind, init_std-like token rows (row 0 non-zero), Conv1d-like uniform +-1/sqrt(2d) weights,
    batch-norm weight in [0.5, 1.5), non-trivial running statistics and counter"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, vocab, (n_ids, L), generator=g, dtype=torch.int32)
    pos = torch.arange(L)[None, :]
    if kind == "full":
        lens = torch.full((n_ids,), L)
    elif kind == "short":                                # length 1 or 0: no live bigram anywhere
        lens = torch.randint(0, 2, (n_ids,), generator=g)
    elif kind == "dw16":                                 # all length 1 but one full row
        lens = torch.ones(n_ids, dtype=torch.int64)
        lens[int(torch.randint(0, n_ids, (1,), generator=g))] = L
    else:
        lens = torch.randint(0, L + 4, (n_ids,), generator=g).clamp_(max=L)
    tok[pos >= lens[:, None]] = 0
    if kind == "mixed":
        tok[(torch.rand(n_ids, L, generator=g) < 0.15) & (pos > 0) & (lens[:, None] < L)] = 0
    if kind == "inner0":                                 # a 0 token inside every row: it kills the bigram to its left only
        tok[torch.arange(n_ids), torch.randint(1, L - 1, (n_ids,), generator=g)] = 0
    if kind == "tie":                                    # rows [a, b, a, b, ...]: bigrams (a, b) tie exactly under max
        a, b = tok[:, 0].clone(), tok[:, 1].clone()
        tok[:, 0::2], tok[:, 1::2] = a[:, None], b[:, None]
    W = torch.randn(vocab, d, generator=g) * 0.3
    conv = (torch.rand(d, d, 2, generator=g) * 2 - 1) / np.sqrt(2 * d)
    bn = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1)
    running = (torch.randn(d, generator=g) * 0.1, torch.rand(d, generator=g) * 0.5 + 0.5)
    return dict(W=W, tok=tok, conv=conv, bn=bn, running=running, counter=5, g=g, lens=lens)


def make_calls(spec, data):
    """spec: ints (an id list of that many rows; a call under TINY_CALL rows gets distinct ids of full-length rows, the others
    draw ids with repeats) or ("range", first, n)"""
    g, (n_ids, L) = data["g"], data["tok"].shape
    full = torch.nonzero((data["tok"] > 0).all(1)).reshape(-1)
    calls = []
    for c in spec:
        if isinstance(c, tuple):
            calls.append((None, c[1], c[2]))
        elif c < TINY_CALL:
            assert full.numel() >= c
            calls.append((full[torch.randperm(full.numel(), generator=g)[:c]].to(torch.int32), 0, c))
        else:
            calls.append((torch.randint(0, n_ids, (c,), generator=g, dtype=torch.int32), 0, c))
    return calls


def gpu_pass(data, calls, pool, normalize, training=True, d_out=None, pad=0, ps=None, dW=None, d_conv=None, d_bn=None):
    """one BigramPass encode (and backward with d_out) on cuda; out / d_out are column slices of d + pad wide buffers filled
    with NaN; d_conv and d_bn start as NaN unless given"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramPass, BigramSlot
    W, d = data["W"], data["W"].shape[1]
    bn = normalize == "batchnorm"
    slot = BigramSlot(W.cuda(), data["tok"].cuda(), data["conv"].cuda(), pool, normalize, tuple(x.cuda() for x in data["bn"]) if bn else None,
                      tuple(x.cuda().clone() for x in data["running"]) if bn else None,
                      torch.tensor(data["counter"], dtype=torch.int64, device="cuda") if bn else None)
    gcalls = [(None if ids is None else ids.cuda(), first, n) for ids, first, n in calls]
    R = sum(n for _, _, n in calls)
    outbuf = torch.full((R, d + pad), NAN, device="cuda")
    out = outbuf[:, :d]
    ps = ps or BigramPass("cuda")
    ps.encode(slot, gcalls, training, out)
    res = dict(out=out, outbuf=outbuf, ps=ps, slot=slot)
    if bn:
        res.update(running_mean=slot.running_mean, running_var=slot.running_var, num_batches_tracked=slot.num_batches_tracked)
    if d_out is not None:
        dobuf = torch.full((R, d + pad), NAN, device="cuda")
        dobuf[:, :d] = d_out.cuda()
        dW = torch.zeros_like(slot.W) if dW is None else dW
        d_conv = torch.full_like(slot.conv, NAN) if d_conv is None else d_conv
        if bn and d_bn is None:
            d_bn = torch.full((2 * d,), NAN, device="cuda")
        ps.backward(slot, gcalls, dobuf[:, :d], dW, d_conv, d_bn if bn else None)
        res.update(dW=dW, d_conv=d_conv)
        if bn:
            res["d_bn_weight"], res["d_bn_bias"] = d_bn[:d], d_bn[d:]
    torch.cuda.synchronize()
    return res


def compare(case, mine, data, calls, pool, normalize, training=True, d_out=None, check_var=True):
    """every tensor of `mine` the restatement also gives, against float64 with the band rule (fp32 calibration)"""
    kw = dict(pool=pool, normalize=normalize, bn=data["bn"], running=data["running"], counter=data["counter"], training=training,
              d_out=d_out)
    ref = bigram_pass(data["W"], data["tok"], data["conv"], calls, dtype=torch.float64, **kw)
    r32 = bigram_pass(data["W"], data["tok"], data["conv"], calls, dtype=torch.float32, **kw)
    if normalize == "batchnorm" and training and check_var:
        r0 = 0
        for _, _, n in calls:                            # well-conditioned by construction: see the module docstring
            var = ref["Y"][r0:r0 + n].reshape(-1, ref["Y"].shape[2]).var(0)
            assert var.min() >= MIN_VAR, (case, n, float(var.min()))
            r0 += n
    for k in TENSORS:
        if k in ref and k in mine:
            mx, rms = band_check(f"{case}/{k}", mine[k], ref[k], r32[k])
            print(f"RATIO {case} {k} {mx:.2f} {rms:.2f}")
    if normalize == "batchnorm":
        assert int(mine["num_batches_tracked"]) == ref["num_batches_tracked"] == data["counter"] + (len(calls) if training else 0)
    if "dW" in mine:
        assert not mine["dW"][0].any()
    return ref


# ---- the shape sweep ------------------------------------------------------------------------------------------------------
# (id naming the branch it reaches, d, max_len, calls, token kind, pool, normalize, column padding of out / d_out)
SWEEP = [
    ("d1_L2_one_channel_one_position_bn", 1, 2, [40, 24], "full", "sum", "batchnorm", 0),
    ("d1_L2_one_channel_one_position_max", 1, 2, [40, 24], "full", "max", "", 0),
    ("d33_partial_k_chunk_bn_max", 33, 4, [17, 64, 9], "mixed", "max", "batchnorm", 0),
    ("d200_partial_tiles_bn_sum", 200, 10, [300, 65, 63], "mixed", "sum", "batchnorm", 0),
    ("d200_partial_tiles_none_sum", 200, 10, [300, 65, 63], "mixed", "sum", "", 0),
    ("d257_last_column_tile_holds_one_mean_max", 257, 6, [129], "mixed", "max", "mean", 0),
    ("d257_last_column_tile_holds_one_none_max", 257, 6, [129], "mixed", "max", "", 0),
    ("d512_bn_sum", 512, 5, [130, 70], "mixed", "sum", "batchnorm", 0),
    ("d512_mean_sum", 512, 5, [130, 70], "mixed", "sum", "mean", 0),
    ("d24_L64_every_row_full_bn", 24, 64, [64, 64], "full", "sum", "batchnorm", 0),
    ("d24_L64_every_row_full_max", 24, 64, [64, 64], "full", "max", "mean", 0),
    ("d40_zero_token_inside_rows_bn_max", 40, 8, [100], "inner0", "max", "batchnorm", 0),
    ("d40_zero_token_inside_rows_sum", 40, 8, [100], "inner0", "sum", "mean", 0),
    ("d16_exact_ties_under_max", 16, 4, [50], "tie", "max", "", 0),
    ("d16_exact_ties_under_max_bn", 16, 4, [50], "tie", "max", "batchnorm", 0),
    ("d40_max_calls_bn_per_call", 40, 5, [2, 3, 255, 256, 257, 7, 64, 2], "mixed", "sum", "batchnorm", 0),
    ("d48_ranges_mixed_with_id_lists", 48, 7, [("range", 0, 100), 50, ("range", 37, 9)], "mixed", "max", "batchnorm", 0),
    ("d72_strided_rows_ld_d_plus_5", 72, 5, [40, 40], "mixed", "sum", "mean", 5),
    ("d72_strided_rows_ld_d_plus_5_bn", 72, 5, [40, 40], "mixed", "max", "batchnorm", 5),
    ("d64_L64_dw_16_splits_all_but_one_zero", 64, 64, [300], "dw16", "sum", "", 0),
]


def sweep_case(case_id):
    _, d, L, spec, kind, pool, normalize, pad = next(c for c in SWEEP if c[0] == case_id)
    rows = sum(c[2] if isinstance(c, tuple) else c for c in spec)
    n_ids = max(rows, max((c[1] + c[2] for c in spec if isinstance(c, tuple)), default=0), 64)
    if kind == "dw16":
        n_ids = rows
    data = slot_data(d, L, n_ids, 1000, kind, seed=sum(map(ord, case_id)))
    if kind == "dw16":                                   # the call is every row once, in a shuffled order
        calls = [(torch.randperm(n_ids, generator=data["g"]).to(torch.int32), 0, n_ids)]
    else:
        calls = make_calls(spec, data)
    d_out = torch.randn(rows, d, generator=data["g"])
    return data, calls, d_out, pool, normalize, pad


@pytest.mark.parametrize("case_id", [c[0] for c in SWEEP])
def test_shape_sweep_against_float64(okge_lib, case_id):
    """training encode + backward: pooled rows, running statistics and counter, every gradient; with batch-norm also an
    eval-mode encode on non-trivial running statistics and a non-zero counter (both left unchanged)"""
    data, calls, d_out, pool, normalize, pad = sweep_case(case_id)
    mine = gpu_pass(data, calls, pool, normalize, d_out=d_out, pad=pad)
    compare(case_id, mine, data, calls, pool, normalize, d_out=d_out)
    if pad:                                              # nothing written past column d of a strided row
        assert torch.isnan(mine["outbuf"][:, -pad:]).all()
    if normalize == "batchnorm":
        ev = gpu_pass(data, calls, pool, normalize, training=False, pad=pad)
        compare(case_id + "/eval", ev, data, calls, pool, normalize, training=False)
        assert torch.equal(ev["running_mean"].cpu(), data["running"][0]) and torch.equal(ev["running_var"].cpu(), data["running"][1])


def test_split_k_case_has_one_live_row():
    data, calls, _, _, _, _ = sweep_case("d64_L64_dw_16_splits_all_but_one_zero")
    assert int(((data["tok"][:, 1:] > 0).any(1)).sum()) == 1 and data["tok"].shape[0] * 63 // 256 >= 16


@pytest.mark.parametrize("pool,normalize", [("sum", ""), ("max", ""), ("max", "mean"), ("sum", "batchnorm")])
def test_no_live_bigram_anywhere_gives_exact_zeros(okge_lib, pool, normalize):
    """max_len 64, every row of length 1 or 0: pooled rows, dK and dW are exact zeros (with batch-norm too: every position is
    dead, only the statistics see the rows), and the running statistics still follow the restatement"""
    data = slot_data(24, 64, 96, 1000, "short", seed=640)
    calls = [(None, 0, 96)]
    d_out = torch.randn(96, 24, generator=data["g"])
    mine = gpu_pass(data, calls, pool, normalize, d_out=d_out)
    assert not mine["out"].any() and not mine["d_conv"].any() and not mine["dW"].any()
    compare(f"no_live_bigram_{pool}_{normalize}", mine, data, calls, pool, normalize, d_out=d_out, check_var=False)


# ---- the contract of okge_bigram_backward_calls and of BigramPass -----------------------------------------------------------
def _all(res):
    return {k: v for k, v in res.items() if torch.is_tensor(v) and k != "outbuf"}


def test_backward_adds_into_dW_and_writes_d_conv_and_d_bn(okge_lib):
    """dW prefilled with seeded values ends as prefill + gradient (bit-exact: one fp32 add per element); d_conv and d_bn
    prefilled with NaN (gpu_pass's default) or with random values end equal: they are written"""
    data, calls, d_out, pool, normalize, _ = sweep_case("d40_max_calls_bn_per_call")
    base = gpu_pass(data, calls, pool, normalize, d_out=d_out)
    g = torch.Generator().manual_seed(5)
    prefill = torch.randn(data["W"].shape, generator=g).cuda()
    d_conv = torch.randn(data["conv"].shape, generator=g).cuda()
    d_bn = torch.randn(2 * data["W"].shape[1], generator=g).cuda()
    again = gpu_pass(data, calls, pool, normalize, d_out=d_out, dW=prefill.clone(), d_conv=d_conv, d_bn=d_bn)
    assert torch.equal(again["dW"], prefill + base["dW"])
    for k in ("d_conv", "d_bn_weight", "d_bn_bias"):
        assert torch.isfinite(base[k]).all(), k
        assert torch.equal(again[k], base[k]), k


def test_workspace_reused_from_larger_pass_is_bit_identical(okge_lib):
    """a BigramPass that ran the d = 200 three-call pass, then a smaller one (fewer rows, same d and max_len): pooled rows,
    every gradient and the running statistics equal a fresh BigramPass's on the smaller pass"""
    data, calls, d_out, pool, normalize, _ = sweep_case("d200_partial_tiles_bn_sum")
    big = gpu_pass(data, calls, pool, normalize, d_out=d_out)
    small = [(calls[0][0][:70], 0, 70), (None, 11, 31)]
    d_small = d_out[:101] * 0.5
    reused = gpu_pass(data, small, pool, normalize, d_out=d_small, ps=big["ps"])
    fresh = gpu_pass(data, small, pool, normalize, d_out=d_small)
    assert reused["ps"].ws_bytes > fresh["ps"].ws_bytes
    a, b = _all(reused), _all(fresh)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case_id", ["d64_L64_dw_16_splits_all_but_one_zero", "d40_max_calls_bn_per_call", "d16_exact_ties_under_max_bn"])
def test_bit_reproducible(okge_lib, case_id):
    data, calls, d_out, pool, normalize, pad = sweep_case(case_id)
    a, b = _all(gpu_pass(data, calls, pool, normalize, d_out=d_out)), _all(gpu_pass(data, calls, pool, normalize, d_out=d_out))
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- ABI refusals: the N.check error, and nothing launched ----------------------------------------------------------------
def _encode_raw(lib, data, calls, training, ws_bytes=None, n_calls=None):
    """okge_bigram_encode_calls straight through ctypes, out / pos_tok filled with sentinels; returns them after the call
    (or the raised error)"""
    from open_knowledge_graph_embeddings_amd import _native as N
    from open_knowledge_graph_embeddings_amd.bigram import BigramSlot
    W, d, L = data["W"], data["W"].shape[1], data["tok"].shape[1]
    slot = BigramSlot(W.cuda(), data["tok"].cuda(), data["conv"].cuda(), "sum", "batchnorm", tuple(x.cuda() for x in data["bn"]),
                      tuple(x.cuda().clone() for x in data["running"]), torch.tensor(3, dtype=torch.int64, device="cuda"))
    gids = [None if ids is None else ids.cuda() for ids, _, _ in calls]
    arr = (N.BigramCall * len(calls))()
    for x, ids, (_, first, n) in zip(arr, gids, calls):
        x.ids, x.first_id, x.n = None if ids is None else ids.data_ptr(), first, n
    R = sum(n for _, _, n in calls)
    out = torch.full((R, d), 7.0, device="cuda")
    pos_tok = torch.full((R * L,), -7, dtype=torch.int32, device="cuda")
    need = int(lib.okge_bigram_workspace_bytes(R, L, d, int(training)))
    size = need if ws_bytes is None else ws_bytes(need)
    ws = torch.empty(max(size, 1), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = None
    try:
        N.check(lib.okge_bigram_encode_calls(ctypes.byref(slot.c()), arr, len(calls) if n_calls is None else n_calls, int(training),
                                             out.data_ptr(), d, pos_tok.data_ptr(), ws.data_ptr(), size, stream),
                "okge_bigram_encode_calls")
    except N.OkgeError as e:
        err = e
    torch.cuda.synchronize()
    return err, out, pos_tok, slot


def _small(d=16, L=5, n_ids=40):
    return slot_data(d, L, n_ids, 100, "mixed", seed=77)


def _refused(lib, data, calls, training, match, **kw):
    err, out, pos_tok, slot = _encode_raw(lib, data, calls, training, **kw)
    assert err is not None and match in str(err), err
    assert (out == 7.0).all() and (pos_tok == -7).all() and int(slot.num_batches_tracked) == 3         # nothing launched


def test_abi_refuses_nine_calls(okge_lib):
    data = _small()
    _refused(okge_lib, data, [(None, i, 3) for i in range(9)], True, "1 to 8 bigram calls")
    err, out, _, slot = _encode_raw(okge_lib, data, [(None, i, 3) for i in range(8)], True)             # 8 is the limit
    assert err is None and torch.isfinite(out).all() and int(slot.num_batches_tracked) == 11


@pytest.mark.parametrize("L", [1, 65])
def test_abi_refuses_max_len_1_and_65(okge_lib, L):
    data = _small(L=max(L, 2))
    if L == 1:                                           # (a one-column token matrix)
        data["tok"] = data["tok"][:, :1].contiguous()
    _refused(okge_lib, data, [(None, 0, 4)], True, "max_len must lie in 2..64")


def test_abi_refuses_d_513(okge_lib):
    _refused(okge_lib, _small(d=513, n_ids=8), [(None, 0, 4)], True, "above 512")


@pytest.mark.parametrize("training", [True, False])
def test_abi_refuses_workspace_one_byte_short(okge_lib, training):
    _refused(okge_lib, _small(), [(None, 0, 20), (None, 3, 9)], training, "workspace too small", ws_bytes=lambda need: need - 1)


def test_out_of_vocab_token_counted_and_read_as_row_0(okge_lib):
    """a token id >= vocab in the token matrix: the device id guard counts it, and the position reads token row 0 (the
    documented row-0 substitution; the token still counts as live) and passes no gradient"""
    from open_knowledge_graph_embeddings_amd import _native as N
    data = _small(d=24)
    vocab = data["W"].shape[0]
    bad = torch.nonzero((data["tok"][:, :3] > 0).all(1)).reshape(-1)[:2]
    data["tok"][bad[0], 1] = vocab
    data["tok"][bad[1], 1] = vocab + 1000
    calls = [(None, 0, data["tok"].shape[0])]
    d_out = torch.randn(data["tok"].shape[0], 24, generator=torch.Generator().manual_seed(3))
    mine = gpu_pass(data, calls, "sum", "batchnorm", d_out=d_out)
    assert N.id_errors() > 0                             # (the call also resets the count)
    ref = compare("out_of_vocab_token", mine, data, calls, "sum", "batchnorm", d_out=d_out)
    rows = mine["out"].cpu().double().numpy()
    subst = data["tok"].clone()
    subst[bad, 1] = 0                                # a real padding token there would kill the bigram instead
    dead = bigram_pass(data["W"], subst, data["conv"], calls, "sum", "batchnorm", data["bn"], data["running"], data["counter"])["out"]
    assert not np.allclose(dead[bad[0]], rows[bad[0]], rtol=0, atol=1e-4)
    np.testing.assert_allclose(rows[bad], ref["out"][bad], rtol=1e-5, atol=1e-5)
