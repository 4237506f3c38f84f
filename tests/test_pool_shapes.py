"""The token-pooling kernels (csrc/okge_pool.hip) through token_pooled.PoolEngine.encode_calls / backward_calls, the product's
ctypes path, at the shapes where their branches change, against the float64 restatement of tests/pool_reference.py.

Forward (pool_stats_kernel, bn_finish_kernel<0>, bn_apply_kernel): slot sizes on the scalar path and on one and two column
trips of the 16-byte path, partial row groups and row blocks, 65 row blocks, max_len 1 to 64, strided and misaligned row
blocks, training and eval mode, up to eight calls on two slots.  Backward with float atomics (bn_partial2_kernel,
bn_finish_kernel<2>, pool_backward_kernel): the three poolings, hot and cold tokens, exact ties under max.  Backward through the
scatter plan (scatter_count_block, scatter_alloc_block, pool_dx_kernel, pool_sum_kernel): token tables DESIGNED so that named
tokens have exactly 1, 2, 63, 64, 65, 1 024, 1 025 and >= 2 049 pairs, vocabulary sizes around the 32 hot tokens and the 2 048
token allocation workgroups, histogram chunks of 60 and 16 rows, 257 and 1 025 hot-slab blocks, several calls per table.

Every tensor the restatement gives is held to lstm_reference.band_check (max error <= 3x, rms <= 1.6x the fp32 restatement's, in
bands of >= 64 elements, floor 1e-7 max|want|; the token-table gradient class by class of its rows: see `check`); each
comparison prints `RATIO <case> <tensor> <max ratio> <rms ratio>`.  Held
exactly: sum pooling of one token without batch-norm (a copy of W rows), the max-pooling forward, the touched-row map, the
id-error counter, the scatter state (all zero after a call), run-to-run results of the plan path.

Conditioning.  Training batch-norm maps an error e of a pooled row to w e / sqrt(var + eps); where a channel's variance over a
call's rows nears eps the band rule would compare two implementations' amplified rounding noise.  So every batch-norm call has at
least 2 rows and `check` ASSERTS on the float64 restatement's own raw rows that every channel variance of every call is at least
MIN_VAR = 100 eps.  The inputs are built for that: a token row is 0.3 N(0, 1) noise plus level[token] * u with one N(0, 1.5^2)
level per token and one sign u per channel, so rows with different tokens differ in EVERY channel, and a call of 2 to 7 rows
draws distinct ids spread evenly over the rows' pooled levels."""
import ctypes

import numpy as np
import pytest
import torch

from lstm_reference import band_check, row_ids
from pool_reference import pool_pass, pool_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")
BN_EPS = 1e-5                                            # == token_pooled.BN_EPS (asserted in references())
MIN_VAR = 100 * BN_EPS
TINY_CALL = 8
HOT = 32                                                 # token ids below this are summed per workgroup (okge_pool.hip HOT_TOKENS)
TENSORS = ("raw", "out", "saved_mean", "saved_rstd", "running_mean", "running_var", "dW", "d_bn_weight", "d_bn_bias")


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def slot_data(d, L, n_ids, vocab, pool, bn, seed, kind="mixed", tok=None):
    """token rows (half the tokens hot, lengths 1..L, right-padded with 0), the token table of the module docstring (row 0 an
    ordinary row), batch-norm weight in [0.5, 1.5), non-trivial running statistics.  kind 'repeat': every row repeats its
    first token; 'ties': the table drawn from {-0.5, 0, 0.5}; 'padrows': every fifth row only padding."""
    g = torch.Generator().manual_seed(seed)
    if tok is None:
        tok = torch.randint(1, vocab, (n_ids, L), generator=g, dtype=torch.int32)
        hot = torch.randint(1, min(HOT, vocab), (n_ids, L), generator=g, dtype=torch.int32)
        tok = torch.where(torch.rand(n_ids, L, generator=g) < 0.5, hot, tok)
        lens = torch.randint(1, L + 1, (n_ids,), generator=g)
        if kind == "padrows":
            lens[::5] = 0
        if kind == "repeat" and L > 1:
            tok[:, 1] = tok[:, 0]
            lens.clamp_(min=2)
        tok[torch.arange(L)[None, :] >= lens[:, None]] = 0
    tok = tok.to(torch.int32).contiguous()
    u = torch.randint(0, 2, (d,), generator=g).float() * 2 - 1
    W = torch.randn(vocab, d, generator=g) * 0.3 + (torch.randn(vocab, generator=g) * 1.5)[:, None] * u[None, :]
    if kind == "ties":
        W = (torch.randint(0, 3, (vocab, d), generator=g).float() - 1) * 0.5
    data = dict(W=W, tok=tok, pool=pool, bn=None, running=None, g=g, u=u, d=d, L=tok.shape[1])
    if bn:
        data["bn"] = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1)
        data["running"] = (torch.randn(d, generator=g) * 0.1, torch.rand(d, generator=g) * 0.5 + 0.5)
    return data


def make_calls(spec, data):
    """spec: ints (an id list of that many rows; a call under TINY_CALL rows gets distinct ids spread evenly over the rows'
    pooled levels, the others draw ids with repeats) or ("range", first, n)"""
    g, n_ids = data["g"], data["tok"].shape[0]
    calls = []
    for c in spec:
        if isinstance(c, tuple):
            calls.append((None, c[1], c[2]))
        elif c < TINY_CALL:
            raw, _ = pool_rows(data["W"].double().numpy(), data["tok"].numpy().astype(np.int64), data["pool"])
            order = np.argsort((raw * data["u"].double().numpy()).mean(1), kind="stable")
            pick = order[np.linspace(0, n_ids - 1, c).round().astype(np.int64)]
            assert len(set(pick.tolist())) == c
            calls.append((torch.from_numpy(pick)[torch.randperm(c, generator=g)].to(torch.int32), 0, c))
        else:
            calls.append((torch.randint(0, n_ids, (c,), generator=g, dtype=torch.int32), 0, c))
    return calls


def rows_of(spec):
    return sum(c[2] if isinstance(c, tuple) else c for c in spec)


def ids_needed(spec):
    return max(rows_of(spec), max((c[1] + c[2] for c in spec if isinstance(c, tuple)), default=0), 64)


def random_d_out(slots, batch):
    """a random gradient per slot, rows in the order of the slot's calls"""
    return {k: torch.randn(sum(n for kk, _, _, n in batch if kk == k), s["d"], generator=s["g"]) for k, s in slots.items()}


def random_prefill(slots):
    """the backward ADDS to dW and to the batch-norm gradients: start them from seeded values"""
    return {k: dict(dW=torch.randn(s["W"].shape, generator=s["g"]) * 0.1, d_bn=torch.randn(2 * s["d"], generator=s["g"]) * 0.1)
            for k, s in slots.items()}


# ---- the kernels ----------------------------------------------------------------------------------------------------------
def _layout(layout, d):
    """(leading dimension, first column) of the d-wide row block inside its NaN-filled buffer"""
    return {"ld_d": (d, 0), "ld_d4": (d + 4, 0), "ld_d1": (d + 1, 0), "off1": ((d + 4) // 4 * 4, 1)}[layout]


def gpu_pass(slots, batch, training=True, layout="ld_d", inplace=True, d_out=None, scatter="plan", engine=None, prefill=None,
             stamp=1):
    """one PoolEngine.encode_calls (and backward_calls with d_out) on cuda.  slots {key: slot_data}, batch [(key, ids, first, n)]
    in launch order; a slot's rows lie one call after the other in column slices of NaN-filled buffers (_layout); without
    batch-norm out is raw (inplace) or a buffer of its own."""
    from open_knowledge_graph_embeddings_amd.token_pooled import PoolEngine, TokenSlot
    engine = engine or PoolEngine("cuda")
    engine.scatter = scatter
    res, dev, r0 = {"engine": engine}, {}, {}
    for k, s in slots.items():
        d, R = s["d"], sum(n for kk, _, _, n in batch if kk == k)
        ld, c0 = _layout(layout, d)
        bn = s["bn"] is not None
        sl = TokenSlot(s["W"].cuda(), s["tok"].cuda(), s["pool"], bn, s["bn"][0] if bn else None, s["bn"][1] if bn else None)
        sl.stamp = stamp
        if sl.touched is None:                           # (the product keeps no map at d % 4 != 0; the ABI takes one on both paths)
            sl.touched = torch.zeros(s["W"].shape[0], dtype=torch.uint8, device="cuda")
        if bn:
            sl.running_mean.copy_(s["running"][0])
            sl.running_var.copy_(s["running"][1])
        if prefill is not None:
            sl.dW.copy_(prefill[k]["dW"])
            if bn:
                sl.d_bn.copy_(prefill[k]["d_bn"])
        bufs = [torch.full((R, ld), NAN, device="cuda") for _ in range(3)]
        raw, out, dy = (b[:, c0:c0 + d] for b in bufs)
        if not bn and inplace:
            out = raw
        if d_out is not None:
            dy.copy_(d_out[k])
        n_calls = sum(1 for kk, _, _, _ in batch if kk == k)
        dev[k] = dict(slot=sl, raw=raw, out=out, dy=dy, saved=torch.full((n_calls, 4 * d), NAN, device="cuda") if bn else None, c=0)
        r0[k] = 0
        res[k] = dict(slot=sl, raw=raw, out=out, bufs=bufs, cols=(c0, c0 + d))
    enc, bwd = [], []
    for k, ids, first, n in batch:
        v = dev[k]
        rows = slice(r0[k], r0[k] + n)
        sv = None if v["saved"] is None else v["saved"][v["c"]]
        gids = None if ids is None else ids.cuda()
        enc.append((v["slot"], gids, first, n, v["raw"][rows], v["out"][rows], sv))
        bwd.append((v["slot"], gids, first, n, v["raw"][rows], v["dy"][rows], sv))
        r0[k] += n
        v["c"] += 1
    engine.encode_calls(enc, training)
    torch.cuda.synchronize()
    for k, s in slots.items():
        sl, d = dev[k]["slot"], s["d"]
        if s["bn"] is not None:
            res[k].update(running_mean=sl.running_mean.clone(), running_var=sl.running_var.clone())
            if training:
                res[k].update(saved_mean=dev[k]["saved"][:, :d].clone(), saved_rstd=dev[k]["saved"][:, d:2 * d].clone())
    if d_out is not None:
        engine.backward_calls(bwd)
        torch.cuda.synchronize()
        for k, s in slots.items():
            sl, d = dev[k]["slot"], s["d"]
            res[k].update(dW=sl.dW, touched=sl.touched)
            if s["bn"] is not None:
                res[k].update(d_bn_weight=sl.d_bn[:d], d_bn_bias=sl.d_bn[d:])
    return res


def slot_calls(batch, key):
    return [(ids, first, n) for k, ids, first, n in batch if k == key]


def references(slots, batch, training=True, d_out=None, order_seed=None):
    """{key: (float64 restatement, fp32 restatement)} of the slots' calls, each slot's in launch order"""
    from open_knowledge_graph_embeddings_amd import token_pooled
    assert token_pooled.BN_EPS == BN_EPS
    refs = {}
    for k, s in slots.items():
        kw = dict(pool=s["pool"], bn=s["bn"], running=s["running"], training=training, d_out=None if d_out is None else d_out[k])
        if order_seed is not None:                       # (check's calibration of an unordered scatter: the fp32 restatement alone)
            refs[k] = pool_pass(s["W"], s["tok"], slot_calls(batch, k), dtype=torch.float32, order_seed=order_seed, **kw)
            continue
        refs[k] = tuple(pool_pass(s["W"], s["tok"], slot_calls(batch, k), dtype=dt, **kw) for dt in (torch.float64, torch.float32))
    return refs


def assert_conditioned(case, slots, batch, refs):
    """every channel variance of every training batch-norm call, on the float64 restatement's raw rows, is at least MIN_VAR"""
    for k, s in slots.items():
        if s["bn"] is None:
            continue
        r0 = 0
        for _, _, n in slot_calls(batch, k):
            assert n >= 2, (case, k, n)
            var = refs[k][0]["raw"][r0:r0 + n].var(0)
            assert var.min() >= MIN_VAR, (case, k, n, float(var.min()))
            r0 += n


ORDERS = 16
ROW_CLASSES = ("hot", "1-64", "65-1024", "1025+")      # okge_pool.hip: HOT_TOKENS, SC_SHORT, SC_SORT_MAX


def row_classes(s, calls):
    """the token rows by how their gradient is summed: {class: row indices} over the rows with a pair in the batch (the hot
    tokens; the cold ones by their number of pairs), and the rows without one"""
    t = s["tok"][row_ids(calls)].numpy().astype(np.int64)
    pairs = np.bincount(t[t > 0], minlength=s["W"].shape[0])[:s["W"].shape[0]]
    ids = np.arange(pairs.size)
    cold = ids >= HOT
    cls = {"hot": ~cold & (pairs > 0), "1-64": cold & (pairs >= 1) & (pairs <= 64), "65-1024": cold & (pairs > 64) & (pairs <= 1024),
           "1025+": cold & (pairs > 1024)}
    return {c: np.nonzero(m)[0] for c, m in cls.items()}, np.nonzero(pairs == 0)[0]


def check(case, mine, slots, batch, refs, training=True, prefill=None, pad_rows=None, unordered=None):
    """every tensor of `mine` the restatement also gives, against float64 with the band rule (fp32 calibration); nothing written
    outside the row blocks.

    dW is compared as prefill + gradient, and not as one tensor: the token rows no pair names keep their prefill bit for bit (row
    0 among them), the others go through band_check class by class of ROW_CLASSES.  The reason is one of conditioning: the error
    of a token row is that of its sum -- 2 100 terms for the designed tables' largest, one for most rows -- whatever the value
    the sum ends at, so a |want| band over the whole table holds two or three elements of a long row whose sums nearly cancel
    beside thousands of short rows' elements, and the ratio of two implementations' errors on three elements is a draw.  Within
    a class the rows' errors have one scale.  The factors are band_check's own.

    unordered (the pass's d_out) given: `mine` comes from the float-atomics scatter, whose additions arrive in no fixed order, and
    its dW is calibrated by the fp32 restatement in ORDERS seeded pair orders besides the ascending one: per element the largest
    of their errors.  Measured on the d = 260 designed table before either measure: max ratios of 1.3 to 4.0 over 25 runs of the
    atomics path (4 above 3) against the ascending order over the whole table, 0.9 to 1.4 for the fp32 restatement itself in 12
    random orders.  Both restatements alone set the bound."""
    if training:
        assert_conditioned(case, slots, batch, refs)
    for k, s in slots.items():
        ref, r32 = refs[k]
        c0, c1 = mine[k]["cols"]
        for b in mine[k]["bufs"]:                        # the NaN sentinel outside the column slice
            assert torch.isnan(b[:, :c0]).all() and torch.isnan(b[:, c1:]).all(), (case, k)
        for name in TENSORS:
            if name not in ref or name not in mine[k]:
                continue
            got, want, want32 = mine[k][name].detach().cpu().double().numpy(), ref[name], r32[name]
            if name == "dW":
                pre = torch.zeros_like(s["W"]) if prefill is None else prefill[k]["dW"]
                want = want + pre.double().numpy()
                want32 = (r32[name].astype(np.float32) + pre.numpy()).astype(np.float64)
                if unordered is not None:
                    worst = np.abs(want32 - want)
                    for seed in range(ORDERS):
                        other = references({k: s}, batch, d_out=unordered, order_seed=seed)[k]["dW"].astype(np.float32) + pre.numpy()
                        worst = np.maximum(worst, np.abs(other.astype(np.float64) - want))
                    want32 = want + worst
                classes, unnamed = row_classes(s, slot_calls(batch, k))
                assert 0 in unnamed and np.array_equal(got[unnamed], pre.double().numpy()[unnamed]), (case, k, "a row no pair names changed")
                ratios = [band_check(f"{case}/{k}/dW[{c}]", got[r], want[r], want32[r]) for c, r in classes.items() if r.size]
                mx, rms = (max(x) for x in zip(*ratios)) if ratios else (0.0, 0.0)
                print(f"RATIO {case}/{k} {name} {mx:.2f} {rms:.2f}")
                continue
            if name in ("d_bn_weight", "d_bn_bias") and prefill is not None:
                pre = prefill[k]["d_bn"][:s["d"]] if name == "d_bn_weight" else prefill[k]["d_bn"][s["d"]:]
                want = want + pre.double().numpy()
                want32 = (r32[name].astype(np.float32) + pre.numpy()).astype(np.float64)
            if pad_rows is not None and name in ("raw", "out"):
                # rows of only padding under mean pooling: L x row 0 / 1e-12, compared by relative error.  L - 1 sequential fp32
                # additions of one value, the rounding of 1e-12 to fp32, its reciprocal and the product: (L + 2) 2^-24
                pad = pad_rows[k]
                rel = np.abs(got[pad] - want[pad]) / np.abs(want[pad])
                print(f"PADROWS {case}/{k} {name} max relative error {rel.max():.3e}")
                assert np.abs(want[pad]).min() > 0 and rel.max() <= (s["L"] + 2) * 2.0 ** -24, (case, k, name, rel.max())
                got, want, want32 = got[~pad], want[~pad], want32[~pad]
            mx, rms = band_check(f"{case}/{k}/{name}", got, want, want32)
            print(f"RATIO {case}/{k} {name} {mx:.2f} {rms:.2f}")


def expected_touched(slots, batch, key, stamp):
    """the map the backward must leave: the stamp on exactly the token rows that received a gradient"""
    s = slots[key]
    t = s["tok"][row_ids(slot_calls(batch, key))].numpy().astype(np.int64)
    want = np.zeros(s["W"].shape[0], dtype=np.uint8)
    if s["pool"] == "max":
        _, arg = pool_rows(s["W"].double().numpy(), t, "max")
        t = np.take_along_axis(t, arg, axis=1)
    want[np.unique(t[t > 0])] = stamp
    return want


# ---- forward sweep ----------------------------------------------------------------------------------------------------------
# (id naming the branch it reaches, d, max_len, pool, batch-norm, calls, layout, out is raw)
FORWARD = [
    ("d1_L1_sum_one_row_in_place", 1, 1, "sum", False, [1], "ld_d", True),
    ("d1_L2_mean_bn_two_rows", 1, 2, "mean", True, [2], "ld_d", True),
    ("d3_L17_max_bn_7_8", 3, 17, "max", True, [7, 8], "ld_d", True),
    ("d3_L2_sum_copy_9", 3, 2, "sum", False, [9], "ld_d1", False),
    ("d4_L1_sum_bn_2_15", 4, 1, "sum", True, [2, 15], "ld_d", True),
    ("d4_L17_mean_bn_65_row_blocks", 4, 17, "mean", True, [2080], "ld_d", True),
    ("d4_L64_max_in_place_16", 4, 64, "max", False, [16], "ld_d", True),
    ("d4_L2_sum_bn_scalar_ld_d1", 4, 2, "sum", True, [17], "ld_d1", True),
    ("d8_L2_sum_bn_17_31_ld_d4", 8, 2, "sum", True, [17, 31], "ld_d4", True),
    ("d8_L17_mean_bn_32_ld_d1", 8, 17, "mean", True, [32], "ld_d1", True),
    ("d8_L64_max_bn_33_misaligned_base", 8, 64, "max", True, [33], "off1", True),
    ("d8_L17_sum_bn_three_calls_ranges", 8, 17, "sum", True, [("range", 5, 33), 9, ("range", 40, 17)], "ld_d", True),
    ("d252_L2_sum_bn_65", 252, 2, "sum", True, [65], "ld_d", True),
    ("d252_L17_max_copy_1_9_ld_d4", 252, 17, "max", False, [1, 9], "ld_d4", False),
    ("d256_L17_sum_bn_31_33", 256, 17, "sum", True, [31, 33], "ld_d", True),
    ("d256_L2_mean_bn_2_7_8_misaligned_base", 256, 2, "mean", True, [2, 7, 8], "off1", True),
    ("d256_L1_max_bn_16_ld_d1", 256, 1, "max", True, [16], "ld_d1", True),
    ("d257_L2_sum_bn_15_17", 257, 2, "sum", True, [15, 17], "ld_d", True),
    ("d257_L17_mean_in_place_33", 257, 17, "mean", False, [33], "ld_d", True),
    ("d257_L64_max_bn_9_ld_d4", 257, 64, "max", True, [9], "ld_d4", True),
    ("d260_L2_sum_bn_32_2", 260, 2, "sum", True, [32, 2], "ld_d", True),
    ("d260_L17_mean_bn_65_ld_d4", 260, 17, "mean", True, [65], "ld_d4", True),
    ("d260_L1_max_copy_8_misaligned_base", 260, 1, "max", False, [8], "off1", False),
    ("d260_L64_sum_copy_17", 260, 64, "sum", False, [17], "ld_d", False),
    ("d512_L2_mean_bn_7_33", 512, 2, "mean", True, [7, 33], "ld_d", True),
    ("d512_L17_sum_in_place_17_ld_d1", 512, 17, "sum", False, [17], "ld_d1", True),
    ("d512_L64_max_bn_8", 512, 64, "max", True, [8], "ld_d", True),
    ("d516_L2_sum_bn_16_9", 516, 2, "sum", True, [16, 9], "ld_d", True),
    ("d516_L17_max_bn_31_ld_d4", 516, 17, "max", True, [31], "ld_d4", True),
    ("d516_L1_mean_copy_one_row", 516, 1, "mean", False, [1], "ld_d", False),
    ("d4_L2_mean_bn_eight_calls", 4, 2, "mean", True, [2, 3, 8, 9, 15, 16, 17, 7], "ld_d", True),
]
# batches over two slots: (id, {key: (d, max_len, pool, batch-norm)}, [(key, call)], layout)
FORWARD_TWO_SLOTS = [
    ("step_five_calls_three_and_two", {"e": (260, 17, "sum", True), "r": (260, 2, "sum", True)},
     [("e", 33), ("r", 9), ("e", 9), ("e", 15), ("r", 16)], "ld_d"),
    ("two_slots_differ_in_d_and_L", {"a": (8, 64, "mean", True), "b": (516, 2, "sum", True)}, [("a", 17), ("b", 9), ("a", 2)], "ld_d"),
]
FORWARD_IDS = [c[0] for c in FORWARD] + [c[0] for c in FORWARD_TWO_SLOTS]


def forward_case(case_id):
    seed = sum(map(ord, case_id))
    for cid, d, L, pool, bn, spec, layout, inplace in FORWARD:
        if cid == case_id:
            slots = {"s": slot_data(d, L, ids_needed(spec), 100, pool, bn, seed)}
            return slots, [("s",) + c for c in make_calls(spec, slots["s"])], layout, inplace
    cid, sl, spec, layout = next(c for c in FORWARD_TWO_SLOTS if c[0] == case_id)
    slots = {k: slot_data(d, L, 80, 100, pool, bn, seed + i) for i, (k, (d, L, pool, bn)) in enumerate(sl.items())}
    return slots, [(k,) + make_calls([c], slots[k])[0] for k, c in spec], layout, True


@pytest.mark.parametrize("case_id", FORWARD_IDS)
def test_forward_sweep_against_float64(okge_lib, case_id):
    """training encode: raw and batch-normed rows, the calls' saved mean and rstd, the running statistics after the slot's calls
    in launch order; with batch-norm also an eval-mode encode on the non-trivial running statistics (left unchanged)"""
    slots, batch, layout, inplace = forward_case(case_id)
    mine = gpu_pass(slots, batch, layout=layout, inplace=inplace)
    check(case_id, mine, slots, batch, references(slots, batch), training=True)
    if any(s["bn"] is not None for s in slots.values()):
        ev = gpu_pass(slots, batch, training=False, layout=layout, inplace=inplace)
        check(case_id + "/eval", ev, slots, batch, references(slots, batch, training=False), training=False)
        for k, s in slots.items():
            if s["bn"] is not None:
                assert torch.equal(ev[k]["running_mean"].cpu(), s["running"][0]) and torch.equal(ev[k]["running_var"].cpu(), s["running"][1])


@pytest.mark.parametrize("d,layout,inplace", [(3, "ld_d", True), (4, "ld_d", False), (260, "ld_d4", True), (257, "off1", False)])
def test_sum_of_one_token_is_a_copy_of_the_table_rows(okge_lib, d, layout, inplace):
    slots = {"s": slot_data(d, 1, 80, 100, "sum", False, seed=d)}
    batch = [("s",) + c for c in make_calls([33, ("range", 7, 40)], slots["s"])]
    mine = gpu_pass(slots, batch, layout=layout, inplace=inplace)
    want = slots["s"]["W"][slots["s"]["tok"][row_ids(slot_calls(batch, "s"))].long()[:, 0]]
    assert torch.equal(mine["s"]["raw"].cpu(), want) and torch.equal(mine["s"]["out"].cpu(), want)


@pytest.mark.parametrize("d,L,layout", [(3, 17, "ld_d"), (8, 64, "ld_d4"), (257, 2, "off1"), (260, 17, "ld_d")])
def test_max_pooling_forward_is_exact(okge_lib, d, L, layout):
    """a maximum rounds nothing: the rows equal torch's amax over the gathered fp32 rows bit for bit (padding takes part)"""
    slots = {"s": slot_data(d, L, 80, 100, "max", False, seed=d + L)}
    batch = [("s",) + c for c in make_calls([33, 9], slots["s"])]
    mine = gpu_pass(slots, batch, layout=layout, inplace=False)
    want = slots["s"]["W"][slots["s"]["tok"][row_ids(slot_calls(batch, "s"))].long()].amax(1)
    assert torch.equal(mine["s"]["raw"].cpu(), want) and torch.equal(mine["s"]["out"].cpu(), want)


# ---- backward with float atomics --------------------------------------------------------------------------------------------
# (id, d, max_len, pool, batch-norm, calls, token kind, layout)
ATOMICS = [
    ("d3_sum_bn_15_17", 3, 5, "sum", True, [15, 17], "repeat", "ld_d"),
    ("d3_mean_16", 3, 5, "mean", False, [16], "mixed", "ld_d"),
    ("d3_max_bn_16_9", 3, 5, "max", True, [16, 9], "mixed", "ld_d"),
    ("d8_sum_bn_16_33", 8, 17, "sum", True, [16, 33], "mixed", "ld_d4"),
    ("d8_mean_bn_17", 8, 2, "mean", True, [17], "repeat", "ld_d"),
    ("d8_max_15", 8, 17, "max", False, [15], "repeat", "off1"),
    ("d8_max_exact_ties_bn", 8, 3, "max", True, [16, 17], "ties", "ld_d"),
    ("d257_sum_16", 257, 5, "sum", False, [16], "mixed", "ld_d"),
    ("d257_mean_bn_15_16", 257, 17, "mean", True, [15, 16], "mixed", "ld_d"),
    ("d257_max_bn_17", 257, 5, "max", True, [17], "repeat", "ld_d"),
    ("d257_max_exact_ties", 257, 3, "max", False, [17], "ties", "ld_d"),
    ("d260_sum_bn_17_15", 260, 5, "sum", True, [17, 15], "repeat", "ld_d"),
    ("d260_mean_16", 260, 17, "mean", False, [16], "mixed", "ld_d4"),
    ("d260_max_bn_16_2", 260, 5, "max", True, [16, 2], "mixed", "ld_d"),
]


def atomics_case(case_id):
    _, d, L, pool, bn, spec, kind, layout = next(c for c in ATOMICS if c[0] == case_id)
    slots = {"s": slot_data(d, L, 64, 100, pool, bn, sum(map(ord, case_id)), kind=kind)}
    return slots, [("s",) + c for c in make_calls(spec, slots["s"])], layout


def assert_atomics_fixture(case_id, slots, batch):
    """what the case is there for, on its own inputs: hot and cold tokens, a token repeated inside every row, exact ties for a
    column maximum with row 0 winning some columns (by torch's argmax: the first maximum)"""
    s = slots["s"]
    t = s["tok"][row_ids(slot_calls(batch, "s"))].long()
    assert ((t > 0) & (t < HOT)).any() and (t >= HOT).any()
    kind = next(c[6] for c in ATOMICS if c[0] == case_id)
    if kind == "ties":
        emb = s["W"][t]
        assert ((emb == emb.amax(1, keepdim=True)).sum(1) > 1).any()
        assert (torch.gather(t, 1, emb.argmax(1)) == 0).any()
    if kind == "repeat":
        assert (t[:, 0] == t[:, 1]).all() and (t[:, 0] > 0).all()


@pytest.mark.parametrize("case_id", [c[0] for c in ATOMICS])
def test_backward_atomics_against_float64(okge_lib, case_id):
    """encode + backward with engine.scatter = 'atomics': the token-table gradient ADDED to a seeded dW, the batch-norm
    gradients added up over the calls in launch order, the touched map"""
    slots, batch, layout = atomics_case(case_id)
    assert_atomics_fixture(case_id, slots, batch)
    d_out, prefill = random_d_out(slots, batch), random_prefill(slots)
    refs = references(slots, batch, d_out=d_out)
    mine = gpu_pass(slots, batch, layout=layout, d_out=d_out, scatter="atomics", prefill=prefill, stamp=7)
    check(case_id, mine, slots, batch, refs, prefill=prefill, unordered=d_out)
    assert np.array_equal(mine["s"]["touched"].cpu().numpy(), expected_touched(slots, batch, "s", 7))


# ---- backward through the scatter plan ------------------------------------------------------------------------------------
NAMED_COUNTS = (1, 2, 63, 64, 65, 1024, 1025)            # pairs of the named cold tokens; one more token has `big` pairs


def designed_tokens(n, L, vocab, seed, big=2049):
    """an n x L token matrix in which named cold tokens (spread over [32, vocab), the last one vocab - 1) hold exactly
    NAMED_COUNTS pairs and one holds `big`, at random places; every other position a hot token or padding.
    Returns (tok, {pair count: token})."""
    rng = np.random.default_rng(seed)
    counts = NAMED_COUNTS + (big,)
    assert n * L >= sum(counts) and vocab - HOT >= len(counts)
    flat = rng.integers(0, HOT, n * L)
    where = rng.permutation(n * L)
    names = np.linspace(HOT, vocab - 1, len(counts)).round().astype(np.int64)
    named, p = {}, 0
    for c, token in zip(counts, rng.permutation(names[:-1]).tolist() + [int(names[-1])]):
        flat[where[p:p + c]] = token
        named[c] = int(token)
        p += c
    return torch.from_numpy(flat.reshape(n, L).astype(np.int32)), named


def assert_designed(tok, named, rows, big=2049, both_windows=False):
    """the pair counts of the named tokens over the batch's rows, by np.bincount"""
    t = tok[rows].numpy().astype(np.int64)
    counts = np.bincount(t.reshape(-1), minlength=int(tok.max()) + 1)
    for c in NAMED_COUNTS:
        assert counts[named[c]] == c, (c, counts[named[c]])
    assert counts[named[big]] == big >= 2049
    assert (counts[HOT:] > 0).sum() == len(named)        # no other cold token
    if both_windows:                                     # pair indices on both sides of the first 32 768-pair bitmap window
        assert t.size > 32768
        for c in (big, 1024):
            pairs = np.nonzero(t.reshape(-1) == named[c])[0]
            assert pairs.min() < 32768 <= pairs.max(), c


# (id, d, max_len, rows, vocabulary, pool, batch-norm, pairs of the big token, calls as row ranges)
DESIGNED = [
    ("designed_d4_L17_sum_bn", 4, 17, 310, 2049, "sum", True, 2049, [310]),
    ("designed_d260_L17_mean_bn_three_calls", 260, 17, 310, 4100, "mean", True, 2100, [130, 61, 119]),
    ("designed_d4_L16_two_bitmap_windows", 4, 16, 2080, 4100, "sum", True, 3000, [2080]),
]


def designed_case(case_id):
    _, d, L, n, vocab, pool, bn, big, split = next(c for c in DESIGNED if c[0] == case_id)
    tok, named = designed_tokens(n, L, vocab, sum(map(ord, case_id)), big)
    slots = {"s": slot_data(d, L, n, vocab, pool, bn, sum(map(ord, case_id)), tok=tok)}
    batch, r0 = [], 0
    for c in split:
        batch.append(("s", None, r0, c))
        r0 += c
    return slots, batch, named, big


def plan_checks(case, slots, batch, layout="ld_d", stamp=3):
    """encode + backward through the scatter plan on seeded dW / d_bn: every tensor against float64; the touched map exact; the
    scatter state all zero afterwards; a second run bit-identical; the atomics path on the same inputs within the band (its dW
    calibrated as an unordered scatter: see check)"""
    d_out, prefill = random_d_out(slots, batch), random_prefill(slots)
    refs = references(slots, batch, d_out=d_out)
    mine = gpu_pass(slots, batch, layout=layout, d_out=d_out, prefill=prefill, stamp=stamp)
    eng = mine["engine"]
    assert eng.scatter_plan([(mine[k]["slot"],) for k in slots]) and eng._state is not None
    check(case, mine, slots, batch, refs, prefill=prefill)
    assert not eng._state.any(), (case, "scatter state not left all-zero", torch.nonzero(eng._state).reshape(-1)[:8].tolist())
    for k in slots:
        assert np.array_equal(mine[k]["touched"].cpu().numpy(), expected_touched(slots, batch, k, stamp)), (case, k)
    again = gpu_pass(slots, batch, layout=layout, d_out=d_out, prefill=prefill, stamp=stamp, engine=eng)
    assert not eng._state.any()
    for k in slots:
        for name in ("dW", "d_bn_weight", "d_bn_bias", "raw", "out", "touched"):
            if name in mine[k]:
                assert torch.equal(mine[k][name], again[k][name]), (case, k, name)
    atom = gpu_pass(slots, batch, layout=layout, d_out=d_out, scatter="atomics", prefill=prefill, stamp=stamp)
    check(case + "/atomics", atom, slots, batch, refs, prefill=prefill, unordered=d_out)
    return mine


@pytest.mark.parametrize("case_id", [c[0] for c in DESIGNED])
def test_plan_designed_pair_counts(okge_lib, case_id):
    """segments of exactly 1 (no segment), 2, 63, 64 (one wave), 65, 1 024 (rank sort in LDS), 1 025 and >= 2 049 pairs (bitmap),
    at d = 4, at d = 260 (columns past 256) and with more than 32 768 pairs (two bitmap windows)"""
    slots, batch, named, big = designed_case(case_id)
    assert_designed(slots["s"]["tok"], named, row_ids(slot_calls(batch, "s")), big, both_windows="two_bitmap" in case_id)
    plan_checks(case_id, slots, batch)


def vocab_tokens(n, L, vocab, seed):
    """random token rows over [0, vocab) with vocab - 1 present"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, vocab, (n, L), generator=g, dtype=torch.int32)
    if vocab > 2 * HOT:                                  # a third of the tokens hot, whatever the vocabulary
        hot = torch.randint(1, HOT, (n, L), generator=g, dtype=torch.int32)
        tok = torch.where(torch.rand(n, L, generator=g) < 0.33, hot, tok)
    tok[torch.arange(L)[None, :] >= torch.randint(1, L + 1, (n,), generator=g)[:, None]] = 0
    tok[n // 2, 0] = vocab - 1
    return tok


@pytest.mark.parametrize("vocab", [2, 32, 33, 2048, 2049, 4100])
def test_plan_vocabulary_sizes(okge_lib, vocab):
    """only token 1; no cold token at all; one cold token; one allocation workgroup full, one token over, three workgroups"""
    n, L = 70, 5
    tok = vocab_tokens(n, L, vocab, vocab)
    assert int(tok.max()) == vocab - 1 and bool((tok >= HOT).any()) == (vocab > HOT)
    slots = {"s": slot_data(8, L, n, vocab, "mean" if vocab % 2 else "sum", False, vocab, tok=tok)}
    plan_checks(f"vocab_{vocab}", slots, [("s", None, 0, 40), ("s", None, 40, 30)])


def _chunks(L, n):
    assert n % (1024 // L)                               # the last 1 024-pair histogram chunk is partial
    return {"s": slot_data(8, L, n, 300, "sum", True, L)}, [("s", None, 0, n)]


def _longer_slot():
    slots = {"a": slot_data(8, 64, 80, 300, "sum", True, 1), "b": slot_data(4, 2, 80, 300, "mean", True, 2)}
    return slots, [("a",) + make_calls([21], slots["a"])[0], ("b",) + make_calls([50], slots["b"])[0]]


def _groups(spec):
    slots = {"a": slot_data(260, 17, 80, 300, "sum", True, 11), "b": slot_data(8, 5, 80, 2100, "mean", True, 12)}
    return slots, [(k,) + make_calls([c], slots[k])[0] for k, c in spec]


# batch-normed plan batches by what they reach: id -> (slots, batch)
PLAN_CASES = {
    "L17_chunks_of_60_rows": lambda: _chunks(17, 130),
    "L64_chunks_of_16_rows": lambda: _chunks(64, 41),
    # two token tables in one batch, max_len 64 and 2: both are histogrammed in chunks of 16 rows
    "chunk_size_from_the_longer_slot": _longer_slot,
    # calls that share a token table form a group with row, slab and chunk offsets per call; two groups in one batch
    "groups_three_and_two": lambda: _groups([("a", 33), ("b", 9), ("a", ("range", 3, 70)), ("a", 15), ("b", 40)]),
    "groups_eight_calls": lambda: _groups([("a", 9), ("a", 33), ("b", 17), ("a", 2), ("b", ("range", 0, 65)), ("a", 64), ("b", 8), ("a", 31)]),
}


@pytest.mark.parametrize("case_id", list(PLAN_CASES))
def test_plan_chunks_and_groups(okge_lib, case_id):
    slots, batch = PLAN_CASES[case_id]()
    plan_checks(case_id, slots, batch)


@pytest.mark.parametrize("blocks", [257, 1025])
def test_plan_hot_slab_blocks(okge_lib, blocks):
    """hot tokens only, one token a row: 257 and 1 025 workgroup slabs (listed 256 at a time, a quarter of them per wave)"""
    n = 32 * blocks
    g = torch.Generator().manual_seed(blocks)
    tok = torch.randint(0, HOT, (n, 1), generator=g, dtype=torch.int32)
    slots = {"s": slot_data(4, 1, n, 40, "sum", False, blocks, tok=tok)}
    assert (n + 31) // 32 == blocks
    plan_checks(f"hot_slabs_{blocks}", slots, [("s", None, 0, n)])


def test_plan_rows_of_only_padding_under_mean_pooling(okge_lib):
    """a row without a live token divides by 1e-12: its pooled row is 1e12 x the sum (compared by relative error, separately),
    its dx 1e12 x d_out -- which no token receives, and which must not leak into the hot tokens' slabs (0 x 1e12 d_out is 0).
    No batch-norm: the statistics of such a call mean nothing."""
    slots = {"s": slot_data(8, 5, 96, 100, "mean", False, 5, kind="padrows")}
    batch = [("s", None, 0, 96)]
    pad = (slots["s"]["tok"] == 0).all(1).numpy()
    assert pad.sum() >= 19 and (~pad).sum() >= 64
    d_out, prefill = random_d_out(slots, batch), random_prefill(slots)
    refs = references(slots, batch, d_out=d_out)
    for scatter in ("plan", "atomics"):
        mine = gpu_pass(slots, batch, d_out=d_out, prefill=prefill, scatter=scatter)
        check(f"padding_only_rows/{scatter}", mine, slots, batch, refs, prefill=prefill, pad_rows={"s": pad},
              unordered=d_out if scatter == "atomics" else None)


def test_plan_adds_into_dW_exactly_once(okge_lib):
    """every element of a token row takes ONE read-modify-write: seeded dW ends as prefill + (the gradient from zero), bit for bit"""
    slots, batch, _, _ = designed_case("designed_d260_L17_mean_bn_three_calls")
    d_out, prefill = random_d_out(slots, batch), random_prefill(slots)
    base = gpu_pass(slots, batch, d_out=d_out)
    again = gpu_pass(slots, batch, d_out=d_out, prefill=prefill)
    assert torch.equal(again["s"]["dW"], prefill["s"]["dW"].cuda() + base["s"]["dW"])
    touched = base["s"]["touched"].bool()
    assert not base["s"]["dW"][~touched].any() and not touched[0]


def test_plan_smaller_batch_on_a_used_engine_gives_a_fresh_engines_bits(okge_lib):
    slots, batch, _, _ = designed_case("designed_d4_L17_sum_bn")
    d_out = random_d_out(slots, batch)
    big = gpu_pass(slots, batch, d_out=d_out)
    small = [("s", None, 20, 70), ("s", torch.arange(200, 233, dtype=torch.int32), 0, 33)]
    d_small = {"s": d_out["s"][:103] * 0.5}
    reused = gpu_pass(slots, small, d_out=d_small, engine=big["engine"])
    fresh = gpu_pass(slots, small, d_out=d_small)
    assert reused["engine"]._ws_bytes > fresh["engine"]._ws_bytes and not reused["engine"]._state.any()
    for name in ("raw", "out", "saved_mean", "saved_rstd", "running_mean", "running_var", "dW", "d_bn_weight", "d_bn_bias", "touched"):
        assert torch.equal(reused["s"][name], fresh["s"][name]), name


# ---- refusals: the N.check error, nothing launched, the outputs keep their NaN sentinel --------------------------------------
def _backward_raw(slots, batch, stamp=1, state=True, state_delta=0, ws_delta=0):
    """okge_pool_backward_calls straight through ctypes after a good encode; dW and d_bn hold NaN sentinels.  Returns (error or
    None, the slot)."""
    from open_knowledge_graph_embeddings_amd import _native as N
    from open_knowledge_graph_embeddings_amd.token_pooled import PoolEngine
    d_out = random_d_out(slots, batch)
    nan = {k: dict(dW=torch.full(s["W"].shape, NAN), d_bn=torch.full((2 * s["d"],), NAN)) for k, s in slots.items()}
    eng = PoolEngine("cuda")
    calls, sl = [], None
    orig = eng.backward_calls
    eng.backward_calls = lambda c: calls.extend(c)       # (gpu_pass builds the calls; the launch is made below)
    mine = gpu_pass(slots, batch, d_out=d_out, prefill=nan, engine=eng)
    eng.backward_calls = orig
    sl = mine["s"]["slot"]
    sl.stamp = stamp
    arr, keep = eng._calls(calls, True)
    lib = eng.lib
    need_ws, need_state = int(lib.okge_pool_backward_workspace_bytes(arr, len(calls))), int(lib.okge_pool_scatter_state_bytes(arr, len(calls)))
    ws = torch.empty(max(need_ws, 1 << 16), dtype=torch.uint8, device="cuda")
    st = torch.zeros(max(need_state, 1 << 16), dtype=torch.uint8, device="cuda")
    err = None
    try:
        N.check(lib.okge_pool_backward_calls(arr, len(calls), ws.data_ptr(), (need_ws or ws.numel()) + ws_delta,
                                             st.data_ptr() if state else None, ((need_state or st.numel()) + state_delta) if state else 0,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "okge_pool_backward_calls")
    except N.OkgeError as e:
        err = e
    torch.cuda.synchronize()
    del keep
    return err, sl, st


def _refused(match, d=8, pool="sum", **kw):
    slots = {"s": slot_data(d, 5, 64, 100, pool, True, 3)}
    err, sl, st = _backward_raw(slots, [("s", None, 0, 20), ("s", None, 30, 9)], **kw)
    assert err is not None and match in str(err), err
    assert torch.isnan(sl.dW).all() and torch.isnan(sl.d_bn).all() and not sl.touched.any() and not st.any()     # nothing launched


def test_abi_accepts_what_the_refusals_vary(okge_lib):
    """the same call with exact sizes and a stamp of 255 runs (so the refusals below are refusals of ONE argument)"""
    slots = {"s": slot_data(8, 5, 64, 100, "sum", True, 3)}
    err, sl, st = _backward_raw(slots, [("s", None, 0, 20), ("s", None, 30, 9)], stamp=255)
    assert err is None and (sl.touched == 255).any() and not st.any()
    assert torch.isnan(sl.dW[1:][sl.touched[1:] == 255]).all()      # (NaN + gradient: the rows were reached)


def test_abi_refuses_a_stamp_of_0(okge_lib):
    _refused("touched_stamp must lie in 1..255", stamp=0)


def test_abi_refuses_a_scatter_state_with_d_not_a_multiple_of_4(okge_lib):
    _refused("the scatter plan needs sum / mean pooling, slot sizes that are a multiple of 4", d=6)


def test_abi_refuses_scatter_state_one_byte_short(okge_lib):
    _refused("scatter state too small", state_delta=-1)


def test_abi_refuses_scatter_workspace_one_byte_short(okge_lib):
    _refused("workspace too small", ws_delta=-1)


# ---- tokens outside the vocabulary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,pool,scatter", [(8, "sum", "plan"), (8, "mean", "atomics"), (67, "max", "atomics")])
def test_out_of_vocabulary_tokens_read_row_0_and_are_counted(okge_lib, d, pool, scatter):
    """tokens equal to vocab and to -1 in the token matrix: every tensor equals the restatement with those tokens set to 0 (they
    read row 0, count as padding and receive no gradient), and the id-error word counts each (row, position) once per encode"""
    from open_knowledge_graph_embeddings_amd import _native as N
    vocab = 100
    slots = {"s": slot_data(d, 5, 64, vocab, pool, True, 41)}
    tok = slots["s"]["tok"]
    live = torch.nonzero((tok[:40, :2] > 0).all(1)).reshape(-1)
    tok[live[0], 1], tok[live[1], 0], tok[live[2], 1], tok[live[3], 0] = vocab, -1, -1, vocab
    batch = [("s", None, 0, 40), ("s", live[:9].to(torch.int32), 0, 9)]
    bad = int(((tok[row_ids(slot_calls(batch, "s"))] < 0) | (tok[row_ids(slot_calls(batch, "s"))] >= vocab)).sum())
    assert bad == 8
    clean = {"s": dict(slots["s"], tok=torch.where((tok < 0) | (tok >= vocab), torch.zeros_like(tok), tok))}
    d_out, prefill = random_d_out(slots, batch), random_prefill(slots)
    mine = gpu_pass(slots, batch, d_out=d_out, prefill=prefill, scatter=scatter)
    assert N.id_errors() == bad                          # (the call also resets the count)
    check(f"out_of_vocabulary_{pool}_{scatter}", mine, clean, batch, references(clean, batch, d_out=d_out), prefill=prefill,
          unordered=d_out if scatter == "atomics" else None)
    assert np.array_equal(mine["s"]["touched"].cpu().numpy(), expected_touched(clean, batch, "s", 1))
