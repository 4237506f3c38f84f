"""A plain torch-CPU restatement of one LSTM pass (okge_lstm_encode_calls / okge_lstm_backward_calls, csrc/okge_lstm.hip) at a
chosen dtype -- float64 as the reference, float32 to calibrate error bounds -- and the per-magnitude-band rule the HIP results
are held to.  Not a conftest: the tests import it.

One pass: the calls' rows one after the other (ids, or first_id .. first_id + n - 1) -> their token rows -> embedding rows
(a token id outside the vocabulary reads row 0, the kernels' documented substitution; it still counts as live) -> one-layer
LSTM (torch._VF.lstm, h0 = c0 = 0) -> h at last = count(tokens > 0) - 1 (-1 wraps to max_len - 1) -> BatchNorm1d per call:
training mode with that call's statistics, the running mean and unbiased variance updated call after call (momentum 0.1,
eps 1e-5), or eval mode with the running statistics.  Gradients are those of sum(out * d_out), the token table's row 0
zeroed (padding_idx=0)."""
import numpy as np
import torch

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
GRAD_NAMES = ("dW", "dW_ih", "dW_hh", "db_ih", "db_hh", "d_bn_weight", "d_bn_bias")

torch.set_num_threads(max(1, min(16, torch.get_num_threads())))      # the GPU box gives a test 16 CPUs


def row_ids(calls):
    """calls [(ids or None, first_id, n)] -> the pass's row ids, int64, in row order"""
    out = []
    for ids, first, n in calls:
        if ids is None:
            out.append(torch.arange(int(first), int(first) + int(n), dtype=torch.int64))
        else:
            out.append(torch.as_tensor(ids).detach().cpu().reshape(-1)[:int(n)].to(torch.int64))
    return torch.cat(out)


def lstm_pass(W, tok, lstm, calls, bn=None, running=None, training=True, d_out=None, dtype=torch.float64):
    """W (vocab x d), tok (n_ids x max_len), lstm = (w_ih, w_hh, b_ih, b_hh), bn = (weight, bias) or None,
    running = (mean, var) or None (fresh: zeros, ones).  Returns a dict: raw, out (= raw without batch-norm), running_mean /
    running_var (after the pass), and with d_out (rows x d) the GRAD_NAMES (the batch-norm ones only with batch-norm), all
    float64 numpy."""
    W, tok = W.detach().cpu(), tok.detach().cpu()
    vocab, d = W.shape
    grad = d_out is not None
    leaves = [x.detach().cpu().to(dtype).clone().requires_grad_(grad) for x in (W,) + tuple(lstm) + (tuple(bn) if bn else ())]
    W_, w_ih, w_hh, b_ih, b_hh = leaves[:5]
    rows = row_ids(calls)
    t = tok[rows].to(torch.int64)
    last = (t > 0).sum(1) - 1                                         # -1 indexes max_len - 1
    gather = torch.where((t >= 0) & (t < vocab), t, torch.zeros_like(t))
    with torch.set_grad_enabled(grad):
        z = torch.zeros(1, t.shape[0], d, dtype=dtype)
        h = torch._VF.lstm(W_[gather], (z, z), [w_ih, w_hh, b_ih, b_hh], True, 1, 0.0, False, False, True)[0]
        raw = h[torch.arange(t.shape[0]), last]
        out, res = raw, {}
        if bn:
            if running is None:
                running = (torch.zeros(d), torch.ones(d))
            rm, rv = (x.detach().cpu().to(dtype).clone() for x in running)
            parts, r0 = [], 0
            for _, _, n in calls:
                n = int(n)
                parts.append(torch.nn.functional.batch_norm(raw[r0:r0 + n], rm, rv, leaves[5], leaves[6], training, BN_MOMENTUM, BN_EPS))
                r0 += n
            out = torch.cat(parts)
            res["running_mean"], res["running_var"] = rm.double().numpy(), rv.double().numpy()
        if grad:
            (out * d_out.detach().cpu().to(dtype)).sum().backward()
    res["raw"], res["out"] = raw.detach().double().numpy(), out.detach().double().numpy()
    if grad:
        W_.grad[0] = 0                                                # padding_idx=0
        for name, x in zip(GRAD_NAMES, leaves):
            res[name] = x.grad.double().numpy()
    return res


def _bands(mag, min_band):
    """quantile bands [lo, hi] of |want| (0, 0.5, 0.9, 0.99, 1); with min_band, adjacent bands merged until each holds at least
    min_band elements (one band for a tensor smaller than that)"""
    qs = list(np.quantile(mag, [0.0, 0.5, 0.9, 0.99, 1.0]))
    if min_band is None:
        return list(zip(qs[:-1], qs[1:]))
    if mag.size < min_band:
        return [(qs[0], qs[-1])]
    edges = qs
    while len(edges) > 2:
        counts = [int(((mag >= lo) & (mag <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]
        small = [i for i, c in enumerate(counts) if c < min_band]
        if not small:
            break
        i = small[0]
        j = i - 1 if i > 0 else i + 1                               # merge with the lower neighbour (the first: the upper)
        del edges[max(i, j)]
    return list(zip(edges[:-1], edges[1:]))


def band_check(name, got, want, want32, min_band=64, max_factor=3.0, rms_factor=1.6):
    """per |want| band: max error <= max_factor x the fp32 restatement's, rms error <= rms_factor x its rms, each plus a floor
    of 1e-7 max|want|.  min_band=None: the plain quantile bands (test_full_size_against_float64's rule as first written).
    Returns the worst (max-error ratio, rms ratio) against the fp32 restatement over the bands, for the record."""
    x = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    x, want, want32 = x.reshape(-1), np.asarray(want).reshape(-1), np.asarray(want32).reshape(-1)
    assert np.isfinite(x).all(), (name, "non-finite values")
    err, err32, mag = np.abs(x - want), np.abs(want32 - want), np.abs(want)
    floor = 1e-7 * max(mag.max(), 1e-30)
    worst = [0.0, 0.0]
    for lo_, hi_ in _bands(mag, min_band):
        band = (mag >= lo_) & (mag <= hi_)
        if not band.any():
            continue
        emax, emax32 = err[band].max(), err32[band].max()
        erms, erms32 = np.sqrt((err[band] ** 2).mean()), np.sqrt((err32[band] ** 2).mean())
        assert emax <= max_factor * emax32 + floor, (name, lo_, emax, emax32)
        assert erms <= rms_factor * erms32 + floor, (name, lo_, erms, erms32)
        worst[0] = max(worst[0], emax / max(emax32, floor))
        worst[1] = max(worst[1], erms / max(erms32, floor))
    return tuple(worst)
