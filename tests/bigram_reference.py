"""A plain torch-CPU restatement of one bigram pass (okge_bigram_encode_calls / okge_bigram_backward_calls,
csrc/okge_bigram.hip) at a chosen dtype -- float64 as the reference, float32 to calibrate error bounds.  Not a conftest: the
tests import it (the per-magnitude-band rule is lstm_reference.band_check).

One pass: the calls' rows one after the other (ids, or first_id .. first_id + n - 1) -> their token rows (the id -> token
mapping the reference's encode_* leave out; the fixtures come from the reference through a shim that does the same) ->
embedding rows x_t (a token id outside the vocabulary reads row 0, the kernels' documented substitution; it still counts as
live) -> Y[t] = K0 x_t + K1 x_{t+1} with K_j = conv[:, :, j], t = 0 .. L-2 -> normalize 'batchnorm': BatchNorm1d(d,
momentum=None, eps 1e-5) per call over all n (L-1) positions, padded ones included: training mode with that call's
statistics, the running mean and unbiased variance a cumulative average with factor 1 / num_batches_tracked (one count per
call), or eval mode with the running statistics -> + x_{t+1} -> x mask[t] = token[t+1] > 0 -> max over t (pool 'max') or sum
(any other) -> normalize 'mean': / (sum mask + 1e-12).  Gradients are those of sum(out * d_out), the token table's row 0
zeroed (padding_idx=0)."""
import torch

from lstm_reference import row_ids

BN_EPS = 1e-5
GRAD_NAMES = ("dW", "d_conv", "d_bn_weight", "d_bn_bias")


def encode(W, tok, conv, calls, pool="sum", normalize="", bn=None, running=None, counter=0, training=True):
    """The differentiable forward on tensors of one dtype (W, conv, bn = (weight, bias) may require grad).  running =
    [mean, var] is updated IN PLACE in training mode; returns (out [rows, d], Y [rows, L-1, d], counter after the pass)."""
    vocab, d = W.shape
    rows = row_ids(calls)
    t = tok[rows].to(torch.int64)
    gather = torch.where((t >= 0) & (t < vocab), t, torch.zeros_like(t))
    x = W[gather]                                                      # [rows, L, d]
    mask = (t > 0)[:, 1:].to(W.dtype).unsqueeze(2)                     # [rows, L-1, 1]
    Y = x[:, :-1] @ conv[:, :, 0].t() + x[:, 1:] @ conv[:, :, 1].t()   # [rows, L-1, d]
    Z = Y
    if normalize == "batchnorm":
        parts, r0 = [], 0
        for _, _, n in calls:
            n = int(n)
            y = Y[r0:r0 + n].transpose(1, 2)                           # (n, d, L-1), the Conv1d output layout
            if training:
                counter += 1
                z = torch.nn.functional.batch_norm(y, running[0], running[1], bn[0], bn[1], True, 1.0 / counter, BN_EPS)
            else:
                z = torch.nn.functional.batch_norm(y, running[0], running[1], bn[0], bn[1], False, 0.0, BN_EPS)
            parts.append(z.transpose(1, 2))
            r0 += n
        Z = torch.cat(parts)
    enc = (Z + x[:, 1:]) * mask
    out = enc.max(dim=1)[0] if pool == "max" else enc.sum(dim=1)
    if normalize == "mean":
        out = out / (mask.sum(1) + 1e-12)
    return out, Y, counter


def bigram_pass(W, tok, conv, calls, pool="sum", normalize="", bn=None, running=None, counter=0, training=True, d_out=None,
                dtype=torch.float64):
    """W (vocab x d), tok (n_ids x max_len), conv (d, d, 2), bn = (weight, bias) with normalize 'batchnorm', running = (mean,
    var) or None (fresh: zeros, ones), counter = num_batches_tracked before the pass.  Returns a dict: out, Y (the convolution
    output, rows x (L-1) x d), running_mean / running_var / num_batches_tracked (after the pass), and with d_out (rows x d) the
    GRAD_NAMES (the batch-norm ones only with batch-norm), all float64 numpy."""
    W, tok = W.detach().cpu(), tok.detach().cpu()
    d = W.shape[1]
    grad = d_out is not None
    batchnorm = normalize == "batchnorm"
    leaves = [x.detach().cpu().to(dtype).clone().requires_grad_(grad) for x in (W, conv) + (tuple(bn) if batchnorm else ())]
    run = None
    if batchnorm:
        if running is None:
            running = (torch.zeros(d), torch.ones(d))
        run = [x.detach().cpu().to(dtype).clone() for x in running]
    with torch.set_grad_enabled(grad):
        out, Y, counter = encode(leaves[0], tok, leaves[1], calls, pool, normalize, leaves[2:] if batchnorm else None, run,
                                 int(counter), training)
        if grad:
            (out * d_out.detach().cpu().to(dtype)).sum().backward()
    res = {"out": out.detach().double().numpy(), "Y": Y.detach().double().numpy()}
    if batchnorm:
        res.update(running_mean=run[0].double().numpy(), running_var=run[1].double().numpy(), num_batches_tracked=counter)
    if grad:
        leaves[0].grad[0] = 0                                         # padding_idx=0
        for name, x in zip(GRAD_NAMES, leaves):
            res[name] = x.grad.double().numpy()
    return res
