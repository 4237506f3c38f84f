"""CPU restatement (torch, float64 or float32) of what LookupTucker3RelationModel computes through AddLossModule
(openkge/model.py:142-173, :402-408, :455-510; openkge/trainer.py:48-113) with HAND-WRITTEN gradients, and of the reference's
Adagrad (utils/optim.py:139-160).  Test infrastructure: never imported by the package.  tests/test_tucker3_reference.py pins it
to the g18 fixtures the reference itself produced; the GPU tests then use it where no fixture can reach (full-size shapes)."""
import numpy as np
import torch


def T(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def project(W, rho, d):
    """encode_rel's Linear: (b, r_e) -> (b, d, d)"""
    return (rho @ W.t()).view(rho.shape[0], d, d)


def fold(W, ent_rows, rel_rows, n_po):
    """q rows of the prefix scorer: po rows (first n_po) M e, sp rows e^T M (model.py:160-164); also returns M"""
    d = ent_rows.shape[1]
    M = project(W, rel_rows, d)
    q_po = torch.bmm(M[:n_po], ent_rows[:n_po, :, None]).reshape(n_po, d)
    q_sp = torch.bmm(ent_rows[n_po:, None, :], M[n_po:]).reshape(-1, d)
    return torch.cat([q_po, q_sp]), M


def fold_backward(W, ent_rows, rel_rows, dq, n_po, M=None):
    """(d_ent_rows, d_rel_rows, dW) from the gradient of the q rows: autograd's walk through bmm and Linear, written out"""
    d = ent_rows.shape[1]
    if M is None:
        M = project(W, rel_rows, d)
    e_po, e_sp, g_po, g_sp = ent_rows[:n_po], ent_rows[n_po:], dq[:n_po], dq[n_po:]
    d_ent = torch.cat([torch.bmm(M[:n_po].transpose(1, 2), g_po[:, :, None]).reshape(n_po, d),       # q = M e     -> de = M^T dq
                       torch.bmm(M[n_po:], g_sp[:, :, None]).reshape(-1, d)])                         # q = e^T M   -> de = M dq
    dM = torch.cat([g_po[:, :, None] * e_po[:, None, :], e_sp[:, :, None] * g_sp[:, None, :]]).reshape(-1, d * d)
    return d_ent, dM @ W, dM.t() @ rel_rows


def triple_scores(W, subj, rel_rows, obj):
    """subj.bmm(rel.bmm(obj)) (model.py:167-171)"""
    d = subj.shape[1]
    M = project(W, rel_rows, d)
    return torch.bmm(subj[:, None, :], torch.bmm(M, obj[:, :, None])).reshape(-1, 1)


def _mask(fx, key, p, dtype, shape):
    if p <= 0:
        return torch.ones(shape, dtype=dtype)
    return T(fx[key], dtype) * (1.0 / (1.0 - p))


def ids_of(fx, prefix=""):
    """(po_rel, po_obj, sp_subj, sp_rel, cand) as int64 vectors (empty where a direction is absent)"""
    get = lambda k: torch.as_tensor(np.asarray(fx[prefix + k]).reshape(-1).astype(np.int64)) if (prefix + k) in fx else \
        torch.zeros(0, dtype=torch.int64)      # noqa: E731
    return get("po_rel"), get("po_obj"), get("sp_subj"), get("sp_rel"), get("cand")


def step(E, R, W, fx, dtype, prefix="", loss_kind="bce", smoothing=0.0, p_in=0.0, p_rel=0.0, normalizer=None):
    """AddLossModule.forward in training mode + (loss / normalizer).backward(): loss, outputs and the three dense gradients"""
    E, R, W = T(E, dtype), T(R, dtype), T(W, dtype)
    po_rel, po_obj, sp_subj, sp_rel, cand = ids_of(fx, prefix)
    y = T(fx[prefix + "labels"], dtype)
    n_po, n_sp, N = po_rel.numel(), sp_subj.numel(), cand.numel()
    B, d, r = n_po + n_sp, E.shape[1], R.shape[1]
    m_c = _mask(fx, "mask_cand", p_in, dtype, (N, d))
    m_e = torch.cat([_mask(fx, "mask_po_ent", p_in, dtype, (n_po, d)) if n_po else torch.zeros((0, d), dtype=dtype),
                     _mask(fx, "mask_sp_ent", p_in, dtype, (n_sp, d)) if n_sp else torch.zeros((0, d), dtype=dtype)])
    m_r = torch.cat([_mask(fx, "mask_po_rel", p_rel, dtype, (n_po, r)) if n_po else torch.zeros((0, r), dtype=dtype),
                     _mask(fx, "mask_sp_rel", p_rel, dtype, (n_sp, r)) if n_sp else torch.zeros((0, r), dtype=dtype)])
    ent_ids, rel_ids = torch.cat([po_obj, sp_subj]), torch.cat([po_rel, sp_rel])
    C = E[cand] * m_c
    ent_rows, rel_rows = E[ent_ids] * m_e, R[rel_ids] * m_r
    q, M = fold(W, ent_rows, rel_rows, n_po)
    x = q @ C.t()
    if normalizer is None:
        normalizer = float(B * N)
    if loss_kind == "bce":
        if smoothing > 0:                                        # trainer.py:103-105
            y = (y + 1.0 / N) * (1.0 - smoothing)
        loss = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum()
        G = (torch.sigmoid(x) - y) / normalizer
    else:                                                        # KLDivLoss(sum)(log_softmax(x), y), y not normalised (trainer.py:99-101)
        logp = torch.log_softmax(x, dim=1)
        loss = torch.where(y > 0, y * (torch.log(torch.where(y > 0, y, torch.ones_like(y))) - logp), torch.zeros_like(y)).sum()
        G = (torch.softmax(x, dim=1) * y.sum(1, keepdim=True) - y) / normalizer
    dC, dq = G.t() @ q, G @ C
    d_ent, d_rel, dW = fold_backward(W, ent_rows, rel_rows, dq, n_po, M)
    dE, dR = torch.zeros_like(E), torch.zeros_like(R)
    dE.index_add_(0, cand, dC * m_c)
    dE.index_add_(0, ent_ids, d_ent * m_e)
    dR.index_add_(0, rel_ids, d_rel * m_r)
    return dict(loss=float(loss), outputs=x, dE=dE, dR=dR, dW=dW, q=q, dq=dq, ent_rows=ent_rows, rel_rows=rel_rows, d_ent=d_ent,
                d_rel=d_rel)


def eval_scores(E, R, W, fx, dtype, prefix=""):
    """eval-mode (sp_prefix_score, po_prefix_score) against all entities from id 2, and the triple scores of t_subj / t_rel / t_obj"""
    E, R, W = T(E, dtype), T(R, dtype), T(W, dtype)
    po_rel, po_obj, sp_subj, sp_rel, _ = ids_of(fx, prefix)
    n_po = po_rel.numel()
    q, _ = fold(W, E[torch.cat([po_obj, sp_subj])], R[torch.cat([po_rel, sp_rel])], n_po)
    x = q @ E[2:].t()
    i = lambda k: torch.as_tensor(np.asarray(fx[k]).reshape(-1).astype(np.int64))      # noqa: E731
    tri = triple_scores(W, E[i("t_subj")], R[i("t_rel")], E[i("t_obj")])
    return x[n_po:], x[:n_po], tri


def adagrad(p, g, s, lr, wd, eps):
    """utils/optim.py:139-160 as torch.optim.Adagrad runs it: g += wd p; sum += g g; p -= lr g / (sqrt(sum) + eps)"""
    g = g + wd * p
    s = s + g * g
    return p - lr * g / (s.sqrt() + eps), s
