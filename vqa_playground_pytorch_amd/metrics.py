"""What the reference's loops report from the logits: top-k accuracy (train.py:22-38) and the predictions of test()
(train.py:110-191) and visu.py:188-194.

GPU tensors go through the HIP kernels of csrc/loss.hip (ops.predict_topk / ops.predict_candidates /
ops.kld_sum_loss_and_grad_hits); CPU tensors (the gloo tests, the CPU trainer) through torch ops with the same semantics.

One order everywhere: NaN ranks above every number (as in torch's topk / sort / max), otherwise the larger value ranks
higher, and ties go to the lower column.  The target class of a row is the FIRST index of its largest target value
(``torch.max(target, 1)``); its rank is the number of columns that beat it, and rank r < k is a top-k hit.
``hits[j]`` counts the rows whose target ranks <= j: Acc@1 is ``hits[0]``, Acc@5 ``hits[4]``.
"""
import torch


def _order(logits):
    """Column order of every row, best first: a stable descending sort puts NaN first and keeps ties in column order."""
    return torch.sort(logits, dim=1, descending=True, stable=True).indices


def target_rank(logits, target):
    """int64 [B]: the rank of each row's target class among its logits (torch ops; any device).  A 1-D integer target holds
    the classes themselves (sampled answers, train.py:30-32 leaves them as they are)."""
    if target.dim() == 1:
        if target.is_floating_point() or target.size(0) != logits.size(0):
            raise ValueError("a 1-D target must hold one integer class per row, got %s %s" % (target.dtype, tuple(target.shape)))
        t = target.to(torch.int64)
    else:
        t = torch.max(target, 1).indices
    zt = logits.gather(1, t[:, None])
    col = torch.arange(logits.size(1), device=logits.device)
    lower = col[None, :] < t[:, None]
    nan = torch.isnan(logits)
    better = torch.where(torch.isnan(zt), nan & lower, nan | (logits > zt) | ((logits == zt) & lower))
    return better.sum(1)


def _hits_from_rank(rank, kmax):
    return (rank[None, :] <= torch.arange(kmax, device=rank.device)[:, None]).sum(1).to(torch.int32)


def _check_k(C, k):
    if not 1 <= k <= min(16, C):
        raise ValueError("k=%d outside [1, min(16, C=%d)]" % (k, C))


def _dense(logits, target):
    """A sparse answer target -- the pair (a_idx int32 [B,K], a_val float32 [B,K]) or a dict holding the two -- as the dense
    [B,C] row it stands for (ops.densify); anything else as it is."""
    if isinstance(target, dict):
        target = (target["a_idx"], target["a_val"])
    if isinstance(target, (tuple, list)):
        from . import ops
        a_idx, a_val = target
        return ops.densify(a_idx, a_val, logits.size(1))
    return target


def topk_hits(logits, target, kmax):
    """int32 [kmax]: hits[j] = rows whose target ranks <= j.  target: [B,C] soft targets, a sparse pair (a_idx, a_val) of them
    (ops.densify), or (CPU tensors) integer classes [B]."""
    logits = logits.detach()
    target = _dense(logits, target)
    _check_k(logits.size(1), int(kmax))
    if logits.is_cuda:
        from . import ops
        return ops.predict_topk(logits, int(kmax), target=target, probs=False)[2]
    return _hits_from_rank(target_rank(logits, target), int(kmax))


def predict_topk(logits, k, target=None, probs=True):
    """(top_idx int64 [B,k] best first -- column 0 is output.max(1) --, top_prob [B,k] = the softmax over the whole row at
    those columns (None with probs=False), hits int32 [k] when a target is given (else None))."""
    logits = logits.detach()
    k = int(k)
    _check_k(logits.size(1), k)
    if logits.is_cuda:
        from . import ops
        return ops.predict_topk(logits, k, target=target, probs=probs)
    top_idx = _order(logits)[:, :k].contiguous()
    top_prob = torch.softmax(logits.float(), 1).gather(1, top_idx) if probs else None
    hits = _hits_from_rank(target_rank(logits, target), k) if target is not None else None
    return top_idx, top_prob, hits


def predict_candidates(logits, cand):
    """int64 [B]: the MultipleChoice answer of test() -- among the columns cand[b] (int64 [B,M]; entries outside [0, C),
    the -1 padding, are ignored) the one with the best logit, ties to the lower column; -1 if the row has none."""
    logits = logits.detach()
    if logits.is_cuda:
        from . import ops
        return ops.predict_candidates(logits, cand.to(device=logits.device, dtype=torch.int64))
    B, C = logits.shape
    cand = cand.to(torch.int64)
    valid = (cand >= 0) & (cand < C)
    # one spare column C receives every invalid entry, so an entry outside [0, C) can never clear a real candidate's mark
    allowed = torch.zeros(B, C + 1, dtype=torch.bool)
    allowed.scatter_(1, torch.where(valid, cand, torch.full_like(cand, C)), True)
    allowed = allowed[:, :C]
    order = _order(logits)
    hit = allowed.gather(1, order)
    first = hit.to(torch.int8).argmax(1)            # first allowed column in rank order (argmax returns the first maximum)
    pred = order.gather(1, first[:, None])[:, 0]
    return torch.where(hit.any(1), pred, torch.full_like(pred, -1))


def accuracy(hits, batch, topk=(1, 5)):
    """[Acc@k for k in topk] in percent, as the reference's accuracy() (train.py:22-38) returns them; hits[k-1] counts the
    top-k hits among `batch` rows."""
    hits = hits.tolist() if torch.is_tensor(hits) else list(hits)
    return [100.0 * hits[k - 1] / batch for k in topk]
