"""Losses with fused analytic backward (semilearn/core/criterions/cross_entropy.py:11-31, consistency.py:13-45).

Each call returns (loss, dlogits [B,C]); dlogits already carries the loss weight (``grad_scale``) so the backbone backward can start from
it directly.  ``dl_out`` (a [B,C] row block -- or column block, rows dense -- of a larger buffer): the gradient is written there -- the step's
losses fill ONE upstream-gradient buffer instead of being torch.cat'ed.  ``logits`` may be such a block too (it is read in place).

The hard-label mean path the five algorithms use (``CELoss(reduction='mean')``, ``ConsistencyLoss(name='ce')`` with integer targets) is the one
``ops.masked_ce`` launch it always was.  Everything else the reference's two functions accept runs on the kernels of csrc/criterions.hip:
soft targets (chosen, as in the reference, by ``logits.shape == targets.shape``), ``reduction='none' | 'sum'``, ``name='mse' | 'l1'``.

reduction='none': ``loss`` is the [B] vector of per-row losses (times the masks).  There is no reduced scalar to differentiate, so with
``want_grad`` the caller hands the per-row upstream weights d(total)/d(loss_b) in through ``mask`` (that is what re-weighting a per-row loss
before reducing it amounts to): dlogits[b] = grad_scale * mask[b] * mask2[b] * d loss_b / d logits[b].  Without a mask the weights are 1
(the gradient of the plain sum)."""
import torch

from .. import ops

_REDUCTIONS = {"none": ops.REDUCE_NONE, "mean": ops.REDUCE_MEAN, "sum": ops.REDUCE_SUM}
_ONE_WORKGROUP_ROWS = 64          # up to here the launch finishes the scalar itself and needs no per-row buffer (include/srhip.h)


def _dense_rows(t):
    return t if t.dim() == 2 and t.stride(1) == 1 else t.contiguous()


def _is_soft(logits, targets):
    return logits.shape == targets.shape          # cross_entropy.py:21


def _launch(fn, logits, targets, mask, mask2, reduction, grad_scale, want_grad, dl_out):
    if reduction not in _REDUCTIONS:
        raise ValueError("reduction must be one of 'none', 'mean', 'sum', not %r" % (reduction,))
    B, C = logits.shape
    dev = logits.device
    none = reduction == "none"
    loss = None if none else torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev) if none or B > _ONE_WORKGROUP_ROWS else None
    dl = (dl_out if dl_out is not None else torch.empty(B, C, dtype=torch.float32, device=dev)) if want_grad else None
    fn(_dense_rows(logits), targets, mask, mask2, grad_scale, _REDUCTIONS[reduction], rows, loss, dl, B, C)
    return (rows if none else loss[0]), dl


def _soft_targets(targets):
    return _dense_rows(targets if targets.dtype == torch.float32 else targets.to(torch.float32))


class CELoss:
    def __call__(self, logits, targets, reduction="mean", grad_scale=1.0, want_grad=True, dl_out=None, mask=None):
        """ce_loss.  NOTE the default reduction stays 'mean' (the engine's callers rely on it); the reference's default is 'none'.
        Integer targets [B] or soft targets [B, C] (fp32, not normalised), chosen by shape as the reference does.  With soft targets the
        reference returns the MEAN for every reduction other than 'none' (cross_entropy.py:25-28), 'sum' included; so does this.
        ``mask``: optional per-row weights (see the module docstring for reduction='none')."""
        if _is_soft(logits, targets):
            if reduction not in _REDUCTIONS:
                raise ValueError("reduction must be one of 'none', 'mean', 'sum', not %r" % (reduction,))
            return _launch(ops.ce_soft, logits, _soft_targets(targets), mask, None, "none" if reduction == "none" else "mean", grad_scale,
                           want_grad, dl_out)
        if reduction == "mean" and mask is None:
            B, C = logits.shape
            loss = torch.empty(1, dtype=torch.float32, device=logits.device)
            dl = (dl_out if dl_out is not None else torch.empty_like(logits)) if want_grad else None
            ops.masked_ce(logits.contiguous(), targets.contiguous(), None, None, grad_scale, loss, dl, B, C)
            return loss[0], dl
        return _launch(ops.ce_hard, logits, targets.contiguous(), mask, None, reduction, grad_scale, want_grad, dl_out)


class ConsistencyLoss:
    def __call__(self, logits, targets, name="ce", mask=None, mask2=None, grad_scale=1.0, want_grad=True, dl_out=None, reduction="mean"):
        """consistency_loss: 'ce' (integer or soft targets), 'mse' (softmax(logits) against target probabilities, mean over classes), 'l1'
        (logits against targets, mean over classes), each row times mask * mask2, then the mean over ALL rows (consistency.py:39-45).
        ``reduction`` (not in the reference, which always takes the mean) also offers 'none' / 'sum' of the masked per-row losses."""
        if name not in ("ce", "mse", "l1"):
            raise ValueError("name must be one of 'ce', 'mse', 'l1', not %r" % (name,))
        if name == "ce" and not _is_soft(logits, targets):
            if reduction == "mean":
                B, C = logits.shape
                loss = torch.empty(1, dtype=torch.float32, device=logits.device)
                dl = (dl_out if dl_out is not None else torch.empty_like(logits)) if want_grad else None
                ops.masked_ce(logits.contiguous(), targets.contiguous(), mask, mask2, grad_scale, loss, dl, B, C)
                return loss[0], dl
            return _launch(ops.ce_hard, logits, targets.contiguous(), mask, mask2, reduction, grad_scale, want_grad, dl_out)
        if not _is_soft(logits, targets):
            raise ValueError("name=%r needs targets of the logits' shape %s, got %s" % (name, tuple(logits.shape), tuple(targets.shape)))
        fn = {"ce": ops.ce_soft, "mse": ops.consistency_mse, "l1": ops.consistency_l1}[name]
        return _launch(fn, logits, _soft_targets(targets), mask, mask2, reduction, grad_scale, want_grad, dl_out)
