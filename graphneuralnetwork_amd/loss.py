"""The head of the supervised training loops on the device (csrc/sup_head.hip).

GCN/train_eval.py:45-47 and GAT/train_eval.py:73-75 end every step in
``loss(output[idx_train], labels[idx_train])``, ``accuracy(output[idx_train], labels[idx_train])``
and ``backward()``; GraphSAGE/train_eval.py:116-117 has the same loss with no index.
``supervised_loss`` is the drop-in for the loss line (and, with ``count_correct=True``, for the
count behind the accuracy line in the same pass), ``accuracy`` for the helper:

* the loss and the count of correct predictions in one pass over the selected rows and a
  one-wavefront finish; nothing of size [N, C] or [n, C] is allocated;
* the gradient with respect to the whole logits tensor in one pass that writes every element
  once, through the selection's multiplicity ``count[N]`` (integer atomic adds): no zero fill,
  no sort plus scatter; the incoming gradient stays on the device;
* rows evaluated in double and summed in double in a fixed order, each result rounded once: no
  float atomics, bit-identical from run to run, with duplicates in the index as well.

``SUPERVISED_HEAD_FUSED = False``, CPU tensors, logits with fewer rows than
``SUPERVISED_HEAD_MIN_ROWS`` (``SUPERVISED_HEAD_MIN_ROWS_INDEXED`` with an index: the measured
sizes from which the device head is faster) and every layout the ops decline (logits that are
not fp32 [N, C] with 2 <= C <= 64 and unit stride along C, labels that are not int64 [N], an
index that is not an int64 vector or a bool mask [N]) evaluate torch's own expression, bit for bit
what the loops compute today, exceptions included.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .ops import sup_head_backward, sup_head_count, sup_head_forward

# False: torch's cross entropy and argmax everywhere (tools/sup_head_ab.py times both).
SUPERVISED_HEAD_FUSED = True
# Logits with fewer rows keep torch's path. The device head's cost is the host's (about
# 0.08-0.09 ms per step whatever the shape), torch's grows with the rows; the head alone,
# forward + backward (tools/sup_head_ab.py --head-only --rows, C = 7):
#   no index: 8,192 and 32,768 rows 0.050 ms torch against 0.077 fused; 131,072 rows 0.177
#     against 0.086 and 524,288 rows 0.662 against 0.088, block ranges apart;
#   idx = arange(0, N, 10): 1M rows 0.236 against 0.096, block ranges apart; at 32,768, 131,072
#     and 524,288 rows the medians favour the device head (0.104 / 0.091, 0.110 / 0.092,
#     0.157 / 0.090) but single slow blocks of the host-bound side overlap torch's range, so
#     those shapes stay with torch.
SUPERVISED_HEAD_MIN_ROWS = 131072
SUPERVISED_HEAD_MIN_ROWS_INDEXED = 1_000_000


def _select(output, labels, index):
    return (output, labels) if index is None else (output[index], labels[index])


def _torch_accuracy(y_hat, y):
    """The reference's helper (GCN/train_eval.py:9-17), as it stands there."""
    if len(y_hat.shape) > 1 and y_hat.shape[1] > 1:
        y_hat = torch.argmax(y_hat, axis=1)
    cmp = y_hat.to(dtype=y.dtype) == y
    cmp = cmp.to(dtype=y.dtype)
    return float(cmp.sum()) / len(cmp)


def _fused_ok(output, labels, index) -> bool:
    """Whether the device head takes the call: the switch is on, everything is a device tensor,
    the shapes are the loops' ([N, C] logits, [N] labels, an int64 vector or a bool mask [N] or
    no index), there are enough rows for it to pay and the kernels take the layout."""
    if not (SUPERVISED_HEAD_FUSED and isinstance(output, torch.Tensor)
            and isinstance(labels, torch.Tensor) and output.is_cuda and labels.is_cuda
            and output.dim() == 2 and labels.dim() == 1 and labels.shape[0] == output.shape[0]
            and output.dtype == torch.float32 and labels.dtype == torch.int64
            and not labels.requires_grad
            and output.shape[0] >= (SUPERVISED_HEAD_MIN_ROWS if index is None
                                    else SUPERVISED_HEAD_MIN_ROWS_INDEXED)):
        return False
    if index is not None and not (
            isinstance(index, torch.Tensor) and index.is_cuda and index.dim() == 1
            and (index.dtype == torch.int64
                 or (index.dtype == torch.bool and index.shape[0] == output.shape[0]))):
        return False
    N, C = output.shape
    return bool(_lib.load().gnn_sup_head_supported(C) and output.stride(1) == 1
                and (N <= 1 or output.stride(0) >= C))


class _SupHeadFn(torch.autograd.Function):
    """(loss, n_correct, status) of ``sup_head_forward`` over logits z [N, C]; backward is one
    launch of ``sup_head_backward``. Saved for it: the logits, the labels, the selection's
    multiplicity count[N] (built only when a gradient is wanted, or for a mask) and the device
    scalars 1 / n_valid and status."""

    @staticmethod
    def forward(ctx, z, labels, index, count_correct):
        need = ctx.needs_input_grad[0]
        count = status = None
        if index is not None and (need or index.dtype == torch.bool):
            count, status = sup_head_count(index, z.shape[0])
        by_index = index is not None and index.dtype == torch.int64
        r = sup_head_forward(z, labels, index if by_index else None,
                             None if by_index else count, status, count_correct)
        if r is None:  # _fused_ok said the kernels take these operands
            raise RuntimeError("the supervised head refused operands it reports as covered")
        loss, correct, inv_valid, status = r
        if need:
            ctx.save_for_backward(z, labels, count, inv_valid, status)
        ctx.mark_non_differentiable(status)
        if correct is not None:
            ctx.mark_non_differentiable(correct)
        return loss, correct, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _correct, _status):
        z, labels, count, inv_valid, status = ctx.saved_tensors
        dz = sup_head_backward(z, labels, count, g.to(torch.float32).reshape(1), inv_valid,
                               status)
        if dz is None:
            raise RuntimeError("the supervised head refused operands it reports as covered")
        return dz, None, None, None


def _raise_on_status(status) -> None:
    bits = int(status.item())
    if bits & 1:
        raise IndexError("supervised_loss: an index entry is outside [-N, N)")
    if bits & 2:
        raise ValueError("supervised_loss: a selected label is outside [0, C) and is not "
                         "ignore_index (-100)")


def supervised_loss(output, labels, index=None, *, count_correct=False, check=False):
    """``nn.CrossEntropyLoss()(output[index], labels[index])`` of the reference's loops
    (``index=None``: of ``output`` and ``labels`` themselves), a 0-dim tensor whose gradient
    flows to ``output``; with ``count_correct=True`` the pair (loss, n_correct), n_correct the
    0-dim int64 device tensor ``(argmax(output[index], 1) == labels[index]).sum()`` from the same
    pass. ``index``: an int64 vector (duplicates and negative entries as torch's indexing) or a
    bool mask [N]. On the device path an index entry outside [-N, N) or a selected label outside
    [0, C) (other than -100) is never used as an address: the loss and the whole gradient are
    NaN, and ``check=True`` reads the status word (one host read) and raises IndexError /
    ValueError instead. Elsewhere (see the module's docstring) this is torch's expression."""
    if _fused_ok(output, labels, index):
        loss, correct, status = _SupHeadFn.apply(output, labels, index, bool(count_correct))
        if check:
            _raise_on_status(status)
        return (loss, correct) if count_correct else loss
    sel, lab = _select(output, labels, index)
    loss = F.cross_entropy(sel, lab)
    if count_correct:
        return loss, (torch.argmax(sel, 1) == lab).sum()
    return loss


def accuracy(output, labels, index=None) -> float:
    """The reference's ``accuracy(output[index], labels[index])`` (GCN/train_eval.py:9-17): the
    share of selected rows whose label is the argmax of their logits, a Python float after one
    host read; no gradient, nothing of size [n, C] gathered on the device path."""
    if not _fused_ok(output, labels, index):
        return _torch_accuracy(*_select(output, labels, index))
    with torch.no_grad():
        _, correct, _ = _SupHeadFn.apply(output.detach(), labels, index, True)
        if index is not None and index.dtype == torch.bool:
            correct, n = torch.stack((correct, index.sum())).tolist()
        else:
            correct, n = int(correct), output.shape[0] if index is None else index.shape[0]
    return float(correct) / n
