"""The plain reference of ctc_loss_from_logits: torch.nn.functional.ctc_loss on the CPU over a log_softmax of the logits
as they are stored, in float64 (or, as the yardstick of an fp32 implementation, in float32), with the package's
conventions on top: batch-major logits, +inf and a zero gradient for an utterance without a path, its reductions."""
import torch
import torch.nn.functional as F


def ctc_reference(logits, labels, frames_lengths, labels_lengths, blank=0, reduction="none", grad_output=None,
                  dtype=torch.float64):
    """(loss, d loss / d logits) in ``dtype`` on the CPU; ``grad_output``: the upstream gradient of the loss (ones)."""
    z = logits.detach().cpu().to(dtype).requires_grad_(True)
    lp = torch.log_softmax(z, -1).transpose(0, 1)
    args = (labels.cpu().long(), frames_lengths.cpu().long(), labels_lengths.cpu().long())
    no_path = torch.isinf(F.ctc_loss(lp.detach(), *args, blank=blank, reduction="none"))
    finite = F.ctc_loss(lp, *args, blank=blank, reduction="none", zero_infinity=True)      # (and its gradient zero)
    costs = torch.where(no_path, torch.full_like(finite, float("inf")), finite)
    loss = costs if reduction == "none" else costs.sum() if reduction == "sum" else costs.mean()
    go = torch.ones_like(loss) if grad_output is None else grad_output.detach().cpu().to(dtype)
    upstream = go.expand_as(costs) / (costs.numel() if reduction == "mean" else 1)
    grad, = torch.autograd.grad(finite, z, upstream.contiguous())
    return loss.detach(), grad
