"""``BVRNN.forward`` as a node of a torch.autograd graph: the values come from ``BVRNN.forward`` (``bvc_bvrnn_forward``), the gradients
from ``BVRNN.backward`` (``bvc_bvrnn_backward``), which runs its own forward with the same random numbers.  Thin by design: no state
of its own and no optimiser: ``bvrnn.optimizer()`` (``bvcodec.optim``) takes the ``.grad`` tensors, updates the live model in place and,
given ``params=``, writes the new values back into the leaf tensors, so that they keep holding the model's values."""
import torch

from .coder import _draw_randomness


class _ForwardTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bvrnn, y, p_use_gen, greedy, varBitrate, r, noise, names, *params):
        ctx.bvrnn, ctx.call, ctx.names = bvrnn, (p_use_gen, greedy, varBitrate, r, noise), names
        ctx.y = y.detach()
        ctx.param_devices = [p.device for p in params]
        dec, kld = bvrnn.forward(ctx.y, p_use_gen, greedy, varBitrate, r=r, noise=noise)
        return dec, kld

    @staticmethod
    def backward(ctx, grad_dec, grad_kld):
        p_use_gen, greedy, varBitrate, r, noise = ctx.call
        B, T, X = ctx.y.shape
        grad_dec = torch.zeros(B, T, X) if grad_dec is None else grad_dec
        g = ctx.bvrnn.backward(ctx.y, p_use_gen, greedy, varBitrate, grad_dec, 0.0 if grad_kld is None else float(grad_kld), r=r, noise=noise,
                               grad_input=ctx.needs_input_grad[1])
        gp = [g[n].to(d) if need else None for n, d, need in zip(ctx.names, ctx.param_devices, ctx.needs_input_grad[8:])]
        return (None, g["y"].to(ctx.y.device) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None, *gp)


def forward_train(bvrnn, y, p_use_gen, greedy, varBitrate, params, *, r=None, noise=None):
    """(all_dec_mean, kld) of ``bvrnn.forward(y, p_use_gen, greedy, varBitrate)``, attached to the graph: a loss built from them fills,
    on ``.backward()``, ``.grad`` of ``y`` (if it requires grad) and of the tensors in ``params`` that require grad.  ``params``: a dict
    keyed like ``bvrnn.grad_parameters()``.  The values are the MODEL's: ``params`` must hold the model's values, nothing checks it.
    Randomness as in ``forward``; it is drawn once, here, and shared by the forward and the backward call."""
    names = tuple(params)
    known = {n for n, _, _ in bvrnn.grad_layout()[0]}
    unknown = [n for n in names if n not in known]
    if unknown:
        raise ValueError(f"forward_train: {unknown} are no trainable tensors of BVRNN.forward")
    if not torch.is_tensor(y) or y.dim() != 3:
        raise ValueError("forward_train: y must be (B, T, num_mels)")
    B, T, _ = y.shape
    r, noise = _draw_randomness(B, T, bvrnn.z_dim, greedy, r, noise)
    return _ForwardTrain.apply(bvrnn, y, p_use_gen, greedy, varBitrate, r, noise, names, *[params[n] for n in names])
