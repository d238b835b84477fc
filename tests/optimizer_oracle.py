"""Oracle of the optimiser step (``bvc_optimizer_step``, include/bvcodec.h): the AdamW update restated in numpy at float64 and at
float32, operation for operation as the header lists them, with the 2-norm clip of torch.nn.utils.clip_grad_norm_ in front (test
infrastructure).  tests/test_optimizer_cpu.py holds the float64 form to torch.optim.AdamW; tests/test_gpu_optimizer.py holds the
library to the float64 form at the project's bar, with the float32 form as the yardstick of float32's own error.

Also here, because both test files need them: the synthetic gradients of the arithmetic test and the fixed batch, learning rate and
loss of the "it learns" case."""
import numpy as np
import torch

import backward_oracle as bo
import bvrnn_draws as bd

CLIP_EPS = 1e-6


class AdamWOracle:
    """State of one optimiser over a dict of arrays: ``p`` (updated in place by ``step``), ``m``, ``v`` of ``dtype`` and the step
    count ``t``."""

    def __init__(self, params, dtype):
        self.dtype = np.dtype(dtype)
        self.p = {k: np.array(torch.as_tensor(v).detach().cpu().numpy(), dtype=self.dtype) for k, v in params.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.t = 0

    def step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
        """One step; returns the 2-norm of all gradients before clipping (float64).  The scalars are computed in double and rounded to
        ``dtype`` once, as the host code does; every elementwise operation is one numpy call, so each is rounded on its own."""
        f = self.dtype.type
        g = {k: np.array(torch.as_tensor(grads[k]).detach().cpu().numpy(), dtype=self.dtype) for k in self.p}
        norm = float(np.sqrt(sum(float(np.sum(np.square(v.astype(np.float64)))) for v in g.values())))
        c = min(1.0, max_grad_norm / (norm + CLIP_EPS)) if max_grad_norm > 0 else 1.0
        self.t += 1
        b1, b2 = betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        decay, one_b1, one_b2, step_size, bc2_sqrt = f(1.0 - lr * weight_decay), f(1.0 - b1), f(1.0 - b2), f(lr / bc1), f(np.sqrt(bc2))
        for k in self.p:
            gk = g[k] * f(c)
            p = self.p[k] * decay
            self.m[k] = f(b1) * self.m[k] + one_b1 * gk
            self.v[k] = f(b2) * self.v[k] + (one_b2 * gk) * gk
            self.p[k] = p - step_size * (self.m[k] / (np.sqrt(self.v[k]) / bc2_sqrt + f(eps)))
            assert self.p[k].dtype == self.dtype and self.m[k].dtype == self.dtype and self.v[k].dtype == self.dtype
        return norm


def torch_adamw(params, grads_seq, lr, betas, eps, weight_decay, max_grad_norm):
    """torch.optim.AdamW (+ clip_grad_norm_) on CPU float64 leaves over the same sequence of gradients: (params, exp_avg, exp_avg_sq
    as dicts of arrays, [norms])."""
    leaves = {k: torch.as_tensor(v).detach().double().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False)
    norms = []
    for grads in grads_seq:
        for k, p in leaves.items():
            p.grad = torch.as_tensor(grads[k]).detach().double().clone()
        total = torch.sqrt(sum(p.grad.pow(2).sum() for p in leaves.values()))
        if max_grad_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_grad_norm)
        norms.append(float(total))
        opt.step()
    st = opt.state_dict()["state"]
    names = list(leaves)
    return ({k: leaves[k].detach().numpy() for k in names}, {k: st[i]["exp_avg"].numpy() for i, k in enumerate(names)},
            {k: st[i]["exp_avg_sq"].numpy() for i, k in enumerate(names)}, norms)


# ---------------------------------------------------------------------------------------------- synthetic gradients
ZERO_TENSOR, ONE_ELEMENT_TENSOR = "phi_z.2.bias", "enc.0.weight"


def synthetic_grads(shapes, seed):
    """{name: float32 tensor}: randn times 10^u, u uniform in [-6, 2], every non-zero magnitude raised to at least 1e-12;
    ZERO_TENSOR all zero, ONE_ELEMENT_TENSOR zero but for one element."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in shapes.items():
        g = rng.standard_normal(shape) * 10.0 ** rng.uniform(-6.0, 2.0, shape)
        g = np.where((g != 0) & (np.abs(g) < 1e-12), np.copysign(1e-12, g), g).astype(np.float32)
        if name == ZERO_TENSOR:
            g[...] = 0.0
        if name == ONE_ELEMENT_TENSOR:
            keep = g.reshape(-1)[g.size // 3]
            g[...] = 0.0
            g.reshape(-1)[g.size // 3] = keep if keep != 0 else np.float32(0.25)
        out[name] = torch.from_numpy(g)
    return out


# ---------------------------------------------------------------------------------------------- it learns
# One fixed batch at h_dim 64, greedy, teacher-forced; loss = mean squared error + 0.01 kld; 30 AdamW steps without decay or clipping.
# The float64 loop (backward_oracle + AdamWOracle) falls from 18.62 to 2.677, a factor of 6.96 (the batch is noise of variance 2.56:
# its mean is what there is to learn); at lr 0.01 it is 7.08, at 0.03 6.29 and no longer monotone.  tests/test_optimizer_cpu.py
# asserts LEARN_FALL, chosen below that after seeing it; the GPU test asserts half of it in log terms, sqrt(LEARN_FALL).
LEARN_H, LEARN_B, LEARN_T, LEARN_STEPS, LEARN_LR, LEARN_KLD = 64, 4, 8, 30, 0.003, 0.01
LEARN_FALL = 5.0


def learn_batch():
    y, bits = bd.inputs(LEARN_B, LEARN_T, seed=31)
    return y, bits, torch.zeros(LEARN_T)


def learn_loss_and_grads(dec, kld, y):
    """(loss, grad_dec, grad_kld) of mean((dec - y)^2) + LEARN_KLD kld, for tensors of any dtype and device."""
    diff = dec - y.to(dec)
    return float((diff * diff).mean() + LEARN_KLD * kld), 2.0 * diff / diff.numel(), LEARN_KLD


def learn_curve_oracle():
    """The float64 loop: [loss before step 0, ..., loss before step LEARN_STEPS]."""
    sd = bd.state_dict(LEARN_H, "default")
    y, bits, r = learn_batch()
    names = bo.trainable(sd)
    opt = AdamWOracle({k: sd[k] for k in names}, np.float64)
    fixed = {k: v.double() for k, v in sd.items() if k not in names and k != "log_sigma"}
    curve = []
    for it in range(LEARN_STEPS + 1):
        cur = dict(fixed, **{k: torch.from_numpy(v) for k, v in opt.p.items()})
        with torch.no_grad():
            out = bo.forward(cur, y.double(), bits, 0.0, True, r, None)
        loss, gdec, gkld = learn_loss_and_grads(out["dec"], out["kld"], y)
        curve.append(loss)
        if it == LEARN_STEPS:
            break
        g, _ = bo.grads(cur, y, bits, 0.0, True, r, None, gdec, gkld, torch.float64)
        opt.step({k: g[k] for k in names}, LEARN_LR)
    return curve
