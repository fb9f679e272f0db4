"""float64 restatement of the fit's optimiser update on the CPU: torch.optim.Adam's arithmetic (amsgrad off, weight decay 0, maximize
off) for a list of tensors, plus the reference's whole-tensor quaternion division (reference fit.py:610-618, quirk Q3).  The yardstick of
tests/test_gpu_adam.py and of the fit-level skip tests; it knows nothing of skipped steps -- a skipped step is a step this reference is
never asked to take, and the caller hands it the learning rates of the run that never drew it."""
import math

import torch


class AdamRef:
    """params: the starting values (any device, any float dtype; copied to float64 CPU tensors).  renorm: positions of the tensors the
    reference divides by the norm of the whole tensor after every step, whether or not they received a gradient in it."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8, renorm=()):
        self.p = [t.detach().to('cpu', torch.float64).clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.step = [0] * len(self.p)
        self.beta1, self.beta2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.renorm = set(renorm)

    def load(self, k, param, exp_avg, exp_avg_sq, step):
        """Tensor k's state from elsewhere (a checkpoint): value, both moments and the number of updates it has taken."""
        self.p[k] = param.detach().to('cpu', torch.float64).clone()
        self.m[k] = exp_avg.detach().to('cpu', torch.float64).clone()
        self.v[k] = exp_avg_sq.detach().to('cpu', torch.float64).clone()
        self.step[k] = int(step)

    def update(self, grads, lrs):
        """One step.  grads[k]: tensor k's gradient, or None (it takes no Adam step and its step count stays); lrs[k]: its learning rate
        in this step, the schedule already applied."""
        assert len(grads) == len(lrs) == len(self.p)
        b1, b2 = self.beta1, self.beta2
        for k, (g, lr) in enumerate(zip(grads, lrs)):
            if g is not None:
                g = g.detach().to('cpu', torch.float64)
                assert g.shape == self.p[k].shape
                self.step[k] += 1
                n = self.step[k]
                self.m[k] = b1 * self.m[k] + (1.0 - b1) * g
                self.v[k] = b2 * self.v[k] + (1.0 - b2) * g * g
                denom = self.v[k].sqrt() / math.sqrt(1.0 - b2 ** n) + self.eps
                self.p[k] = self.p[k] - (float(lr) / (1.0 - b1 ** n)) * (self.m[k] / denom)
            if k in self.renorm:
                self.p[k] = self.p[k] / self.p[k].square().sum().sqrt()
