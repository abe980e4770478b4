"""Dynamic loss balancing of the EBEN train step (``vibravox/lightning_modules/eben.py:105-108, 222-240``)."""
import torch

from . import ops
from ._lib import check, load, ptr, stream


class LossBalancer:
    """Owns the EMA of the gradient norms at ``generator.last_conv.weight`` and forms what a step needs from it: the loss weights,
    the backprop loss and the seed of the generator backward.  Two routes over the one state, free to alternate from call to call:
    one-element torch kernels (``lambdas``: the reference's formula, op for op) or two launches (``eben_balance`` +
    ``eben_weighted_sum``: the same operations and roundings, tests/test_gpu_ops.py) instead of ~35 of those."""

    def __init__(self):
        self.old = None   # the state, assignable: one 0-dim tensor per loss (the reference's ``atomic_norms_old``), None before the first call
        self.last_norms = self.last_lambdas = None
        self._buf = self._views = None   # the launches' state, one device vector, and its elements: current while ``old is _views``
        self._ones = None                # unit weights of a step without balancing

    def lambdas(self, norms, mode, beta) -> list:
        """eben.py:229-237: the state is initialised with the first norms and -- quirk kept -- the EMA update is applied on that
        same call; rank-local like the reference's."""
        if self.old is None or mode == "simple":
            self.old = norms
        if mode == "ema":
            self.old = [beta * old + (1 - beta) * new for old, new in zip(self.old, norms)]
        self.last_norms, self.last_lambdas = norms, [torch.clamp(1 / (norm + 1e-4), min=0.0, max=1e4) for norm in self.old]
        return self.last_lambdas

    def _launch(self, norms, losses, mode, beta):
        """``lambdas`` and the backprop loss in one launch: (lambdas, backprop loss, the lambdas as one device vector)."""
        n, dev = len(norms), norms[0].device
        init = self.old is None or mode == "simple"
        if self.old is None or self.old is not self._views or self._buf.numel() != n or self._buf.device != dev:
            # first call, or the state was written since (the torch route, a restore, the user): the vector follows it
            given = self.old is not None and len(self.old) == n
            self._buf = (torch.stack([torch.as_tensor(t, dtype=torch.float32).to(dev).reshape(()) for t in self.old]) if given
                         else torch.zeros(n, dtype=torch.float32, device=dev))
            self._views = [self._buf[i] for i in range(n)]
        out = torch.empty(n + 1, dtype=torch.float32, device=dev)   # fresh per step: last_lambdas of earlier steps stay what they were
        check(load().eben_balance(ops._ptr_array([t.contiguous() for t in norms]), ops._ptr_array([t.to(torch.float32).contiguous() for t in losses]),
                                  n, ptr(self._buf), int(init), int(mode == "ema"), float(beta), float(1 - beta), ptr(out), ptr(out[n:]),
                                  stream()), "balance")
        self.old = self._views   # updated in place
        self.last_norms, self.last_lambdas = norms, [out[i] for i in range(n)]
        return self.last_lambdas, out[n], out[:n]

    def balance(self, norms, losses, seeds=None, *, mode, beta=0.9, fused=True):
        """One step's balancing: ``norms[i]`` = ||d losses[i] / d last_conv.weight|| (not read when ``mode`` is None), ``seeds[i]`` =
        d losses[i] / d bands or None.  Returns (lambdas, sum_i losses[i] lambdas[i], sum_i seeds[i] lambdas[i] or None).  ``mode``
        None is eben.py:107-108: the plain sum, every lambda 1, nothing recorded.  ``fused`` asks for the launches; they take seeds
        on the device, at most 8 of them (BAL_MAX, csrc/direct.hip)."""
        n = len(losses)
        if fused and seeds is not None and n <= 8 and seeds[0].is_cuda:
            if mode is not None:
                lambdas, backprop_loss, weights = self._launch(norms, losses, mode, beta)
            else:
                if self._ones is None or self._ones.numel() != n or self._ones.device != seeds[0].device:
                    self._ones = torch.ones(n, dtype=torch.float32, device=seeds[0].device)
                lambdas, backprop_loss, weights = [1.0] * n, sum(losses), self._ones
            return lambdas, backprop_loss, ops.weighted_sum(seeds, weights)
        lambdas = [1.0] * n if mode is None else self.lambdas(norms, mode, beta)
        backprop_loss, seed = sum(loss * lam for loss, lam in zip(losses, lambdas)), None
        for s, lam in zip(seeds or (), lambdas):
            seed = s * lam if seed is None else seed + s * lam
        return lambdas, backprop_loss, seed
