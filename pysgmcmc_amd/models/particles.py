"""The MLP-BNN cost on FLAT particles, for particle methods (``SVGDSampler``).

A particle is one flat parameter vector in the order of a device-trace row -- ``W1`` (``[in][out]``), ``b1``, ..., ``WL``,
``bL``, ``log_var`` -- so the ``(n, P)`` particle matrix of a sampler is at once what ``posterior_predictive``,
``heldout_score`` and ``predictive_gradients`` read. ``BNNParticleCost`` is the cost of ONE such particle in torch ops (any
device, differentiable) and, on a GPU, the launch of kernel K15 (``kernels.bnn_particles_cost_grad``), which gives the costs
and the parameter gradients of all particles of the matrix in one launch without autograd.
"""
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params, mlp_forward

__all__ = ("BNNParticleCost", "bnn_particles")


def bnn_particles(n, n_inputs, hidden=(50, 50, 50), seed=None, dtype=torch.float64, device="cpu"):
    """``n`` flat particles of the net ``[n_inputs, *hidden, 1]``: particle ``i`` is ``init_mlp_params(seed + i)`` flattened
    in its own order (``seed=None``: unseeded draws)."""
    out = []
    for i in range(int(n)):
        params = init_mlp_params(n_inputs, hidden=hidden, seed=None if seed is None else int(seed) + i, dtype=dtype,
                                 device=device)
        out.append(torch.cat([p.reshape(-1) for p in params]))
    return out


class BNNParticleCost(object):
    """Negative log likelihood of the MLP BNN ``layer_sizes`` (``[inputs, hidden ..., 1]``) at one flat particle, as the
    ``cost_fun`` of a particle sampler. ``x_placeholder`` / ``y_placeholder`` are fed by the batch generator; ``batch_size``
    and ``n_examples`` are the configured constants of the cost, as for ``BNNCost``.

    ``use_hip_kernel`` (attribute, default True): a sampler that knows :meth:`particles_cost_and_grad` takes the costs and
    gradients of all its particles from kernel K15 when the call fits it; ``False`` keeps the sampler on torch autograd."""

    __name__ = "negative_log_likelihood"

    def __init__(self, layer_sizes, x_placeholder, y_placeholder, batch_size, n_examples, wdecay=1.0, prior_mean=1e-6,
                 prior_var=0.01):
        self.layer_sizes = [int(v) for v in layer_sizes]
        assert len(self.layer_sizes) >= 2 and self.layer_sizes[-1] == 1, "layer_sizes: [inputs, hidden ..., 1]"
        self.x_placeholder = x_placeholder
        self.y_placeholder = y_placeholder
        self.batch_size = int(batch_size)
        self.n_examples = int(n_examples)
        self.wdecay = float(wdecay)
        self.prior_mean = float(prior_mean)
        self.prior_var = float(prior_var)
        s = self.layer_sizes
        self.n_params = sum(s[l] * s[l + 1] + s[l + 1] for l in range(len(s) - 1)) + 1
        self.use_hip_kernel = True
        self.last_mse = None
        self._const = {}

    def views(self, particle):
        """The parameters ``[W1, b1, ..., WL, bL, log_var (1, 1)]`` as views into the flat ``particle``."""
        flat = particle.reshape(-1)
        assert flat.numel() == self.n_params, "a particle of this net has %d elements" % self.n_params
        s, at, params = self.layer_sizes, 0, []
        for l in range(len(s) - 1):
            params.append(flat[at:at + s[l] * s[l + 1]].reshape(s[l], s[l + 1]))
            at += s[l] * s[l + 1]
            params.append(flat[at:at + s[l + 1]])
            at += s[l + 1]
        params.append(flat[at:at + 1].reshape(1, 1))
        return params

    def _constants(self, dtype, device):
        """The tensors ``BNNCost.negative_log_likelihood`` derives from the prior's constants on every call -- ``log(mean)``,
        the two ``safe_divide`` denominators, ``0.5 * log(var)`` -- made by the same ops, once per dtype and device: the
        call then copies nothing from the host and can be recorded into a hipGraph."""
        key = (dtype, str(device))
        c = self._const.get(key)
        if c is None:
            tiny = 1e-16                                                       # safe_divide: y + (2 sign(y) tiny + tiny)
            mean_t = torch.tensor(self.prior_mean, dtype=dtype, device=device)
            var_t = torch.tensor(self.prior_var, dtype=dtype, device=device)
            two_var = 2.0 * var_t
            count = torch.tensor(float(self.n_params), dtype=dtype, device=device)
            c = self._const[key] = (torch.log(mean_t), two_var + (2.0 * torch.sign(two_var) * tiny + tiny),
                                    0.5 * torch.log(var_t), count + (2.0 * torch.sign(count) * tiny + tiny))
        return c

    def __call__(self, particle, *_):
        """The statements of ``BNNCost.negative_log_likelihood`` (with ``log_variance_prior_log_like`` and
        ``weight_prior_log_like`` written out) on the views of one flat particle: the same values, bit for bit."""
        X, Y = self.x_placeholder.value, self.y_placeholder.value
        params = self.views(particle)
        ln_mean, lvp_den, half_ln_var, wp_den = self._constants(particle.dtype, particle.device)
        out = mlp_forward(params, X)
        f_mean = out[:, 0].reshape(-1, 1)
        f_log_var = out[:, 1].reshape(-1, 1)
        f_var_inv = 1.0 / (torch.exp(f_log_var) + 1e-16)
        mse = torch.square(Y.reshape(-1, 1) - f_mean)
        log_like = torch.sum(torch.sum(-mse * (0.5 * f_var_inv) - 0.5 * f_log_var, dim=1))
        log_like = log_like / self.batch_size
        lvp = torch.mean(torch.sum(-torch.square(f_log_var - ln_mean) / lvp_den - half_ln_var, dim=1))
        log_like = log_like + lvp / self.n_examples
        wp = torch.zeros((), dtype=particle.dtype, device=particle.device)
        for p in params:
            wp = wp + torch.sum(-self.wdecay * 0.5 * torch.square(p))
        log_like = log_like + (wp / wp_den) / self.n_examples
        self.last_mse = torch.mean(mse).detach()
        return -log_like

    def fits(self, dtype, batch=None):
        """Kernel K15 takes this net in ``dtype`` at ``batch`` rows (default: the rows fed last, else ``batch_size``)."""
        if batch is None:
            X = self.x_placeholder.value
            batch = int(X.shape[0]) if torch.is_tensor(X) and X.dim() == 2 else self.batch_size
        if dtype not in (torch.float32, torch.float64) or self.layer_sizes[-1] != 1 or len(self.layer_sizes) - 1 > 8:
            return False
        return kernels.bnn_particles_lds_bytes(self.layer_sizes, batch, dtype) > 0

    def particles_cost_and_grad(self, theta_row, grad_row, n, pitch, costs):
        """Costs of the ``n`` particles at ``theta_row[p * pitch:][:n_params]`` into ``costs`` and their full gradients
        (weight prior included) into ``grad_row`` at the same pitch, at the placeholders' current values: ONE launch of
        K15. Returns ``costs``."""
        X, Y = self.x_placeholder.value, self.y_placeholder.value
        return kernels.bnn_particles_cost_grad(theta_row, n, pitch, self.layer_sizes, X, Y, grad_row, pitch, costs,
                                               self.batch_size, self.n_examples, self.wdecay, self.prior_mean,
                                               self.prior_var, add_prior=True)
