"""Many independent chains of one small BNN (all SGHMC, all SGLD or all relativistic SGHMC) advanced together by the
fused-step kernel.

The reference runs chains one after the other, each in a fresh TF graph
(``pysgmcmc/diagnostics/sample_chains.py:369-382``). ``sgmcmc_bnn_fused_sghmc_steps_*`` runs one
workgroup per chain, so up to one chain per CU (256 on MI355X) advance in the time of one: the chains'
states are re-homed back to back in ONE allocation (chain ``c`` at ``+ c * chain_stride`` in every state
row) and every launch covers ``n_steps`` steps of all of them. Each chain stays a normal sampler
(:class:`~pysgmcmc_amd.samplers.sghmc.SGHMCSampler`, ``SGLDSampler`` or ``RelativisticSGHMCSampler``: ``next()``,
``minv``, ``state_dict`` ... keep working on the shared memory); chain ``c`` uses Philox seed ``seed_0 + c`` and its own
window stream. The stepsize may follow a schedule as long as every chain's schedule yields the same values: the launch
then reads ONE table of per-step scalars that all chains share.
"""
import numpy as np
import torch

from pysgmcmc_amd.samplers.sghmc import SGHMCSampler

__all__ = ("FusedBNNChains",)


class FusedBNNChains(object):
    """Group of SGHMC (or of SGLD, or of relativistic SGHMC) chains that fit the fused small-model kernel.

    Parameters
    ----------
    samplers : list of SGHMCSampler (or list of SGLDSampler, or list of RelativisticSGHMCSampler)
        Chains over the SAME dataset and network shape, built with ``seed = s, s + 1, s + 2, ...``, equal
        hyper-parameters and ``fused_bnn_available()``; all at the same iteration.
    """

    def __init__(self, samplers):
        samplers = list(samplers)
        assert samplers, "FusedBNNChains needs at least one chain"
        first = samplers[0]
        for c, s in enumerate(samplers):
            if type(s) is not type(first) or not hasattr(s, "_fused_bnn_launch") or not s.fused_bnn_available():
                raise ValueError("chain %d does not fit the fused small-model kernel" % c)
            same = (s._bnn_layer_sizes() == first._bnn_layer_sizes()
                    and s._torch_dtype == first._torch_dtype and s.device == first.device
                    and s.batch_generator.x_dev.data_ptr() == first.batch_generator.x_dev.data_ptr()
                    and s.batch_generator.y_dev.data_ptr() == first.batch_generator.y_dev.data_ptr()
                    and s.batch_generator.batch_size == first.batch_generator.batch_size
                    and s.n_iterations == first.n_iterations
                    # hyper-parameters: whichever of them the sampler class has
                    and all(getattr(s, k, None) == getattr(first, k, None)
                            for k in ("burn_in_steps", "scale_grad", "mdecay", "A", "mass", "speed_of_light", "D", "Bhat"))
                    and all(getattr(s.cost_fun, k) == getattr(first.cost_fun, k)
                            for k in ("batch_size", "n_examples", "wdecay", "prior_mean", "prior_var")))
            if not same:
                raise ValueError("chain %d differs from chain 0 in data, network or hyper-parameters" % c)
            if s._philox_seed != ((first._philox_seed + c) & 0xFFFFFFFFFFFFFFFF):
                raise ValueError("chain seeds must be consecutive (seed_0 + chain index); chain %d is not" % c)
        self.samplers = samplers
        self.n_chains = len(samplers)
        self.chain_stride = int(first.arena.storage.numel())
        # one allocation, the chains' arenas back to back
        self.storage = torch.empty(self.n_chains * self.chain_stride, dtype=first._torch_dtype, device=first.device)
        for c, s in enumerate(samplers):
            s._rebind_arena(self.storage[c * self.chain_stride:(c + 1) * self.chain_stride])

    @property
    def n_iterations(self):
        return self.samplers[0].n_iterations

    def theta(self):
        """``[n_chains, n_params]`` view of every chain's current parameters (no copy)."""
        a = self.samplers[0].arena
        return torch.as_strided(self.storage, (self.n_chains, a.n), (self.chain_stride, 1),
                                a.row("theta").storage_offset() - self.storage.storage_offset())

    def steps(self, n_steps, trace=None, keep_every=1, trace_row=0, trace_phase=0):
        """Advance every chain by ``n_steps`` steps in one launch; returns the ``[n_chains, n_steps]`` costs
        (cost at the parameters before each step). The stepsize may move inside the chunk when every chain's schedule
        yields the same ``n_steps`` values (one shared table of per-step scalars); chains whose schedules disagree raise.

        ``trace``: a contiguous ``(n_chains, capacity, n_params)`` device tensor of the chains' dtype. The launch keeps
        every chain's theta after each step ``t`` (0-based) with ``(trace_phase + t + 1) % keep_every == 0`` in its slab,
        from row ``trace_row`` on (``kernels.bnn_fused_steps``); the chains and the costs are those of the untraced call."""
        n_steps = int(n_steps)
        first = self.samplers[0]
        traced = {} if trace is None else dict(trace=trace, trace_every=keep_every, trace_row=trace_row,
                                               trace_phase=trace_phase)
        if trace is not None and not (torch.is_tensor(trace) and trace.dim() == 3):
            raise TypeError("FusedBNNChains.steps: trace must be an (n_chains, capacity, n_params) device tensor")
        if any(s.n_iterations != first.n_iterations for s in self.samplers):
            raise ValueError("FusedBNNChains.steps: the chains are no longer at the same iteration "
                             "(a member was stepped on its own)")
        eps = [s._fused_stepsizes(n_steps) for s in self.samplers]
        if any(e != eps[0] for e in eps):
            raise ValueError("FusedBNNChains.steps needs one stepsize sequence for all chains over the chunk")
        starts = np.stack([s._fused_window_starts(n_steps) for s in self.samplers])
        starts = torch.as_tensor(starts).to(first.device).reshape(-1)
        costs = torch.empty(self.n_chains * n_steps, dtype=first._torch_dtype, device=first.device)
        # chain 0's rows are the bases; the kernel adds chain * chain_stride. Hand it views that span all chains.
        a = first.arena
        span = (self.n_chains - 1) * self.chain_stride + a.n
        bases = [torch.as_strided(self.storage, (span,), (1,), a.row(k).storage_offset() - self.storage.storage_offset())
                 for k in first._FUSED_ROWS]
        first._fused_bnn_launch(starts, costs, eps[0][0], n_steps, n_chains=self.n_chains, chain_stride=self.chain_stride,
                                bases=bases, scalars_steps=first._fused_scalars_table(eps[0]), **traced)
        costs = costs.view(self.n_chains, n_steps)
        for c, s in enumerate(self.samplers):
            s._fused_steps_done(n_steps, costs[c, -1])
        return costs

    def collect(self, n_samples, every=100):
        """``n_samples`` thinned snapshots of all chains: a ``[n_chains, n_samples, n_params]`` device tensor, written
        by ONE launch of ``n_samples * every`` steps that keeps every ``every``-th theta itself (no launch boundary and no
        copy per snapshot), ready for :meth:`diagnose` (R-hat and ESS of every parameter over ALL the chains),
        :meth:`predict` and :meth:`score`. ``diagnostics.device_trace.effective_n_all`` takes up to 64 of the chains (``t[:64]``);
        ``diagnostics.sampler_diagnostics.gelman_rubin_from_chains`` works on a float64 copy, ``effective_n`` on one parameter."""
        n_samples, every = int(n_samples), int(every)
        a = self.samplers[0].arena
        out = torch.empty(self.n_chains, n_samples, a.n, dtype=self.storage.dtype, device=self.storage.device)
        if n_samples > 0:
            self.steps(n_samples * every, trace=out, keep_every=every)
        return out

    def diagnose(self, trace, details=False, rank_normalized=False):
        """R-hat and effective sample size of every parameter over all the chains of ``trace`` (what :meth:`collect`
        returns) in one device launch: ``diagnostics.chain_diagnostics_all(trace, details)`` -> ``(rhat, ess)``, or
        ``(rhat, ess, raw, stop_lag)`` with ``details=True``. Nothing waits for the host.

        ``rank_normalized=True``: the rank-normalised split R-hat and the bulk and tail effective sample sizes instead,
        ``diagnostics.rank_diagnostics_all(trace, details)`` -> ``(rhat_rank, ess_bulk, ess_tail)``: they also see chains
        that agree in location and differ in scale, and do not need a finite variance."""
        if rank_normalized:
            from pysgmcmc_amd.diagnostics.device_trace import rank_diagnostics_all
            return rank_diagnostics_all(trace, details)
        from pysgmcmc_amd.diagnostics.device_trace import chain_diagnostics_all
        return chain_diagnostics_all(trace, details)

    def predict(self, X, trace, **kw):
        """Posterior predictive of the samples in ``trace`` (what :meth:`collect` returns, or anything
        ``models.posterior_predictive`` accepts) at the rows of ``X``, with the group's own layer sizes, in one device
        call: ``chains.collect(n, every)`` -> ``chains.diagnose(t)`` -> ``chains.predict(X, t)`` is three launches and
        no host copy of a parameter. ``X``: a device tensor of the chains' dtype, or an array that is uploaded; already
        normalised. Returns device tensors: ``(ens_mean, ens_var)``, or ``(means, noise_var)`` with
        ``return_individual_predictions=True``."""
        from pysgmcmc_amd.models.predictive import posterior_predictive
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=self.storage.dtype, device=self.storage.device)
        return posterior_predictive(trace, X, self.samplers[0]._bnn_layer_sizes(), **kw)

    def score(self, X, y, trace, **kw):
        """Held-out score of the samples in ``trace`` (what :meth:`collect` returns, or anything ``models.heldout_score``
        accepts) against the targets ``y`` at the rows of ``X``, with the group's own layer sizes, in one device call:
        ``chains.collect(n, every)`` -> ``chains.diagnose(t)`` -> ``chains.predict(X, t)`` -> ``chains.score(X, y, t)``
        never copies a parameter or a prediction to the host. ``X``, ``y``: device tensors of the chains' dtype, or arrays
        that are uploaded; normalised like the training data. Returns a ``models.HeldOutScore`` of device tensors (lppd,
        WAIC, RMSE and their per-row parts; ``pointwise=True`` / ``per_sample=True`` add the log densities)."""
        from pysgmcmc_amd.models.scoring import heldout_score
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=self.storage.dtype, device=self.storage.device)
        if not torch.is_tensor(y):
            y = torch.as_tensor(np.asarray(y), dtype=self.storage.dtype, device=self.storage.device)
        return heldout_score(trace, X, y, self.samplers[0]._bnn_layer_sizes(), **kw)

    def loo(self, X, y, trace, **kw):
        """PSIS-LOO of the samples in ``trace`` (what :meth:`collect` returns, or anything ``models.loo_score`` accepts) on
        the observations ``(X, y)``, with the group's own layer sizes: ``models.loo_score(trace, X, y, sizes, **kw)``, K13's
        pointwise log densities through K19. ``X``, ``y``: as for :meth:`score`. Returns a ``diagnostics.PsisLoo`` of device
        tensors (``elpd_loo``, ``p_loo``, ``se``, the per-observation ``khat``, ...); nothing waits for the host."""
        from pysgmcmc_amd.models.scoring import loo_score
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=self.storage.dtype, device=self.storage.device)
        if not torch.is_tensor(y):
            y = torch.as_tensor(np.asarray(y), dtype=self.storage.dtype, device=self.storage.device)
        return loo_score(trace, X, y, self.samplers[0]._bnn_layer_sizes(), **kw)

    def calibration(self, X, y, trace, **kw):
        """Calibration of the samples in ``trace`` (what :meth:`collect` returns, or anything ``models.calibration_score``
        accepts) against the held-out targets ``y`` at the rows of ``X``, with the group's own layer sizes:
        ``models.calibration_score(trace, X, y, sizes, **kw)``, K11's means through K20. ``X``, ``y``: as for :meth:`score`.
        Returns a ``diagnostics.Calibration`` of device tensors (``pit``, ``crps``, ``mean_crps``, ``coverage``, ``pit_hist``,
        ...); nothing waits for the host."""
        from pysgmcmc_amd.models.scoring import calibration_score
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=self.storage.dtype, device=self.storage.device)
        if not torch.is_tensor(y):
            y = torch.as_tensor(np.asarray(y), dtype=self.storage.dtype, device=self.storage.device)
        return calibration_score(trace, X, y, self.samplers[0]._bnn_layer_sizes(), **kw)

    def predictive_gradients(self, X, trace, **kw):
        """Predictive moments of the samples in ``trace`` (what :meth:`collect` returns, or anything
        ``models.predictive_gradients`` accepts) at the rows of ``X`` and their gradients with respect to those rows, with
        the group's own layer sizes, on the device: what an acquisition function is climbed with. ``X``: a device tensor of
        the chains' dtype, or an array that is uploaded; already normalised. Returns a ``models.PredictiveGradients`` of
        float64 device tensors ``(mean, var, dmean, dvar)``, or ``(means, grads)`` with ``return_individual=True``."""
        from pysgmcmc_amd.models.predictive import predictive_gradients
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=self.storage.dtype, device=self.storage.device)
        return predictive_gradients(trace, X, self.samplers[0]._bnn_layer_sizes(), **kw)

    def posterior_scores(self, trace, **kw):
        """``grad log p(theta | X, y)`` at every row of ``trace`` (what :meth:`collect` returns, or an ``(n, P)`` matrix),
        from the group's own resident data set and cost constants: ``models.bnn_posterior_scores``, K15 without
        autograd. Returns ``(rows, P)`` with the chains flattened."""
        from pysgmcmc_amd.models.scores import bnn_posterior_scores
        first = self.samplers[0]
        gen, cost = first.batch_generator, first.cost_fun
        return bnn_posterior_scores(trace, first._bnn_layer_sizes(), gen.x_dev, gen.y_dev, wdecay=cost.wdecay,
                                    prior_mean=cost.prior_mean, prior_var=cost.prior_var, **kw)

    def stein_discrepancy(self, trace, **kw):
        """Kernel Stein discrepancy of the samples in ``trace`` (what :meth:`collect` returns, or an ``(n, P)`` matrix)
        against the posterior of the group's own data set: the scores from :meth:`posterior_scores`, then
        ``diagnostics.kernel_stein_discrepancy(samples, scores, **kw)`` (kernel K16). Unlike R-hat and ESS it sees the bias
        of the chains' stationary distribution at their stepsize. A trace of more than 4096 rows in all is thinned evenly
        (every ``k``-th sample of every chain, ``k`` the smallest that fits) and the result's ``thinning`` is that ``k``.
        Returns a ``diagnostics.SteinDiscrepancy`` of device tensors; nothing waits for the host."""
        from pysgmcmc_amd.diagnostics.stein import MAX_SAMPLES, kernel_stein_discrepancy
        if not torch.is_tensor(trace):
            trace = trace.values()
        x = trace if trace.dim() == 3 else trace.unsqueeze(0)
        m, n = int(x.shape[0]), int(x.shape[1])
        if m > MAX_SAMPLES:
            raise ValueError("FusedBNNChains.stein_discrepancy: %d chains, the limit is %d samples in all" % (m, MAX_SAMPLES))
        k = 1
        while m * len(range(0, n, k)) > MAX_SAMPLES:
            k += 1
        if k > 1:
            x = x[:, ::k]
        x = x.reshape(-1, x.shape[-1])
        out = kernel_stein_discrepancy(x, self.posterior_scores(x), **kw)
        return out._replace(thinning=k)

    def thin(self, trace, m, per_chain=False, **kw):
        """A small ensemble from ``trace`` (what :meth:`collect` returns, or an ``(n, P)`` matrix) by greedy Stein thinning
        instead of every k-th row: the scores from :meth:`posterior_scores`, then
        ``diagnostics.stein_thinning(samples, scores, m, per_chain=per_chain, **kw)`` (kernels K16 and K17), then the picked
        rows gathered on the device. Returns ``(ensemble, result)``: ``ensemble`` is an ``(m, P)`` matrix, or
        ``(chains * m, P)`` with ``per_chain=True`` (``m`` rows of every chain, picked on that chain alone), which
        :meth:`predict`, :meth:`score` and :meth:`predictive_gradients` accept as they accept a trace; ``result`` is the
        ``diagnostics.SteinThinning`` of device tensors. A trace of more than 4096 rows in all is first strided evenly as
        :meth:`stein_discrepancy` does: ``result.indices`` still index the rows of ``trace`` itself (the flattened rows, or
        the rows of the chain with ``per_chain=True``) and ``result.discrepancy.thinning`` reports the stride. Nothing waits
        for the host."""
        from pysgmcmc_amd.diagnostics.stein import MAX_SAMPLES, stein_thinning
        if not torch.is_tensor(trace):
            trace = trace.values()
        x = trace if trace.dim() == 3 else trace.unsqueeze(0)
        chains, n, P = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if chains > MAX_SAMPLES:
            raise ValueError("FusedBNNChains.thin: %d chains, the limit is %d samples in all" % (chains, MAX_SAMPLES))
        k = 1
        while chains * len(range(0, n, k)) > MAX_SAMPLES:
            k += 1
        xs = (x[:, ::k] if k > 1 else x).reshape(-1, P)
        kept = int(xs.shape[0]) // chains
        scores = self.posterior_scores(xs)
        result = stein_thinning(xs.view(chains, kept, P), scores.view(chains, kept, P), m, per_chain=per_chain, **kw)
        idx = result.indices.long()
        if per_chain:
            local = idx * k                                                   # (chains, m), rows of the chain
            flat = (local + n * torch.arange(chains, device=idx.device).unsqueeze(1)).reshape(-1)
        else:
            flat = local = (idx // kept) * n + (idx % kept) * k               # (m,), rows of the flattened trace
        ensemble = x.reshape(-1, P).index_select(0, flat)
        result = result._replace(indices=local.to(torch.int32), discrepancy=result.discrepancy._replace(thinning=k))
        return ensemble, result

    @classmethod
    def for_dataset(cls, X, y, n_chains, hidden=(50, 50, 50), batch_size=20, seed=0, dtype=torch.float32,
                    device="cuda:0", stepsize=0.01, burn_in_steps=1000, mdecay=0.05, init_seed=None):
        """``n_chains`` chains of the reference's default BNN set-up
        (``pysgmcmc/models/bayesian_neural_network.py:151-155,451-457``: ``scale_grad = N``) over one dataset."""
        from pysgmcmc_amd.data_batches import Placeholder, generate_batches
        from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
        from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule
        X = np.asarray(X)
        X = X.reshape(X.shape[0], -1)
        xp, yp = Placeholder(dtype=dtype, device=device), Placeholder(dtype=dtype, device=device)
        shared = generate_batches(X, y, xp, yp, batch_size, seed=seed)       # ONE resident copy of the dataset
        chains = []
        for c in range(int(n_chains)):
            gen = type(shared)(shared.x_dev, shared.y_dev, xp, yp, shared.batch_size,
                               np.random.RandomState(seed + c))
            params = init_mlp_params(X.shape[1], hidden=hidden, seed=(seed if init_seed is None else init_seed) + c,
                                     dtype=dtype, device=device)
            chains.append(SGHMCSampler(
                params=params, cost_fun=BNNCost(xp, yp, batch_size=shared.batch_size, n_examples=X.shape[0]),
                batch_generator=gen, stepsize_schedule=ConstantStepsizeSchedule(stepsize),
                burn_in_steps=burn_in_steps, mdecay=mdecay, scale_grad=float(X.shape[0]),
                session=device, dtype=dtype, seed=seed + c))
        return cls(chains)
