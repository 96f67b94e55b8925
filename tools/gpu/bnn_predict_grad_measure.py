"""Times ``models.predictive_gradients`` (K14, include/sgmcmc_hip_predict_grad.h) against
``BayesianNeuralNetwork.predictive_gradients``'s host path (autograd through one batched forward pass with activations in
HBM, one copy to the host, numpy reduction) on the same kept networks: 100 networks x 1 000 rows in f32 and f64, and a
(256, 100, 5252) f32 trace x 1 000 rows on the device alone. Medians of 11 runs after a warm-up call: device events on the
stream for the device call, a host clock around calls that end in a device-to-host copy. The record is
profiles/bnn_predict_grad.txt.

    python tools/gpu/bnn_predict_grad_measure.py [output file]
"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from pysgmcmc_amd import kernels
from pysgmcmc_amd.models import BayesianNeuralNetwork, posterior_predictive, predictive_gradients
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else open(os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

dev = torch.device("cuda:0")
sizes = [1, 50, 50, 50, 1]
P = 5252
shapes = [(1, 50), (50,), (50, 50), (50,), (50, 50), (50,), (50, 1), (1,), (1, 1)]
say("device", torch.cuda.get_device_name(0), "torch", torch.__version__)
say("row tile f32", kernels.bnn_predict_grad_row_tile(sizes, torch.float32), "f64",
    kernels.bnn_predict_grad_row_tile(sizes, torch.float64), "(K11: f32", kernels.bnn_predict_row_tile(sizes, torch.float32),
    "f64", kernels.bnn_predict_row_tile(sizes, torch.float64), ")")

def trace(m, n, dt):
    g = torch.Generator(device="cpu").manual_seed(7)
    base = torch.cat([p.reshape(-1) for p in init_mlp_params(1, seed=5)])
    t = base[None, None, :] + 0.1 * torch.randn(m, n, P, generator=g, dtype=torch.float64)
    t[:, :, -1] = np.log(1e-3) + 0.01 * torch.rand(m, n, generator=g, dtype=torch.float64)
    return t.to(dt).to(dev)

def nets_of(flat):
    nets = []
    for s in range(flat.shape[0]):
        row, off, net = flat[s], 0, []
        for shp in shapes:
            k = int(np.prod(shp)); net.append(row[off:off + k].view(shp)); off += k
        nets.append(net)
    return nets

def events(fn, runs=11):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)

def wall(fn, runs=11):
    r = fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, r

X = np.random.RandomState(0).uniform(-1, 1, size=(1000, 1))
for dt in (torch.float32, torch.float64):
    for (m, n) in ((1, 100), (256, 100)):
        S = m * n
        if dt == torch.float64 and S > 100:
            continue
        t = trace(m, n, dt)
        Xd = torch.as_tensor(X, dtype=dt, device=dev)
        say("---- %d networks x 1000 rows, %s" % (S, dt))
        med, lo, hi = events(lambda: predictive_gradients(t, Xd, sizes))
        say("predictive_gradients (mean, var, dmean, dvar), device events: median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
        med, lo, hi = events(lambda: predictive_gradients(t, Xd, sizes, return_individual=True))
        say("predictive_gradients (means, grads), device events:           median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
        med, lo, hi = events(lambda: posterior_predictive(t, Xd, sizes, return_individual_predictions=True))
        say("posterior_predictive (means, noise_var) = K11's forward pass: median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
        if S > 100:
            med, lo, hi = events(lambda: predictive_gradients(t, Xd, sizes, scratch_bytes=1 << 26))
            say("predictive_gradients with 64 MiB of scratch (row chunks):     median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
            del t
            torch.cuda.empty_cache()
            continue
        bnn = BayesianNeuralNetwork(session=dev, dtype=dt, n_nets=S, normalize_input=False, normalize_output=False)
        bnn.is_trained = True
        bnn.samples.extend(nets_of(t.view(S, P)))
        med, lo, hi, dev_out = wall(lambda: bnn.predictive_gradients(X, on_device=True))
        say("predictive_gradients(on_device=True) to numpy, host clock:    median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
        med, lo, hi, host_out = wall(lambda: bnn.predictive_gradients(X))
        say("predictive_gradients() host autograd path to numpy, host clock: median %.3f ms (min %.3f, max %.3f) of 11" % (med, lo, hi))
        say("max |dmean difference| %.3e, max |dvar difference| %.3e (max |dmean| %.3e, max |dvar| %.3e)" % (
            np.abs(dev_out[0] - host_out[0]).max(), np.abs(dev_out[1] - host_out[1]).max(), np.abs(host_out[0]).max(),
            np.abs(host_out[1]).max()))
        del bnn, t
        torch.cuda.empty_cache()
say("done")
