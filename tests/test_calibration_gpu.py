"""K20, PIT, coverage and CRPS of a mixture of Gaussians on the device (csrc/sgmcmc_calib.hip, include/sgmcmc_hip_calib.h),
and its public front ends (``kernels.mixture_calibration``, ``diagnostics.calibration``, ``models.calibration_score``,
``FusedBNNChains.calibration``, ``BayesianNeuralNetwork.calibration``) against the host statement
``diagnostics.calibration.mixture_calibration_host`` on a copy of the same inputs.

Exact: repeated runs, a row alone against the row in a batch, pitches, canaries, optional outputs, the placement of NaN,
graph replay, ``summary`` as the stated function of the device's own rows, and the front ends against K11 followed by K20
called by hand. Within a measured bound (calibration_cases.py, profiles/calibration.txt): ``pit`` and ``crps`` against the
host, which differ through the vendor's erf / erfc / exp against the host's; the tests allow 4 times the largest difference
measured over all the cases here."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels, models

import calibration_cases as C

pytestmark = pytest.mark.gpu

F64 = torch.float64
CANARY = -77.25
DTYPES = {"f32": (torch.float32, "float32"), "f64": (torch.float64, "float64")}


class Outputs(object):
    """Every output of one call inside a canary-filled buffer of its own; means inside a wider NaN-filled one, var and y
    between NaN elements."""

    def __init__(self, means, var, y, dev, pad=3, summary=True, levels=C.LEVELS, n_bins=C.N_BINS):
        S, n = means.shape
        dt = torch.from_numpy(np.zeros(1, dtype=means.dtype)).dtype
        self.S, self.n, self.levels, self.n_bins = S, n, tuple(levels), n_bins
        self.buf = torch.full((S + 1, n + pad), float("nan"), dtype=dt, device=dev)
        self.buf[:S, :n] = torch.as_tensor(means, device=dev)
        self.means = self.buf[:S, :n]
        self.var_buf = torch.full((S + 2,), float("nan"), dtype=F64, device=dev)
        self.var_buf[1:S + 1] = torch.as_tensor(var, device=dev)
        self.y_buf = torch.full((n + 2,), float("nan"), dtype=dt, device=dev)
        self.y_buf[1:n + 1] = torch.as_tensor(y, device=dev)
        self.n_summary = 2 + len(self.levels) + n_bins
        self.full = dict(pit=torch.full((n + 2,), CANARY, dtype=F64, device=dev),
                         crps=torch.full((n + 2,), CANARY, dtype=F64, device=dev),
                         summary=torch.full((self.n_summary + 2,), CANARY, dtype=F64, device=dev))
        self.on = dict(pit=True, crps=True, summary=summary)

    def view(self, name):
        if not self.on[name]:
            return None
        return self.full[name][1:-1]

    def run(self):
        kernels.mixture_calibration(self.means, self.var_buf[1:self.S + 1], self.y_buf[1:self.n + 1], self.levels, self.n_bins,
                                    **{name: self.view(name) for name in self.full})
        return self

    def result(self):
        """The outputs as numpy arrays (None where off), after the canaries are checked."""
        out = {}
        for name, f in self.full.items():
            h = f.cpu().numpy()
            if not self.on[name]:
                assert (h == CANARY).all(), "%s was not passed and was written" % name
                out[name] = None
            else:
                assert h[0] == CANARY and h[-1] == CANARY, "a canary around %s was overwritten" % name
                out[name] = h[1:-1].copy()
        assert torch.isnan(self.buf[self.S:]).all() and torch.isnan(self.buf[:, self.n:]).all(), "means' pitch gap was written"
        return out


def _device(means, var, y, dev, **kw):
    return Outputs(means, var, y, dev, **kw).run().result()


def _assert_same_bits(a, b, what):
    for name in a:
        if a[name] is None or b[name] is None:
            continue
        assert C.same_bits(a[name], b[name]), "%s: %s differs in its bits" % (what, name)


def _assert_summary_is_the_stated_function(got, levels=C.LEVELS, n_bins=C.N_BINS):
    want = C.summary(got["pit"], got["crps"], levels, n_bins)
    if np.isnan(want[0]):                                 # a NaN's sign and payload are no part of the statement
        assert np.isnan(got["summary"][0])
        assert C.same_bits(got["summary"][1:], want[1:]), "summary is %s, its rows give %s" % (got["summary"], want)
    else:
        assert C.same_bits(got["summary"], want), "summary is %s, its rows give %s" % (got["summary"], want)


def _assert_against_host(got, ref, n, what):
    """NaN where the host has it, within 4 times the measured bound elsewhere. Returns the measured differences."""
    d = {}
    for name in ("pit", "crps"):
        want = ref[name][:n]
        assert np.array_equal(np.isnan(got[name]), np.isnan(want)), "%s: %s is NaN in other rows than on the host" % (what, name)
        d[name] = C.rel_or_abs(got[name], want)
    print("%s: d pit %.3e  d crps %.3e" % (what, d["pit"], d["crps"]))
    assert max(d.values()) <= C.SAME_STATEMENT_LIMIT, "%s: the two sides do not execute the same statement" % what
    assert d["pit"] <= C.MARGIN * C.PIT_REL_MEASURED, "%s: pit is %.3e from the host" % (what, d["pit"])
    assert d["crps"] <= C.MARGIN * C.CRPS_REL_MEASURED, "%s: crps is %.3e from the host" % (what, d["crps"])
    return d["pit"], d["crps"]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("S", C.DRAWS)
def test_every_shape_against_the_host(gpu, S, dtype):
    means, var, y, ref = C.reference(S, DTYPES[dtype][1])
    for n in C.rows_for(S):
        got = _device(means[:, :n], var, y[:n], gpu)
        _assert_against_host(got, ref, n, "S = %d, n_rows = %d, %s" % (S, n, dtype))
        assert (got["pit"] >= 0.0).all() and (got["pit"] <= 1.0).all() and (got["crps"] >= 0.0).all()
        _assert_summary_is_the_stated_function(got)
        assert got["summary"][1] == 0.0 and got["summary"][-C.N_BINS:].sum() == float(n)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("S", [3, 257, 4096])
def test_bits_do_not_depend_on_the_call(gpu, S, dtype):
    """A second run, a row alone against the batch, dense against padded pitches, summary on or off, other levels and bins."""
    means, var, y, _ = C.reference(S, DTYPES[dtype][1])
    n = means.shape[1]
    first = Outputs(means, var, y, gpu)
    a = first.run().result()
    b = first.run().result()
    _assert_same_bits(a, b, "a second run")
    for r in (0, n // 2, n - 1):
        one = _device(means[:, r:r + 1], var, y[r:r + 1], gpu, pad=0)
        for name in ("pit", "crps"):
            assert C.same_bits(one[name], a[name][r:r + 1]), "row %d alone: %s" % (r, name)
    _assert_same_bits(_device(means, var, y, gpu, pad=0), a, "dense pitches")
    _assert_same_bits(_device(means, var, y, gpu, pad=61), a, "wide pitches")
    off = _device(means, var, y, gpu, summary=False)
    _assert_same_bits(off, a, "without summary")
    for levels, n_bins in (((), 0), ((0.5,), 0), ((), 64), (tuple((k + 1) / 17.0 for k in range(16)), 64)):
        got = _device(means, var, y, gpu, levels=levels, n_bins=n_bins)
        assert C.same_bits(got["pit"], a["pit"]) and C.same_bits(got["crps"], a["crps"])
        assert got["summary"].shape == (2 + len(levels) + n_bins,)
        _assert_summary_is_the_stated_function(got, levels, n_bins)


def test_summary_over_more_rows_than_partials(gpu):
    means, var, y = C.ensemble(5, 700, seed=9)
    got = _device(means, var, y, gpu)
    _assert_summary_is_the_stated_function(got)
    assert got["summary"][1] == 0.0 and got["summary"][-C.N_BINS:].sum() == 700.0
    # pit = 1.0 and pit = 0.0 exactly: targets far outside a narrow ensemble land in the outer bins
    y = y.copy()
    y[3], y[4] = 1e3, -1e3
    got = _device(means, var, y, gpu)
    assert got["pit"][3] == 1.0 and got["pit"][4] == 0.0
    _assert_summary_is_the_stated_function(got)
    assert got["summary"][-C.N_BINS:].sum() == 700.0


def test_nan_poisons_its_own_row_only(gpu):
    means, var, y, ref = C.reference(257, "float64")
    n = means.shape[1]
    clean = _device(means, var, y, gpu)
    bad_y, bad_means = y.copy(), means.copy()
    bad_y[5] = np.nan
    bad_means[200, 40] = np.nan
    got = _device(bad_means, var, bad_y, gpu)
    keep = [r for r in range(n) if r not in (5, 40)]
    for name in ("pit", "crps"):
        assert np.isnan(got[name][[5, 40]]).all(), name
        assert C.same_bits(got[name][keep], clean[name][keep]), name
    assert np.isnan(got["summary"][0]) and got["summary"][1] == 2.0
    assert got["summary"][-C.N_BINS:].sum() == float(n - 2)
    _assert_summary_is_the_stated_function(got)
    host = diagnostics.mixture_calibration_host(bad_means, var, bad_y)
    assert np.array_equal(np.isnan(host["pit"]), np.isnan(got["pit"])) and np.array_equal(np.isnan(host["crps"]), np.isnan(got["crps"]))
    # an infinite variance belongs to a draw, so it reaches every row: crps is inf - inf, pit stays a number, as on the host
    bad_var = var.copy()
    bad_var[100] = np.inf
    got = _device(means, bad_var, y, gpu)
    host = diagnostics.mixture_calibration_host(means, bad_var, y)
    assert np.isnan(got["crps"]).all() and np.isnan(host["crps"]).all()
    assert np.isfinite(got["pit"]).all() and C.rel_or_abs(got["pit"], host["pit"]) <= C.MARGIN * C.PIT_REL_MEASURED
    assert got["summary"][1] == float(n) and (got["summary"][2:] == 0.0).all()
    _assert_same_bits(_device(means, var, y, gpu), clean, "a clean call after the poisoned ones")


def test_allocated_outputs_and_no_rows(gpu):
    means, var, y, _ = C.reference(65, "float32")
    want = _device(means, var, y, gpu)
    md, vd, yd = (torch.as_tensor(a, device=gpu) for a in (means, var, y))
    pit, crps = kernels.mixture_calibration(md, vd, yd)
    assert pit.dtype == F64 and crps.dtype == F64 and tuple(pit.shape) == tuple(crps.shape) == (means.shape[1],)
    assert C.same_bits(pit.cpu().numpy(), want["pit"]) and C.same_bits(crps.cpu().numpy(), want["crps"])
    pit, crps = kernels.mixture_calibration(md[:, :0], vd, yd[:0], C.LEVELS, C.N_BINS)
    assert pit.numel() == crps.numel() == 0
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    with pytest.raises(SgmcmcLibraryError, match=r"mixture_calibration: pit is NULL"):     # the library's own check, by name
        rc = kernels.lib().sgmcmc_mixture_calibration_f32(md.data_ptr(), md.stride(0), 65, 3, vd.data_ptr(), yd.data_ptr(), None,
                                                          0, 0, None, None, None, None)
        kernels.check(rc, "sgmcmc_mixture_calibration")
    got = diagnostics.calibration(md, vd, yd)
    assert isinstance(got, diagnostics.Calibration) and got.thinning == 1
    for name in ("mean_crps", "calibration_error", "n_bad"):
        v = getattr(got, name)
        assert v.dim() == 0 and v.dtype == F64 and v.device == md.device, name
    s = C.summary(want["pit"], want["crps"])
    n = means.shape[1]
    assert C.same_bits(got.pit.cpu().numpy(), want["pit"]) and C.same_bits(got.crps.cpu().numpy(), want["crps"])
    assert float(got.mean_crps) == s[0] / n and float(got.n_bad) == 0.0
    assert np.array_equal(got.coverage.cpu().numpy(), s[2:2 + len(C.LEVELS)] / n)
    assert np.array_equal(got.pit_hist.cpu().numpy(), s[-C.N_BINS:]) and list(got.levels.cpu().numpy()) == list(C.LEVELS)
    assert float(got.calibration_error) == np.abs(s[2:2 + len(C.LEVELS)] / n - np.array(C.LEVELS)).mean()


def test_graph_capture_and_replay(gpu):
    means, var, y, _ = C.reference(257, "float32")
    means, y = means[:, :13], y[:13]
    eager = _device(means, var, y, gpu)
    out = Outputs(means, var, y, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        out.run()                                         # warm-up on the side stream, as capture wants
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    for f in out.full.values():
        f.fill_(CANARY)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out.run()
    torch.cuda.synchronize()
    assert float((out.full["crps"] != CANARY).sum()) == 0.0       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _assert_same_bits(out.result(), eager, "the replayed graph")


# ---- the front ends

def _small_net_case(dev, dtype=torch.float32):
    sizes = [2, 5, 1]
    P = kernels._bnn_n_params(sizes)
    g = torch.Generator().manual_seed(7)
    trace = (0.7 * torch.randn(4, 25, P, generator=g)).to(dtype).to(dev)
    X = torch.randn(23, 2, generator=g).to(dtype).to(dev)
    y = torch.randn(23, generator=g).to(dtype).to(dev)
    return sizes, trace, X, y


def _by_hand(trace, X, y, sizes, levels=C.LEVELS, n_bins=C.N_BINS):
    """K11 and then K20, called one after the other."""
    rows = trace.reshape(-1, trace.shape[-1])
    means = torch.empty(rows.shape[0], X.shape[0], dtype=trace.dtype, device=trace.device)
    kernels.bnn_predict(trace, sizes, X, means)
    var = torch.exp(rows[:, kernels._bnn_n_params(sizes) - 1].double()) + 1e-16
    summary = torch.empty(2 + len(levels) + n_bins, dtype=F64, device=trace.device)
    pit, crps = kernels.mixture_calibration(means, var, y, levels, n_bins, summary=summary)
    return dict(pit=pit.cpu().numpy(), crps=crps.cpu().numpy(), summary=summary.cpu().numpy(), means=means, var=var)


def _assert_is(got, hand, levels=C.LEVELS):
    assert isinstance(got, diagnostics.Calibration)
    n, s = hand["pit"].shape[0], hand["summary"]
    assert C.same_bits(got.pit.cpu().numpy(), hand["pit"]) and C.same_bits(got.crps.cpu().numpy(), hand["crps"])
    assert float(got.mean_crps) == s[0] / n and float(got.n_bad) == s[1]
    assert np.array_equal(got.coverage.cpu().numpy(), s[2:2 + len(levels)] / (n - s[1]))
    assert np.array_equal(got.pit_hist.cpu().numpy(), s[2 + len(levels):])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_calibration_score_is_predict_then_calibrate(gpu, dtype):
    sizes, trace, X, y = _small_net_case(gpu, DTYPES[dtype][0])
    hand = _by_hand(trace, X, y, sizes)
    got = models.calibration_score(trace, X, y, sizes)
    assert got.thinning == 1 and tuple(got.pit.shape) == (23,)
    _assert_is(got, hand)
    # against the host statement of the same means and variances
    ref = diagnostics.mixture_calibration_host(hand["means"].cpu().numpy(), hand["var"].cpu().numpy(), y.cpu().numpy())
    _assert_against_host(hand, ref, 23, "calibration_score, %s" % dtype)
    # a particle matrix, a list of chains, other levels
    _assert_is(models.calibration_score(trace.reshape(100, -1), X, y, sizes), hand)
    _assert_is(models.calibration_score([c for c in trace], X, y, sizes), hand)
    other = models.calibration_score(trace, X, y, sizes, levels=(0.3,), n_bins=4)
    _assert_is(other, _by_hand(trace, X, y, sizes, (0.3,), 4), (0.3,))


def test_calibration_score_strides_a_long_trace(gpu):
    sizes = [2, 5, 1]
    P = kernels._bnn_n_params(sizes)
    g = torch.Generator().manual_seed(8)
    trace = (0.5 * torch.randn(3, 2050, P, generator=g)).to(gpu)
    X, y = torch.randn(4, 2, generator=g).to(gpu), torch.randn(4, generator=g).to(gpu)
    got = models.calibration_score(trace, X, y, sizes)
    assert got.thinning == 2                              # 3 * 2050 > 4096 >= 3 * 1025
    want = models.calibration_score(trace[:, ::2].contiguous(), X, y, sizes)
    assert want.thinning == 1
    assert C.same_bits(got.pit.cpu().numpy(), want.pit.cpu().numpy())
    assert C.same_bits(got.crps.cpu().numpy(), want.crps.cpu().numpy())


def test_chain_group_calibration(gpu):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(3)
    X = rng.uniform(-3.0, 3.0, size=(60, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(60)
    chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=gpu, burn_in_steps=4)
    trace = chains.collect(8, every=2)
    got = chains.calibration(X, y, trace)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=gpu)
    yd = torch.as_tensor(y, dtype=torch.float32, device=gpu)
    assert tuple(trace.shape)[:2] == (4, 8) and tuple(got.pit.shape) == (60,)
    _assert_is(got, _by_hand(trace, Xd, yd, chains.samplers[0]._bnn_layer_sizes()))
    other = chains.calibration(Xd, yd, trace, levels=(0.5,), n_bins=0)
    assert C.same_bits(other.pit.cpu().numpy(), got.pit.cpu().numpy()) and other.pit_hist.numel() == 0


def test_bnn_calibration_on_the_device_agrees_with_the_host_route(gpu):
    """The two routes run different forward passes (batched products in torch against K11), so their means differ by the
    rounding of a float64 forward pass, measured here from ``predict``'s two routes. The CRPS is 1-Lipschitz in the target
    and in a common shift of the means, and the PIT's slope is at most the largest density ``1 / (sqrt(2 pi) sd_min)``: those
    two products are added to the kernel's measured bound."""
    from pysgmcmc_amd.models import BayesianNeuralNetwork
    rng = np.random.RandomState(4)
    X = rng.uniform(-3.0, 3.0, size=(50, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(50)
    bnn = BayesianNeuralNetwork(session=gpu, dtype=torch.float64, n_nets=6, n_iters=80, burn_in_steps=10, sample_steps=2, seed=1)
    with pytest.raises(ValueError, match="untrained"):
        bnn.calibration(X, y)
    bnn.train(X, y)
    Xt = rng.uniform(-3.0, 3.0, size=(40, 1))
    yt = np.sinc(Xt[:, 0]) + 0.05 * rng.randn(40)
    host = bnn.calibration(Xt, yt)
    dev = bnn.calibration(Xt, yt, on_device=True)
    assert sorted(dev) == sorted(host) == ["calibration_error", "coverage", "crps", "levels", "mean_crps", "n_bad", "pit",
                                           "pit_hist", "thinning"]
    f_host, noise = bnn.predict(Xt, return_individual_predictions=True)
    f_dev, _ = bnn.predict(Xt, return_individual_predictions=True, on_device=True)
    d_mu = float(np.abs(f_host - f_dev).max())
    sd_min = float(np.sqrt(noise.min()))
    d_pit = float(np.abs(dev["pit"] - host["pit"]).max())
    d_crps = C.rel_or_abs(dev["crps"], host["crps"])
    print("d means %.3e, d pit %.3e, d crps %.3e" % (d_mu, d_pit, d_crps))
    assert d_pit <= C.MARGIN * C.PIT_REL_MEASURED + 2.0 * d_mu / (np.sqrt(2.0 * np.pi) * sd_min)
    assert d_crps <= C.MARGIN * C.CRPS_REL_MEASURED * float(bnn.y_std) + 2.0 * d_mu
    assert dev["crps"].shape == dev["pit"].shape == (40,) and dev["pit_hist"].sum() == 40.0 and dev["n_bad"] == 0
    assert isinstance(dev["mean_crps"], float) and dev["thinning"] == 1
