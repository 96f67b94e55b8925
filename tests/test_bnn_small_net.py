"""The small-net core (csrc/sgmcmc_bnn_small_net.hpp) without a GPU: K11 (posterior predictive), K13 (held-out score) and K14
(input gradients) refuse a net on its sizes, or on its parameters alone, in one text, and what the core defines is defined
nowhere else in their translation units. What the kernels compute is checked on the GPU (tests/test_bnn_predict_gpu.py,
tests/test_bnn_score_gpu.py, tests/test_bnn_predict_grad_gpu.py)."""
import ctypes
import os
import re

import pytest

from pysgmcmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pysgmcmc_amd", "csrc")
UNITS = ("sgmcmc_bnn_predict.hip", "sgmcmc_bnn_score.hip", "sgmcmc_bnn_predict_grad.hip")
EINVAL = -1

# nets refused on their sizes or on their parameters alone, and the text behind the `what:` prefix
REFUSED = [
    ((3,), b"1..8 layers"),                                              # 0 layers
    ((3,) + (4,) * 8 + (1,), b"1..8 layers"),                            # 9 layers
    ((3, 0, 1), b"bad layer size"),
    ((3, 7, 2), b"the last layer must have one unit"),
    ((46341, 46341, 1), b"the parameters alone need more than 160 KiB of LDS"),       # 46341^2 > 2^31
    ((2147483647, 2147483647, 1), b"the parameters alone need more than 160 KiB of LDS"),
]


def _row_tile(entry, sizes, esize):
    lib = _lib.lib()
    rc = getattr(lib, entry)((ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, esize)
    return rc, lib.sgmcmc_last_error()


def _score(sizes, esize):
    """The score entry with dummy DEVICE pointers: it refuses on the host, before it reads one of them."""
    lib = _lib.lib()
    chains = (ctypes.c_void_p * 64)(*[4096 * (c + 1) for c in range(64)])
    f = getattr(lib, "sgmcmc_bnn_score_" + {4: "f32", 8: "f64"}[esize])
    rc = f(chains, 1, 7, 2 ** 62, (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, 4096, 4096, 5, 4096, 4096, 4096, 4096,
           4096, None, None, None, None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("esize", [4, 8])
@pytest.mark.parametrize("sizes, text", REFUSED, ids=[str(k) for k in range(len(REFUSED))])
def test_the_three_kernels_refuse_a_net_in_one_text(sizes, text, esize):
    got = {}
    for what, (rc, msg) in (("bnn_predict_row_tile", _row_tile("sgmcmc_bnn_predict_row_tile", sizes, esize)),
                            ("bnn_predict_grad_row_tile", _row_tile("sgmcmc_bnn_predict_grad_row_tile", sizes, esize)),
                            ("bnn_predict", _score(sizes, esize))):          # K13 refuses under K11's name
        assert rc == EINVAL and msg.startswith(what.encode() + b": "), (what, rc, msg)
        got[what] = msg[len(what) + 2:]
    assert set(got.values()) == {text}, got


def test_what_the_core_defines_is_defined_once():
    core = open(os.path.join(CSRC, "sgmcmc_bnn_small_net.hpp")).read()
    defined_once = {
        "the primitives": r"\b(tanh_t|fma_t)\((float|double) |struct Pair\b|\b(ld2|st2)\((const )?T \*p",
        "the row copy": r"alignas\(16\) Q\b",
        "the forward loop": r"acc\.x = fma_t\(h, w\.x, acc\.x\)|hout\[idx\] = tanh_t\(acc\)",
        "the net rules": r"1\.\.8 layers|bad layer size|the last layer must have one unit|the parameters alone need",
        "the ensemble kernel": r"ens_var\[r\] = q / \(double\)S",
        "the grid rule and the LDS opt-in": r"hipFuncSetAttribute|GRID_TARGET",
    }
    for what, pattern in defined_once.items():
        assert re.search(pattern, core), what
        for unit in UNITS:
            text = open(os.path.join(CSRC, unit)).read()
            assert '#include "sgmcmc_bnn_small_net.hpp"' in text, unit
            if what == "the ensemble kernel" and unit == "sgmcmc_bnn_score.hip":
                continue                                # the row kernel forms ens_var inside its own two passes
            assert not re.search(pattern, text), (what, unit)
    # the three add-ons share one table of chain pointers
    assert "static_assert(SGMCMC_PREDICT_MAX_CHAINS == SGMCMC_SCORE_MAX_CHAINS" in core
