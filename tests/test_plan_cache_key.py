"""The rollout plan cache (mrbo.rollout._plan_for) keys a plan on what it is built from, not on the
surrogate's id() and version alone: CPython hands a freed surrogate's id to the next one, which starts
at the same version, and the successor then met the plan of the surrogate that was gone (the raw and
the standardised surrogate of tests/test_gpu_standardize.py, depending on the heap's history)."""
import numpy as np

import conftest  # noqa: F401  (sys.path)


def _surrogate(standardize, scale=1.0):
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    X = -2.0 + 4.0 * kronecker_quasirand(2, 12, 3)
    y = scale * ((X ** 2).sum(axis=0) + 100.0 * np.sin(X[0]))
    return Surrogate(Matern52([1.0]), X, y, capacity=12, σn2=1e-6, standardize=standardize)


def test_state_key_tells_surrogates_at_one_address_apart():
    from mrbo.rollout import _state_key
    raw, std, scaled = _surrogate(False), _surrogate(True), _surrogate(False, scale=3.0)
    assert raw.version == std.version == scaled.version
    content = lambda s: _state_key(s)[2:]          # the key without id and version
    assert content(raw) != content(std) and content(raw) != content(scaled)
    assert _state_key(raw) == _state_key(raw)
    assert content(raw) == content(_surrogate(False))
