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


def test_plain_and_single_surrogate_batch_plans_share_one_cache_entry(monkeypatch):
    """One cache, one key shape: _plan_for(s, ...) is _plan_for_multi([s], ...), so the plain plan
    and the S = 1 batch plan of the same inputs are one object (they are the same library plan)."""
    from mrbo import rollout

    class CountingPlan:
        built = 0

        def __init__(self, *args, **kwargs):
            CountingPlan.built += 1

        @classmethod
        def from_surrogates(cls, surrogates, *args, **kwargs):
            return cls(surrogates, *args, **kwargs)

    monkeypatch.setattr(rollout, "RolloutPlan", CountingPlan)
    monkeypatch.setattr(rollout, "_PLANS", {})
    s, other = _surrogate(False), _surrogate(False, scale=3.0)
    lbs, ubs = np.zeros(2), np.ones(2)
    args = (1, 16, 4, 4, lbs, ubs, 0.0, 0, {})
    p = rollout._plan_for(s, *args)
    assert CountingPlan.built == 1 and rollout._plan_for(s, *args) is p and CountingPlan.built == 1
    assert rollout._plan_for_multi([s], *args) is p and CountingPlan.built == 1
    assert len(rollout._PLANS) == 1
    q = rollout._plan_for(other, *args)
    assert q is not p and CountingPlan.built == 2 and len(rollout._PLANS) == 2
    assert rollout._plan_for_multi([other], *args) is q and CountingPlan.built == 2
