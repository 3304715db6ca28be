"""The failure recipes of tests/failure_inputs.py on the oracle alone: the conditions that make
tests/test_gpu_failure_paths.py meaningful, at every shape and recipe that file runs.

Per (layout, recipe), on the oracle's two builds (-ffp-contract=off checker, -O3 -march=native):
  - the builds agree on every trajectory's status (the margin of the recipe is above rounding);
  - the recipe's bit is on ≥ 10 % of the trajectories and nothing outside the recipe's listed
    status values occurs;
  - a mixed recipe leaves ≥ 10 % finished and a restart that holds both kinds;
  - an h = 3 twin fails at its last step somewhere (factor / noise: the bit can come at any step);
  - the plain input of every layout fails nowhere, and NaN in every other inner start fails nowhere
    (the NaN filter of the multistart).
The inputs come from the oracle's Sobol stream and inner starts and the package's CPU surrogate, so
nothing here needs libmrbo.so.  -s prints the counts.

Oracle status counts (value: trajectories, of 128; Gauss–Hermite of 500), both builds:
  layout                      factor                 noise                  noise_near  nan_starts  singular
  half_d2_n12 (+ half_off,    0:61 1:67              0:54 1:74              4:128       8:128       0:25 16:103
    generic_h2)
  generic_d2_n12_h3           0:54 1:74              0:47 1:81              4:128       8:128       0:25 16:103
  half_d3_n24 (+ half_off)    0:86 1:42              0:81 1:47              4:128       8:128       0:112 16:16
  full_d6_n40_h2 (+ tables    0:74 1:44 2:10         0:89 1:39              4:128       8:128       0:92 16:36
    off)
  full_d6_n40_h3 (+ off)      0:64 1:54 2:10         0:70 1:58              4:128       8:128       0:92 16:36
  two_rows_d4_n96_h2          dropped (1: 12)        0:99 1:29              4:128       8:128       0:68 16:60
  two_rows_d4_n96_h3          0:105 1:23             0:60 1:63 2:5          4:128       8:128       0:68 16:60
  four_rows_d3_n150_h2        0:76 1:48 2:4          0:37 1:7 2:84          4:128       8:128       dropped (16: 4)
  four_rows_d3_n150_h3        0:72 1:48 2:8          0:32 1:7 2:89          4:128       8:128       dropped (16: 4)
  wide_d9_n20_h2              0:78 1:50              0:82 1:45 2:1          4:128       8:128       0:101 16:27
  wide_d9_n20_h3              0:68 1:60              0:54 1:73 2:1          4:128       8:128       0:101 16:27
  se_d2_n12_h2                0:58 1:38 2:32         0:115 1:13             4:128       8:128       0:21 16:107
  se_d2_n12_h3                0:50 1:46 2:32         0:62 1:66              4:128       8:128       0:21 16:107
  poi_d2_n12_h2               0:81 1:47              0:16 1:100 2:12        4:128       8:128       0:25 16:103
  poi_d2_n12_h3               0:63 1:65              dropped (0: 7)         4:128       8:128       0:25 16:103
  cost_generic_d2_n12         0:59 1:69              dropped (1: 7)         4:128       8:128       0:25 16:103
  cost_kernel_d3_n70_h4       0:68 1:53 2:7          0:39 1:59 2:30         4:128       8:128       dropped (16: 8)
  ghq_d2_n12                  0:405 1:95             0:215 1:285            4:500       8:500       0:230 16:270
Dropped pairs and their reasons: failure_inputs.DROPPED.
"""
import os

import numpy as np
import pytest

import failure_inputs as F
from conftest import ROOT, load_golden

ORACLE_FAST = os.path.join(ROOT, "oracle", "build", "librbo_oracle_fast.so")


def both_builds(oracle, g, opts, **kw):
    assert os.path.exists(ORACLE_FAST), "the oracle's timing build (make -C oracle) is needed"
    a = F.oracle_run(oracle, g, opts, **kw)
    try:
        oracle.use_library(ORACLE_FAST)
        b = F.oracle_run(oracle, g, opts, **kw)
    finally:
        oracle.use_library(None)
    return a, b


@pytest.fixture(scope="module")
def golden_c2():
    return load_golden("c2")


@pytest.mark.parametrize("cid,recipe", F.PAIRS)
def test_recipe_meets_conditions_on_both_builds(oracle, golden_c2, cid, recipe):
    case = F.CASE_BY_ID[cid]
    g0 = case.problem(oracle, golden_c2)
    g, opts = case.apply(recipe, g0)
    a, b = both_builds(oracle, g, opts, **case.oracle_kw(g))
    bit, mixed, allowed = case.expect(recipe)
    ok, counts = F.conditions(a["status"], bit, mixed)
    w = F.written_columns(a["policy_x"])
    failed = a["status"] != 0
    steps = np.bincount(w[failed], minlength=case.h + 2).tolist()
    print(f"\n{cid} {recipe}: status counts {counts}, failures per restart {failed.sum(axis=0).tolist()}, "
          f"failed trajectories by policy columns written {steps}")
    np.testing.assert_array_equal(a["status"], b["status"])
    assert ok, counts
    assert set(counts) <= allowed, (counts, allowed)
    # a failed trajectory: NaN value, gradients and observations, and a NaN ETO row for its restart
    # (bit 16 comes from the adjoint, after the observations were written: they stay)
    in_loop = failed & ((a["status"] & 16) == 0)
    assert np.isnan(a["values"][failed]).all() and np.isnan(a["obs"][:, in_loop]).all()
    assert np.isnan(a["grad_x"][:, failed]).all() and np.isnan(a["grad_theta"][:, failed]).all()
    assert np.isfinite(a["values"][~failed]).all() and np.isfinite(a["obs"][:, ~in_loop]).all()
    np.testing.assert_array_equal(np.isnan(a["eto"]).all(axis=0), failed.any(axis=0))
    if (cid, recipe) in F.LAST_STEP:
        assert (w[failed] >= case.h).any(), steps


@pytest.mark.parametrize("cid", [c.id for c in F.CASES])
def test_plain_input_and_nan_filter_fail_nowhere(oracle, golden_c2, cid):
    case = F.CASE_BY_ID[cid]
    g0 = case.problem(oracle, golden_c2)
    a, b = both_builds(oracle, g0, {}, **case.oracle_kw(g0))
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    g, opts = F.nan_starts(g0, every=2)
    a, b = both_builds(oracle, g, opts, **case.oracle_kw(g))
    assert (a["status"] == 0).all() and (b["status"] == 0).all()


def test_singular_needs_both_settings(oracle, golden_c2):
    """sigma_tol = 10 with the default htol = 1e-4 zeroes the x-duals (det(H) < htol) and nothing
    fails; htol = −1 fails as htol = 0 does"""
    case = F.CASE_BY_ID["half_d2_n12"]
    g0 = case.problem(oracle, golden_c2)
    a = F.oracle_run(oracle, g0, dict(sigma_tol=10.0))
    assert (a["status"] == 0).all()
    z = F.oracle_run(oracle, *F.singular(g0, htol=0.0))
    n = F.oracle_run(oracle, *F.singular(g0, htol=-1.0))
    np.testing.assert_array_equal(z["status"], n["status"])
    assert (z["status"] == 16).sum() == 103


def test_every_dropped_pair_has_a_reason():
    for cid, recipe, why in F.DROPPED:
        assert recipe in F.RECIPES and len(why) > 20, (cid, recipe)
    assert len(F.PAIRS) + len(F.DROPPED) == len(F.CASES) * len(F.RECIPES)
