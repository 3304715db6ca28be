"""Full-size GPU-vs-oracle parity and the multi-rank exchange on the device.

The Julia reference cannot run here (no julia, no golden vectors in the reference), so parity
against it is unpinned; the oracle (oracle/rbo_oracle.c, a line-by-line C restatement pinned by
the NumPy goldens, scipy's Sobol and finite differences) stands in, and these tests hold the GPU
to it EXHAUSTIVELY at the headline size and per full restart of the other configurations.
The tolerances, the non-vacuity guard and the statistics recorded per case are defined in
tests/parity.py; $MRBO_PARITY_REPORT names the JSON file the statistics of every case go to.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from parity import _REPORT, _end_to_end, _osur, _plan, _problem_arrays, _run

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("MRBO_PARITY_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


def test_full_size_c3_vs_oracle(gpu, oracle):
    """The headline launch, exhaustively: all 65 536 C3 trajectories (1 024 MC × 64 restarts)."""
    g = _problem_arrays("C3", 1024, 64)
    _end_to_end(oracle, "C3 full (1024 x 64, l=1)", g, 1024)


@pytest.mark.parametrize("name,M,R,kind", [("C1", 32, 4, "forward"), ("C2", 256, 16, "full")])
def test_full_size_c1_c2_vs_oracle(gpu, oracle, name, M, R, kind):
    """BASELINE's configurations 0 and 1 at their full launch sizes, exhaustively: C1 (32 MC × 4
    restarts; d = 1, where every inner maximum meets the reference's det(H) < 1e-4 test, Q4, so its
    adjoint zeroes the x-duals and the case is forward-only) and C2 (256 × 16, the whole launch)."""
    g = _problem_arrays(name, M, R)
    _end_to_end(oracle, f"{name} full ({M} x {R}, l=1, {kind})", g, M, kind=kind)


def _mle_arrays(name, M, R):
    """base data of `name` with the lengthscale fitted by optimize! (radial_basis_surrogates.jl:805-829,
    bounds [0.1, 5] as nonmyopic_bayesopt.jl:230) on the device"""
    from mrbo import configs
    from mrbo.mle import optimize
    pb = configs.problem(name, M=M, R=R)
    res = optimize(pb.surrogate, [0.1], [5.0])
    ell = float(res["theta"][0])
    return _problem_arrays(name, M, R, ell=ell), ell


# (config, restarts, lengthscale, kind, htol).  At ℓ = 1 Hartmann-6 at N = 128 never improves on
# fmini (every C4 value is 0) and C4's MLE ℓ barely does, so C4 runs at ℓ = 0.5 (94 % non-zero
# values, the N = 128 resolution and adjoint at scale) and its MLE case is forward-only.  At C5
# the reference's det(H) < 1e-4 test (Q4, rollout.jl:159-161) zeroes almost every x-dual at
# d = 8; ℓ = 1 is therefore forward-only, and the Q4-off diagnostic (htol = -∞ on both sides,
# not the reference's behaviour) runs the d = 8 back-substitution on real x-duals.
RESTART_CASES = [("C4", 1, 0.5, "full", 1e-4), ("C4", 1, "mle", "forward", 1e-4), ("C5", 1, None, "forward", 1e-4),
                 ("C5", 1, 20.0, "full", 1e-4), ("C5", 1, 20.0, "full", -np.inf), ("C3", 4, "mle", "full", 1e-4)]


@pytest.mark.parametrize("name,R,ell,kind,htol", RESTART_CASES)
def test_full_restart_vs_oracle(gpu, oracle, name, R, ell, kind, htol):
    """One full restart (1 024 MC samples) of C4 and C5, C5 also at a lengthscale at its design
    spacing (ℓ = 20: its MLE within the reference's bounds stays at ℓ = 1, the likelihood being
    flat there), and C3 / C4 at their MLE lengthscales -- surfaces where the Newton solve and the
    adjoint do real work (see RESTART_CASES)."""
    if ell == "mle":
        g, ell_v = _mle_arrays(name, 1024, R)
    else:
        g, ell_v = _problem_arrays(name, 1024, R, ell=ell), (ell or 1.0)
    q4 = "" if htol == 1e-4 else ", Q4 off"
    st = _end_to_end(oracle, f"{name} restart (1024 x {R}, l={ell_v:.4g}{q4}, {kind})", g, 1024, kind=kind, htol=htol,
                     work_exact="steps" if name == "C4" else True, envelope=name == "C4")
    if htol != 1e-4:    # the diagnostic's purpose: the d = 8 adjoint on non-zero x-duals
        assert st["coverage"]["nonzero_grads"] >= 0.5, st


@pytest.mark.parametrize("name,M,R,ell", [("C2", 64, 4, None), ("C3", 64, 4, None), ("C4", 16, 2, 0.5),
                                          ("C5", 16, 1, 20.0)])
@pytest.mark.parametrize("kind", ["quadratic", "loglinear"])
def test_cost_weighted_vs_oracle(gpu, oracle, name, M, R, ell, kind):
    """NonUniformCost (cost_functions.jl:5-20; the build's α/c(x) inner-solve rule, parity unpinned
    against Julia): the weighted primitives at base points, then full rollouts with the inner solves
    and the adjoint on both sides, same T2 / T3 bars as the unweighted rule."""
    g = _problem_arrays(name, M, R, ell=ell)
    d = g["X"].shape[0]
    w = np.linspace(0.5, 1.5, d)
    cost = (kind, 1.0, w)
    opts = dict(cost=kind, cost_c0=1.0, cost_w=tuple(w))
    p = _plan(g, **opts)
    pts = np.asfortranarray(g["xstarts"][:, :8] * 0.9 + 0.05 * g["x0s"][:, :1])
    np.testing.assert_allclose(p.eval_base(pts), oracle.eval_base(_osur(oracle, g), pts, cost=cost, lbs=g["lbs"],
                                                                  ubs=g["ubs"]), rtol=1e-9, atol=1e-12)
    # C4 at ℓ = 0.5 runs ≈ 500 Newton steps per trajectory: its Newton decisions can differ by
    # rounding on identical paths, so per-trajectory work is held to within 3 Newton steps, beside
    # the oracle's two builds' own disagreement (tests/parity.py "steps", envelope)
    _end_to_end(oracle, f"{name} cost={kind} ({M} x {R})", g, M, cost=cost, plan_opts=opts,
                work_exact="steps" if name == "C4" else True, envelope=name == "C4")


@pytest.mark.parametrize("name,M,R", [("C3", 1024, 4), ("C5", 64, 2)])
def test_cost_weighted_bench_surfaces_vs_oracle(gpu, oracle, name, M, R):
    """The NonUniformCost surfaces the bench rows run (bench.py --cost: configs.C5_COST, the
    quadratic family c = 1 + Σ_a u_a², at the config's own ℓ = 1): C3 at 1 024 MC × 4 restarts and
    C5 at 64 × 2, full rollouts + adjoint on both sides under the T2 / T3 bars.  C5 + cost
    resolves at ℓ = 1 (every value non-zero, 90 % of best observations at a fantasy step), but the
    d = 8 x-duals meet Q4 (det(H) < 1e-4), so no adjoint pair runs: kind "forward", as unweighted C5
    at ℓ = 1.  Its ≈ 800 Newton steps per trajectory on the flat α/c make it a rounding-sensitive
    surface: the oracle's two builds flip on 4 of its 128 trajectories, so flips are bounded by
    twice that and identical paths by the 3-Newton-step work rule (tests/parity.py)."""
    from mrbo import configs
    g = _problem_arrays(name, M, R)
    d = g["X"].shape[0]
    pb = configs.problem(name, M=M, R=R, cost=True)
    opts = pb.plan_opts()
    assert opts["cost"] == "quadratic" and opts["cost_c0"] == 1.0, opts
    cost = ("quadratic", float(opts["cost_c0"]), np.asarray(opts["cost_w"], dtype=np.float64))
    c5 = name == "C5"
    _end_to_end(oracle, f"{name} bench cost=quadratic ({M} x {R}, l=1)", g, M, cost=cost, plan_opts=opts,
                kind="forward" if c5 else "full", work_exact="steps" if c5 else True, envelope=c5)


def test_device_moments_merge_equals_eto_reduce(gpu):
    """mrbo_partial_moments over MC shards + Chan merge (the multi-GPU exchange) == mrbo_eto_reduce
    over the whole launch (two-pass mean / std(n-1), rollout.jl:328-337)."""
    import torch
    from mrbo.parallel import eto_from_moments, merge_moments, width
    g = _problem_arrays("C2", 96, 4)
    p = _plan(g)
    r = _run(p, g, want_policy=False)
    d, M, R = p.d, p.M, p.R
    parts = []
    for lo, hi in [(0, 17), (17, 60), (60, 96)]:
        gg = dict(g)
        gg["rnstream"] = np.asfortranarray(g["rnstream"][lo:hi])
        q = _plan(gg, M=hi - lo, sample_offset=lo, samples_total=M)
        out = q.alloc_outputs(with_gradient=True)
        from mrbo.engine import to_device
        q.simulate(to_device(gg["x0s"], "cuda:0"), to_device(gg["rnstream"], "cuda:0"), to_device(gg["xstarts"], "cuda:0"),
                   out)
        mom = q.partial_moments(out, hi - lo)
        torch.cuda.synchronize()
        parts.append((hi - lo, mom.cpu().numpy().reshape((width(d), R), order="F")))
    n, merged = merge_moments(parts, d)
    e = eto_from_moments(merged, n, d)
    np.testing.assert_allclose(e, r["eto"], rtol=1e-12, atol=1e-16)
    with pytest.raises(Exception):     # M_local outside [1, M]
        q.partial_moments(out, M + 5)
    # M_local < the plan's M: the first M_local samples of every restart (the outputs keep the
    # plan's M as the restart stride)
    Mq, ml = hi - lo, 7
    mom = q.partial_moments(out, ml)
    torch.cuda.synchronize()
    mom = mom.cpu().numpy().reshape((width(d), R), order="F")
    vals = out["values"].cpu().numpy().reshape((Mq, R), order="F")[:ml]
    gx = out["grad_x"].cpu().numpy().reshape((d, Mq, R), order="F")[:, :ml]
    np.testing.assert_allclose(mom[0], vals.sum(0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(mom[1], ((vals - vals.mean(0)) ** 2).sum(0), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(mom[2:2 + d], gx.sum(1), rtol=1e-10, atol=1e-14)


def test_merge_moments_on_device_equals_host_merge(gpu):
    """mrbo_merge_moments (the exchange's Chan merge + ETO on the device) equals the host
    restatement mrbo/parallel.py merge_moments + eto_from_moments bit for bit: same operations, same
    order, no contraction.  Shards of unequal size, one empty shard, mean ≫ spread (the case a
    one-pass formula loses), and the one-sample NaN std (Q14)."""
    import torch
    from mrbo import configs
    from mrbo.parallel import eto_from_moments, local_moments, merge_moments, width
    from mrbo.rollout import _plan_for
    cfg = configs.CONFIGS["C2"]
    pb = configs.problem("C2", M=16, R=3)
    d, R = cfg.d, 3
    plan = _plan_for(pb.T.s, cfg.h, 16, R, pb.es.get_starts().shape[1], pb.lbs, pb.ubs, pb.T.θ[0], 0, pb.plan_opts())
    rng = np.random.default_rng(3)
    for sizes in ([5, 0, 11, 3], [1], [7, 9]):
        parts = []
        for n in sizes:
            if n == 0:
                parts.append((0, np.full((width(d), R), np.nan)))     # never read
                continue
            v = 1e6 + rng.normal(size=(n, R))
            gx = rng.normal(size=(d, n, R)) * 1e-3 + 5.0
            gt = rng.normal(size=(n, R))
            parts.append((n, local_moments(v, gx, gt)))
        ntot, merged = merge_moments(parts, d)
        host = eto_from_moments(merged, ntot, d)
        flat = np.concatenate([b.ravel(order="F") for _, b in parts])
        dev = plan.merge_moments(torch.from_numpy(flat).to("cuda:0"), [n for n, _ in parts])
        torch.cuda.synchronize()
        got = dev.cpu().numpy().reshape((width(d), R), order="F")
        np.testing.assert_array_equal(np.isnan(got), np.isnan(host))
        np.testing.assert_array_equal(got[~np.isnan(got)], host[~np.isnan(host)])
    with pytest.raises(Exception):
        plan.merge_moments(torch.zeros(width(d) * R, dtype=torch.float64, device="cuda:0"), [0])


def _bench(args, env, timeout=110):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_sharded_rccl_one_rank_matches_plain(gpu, tmp_path):
    """`bench.py --sharded` at one rank runs the multi-rank path over RCCL (backend nccl: a
    process group, the per-step all-gather of the shard moments as device tensors, the Chan merge
    and ETO on the device (mrbo_merge_moments), the device SGA step, the MAX all-reduce of the
    clock) -- the exchange the 8-GPU run uses, on the one-GPU box.  Its ETO, x0 and stop flags
    equal the plain run's (device ETO + device SGA)."""
    common = ["--steps", "2", "--warmup", "1", "--restarts", "4", "--no-cpu-baseline", "--config", "C2",
              "--mc-per-gpu", "64", "--eta", "0.5"]
    env = {k: v for k, v in os.environ.items() if k != "MRBO_DIST_BACKEND"}
    sh = _bench(common + ["--sharded", "--dump", str(tmp_path / "sh.npz")], env)
    one = _bench(common + ["--dump", str(tmp_path / "one.npz")], env)
    assert sh["n_gpus"] == one["n_gpus"] == 1
    assert sh["config"]["exchange"].startswith("all-gather") and one["config"]["exchange"] == "none"
    a, b = np.load(tmp_path / "sh.npz"), np.load(tmp_path / "one.npz")
    np.testing.assert_allclose(a["eto"], b["eto"], rtol=1e-12, atol=1e-16)
    np.testing.assert_array_equal(a["active"], b["active"])
    np.testing.assert_allclose(a["x0"], b["x0"], rtol=1e-14)


def test_bench_plain_run_dumps_its_last_step_and_repeats(gpu, tmp_path):
    """A plain `bench.py` run (no --full) times exactly --steps steps, reports `ms_per_step` and
    carries no CPU baseline; --dump-outputs writes the last timed step's arrays as float64 .npy
    files, the ETO rows and x0 among them equal to what --dump records, and a second run with the
    same arguments writes the same arrays bit for bit."""
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--restarts", "4", "--config", "C2", "--mc-per-gpu", "64",
              "--eta", "0.5"]
    env = {k: v for k, v in os.environ.items() if k != "MRBO_DIST_BACKEND"}
    a = _bench(common + ["--dump-outputs", str(tmp_path / "a"), "--dump", str(tmp_path / "a.npz")], env)
    b = _bench(common + ["--dump-outputs", str(tmp_path / "b")], env)
    for res in (a, b):
        assert res["steps"] == 2 and res["ms_per_step"] > 0 and "cpu_baseline" not in res
        assert res["unit"] == "trajectories/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
        np.testing.assert_allclose(res["value"], 64 * 4 / (res["ms_per_step"] * 1e-3), rtol=1e-9)
    T, d = 64 * 4, 2
    shapes = dict(values=(T,), status=(T,), grad_x=(d * T,), grad_theta=(T,), evals=(5 * T,), x0=(d, 4), active=(4,))
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(list(shapes) + ["eto"])
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float64 and (n == "eto" or x.shape == shapes[n])
        np.testing.assert_array_equal(x, y)
    assert np.abs(np.load(tmp_path / "a" / "grad_x.npy")).max() > 0      # a launch's results, not zeros
    z = np.load(tmp_path / "a.npz")
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "eto.npy"), z["eto"])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "x0.npy"), z["x0"])


def test_bench_two_ranks_rehearsal_matches_one_rank(gpu, tmp_path):
    """`bench.py --gpus 2` starts its two ranks itself (torch.distributed.run) and exchanges the
    per-restart moments once per step; rehearsed on one GPU over gloo (MRBO_DIST_BACKEND=gloo, both
    ranks on cuda:0).  Its ETO equals the one-rank run over the same 2·M samples."""
    env = dict(os.environ, MRBO_DIST_BACKEND="gloo")
    common = ["--steps", "1", "--warmup", "0", "--restarts", "4", "--no-cpu-baseline", "--config", "C2"]
    two = _bench(["--gpus", "2", "--mc-per-gpu", "32", "--dump", str(tmp_path / "two.npz")] + common, env)
    one = _bench(["--gpus", "1", "--mc-per-gpu", "64", "--dump", str(tmp_path / "one.npz")] + common, dict(os.environ))
    assert two["n_gpus"] == 2 and two["config"]["parallelism"] == "mc-shard x2"
    assert two["config"]["trajectories_per_step"] == one["config"]["trajectories_per_step"] == 64 * 4
    a, b = np.load(tmp_path / "two.npz"), np.load(tmp_path / "one.npz")
    np.testing.assert_allclose(a["eto"], b["eto"], rtol=1e-12, atol=1e-16)
    np.testing.assert_array_equal(a["active"], b["active"])
    np.testing.assert_allclose(a["x0"], b["x0"], rtol=1e-14)


def test_bench_eight_ranks_rehearsal_matches_one_rank(gpu, tmp_path):
    """The 8-GPU node's launch path, rehearsed on the one-GPU box: `bench.py --gpus 8` starts its
    eight ranks (torch.distributed.run), each on cuda:0 (device wrap-around) over gloo
    (MRBO_DIST_BACKEND=gloo; RCCL refuses two ranks on one device), at C4's per-GPU shape (d = 6,
    h = 4, N = 128 -- the rows-per-lane-2 kernel) with 8 MC samples per rank × 4 restarts at
    ℓ = 0.5 (C4 at ℓ = 1 resolves nothing): one step -- the launch, the exchange of the shard
    moments, the merge and the SGA update.  The ETO, x0 and stop flags equal a one-rank run over
    the same 8·8 samples.  (One step: the merged ETO differs from the one-pass reduction in the last
    bits, and a second launch from x0 moved by those bits runs ≈ 500-step Newton paths at ℓ = 0.5
    that amplify them to ≈ 3e-11, measured.)"""
    env = dict(os.environ, MRBO_DIST_BACKEND="gloo")
    common = ["--steps", "1", "--warmup", "0", "--restarts", "4", "--no-cpu-baseline", "--config", "C4",
              "--ell", "0.5", "--eta", "0.5"]
    eight = _bench(["--gpus", "8", "--mc-per-gpu", "8", "--dump", str(tmp_path / "eight.npz")] + common, env,
                   timeout=240)
    one = _bench(["--gpus", "1", "--mc-per-gpu", "64", "--dump", str(tmp_path / "one.npz")] + common,
                 dict(os.environ))
    assert eight["n_gpus"] == 8 and eight["config"]["parallelism"] == "mc-shard x8"
    assert eight["config"]["trajectories_per_step"] == one["config"]["trajectories_per_step"] == 64 * 4
    a, b = np.load(tmp_path / "eight.npz"), np.load(tmp_path / "one.npz")
    assert np.abs(b["eto"]).max() > 0                      # not the degenerate ℓ = 1 surface
    np.testing.assert_allclose(a["eto"], b["eto"], rtol=1e-12, atol=1e-16)
    np.testing.assert_array_equal(a["active"], b["active"])
    np.testing.assert_allclose(a["x0"], b["x0"], rtol=1e-14)
