"""mapfit.py (maximise, hessian, laplace_evidence) without a GPU: on a Gaussian with known mean and precision, and on the
NumPy twin of the device gradient (lumfuncmcmc_amd/grad.py) for a free-completeness and a z-evolving catalogue."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd import grad as G
from lumfuncmcmc_amd import mapfit

D = 4
BOX = np.array([[-1.0, 1.0], [-2.0, 1.0], [0.0, 3.0], [-1.0, 2.0]])
MU = np.array([0.3, -0.7, 1.9, 0.4])


def gaussian(mu, P, lnp0=-3.25):
    calls = []

    def f(th):
        th = np.atleast_2d(th)
        calls.append(len(th))
        d = th - mu
        return lnp0 - 0.5 * np.einsum("ki,ij,kj->k", d, P, d), -d @ P
    f.calls = calls
    return f


def precision(seed=0, scale=40.0):
    A = np.random.default_rng(seed).normal(size=(D, D))
    return scale * (A @ A.T + D * np.eye(D))


def test_gaussian_maximum_hessian_and_evidence():
    P = precision()
    f = gaussian(MU, P)
    starts = np.random.default_rng(1).uniform(BOX[:, 0], BOX[:, 1], (8, D))
    r = mapfit.maximise(f, BOX, starts, tol=1e-6)
    assert r["converged"] and not r["on_bound"].any()
    assert np.max(np.abs(r["theta"] - MU)) <= 1e-8
    assert len(f.calls) == r["niter"] + 1                 # one batched call per iteration, and the first
    H = mapfit.hessian(f, r["theta"], BOX)
    assert np.array_equal(H, H.T)
    assert np.max(np.abs(H + P)) <= 1e-7 * np.max(np.abs(P))      # (a linear gradient: only the rounding term of the step argument)
    assert np.max(np.abs(H + P) / np.abs(P)) <= 1e-7
    lnZ, why = mapfit.laplace_evidence(r["lnprob"], H, BOX)
    exact = -3.25 + 0.5 * D * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(P)[1] - np.sum(np.log(BOX[:, 1] - BOX[:, 0]))
    assert why == "" and abs(lnZ - exact) <= 1e-10


def test_hessian_is_one_call_of_2_ndim_rows_inside_the_box():
    f = gaussian(MU, precision())
    x = np.array([0.99999, -0.7, 1.9, 0.4])               # closer to its bound than the default step
    rows, plus, minus = mapfit.stencil(x, BOX)
    assert rows.shape == (2 * D, D) and np.all(rows >= BOX[:, 0]) and np.all(rows <= BOX[:, 1])
    assert plus[0] == pytest.approx(0.5e-5) and plus[1] == pytest.approx(3e-4)
    mapfit.hessian(f, x, BOX)
    assert f.calls == [2 * D]


def test_maximum_on_a_bound():
    mu = MU.copy()
    mu[2] = 3.5                                            # the mean lies outside the box: the maximum sits on hi_2
    P = precision(3)
    f = gaussian(mu, P)
    starts = np.random.default_rng(4).uniform(BOX[:, 0], BOX[:, 1], (8, D))
    r = mapfit.maximise(f, BOX, starts)
    assert r["converged"] and r["on_bound"].tolist() == [False, False, True, False] and r["theta"][2] == 3.0
    # the constrained maximum of the quadratic over the free coordinates
    fr = ~r["on_bound"]
    want = mu[fr] - np.linalg.solve(P[np.ix_(fr, fr)], P[np.ix_(fr, ~fr)] @ (r["theta"][~fr] - mu[~fr]))
    assert np.max(np.abs(r["theta"][fr] - want)) <= 1e-8
    lnZ, why = mapfit.laplace_evidence(r["lnprob"], r["hessian"], BOX, on_bound=r["on_bound"])
    assert np.isnan(lnZ) and "bound" in why


def test_indefinite_hessian_gives_nan():
    H = -np.diag([1.0, 2.0, -0.5, 3.0])
    lnZ, why = mapfit.laplace_evidence(0.0, H, BOX)
    assert np.isnan(lnZ) and "positive definite" in why
    assert mapfit.newton_decrement(np.ones(D), H) == np.inf


def theta_box(inp):
    L = inp["lims"]
    nf = len(inp["field_ind"]) - 1
    if inp["variant"] == "zevol":
        rows = [L["Lstar"]] * 3 + [L["phistar"]] * 3 + [L["sch_al"]]
    else:
        rows = [L["Lstar"], L["phistar"], L["sch_al"]] + [L["Flim"]] * nf + [L["alpha"]]
    return np.array(rows, dtype=np.float64)


def truth(inp):
    nf = len(inp["field_ind"]) - 1
    if inp["variant"] == "zevol":
        return np.array([synth.LSTAR] * 3 + [synth.PHISTAR] * 3 + [synth.SCH_AL])
    return np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL] + list(synth.FLIM[:nf]) + [synth.ALPHA_C])


@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_maximise_with_the_twin(variant):
    tol = 1e-6
    inp = make_inputs(variant, 300, S=21)
    box = theta_box(inp)
    f = lambda t: G.lnprob_grad(inp, t)          # noqa: E731
    # 8 starts from the prior box (a draw whose lnprob is -inf is drawn again, as fit_model_map does)
    rng = np.random.default_rng(12)
    starts = rng.uniform(box[:, 0], box[:, 1], (8, len(box)))
    for _ in range(100):
        bad = ~np.isfinite(f(starts)[0])
        if not bad.any():
            break
        starts[bad] = rng.uniform(box[:, 0], box[:, 1], (int(bad.sum()), len(box)))
    lp0 = f(starts)[0]
    # (the z-evolving prior excludes its bounds: the iteration works a hair inside them, as fit_model_map has it)
    r = mapfit.maximise(f, box, starts, tol=tol, inset=1e-9 if variant == "zevol" else 0.0)
    assert r["converged"], r
    free = ~r["on_bound"]
    H = mapfit.hessian(f, r["theta"], r["box"])
    dec = mapfit.newton_decrement(r["grad"], H, free)
    print("twin MAP %s: lnprob %.4f niter %d decrement %.2e on_bound %s" % (variant, r["lnprob"], r["niter"], dec, r["on_bound"].tolist()))
    assert dec <= tol
    assert np.linalg.eigvalsh(-H[np.ix_(free, free)])[0] > 0          # -H positive definite (where the box does not hold theta)
    assert np.all(r["lnprob"] >= lp0)
    assert r["lnprob"] >= f(truth(inp))[0]
