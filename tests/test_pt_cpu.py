"""The parallel-tempered sampler without a GPU: the host PTSampler's evidence on Gaussians of known normalisation, its swap
rule against a literal per-walker statement, the C ABI's new entries, and what the compiler made of the lf_pt_* kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import lf_isalib
from lumfuncmcmc_amd import capi
from lumfuncmcmc_amd.philox import draw, u53
from lumfuncmcmc_amd.sampler import PTSampler, default_ntemps, ti_log_evidence, tmax_from_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lfmcmc.h")
PT_NAMES = ("lf_ptsampler_create", "lf_ptsampler_destroy", "lf_ptsampler_start", "lf_ptsampler_run", "lf_ptsampler_read",
            "lf_ptsampler_steps")


def gaussian(d, sigma=0.01):
    mu = np.linspace(0.4, 0.6, d)

    def ll(x):
        x = np.asarray(x)
        inside = np.all((x > 0.0) & (x < 1.0), axis=1)
        return np.where(inside, -0.5 * np.sum(((x - mu) / sigma) ** 2, axis=1), -np.inf)

    return ll, d / 2.0 * np.log(2.0 * np.pi) + d * np.log(sigma)


@pytest.mark.parametrize("d", [2, 5])
def test_evidence_of_a_gaussian_in_the_unit_box(d):
    """lnZ = ln((2 pi)^(d/2) sigma^d) (the unit box's prior density is 1).  Ladder from the data (Tmax = 3.5e3 / 6.1e3,
    25 / 27 temperatures), 32 walkers, 400 steps, seed 1: |error| <= 0.2 nats, dlnZ <= 0.3 (seeds 1-3 gave errors of
    0.02-0.08 at d = 2 and 0.01-0.14 at d = 5, dlnZ <= 0.08)."""
    ll, exact = gaussian(d)
    Tmax = tmax_from_box(ll, np.array([[0.0, 1.0]] * d))
    T = default_ntemps(Tmax)
    s = PTSampler(T, 32, d, ll, Tmax=Tmax, seed=1)
    s.run_mcmc(np.random.default_rng(1).random((T, 32, d)), 400)
    lnZ, dlnZ = s.thermodynamic_integration_log_evidence()
    assert abs(lnZ - exact) <= 0.2, (lnZ, exact)
    assert dlnZ <= 0.3
    assert s.chain.shape == (T, 32, 400, d) and s.lnlikelihood.shape == (T, 32, 400)
    np.testing.assert_array_equal(s.lnprobability, s.betas[:, None, None] * s.lnlikelihood)
    assert s.acceptance_fraction.shape == (T, 32) and s.tswap_acceptance_fraction.shape == (T - 1,)
    assert np.all(s.tswap_acceptance_fraction > 0.3)
    assert s.acor.shape == (T, d)
    # the estimator on its own: exact for a likelihood whose mean does not depend on beta
    assert ti_log_evidence(s.betas, np.full((T, 10), -3.0))[0] == pytest.approx(-3.0, abs=1e-12)


def literal_pt(ll, betas, W, pos, nsteps, seed, a=2.0):
    """The sampler written walker by walker from its statement."""
    T, nd = len(betas), pos.shape[2]
    half = W // 2
    P, L = pos.copy(), np.array([[ll(pos[t, k][None])[0] for k in range(W)] for t in range(T)])
    nacc, nswap = np.zeros((T, W), dtype=np.int64), np.zeros(T - 1, dtype=np.int64)
    chain = np.empty((T, W, nsteps, nd))
    for s in range(nsteps):
        for h in (0, 1):
            props = {}
            for t in range(T):
                for w in range(half):
                    r = draw(s, h, [t * half + w], 0, seed)
                    z = ((a - 1.0) * u53(r[0], r[1])[0] + 1.0) ** 2 / a
                    j = (1 - h) * half + int((int(r[2][0]) * half) >> 32)
                    k = h * half + w
                    props[t, w] = (k, z, P[t, j] - (P[t, j] - P[t, k]) * z)
            newl = ll(np.array([props[t, w][2] for t in range(T) for w in range(half)]))
            for t in range(T):
                for w in range(half):
                    k, z, y = props[t, w]
                    q = draw(s, h, [t * half + w], 1, seed)
                    nl = newl[t * half + w]
                    with np.errstate(all="ignore"):
                        lnq = ((nd - 1.0) * np.log(z) + betas[t] * nl) - betas[t] * L[t, k]
                        if np.log(u53(q[0], q[1])[0]) < lnq and nl > -np.inf:
                            P[t, k], L[t, k] = y, nl
                            nacc[t, k] += 1
        for i in range(T - 1, 0, -1):
            r = [draw(s, 0, [i * W + k], 2, seed) for k in range(W)]
            order = sorted(range(W), key=lambda k: ((int(r[k][0][0]) << 32) | int(r[k][1][0]), k))
            for k in range(W):
                m = order[k]
                if np.log(u53(r[k][2], r[k][3])[0]) < (betas[i - 1] - betas[i]) * (L[i, k] - L[i - 1, m]):
                    P[i, k], P[i - 1, m] = P[i - 1, m].copy(), P[i, k].copy()
                    L[i, k], L[i - 1, m] = L[i - 1, m], L[i, k]
                    nswap[i - 1] += 1
        chain[:, :, s] = P
    return chain, nacc, nswap


def test_swaps_follow_the_stated_rule():
    ll, _ = gaussian(2, sigma=0.05)
    betas = np.array([1.0, 0.4, 0.1, 0.02])
    W, nsteps, seed = 8, 12, 0x0123456789ABCDEF
    pos = 0.4 + 0.2 * np.random.default_rng(5).random((4, W, 2))
    s = PTSampler(4, W, 2, ll, betas=betas, seed=seed)
    s.run_mcmc(pos, 5)
    s.run_mcmc(None, nsteps - 5)                                 # continuing = one longer run
    chain, nacc, nswap = literal_pt(ll, betas, W, pos, nsteps, seed)
    np.testing.assert_array_equal(s.chain, chain)
    np.testing.assert_array_equal(s.naccepted, nacc)
    np.testing.assert_array_equal(s.nswap, nswap)
    assert nswap.sum() > 0
    np.testing.assert_allclose(s.mean_lnlike, s.lnlikelihood.mean(axis=1), rtol=1e-15)


def test_a_single_temperature_is_the_plain_stretch_move():
    """T = 1 draws the ensemble sampler's numbers (stream 0 / 1, index w): the host replay of tests/test_gpu_sampler.py."""
    ll, _ = gaussian(3, sigma=0.05)
    W, seed = 10, 77
    pos = 0.4 + 0.2 * np.random.default_rng(6).random((1, W, 3))
    s = PTSampler(1, W, 3, ll, betas=[1.0], seed=seed)
    s.run_mcmc(pos, 6)
    chain, nacc, _ = literal_pt(ll, np.array([1.0]), W, pos, 6, seed)
    np.testing.assert_array_equal(s.chain, chain)
    np.testing.assert_array_equal(s.naccepted, nacc)
    assert s.nswap.shape == (0,)


def test_a_start_outside_the_box_is_refused():
    ll, _ = gaussian(2)
    s = PTSampler(2, 4, 2, ll, betas=[1.0, 0.5])
    pos = np.full((2, 4, 2), 0.5)
    pos[1, 2] = 2.0
    with pytest.raises(ValueError):
        s.run_mcmc(pos, 1)
    with pytest.raises(ValueError):
        PTSampler(2, 4, 2, ll, betas=[1.0, 1.0])


# ---------------------------------------------------------------------------------------------- the C ABI
def test_new_entries_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lf_[a-z_]+)\s*\(", src))
    for n in PT_NAMES:
        assert n in declared and n in capi.EXPORTS, n
    assert "typedef struct lf_ptsampler lf_ptsampler;" in src
    assert capi.LF_ABI_VERSION == 3


def test_load_rejects_a_library_that_lacks_an_entry(tmp_path, monkeypatch):
    """A library built from older sources has the same ABI version but not every entry: load() says to rebuild."""
    c = tmp_path / "stale.c"
    c.write_text("int lf_abi_version(void) { return %d; }\n" % capi.LF_ABI_VERSION)
    so = tmp_path / "libstale.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(c), "-o", str(so)], check=True)
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(so))
    with pytest.raises(RuntimeError, match="rebuild the library") as e:
        capi.load()
    assert "lf_ptsampler_create" in str(e.value)


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def test_pt_kernels_use_no_scratch_and_the_stated_lds(remarks):
    """no scratch in any lf_pt_* kernel; the swap kernel holds 4096 64-bit keys (32 KiB) and 64
    swap counters, the other two no LDS."""
    hits = {k: v for k, v in remarks.items() if k.startswith("_ZN2lf") and "lf_pt_" in k}
    names = {re.match(r"_ZN2lf\d+(lf_pt_\w+?)E", k).group(1) for k in hits}
    assert names == {"lf_pt_propose", "lf_pt_accept", "lf_pt_swap"}, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == (32 * 1024 + 64 * 4 if "lf_pt_swap" in k else 0), (k, r)
