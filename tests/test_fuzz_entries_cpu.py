"""The ragged cases of tests/lf_fuzzlib.py without a GPU: that the set holds the layouts it is there for, that the NumPy twins the
device is compared with (grad.py, deconv.py with wide=True) take every one of them, and that the device checks of
tests/test_gpu_fuzz_entries.py would notice the host mistakes they are there for - a wrong field of one source, two caller
indices swapped, a chunk one source short - at the standing bound of 1e-12 on the twins' own scales."""
import functools
import time

import numpy as np
import pytest

import lf_fuzzlib as F
from lf_testlib import O
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G

CASES = F.all_params()
IDS = F.case_ids()


@functools.lru_cache(maxsize=None)
def refs(i):
    """the case and every twin's result on it, computed once"""
    inp, th, sg, K, label = F.build(**CASES[i])
    t0 = time.perf_counter()
    r = {"case": (inp, th, sg, K, label), "oracle": O.lnprob_batch(inp, th)}
    r["lp"], r["g"], r["s"] = G.lnprob_grad(inp, th, terms=True)
    r["tot"], r["Di"], r["sabs"] = D.delta(inp, sg, th, K=K, terms=True, wide=True)
    r["val"], r["ge"], r["se"] = D.lnprob_err_grad(inp, sg, th, K=K, terms=True, wide=True)
    r["m1"], r["m2"], r["used"], r["s1"] = D.lum_posterior(inp, sg, th, K=K, wide=True, terms=True)
    print("%s: twins %.2f s" % (label, time.perf_counter() - t0))
    return r


def test_coverage():
    """a condition on the inputs: a missing layout or law is mended in the seeds or the forced list, never here"""
    seen, laws = set(), set()
    for p in CASES:
        inp, th, sg, K, _ = F.build(**p)
        n, nf = len(inp["lum"]), len(inp["field_ind"]) - 1
        assert n >= 1 and 1 <= nf <= 8 and 1 <= len(th) <= 37 and (n <= F.BIG_N or len(th) <= F.BIG_B)
        assert np.all(sg >= 0.0) and np.all(sg <= D.WIDE_SIGMA_MAX)
        facts = F.facts(inp, sg, K)
        seen |= {k for k, v in facts.items() if v}
        laws.add((p["variant"], p["law"]))
        cls = D.wide_class(sg, K)
        want = {"mixed": n < 10 or ((sg == 0.0).any() and (cls >= 0).any() and ((cls < 0) & (sg > 0.0)).any()),
                "narrow": np.all(cls < 0) and (sg > 0.0).any(), "wide": np.all(cls >= 0) and np.all(sg > D.SIGMA_MAX),
                "zero": not sg.any(), "one": np.count_nonzero(sg) == 1}
        assert want[p["law"]], (p["label"], p["law"])
    missing = set(facts) - seen
    assert not missing, "no case with: %s" % sorted(missing)
    assert laws == {(v, l) for v in F.VARIANTS for l in F.LAWS}, sorted({(v, l) for v in F.VARIANTS for l in F.LAWS} - laws)
    assert len(F.sampler_params()) == 4 and {p["variant"] for p in F.sampler_params()} == set(F.VARIANTS)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_references(i):
    """the twins return; the -inf pattern of the plain value is the oracle's; the correction, the convolved gradient and the
    per-source posterior are finite on every finite row and for every source with sigma > 0, exactly 0 for the others"""
    r = refs(i)
    inp, th, sg, K, label = r["case"]
    ref, fin = r["oracle"], np.isfinite(r["oracle"])
    assert not np.isnan(ref).any() and np.array_equal(np.isneginf(r["lp"]), np.isneginf(ref)) and not np.isnan(r["lp"]).any(), label
    assert np.all(np.isfinite(r["g"][fin])) and np.all(np.isnan(r["g"][~fin])), label
    assert np.all(np.isfinite(r["tot"][fin])) and np.all(np.isfinite(r["Di"][fin])) and np.all(r["Di"][:, sg == 0.0] == 0.0), label
    assert np.array_equal(np.isfinite(r["val"]), fin) and np.all(r["val"][~fin] == -np.inf), label
    assert np.all(np.isfinite(r["ge"][fin])) and np.all(np.isfinite(r["se"][fin])) and np.all(np.isnan(r["ge"][~fin])), label
    assert r["used"] == int(fin.sum()), label
    on = sg > 0.0
    assert np.all(r["m1"][~on] == 0.0) and np.all(r["m2"][~on] == 0.0), label
    if r["used"]:
        assert np.all(np.isfinite(r["m1"][on])) and np.all(r["m2"][on] > 0.0) and np.all(r["s1"][on] > 0.0), label
    else:
        assert np.all(np.isnan(r["m1"][on])) and np.all(np.isnan(r["m2"][on])), label


def _ratio(err, scale):
    """max err / scale where scale > 0 (an element without contributions must agree exactly: any difference there counts as inf)"""
    err, scale = np.asarray(err, dtype=float), np.asarray(scale, dtype=float)
    if err.size == 0:
        return 0.0
    if np.any(err[scale == 0.0] != 0.0):
        return np.inf
    return float(np.max(np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), 0.0)))


def test_a_source_in_the_wrong_field_exceeds_every_bound():
    """field_ind shifted by one source at a boundary with a source behind it (what a wrong chunk_field, or a chunk that starts one
    source early across an empty field, does to that source): the plain gradient (FREE: the source reads another Flim), the
    convolved value and gradient and the per-source posterior of the shifted twin leave the right twin's bound"""
    hits = {(k, v): 0 for k in ("grad", "value", "err_grad", "lum_posterior") for v in F.VARIANTS}
    tried = 0
    for i, p in enumerate(CASES):
        if sum(p["sizes"]) > 300:                  # (two more runs of every twin: the small cases, every variant among them)
            continue
        r = refs(i)
        inp, th, sg, K, label = r["case"]
        fi = np.asarray(inp["field_ind"])
        fin = np.isfinite(r["lp"])
        at = [f for f in range(1, len(fi) - 1) if fi[f] < fi[f + 1] and sg[fi[f]] > 0.0]      # (the source that moves has sigma > 0)
        if not at or not fin.any():
            continue
        tried += 1
        bad = dict(inp)
        bad["field_ind"] = fi.copy()
        bad["field_ind"][at[0]] += 1
        lp, g, _ = G.lnprob_grad(bad, th, terms=True)
        tot = D.delta(bad, sg, th, K=K, wide=True)
        val, ge = D.lnprob_err_grad(bad, sg, th, K=K, wide=True)
        m1, m2, used = D.lum_posterior(bad, sg, th, K=K, wide=True)
        fin2 = fin & np.isfinite(lp)
        w = {"grad": _ratio(np.abs(g - r["g"])[fin2], r["s"][fin2]),
             "value": _ratio(np.abs((lp[fin2] + tot[fin2]) - (r["lp"] + r["tot"])[fin2]), (np.abs(r["lp"]) + r["sabs"])[fin2]),
             "err_grad": _ratio(np.abs(ge - r["ge"])[fin2], r["se"][fin2]),
             "lum_posterior": _ratio(np.abs(m1 - r["m1"])[sg > 0.0], r["s1"][sg > 0.0]) if used == r["used"] else np.inf}
        print("%s: boundary %d shifted, |wrong - right| / bound = %s" % (label, at[0], {k: "%.2e" % (v / F.TOL) for k, v in w.items()}))
        if inp["variant"] != "free":
            assert w["grad"] == 0.0                # (fixed completeness: the plain lnprob does not read field_ind)
        for k in w:
            hits[k, inp["variant"]] += w[k] > F.TOL
    print("cases tried %d, beyond the bound: %s" % (tried, hits))
    # (a bright source's completeness is 1 under either field's limit: not every case can tell, one of every variant must)
    assert tried >= 5 and all(n >= 1 for (k, v), n in hits.items() if k != "grad" or v == "free"), hits


def test_two_caller_indices_swapped_exceed_the_posterior_bound():
    """lum_posterior's result with the entries of two sources exchanged, one of them with sigma > 0 (a slot or caller mix-up in
    the fold): outside the bound of `check` in tests/test_gpu_lumpost.py - an entry off its twin by more than 1e-12 s1_abs, or a
    source with sigma = 0 that is not exactly 0"""
    tried = hits = 0
    for i in range(len(CASES)):
        r = refs(i)
        inp, th, sg, K, label = r["case"]
        on = np.flatnonzero(sg > 0.0)
        if r["used"] == 0 or on.size == 0 or len(sg) < 2:
            continue
        tried += 1
        a = int(on[0])
        b = int(on[-1]) if on.size > 1 else (a + 1) % len(sg)
        m1, m2 = r["m1"].copy(), r["m2"].copy()
        m1[[a, b]], m2[[a, b]] = m1[[b, a]], m2[[b, a]]
        off = sg == 0.0
        zeros = bool(np.all(m1[off] == 0.0) and np.all(m2[off] == 0.0))
        w1 = _ratio(np.abs(m1 - r["m1"])[~off], r["s1"][~off])
        w2 = _ratio(np.abs(m2 - r["m2"])[~off], r["m2"][~off])
        hits += (not zeros) or w1 > F.TOL or w2 > F.TOL
    print("cases tried %d, beyond the bound %d" % (tried, hits))
    assert tried >= 20 and hits == tried


def test_a_chunk_one_source_short_exceeds_the_value_bound():
    """Delta without the last source of one chunk - a narrow chunk (CHUNK sources of a field) and a wide one (WIDE_CHUNK sources of
    a field and class), taken in catalogue order: the context sorts a field's sources, so the device's last source is another one
    of the same field, with a term of the same size: outside |dev - (lnprob + Delta)| <= 1e-12 (|lnprob| + sum_i |Delta_i|)"""
    tried = {"narrow": 0, "wide": 0}
    hits = {"narrow": 0, "wide": 0}
    for i in range(len(CASES)):
        r = refs(i)
        inp, th, sg, K, label = r["case"]
        fi = np.asarray(inp["field_ind"])
        fin = np.isfinite(r["lp"])
        if not fin.any():
            continue
        cls = D.wide_class(sg, K)
        last = {}
        for f in range(len(fi) - 1):
            for c, ch in [(-1, D.CHUNK)] + [(k, D.WIDE_CHUNK) for k in range(len(D.WIDE_EDGES))]:
                idx = fi[f] + np.flatnonzero((cls[fi[f]:fi[f + 1]] == c) & (sg[fi[f]:fi[f + 1]] > 0.0)) if c >= 0 else np.arange(fi[f], fi[f + 1])
                ends = [int(idx[min(s + ch, len(idx)) - 1]) for s in range(0, len(idx), ch)]
                ends = [e for e in ends if sg[e] > 0.0 and cls[e] == c]
                if ends:
                    last.setdefault("narrow" if c < 0 else "wide", ends[0])
        for kind, e in last.items():
            tried[kind] += 1
            w = _ratio(np.abs(r["Di"][:, e])[fin], (np.abs(r["lp"]) + r["sabs"])[fin])
            hits[kind] += w > F.TOL
    print("cases tried %s, beyond the bound %s" % (tried, hits))
    assert min(hits.values()) >= 5, (tried, hits)
