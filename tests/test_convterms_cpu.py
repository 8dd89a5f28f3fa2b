"""The element-wise probes of the wide, tiled, per-source-posterior and binned copies of the convolved likelihood's node loop
without a GPU: tests/conv_probe.hip cross-compiles for gfx950 with the library's flags; the inputs of tests/lf_convproblib.py
hold what they promise; the NumPy twins (deconv._row_terms with the wide tables - what deconv.delta(wide=True) runs per class -
its moments, which deconv.lum_posterior adds up, and its node products, which deconv.veff_true bins) stay within their caps
against the 40-digit references, and the figures the caps of tests/test_gpu_convterms.py rest on are measured and printed;
five subtle mutations of the NumPy expressions land far above the caps; and the factor question of DESIGN.md section 3.27 is
answered on the twin: the two-factor product the binned form used to take leaves the binary64 range on the lattice's own
sources, the one-exponent product does not."""
import math
import os

import numpy as np

import lf_convproblib as C
import lf_isalib
from lumfuncmcmc_amd import deconv as D

P = C.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "conv_probe.hip")
KEYS = (4, 32) + tuple(("wide", c) for c in range(len(D.WIDE_EDGES)))
FAR = 100.0            # "far above its cap": a mutation's figure / the form's cap


def test_probe_unit_compiles_for_gfx950_and_launches_the_librarys_kernels():
    seen = {name: r for name, r in lf_isalib.remarks(SRC, "-c").items() if "ScratchSize" in r}
    for kern, count in (("lf_deconv_wide_partILi", 3), ("lf_deconv_wide_grad_partILi", 3), ("lf_deconv_tileILi", 2), ("lf_lumpost_partILi", 3),
                        ("lf_vefftrue_partILi", 3)):
        hits = [r for name, r in seen.items() if kern in name]
        assert len(hits) == count, (kern, sorted(seen))
        assert all(r["ScratchSize"] == 0 for r in hits), kern
    # no kernel of its own: the fourteen it launches and the headers' three untemplated ones (final, fold, reduce)
    assert len(seen) == 17, sorted(seen)


def test_inputs_hold_what_they_promise():
    assert C.WIDE_K == (48, 72, 96, 120, 144)
    assert [K - 64 * ((K - 1) // 64) for K in C.WIDE_K] == [48, 8, 32, 56, 16]          # nodes of the last 64-lane pass
    for c in range(5):
        sg = C.wide_sigmas(c)
        assert sg[0] == np.nextafter(0.09, 1.0) and sg[-1] == D.WIDE_EDGES[c] and len(sg) == (2 if c == 0 else 3)
        assert np.all(D.wide_class(np.array(sg[-2:])) == c)              # the lower and the upper edge are the class's own
        x, lnw = C.table(("wide", c))
        assert len(x) == C.WIDE_K[c] and np.all(np.diff(x) > 0) and abs(x[-1] * math.sqrt(2.0)) < D.WIDE_T
        s = C.wide_sources(P.FREE, c)
        y = (s["logf"] + 17.0) - np.log10(P.FLIM0)
        assert abs(y.min() + 1.5) < 1e-12 and abs(y.max() - 2.0) < 1e-12 and s["lum"].max() == 45.4
        C.node_edges(s, x)
    for v in C.VARIANTS:
        s, full = C.lattice(v), P.deconv_sources(v)
        assert s["n"] == 121 and np.array_equal(s["sigma"][:100], full["sigma"][:100]) and s["lum"][-1] == 45.4
        assert set(s["sigma"]) == set(P.SIGMAS) | {0.0}
        for K in (4, 32):
            C.node_edges(s, D.gauss_hermite(K)[0])
            for pos in (0, K // 2, K):
                x, lnw = C.with_dead_node(*D.gauss_hermite(K), pos)
                assert np.all(np.diff(x) > 0) and lnw[pos] == -np.inf and len(x) == K + 1
                C.node_edges(s, x)
    # the wide tables meet many more rises of the maximum and larger spreads than K = 32
    r32, r144 = C.case(P.FREE, 32)["delta"]["rises"], C.case(P.FREE, ("wide", 4))["delta"]["rises"]
    print("rises of the running maximum, row 0: K = 32 up to %d, K = 144 up to %d" % (r32.max(), r144.max()))
    assert r32.max() >= 20 and r144.max() >= 60
    # the chunk order: sums of integers are exact in any order, the count of sources per wave is what the header says
    one = np.arange(1.0, 258.0)[:, None] * np.ones((1, 3))
    assert np.array_equal(C.chunk_sum(one, 257), np.full(3, 257 * 258 / 2))


def _figures():
    figs = {}

    def put(name, case, got=None):
        f = C.L.measure(case, case["np"] if got is None else got)
        if name not in figs or f[0] > figs[name][0]:
            figs[name] = f + (case["variant"], case["key"])
    for v in C.VARIANTS:
        for key in KEYS:
            c = C.case(v, key)
            route = "wide" if isinstance(key, tuple) else "narrow"
            put("e1_" + route, c["e1"]), put("e2_" + route, c["e2"]), put("node_" + route, c["prod"])
            if route == "wide":
                put("delta_wide", c["delta"]), put("grad_wide", c["grad"])
            elif v != P.FREE:
                put("tile_delta", c["delta"])
    return figs


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the NumPy twins against the 40-digit values: the caps of the GPU tests are 4 x these and never
    below 2 (lf_convproblib.CAPS holds them as constants; this test says when they have moved)"""
    figs = _figures()
    for k, (fig, i, v, key) in figs.items():
        print("numpy %-14s max err / yard %9.3f at index %d (%s, table %s)   cap %g" % (k, fig, i, P.VNAME[v], key, C.CAPS[k]))
    assert set(figs) == set(C.CAPS)
    for k, (fig, i, v, key) in figs.items():
        assert math.isfinite(fig), k
        assert fig <= C.CAPS[k], (k, fig)
        assert C.L.cap_from(fig) <= C.CAPS[k] * 1.05 and C.L.cap_from(fig) >= C.CAPS[k] * 0.8, (k, fig, C.CAPS[k])


def _loop_case(v, key, b, mutate):
    c = C.case(v, key)
    s, th = c["delta"]["src"], c["delta"]["rows"][b]
    x, lnw = C.table(key)
    return c, s, th, C.loop_numpy(v, th, s, x, lnw, mutate)


def _row_fig(case, b, got, per):
    """max err / yard of one row's values"""
    n = len(np.ravel(got))
    sl = slice(b * n, (b + 1) * n)
    sub = {"ref": (case["ref"][0][sl], case["ref"][1][sl]), "yard": case["yard"][sl]}
    return C.L.measure(sub, np.ravel(got))[0]


def test_the_restated_loop_has_the_twins_bits():
    for v in C.VARIANTS:
        for key in (32, ("wide", 4)):
            c, s, th, (Dl, e1, e2, r) = _loop_case(v, key, 0, None)
            n = s["n"]
            assert np.array_equal(Dl, c["delta"]["np"][:n]) and np.array_equal(e1, c["e1"]["np"][:n]) and np.array_equal(e2, c["e2"]["np"][:n])
            assert np.array_equal(r.T.ravel(), c["prod"]["np"][:n * len(r)], equal_nan=True)


def test_the_metric_sees_subtle_errors():
    """each mutation of the NumPy expression lands far above its form's cap"""
    seen = {}
    for v in C.VARIANTS:
        for key, b in ((32, 0), (("wide", 4), 0), (32, 3)):
            wide = isinstance(key, tuple)
            route = "wide" if wide else "narrow"
            for mut, form, name in (("e1_no_rescale", "e1", "e1_" + route), ("e2_delta", "e2", "e2_" + route),
                                    ("fc_catalogued", "prod", "node_" + route), ("first64", "prod", "node_wide"),
                                    ("first64", "e1", "e1_wide"), ("tile_l0", "delta", "tile_delta")):
                if (mut == "first64" and not wide) or (mut == "tile_l0" and (wide or v == P.FREE)):
                    continue
                c, s, th, out = _loop_case(v, key, b, mut)
                got = {"delta": out[0], "e1": out[1], "e2": out[2], "prod": out[3].T}[form]
                fig = _row_fig(c[form], b, got, None)
                k = (mut, form)
                seen[k] = max(seen.get(k, 0.0), fig / C.CAPS[name])
    for k, f in seen.items():
        print("mutation %-14s on %-5s: worst max err / yard = %.3g x the cap" % (k[0], k[1], f))
    assert set(m for m, _ in seen) == {"e1_no_rescale", "e2_delta", "fc_catalogued", "first64", "tile_l0"}
    assert all(f > FAR for f in seen.values()), seen


def test_the_factor_question_on_the_twin():
    """p_k times exp(-l_k), as two factors, is +inf, NaN or exactly 0 where the 40-digit product is a
    finite normal number, on sources the entry accepts (any finite flux; sigma up to 0.30 dex); the one-exponent product is
    finite and non-zero at every such node."""
    tot = {"nodes": 0, "two_inf": 0, "two_nan": 0, "two_zero": 0, "one_bad": 0}
    worst = None
    for v in C.VARIANTS:
        for key in (32, ("wide", 4)):
            c = C.case(v, key)["prod"]
            s, rows, K = c["src"], c["rows"], c["K"]
            x, lnw = C.table(key)
            inp = P.deconv_inp(v, s)
            ref = c["ref"][0].reshape(len(rows), s["n"], K)
            for b, th in enumerate(rows):
                with np.errstate(all="ignore"):
                    p, _, l, r = D._row_terms(inp, s["sigma"], th, x, lnw, nodes="product")
                    two = p * (np.exp(-l) / C.PV)
                on = (s["sigma"] > 0.0)[None, :] & np.isfinite(ref[b].T) & (np.abs(ref[b].T) >= 2.0 ** -1022)
                tot["nodes"] += int(on.sum())
                tot["two_inf"] += int((np.isinf(two) & on).sum())
                tot["two_nan"] += int((np.isnan(two) & on).sum())
                tot["two_zero"] += int(((two == 0.0) & on).sum())
                tot["one_bad"] += int(((~np.isfinite(r) | (r == 0.0)) & on).sum())
                bad = (~np.isfinite(two) | (two == 0.0)) & on
                if bad.any():
                    k, i = np.unravel_index(np.argmax(np.where(bad, ref[b].T, 0.0)), bad.shape)
                    if worst is None or ref[b, i, k] > worst[0]:
                        worst = (ref[b, i, k], P.VNAME[v], key, b, s["sigma"][i], (s["logf"][i] + 17.0) - np.log10(P.FLIM0), k, two[k, i], l[k, i])
    print("nodes whose 40-digit product is a finite normal number:", tot)
    print("largest lost product %.6g: %s, table %s, row %d, sigma %g, log10(f / Flim0) %.3f, node %d: two factors give %r (l = %.6g)" % worst)
    assert tot["two_inf"] > 0 and tot["two_nan"] + tot["two_zero"] > 0 and tot["one_bad"] == 0
