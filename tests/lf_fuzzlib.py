"""Seeded ragged catalogues for the entries that read the catalogue through per-field tables of their own: the gradient's blocks,
the convolved likelihood's narrow chunks (deconv.CHUNK sources of one field), the wide list's chunks (deconv.WIDE_CHUNK sources
of one field and one sigma class), the 8-row tile kernel and lf_lum_posterior's slots and caller permutation (csrc/lf_hostprep.h:
chunk_table, wide_list).

The variant, the fields and the grid are drawn as tests/test_gpu_fuzz.py draws them (random cut points, so fields may be empty;
Om_arr rebuilt for the ragged split), then come a batch of theta rows, one sigma per source after one of five laws, and the
Gauss-Hermite order.  forced_cases() are the layouts a seeded draw must not be trusted to hit, through the same builder.  No GPU;
shared by tests/test_fuzz_entries_cpu.py and tests/test_gpu_fuzz_entries.py.  Test infrastructure only.
"""
import numpy as np

from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D

TOL = 1e-12                                     # the standing device-against-twin bound, on each twin's own S_abs scale
VARIANTS = ("free", "fixcomp", "zevol")
SIZES = (1, 2, 7, 63, 255, 256, 257, 1023, 1025, 2049, 4500)
PIVOTS = ((1.20, 1.53, 1.86), (1.18, 1.36, 1.54))
ORDERS = (4, 32)
# the sigma laws: uniform in [0, top edge] with a tenth at exactly 0; all at or below the order's limit (the wide list is empty
# with the option on); all above 0.09 dex (the narrow kernels find only zeros); all exactly 0; one non-zero source in the catalogue
LAWS = ("mixed", "narrow", "wide", "zero", "one")
SEEDS = tuple(range(24))                        # the seeds the GPU test runs
BIG_N, BIG_B = 1100, 8                          # above BIG_N sources at most BIG_B rows: the twins' time per case stays at seconds


def sigma_law(law, n, K, rng):
    """sigma [n] after `law`; the order's limit itself (narrow) and the top edge itself (wide) are among the values"""
    top, lim = D.WIDE_SIGMA_MAX, D.sigma_max(K)
    if law == "mixed":
        sg = rng.uniform(0.0, top, n)
        sg[rng.permutation(n)[:(n + 5) // 10]] = 0.0
    elif law == "narrow":
        sg = rng.uniform(0.0, lim, n)
        sg[0] = lim
    elif law == "wide":
        sg = rng.uniform(np.nextafter(D.SIGMA_MAX, 1.0), top, n)
        sg[-1] = top
    elif law == "zero":
        sg = np.zeros(n)
    elif law == "one":
        sg = np.zeros(n)
        sg[int(rng.integers(0, n))] = rng.uniform(0.5 * lim, lim) if rng.integers(0, 2) else rng.uniform(0.0901, top)
    else:
        raise ValueError(law)
    return sg


def build(variant, sizes, seed, S, fsa, pivots, B, law, K, label, sigma=None):
    """(inp, theta, sigma, K, label) of one case: `sizes` sources per field.  theta: synth.walkers, with more than three rows one
    underflowing row and one outside the box.  sigma: after `law`, or given (forced cases)."""
    sizes = [int(s) for s in sizes]
    nf, n = len(sizes), int(sum(sizes))
    inp = make_inputs(variant, n, seed=seed, S=S, fix_sch_al=fsa, nf=nf, pivots=pivots)
    inp["field_ind"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if variant != "free":
        # Om_arr was built for the equal split: rebuild it for the ragged one
        om0 = np.zeros(n, dtype=int); fl = np.zeros(n)
        for f in range(nf):
            om0[inp["field_ind"][f]:inp["field_ind"][f + 1]] = inp["Omega_0"][f]
            fl[inp["field_ind"][f]:inp["field_ind"][f + 1]] = inp["Flim0"][f]
        with np.errstate(all="ignore"):
            inp["Om_arr"] = O.omega(inp["lum"], inp["DLz"], om0, 1.0e-17 * fl, synth.ALPHA_C, synth.FCMIN)
    th = synth.walkers(variant, B, seed=seed + 7, fix_sch_al=fsa, nf=nf)
    if B > 3:
        th[0, 0:(3 if variant == "zevol" else 1)] = 40.2       # inside the box, but the bright sources underflow
        th[1, 1] = 5.5                                          # outside the box
    sg = sigma_law(law, n, K, np.random.default_rng(7000 + seed)) if sigma is None else np.asarray(sigma, dtype=np.float64)
    assert sg.shape == (n,)
    return inp, th, sg, K, "%s %s sizes=%s S=%d fsa=%d B=%d law=%s K=%d" % (label, variant, sizes, S, fsa, B, law, K)


def params(seed):
    """what case(seed) is built from: the variant cycles with the seed, the law with seed // 3 (every law for every variant within
    15 seeds), the order with seed // 3 and the pivot set with the seed; the rest is drawn"""
    rng = np.random.default_rng(9000 + seed)
    nf = int(rng.integers(1, 9))
    n = int(rng.choice(SIZES))
    S = int(rng.integers(4, 40))
    fsa = bool(rng.integers(0, 2))
    cuts = np.sort(rng.integers(0, n + 1, nf - 1)) if nf > 1 else np.array([], dtype=int)      # ragged fields, some empty
    B = int(rng.integers(1, 38))
    return dict(variant=VARIANTS[seed % 3], sizes=np.diff(np.concatenate([[0], cuts, [n]])).tolist(), seed=seed, S=S, fsa=fsa,
                pivots=PIVOTS[seed % 2], B=min(B, BIG_B) if n > BIG_N else B, law=LAWS[(seed // 3) % 5], K=ORDERS[(seed // 3) % 2],
                label="seed %d" % seed)


def case(seed):
    return build(**params(seed))


def forced_params():
    """the hand-written layouts, each for every variant: empty fields in front, in the middle and behind; n < nf; one source in the
    last of eight fields; fields of one source next to fields of more than a narrow chunk; and a field whose only sources are
    WIDE_CHUNK + 1 wide sources of one class (0.10 < sigma <= 0.15 dex) between two empty fields"""
    w = D.WIDE_CHUNK + 1
    shapes = [([0, 0, 1, 1, 0], "mixed", None), ([1, 0, 1, 0, 0, 0, 0, 0], "wide", None), ([0, D.CHUNK + 1, 0, 1, D.CHUNK - 1], "mixed", None),
              ([0, w, 0], "wide", np.random.default_rng(41).uniform(0.1001, 0.15, w)), ([0] * 7 + [1], "one", None)]
    out = []
    for i, (sizes, law, sigma) in enumerate(shapes):
        for j, v in enumerate(VARIANTS):
            # (the first shape with a fixed faint-end slope: FREE then has ndim = 8, which 16 walkers can sample)
            out.append(dict(variant=v, sizes=sizes, seed=500 + 3 * i + j, S=9 + 7 * ((i + j) % 3), fsa=(i + j) % 2 == 0, pivots=PIVOTS[(i + j) % 2],
                            B=5 + 3 * ((i + j) % 2), law=law, K=ORDERS[(i + j) % 2], label="forced %d" % i, sigma=sigma))
    return out


def forced_cases():
    return [build(**p) for p in forced_params()]


def all_params():
    return [params(s) for s in SEEDS] + forced_params()


def case_ids():
    return ["%s-%s" % (p["label"].replace(" ", ""), p["variant"]) for p in all_params()]


def sampler_params():
    """four ragged cases for a 16-walker chain (ndim <= 8): per variant the first seeded case of several fields and sources, one
    with an empty field if there is one, and [0, 0, 1, 1, 0] under the FREE completeness (three of its five Flim never meet a
    source)"""
    out = []
    for v in VARIANTS:
        fit = [p for p in map(params, SEEDS) if p["variant"] == v and len(p["sizes"]) > 1 and sum(p["sizes"]) > 1 and
               synth.ndim_of(v, p["fsa"], len(p["sizes"])) <= 8]
        out.append(min(fit, key=lambda p: (0 not in p["sizes"], p["seed"])))
    out.append(next(p for p in forced_params() if p["sizes"] == [0, 0, 1, 1, 0] and p["variant"] == "free"))
    assert synth.ndim_of("free", out[-1]["fsa"], 5) <= 8
    return out


def facts(inp, sigma, K):
    """what a case's layout holds, for the coverage conditions: {name: bool}"""
    fi = np.asarray(inp["field_ind"])
    sizes = np.diff(fi)
    nf, n = len(sizes), int(fi[-1])
    cls = D.wide_class(sigma, K)
    pairs = [int(np.sum(cls[fi[f]:fi[f + 1]] == c)) for f in range(nf) for c in range(len(D.WIDE_EDGES))]
    return {"empty first field": nf > 1 and sizes[0] == 0, "empty last field": nf > 1 and sizes[-1] == 0,
            "empty middle field": nf > 2 and bool(np.any(sizes[1:-1] == 0)), "n < nf": n < nf,
            "field over several narrow chunks": bool(np.any(sizes > D.CHUNK)),
            "(field, class) over several wide chunks": any(p > D.WIDE_CHUNK for p in pairs),
            "(field, class) of one source": any(p == 1 for p in pairs)}
