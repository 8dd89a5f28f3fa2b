"""Shared pieces of the tests of the cut process's mock catalogues (tests/test_mock_cut_cpu.py,
tests/test_gpu_mock_cut.py): grids with their own lower edge per redshift column (lf_cutlib.cut_inputs), sigma tables with zero
entries, generators set up with a band, rows whose candidate counts are steered through phi*, and the two halves of Delta B.
Test infrastructure only."""
import functools

import numpy as np

import lf_cutlib as C
from lumfuncmcmc_amd import deconv, mock, synth

NF = 2


@functools.lru_cache(maxsize=None)
def inputs(variant, S, fix_sch_al=False, nf=NF):
    return C.cut_inputs(variant, n=60, S=S, nf=nf, fix_sch_al=fix_sch_al)


def table(M, nf=NF):
    """M nodes around the flux of the cut, sigma in 0.02 .. 0.3 dex with zero entries: M = 1: one value per field, the last
    field's 0 (it keeps no band source); M = 2: field 0 rises from 0; M = 64: every fifth node 0, the first among them"""
    nodes = np.log10(C.FCUT) + (np.linspace(-0.5, 0.8, M) if M > 1 else np.zeros(1))
    sig = np.random.default_rng(M).uniform(0.02, 0.3, (nf, M))
    if M >= 5:
        sig[:, ::5] = 0.0
    elif M > 1:
        sig[0, 0] = 0.0
    else:
        sig[nf - 1, 0] = 0.0
    return nodes, sig


def arm(gen, inp, nodes, sig, H=None):
    """the error model and the band of depth H (default: 7.5 max sigma) on a twin or a device generator"""
    gen.set_error_model(nodes, sig)
    lb = mock.band_grid(inp, mock.cut_depth(sig) if H is None else H)
    gen.set_cut_band(lb, None if inp["variant"] == "free" else mock.band_integ_part(inp, lb))
    return gen


def _phi(variant):
    return [3, 4, 5] if variant == "zevol" else [1]


def rows_for_means(tw, variant, fix_sch_al, targets, piece, seed=5):
    """rows of the prior box with phi* shifted so that field 0's expected count of `piece` (0 above, 1 below) is targets[i]; a
    target of 0 puts L* so far below the grid that every node of both pieces underflows"""
    th = synth.walkers(variant, len(targets), seed=seed, fix_sch_al=fix_sch_al, nf=tw.nf)
    gen = (tw, tw._band)[piece]
    if piece and not fix_sch_al:
        th[:, 6 if variant == "zevol" else 2] = -2.8          # a steep faint end: the band is not dwarfed by the grid above it
    for i, t in enumerate(targets):
        if t > 0:
            th[i, _phi(variant)] += np.log10(t / gen.means(th[i:i + 1])[0, 0])
        else:
            th[i, [0, 1, 2] if variant == "zevol" else [0]] = 20.0
    return th


def rows_for_counts(tw, variant, targets, piece, seed, row_ids):
    """rows whose field 0 has exactly targets[i] candidates of `piece` under (seed, row_ids[i]): phi* is stepped in 1e-3 of the
    mean around the target until the twin's Poisson draw gives it"""
    th = rows_for_means(tw, variant, False, targets, piece)
    for i, t in enumerate(targets):
        base = th[i].copy()
        for step in range(2000 if t else 0):
            th[i] = base
            th[i, _phi(variant)] += np.log10(1.0 + 1.0e-3 * (step // 2) * (1 if step % 2 else -1))
            mean = (tw, tw._band)[piece].means(th[i:i + 1])[0, 0]
            if mock.poisson(mean, row_ids[i], piece * mock.CUT_BAND, seed) == t:
                break
        else:
            assert t == 0, "no phi* gives %d candidates" % t
    return th


def halves(inp, nodes, sig, theta):
    """(up, down) >= 0 per field [nf]: the two halves of Delta B = up - down at one theta - the expected number of sources
    that scatter in from below the edge and out from above it (deconv.cut_nodes' weights are + below the edge, - above)"""
    nl, _ = deconv.cut_nodes(inp, nodes, sig)
    up, down = np.zeros(len(nl)), np.zeros(len(nl))
    for f, n in enumerate(nl):
        if n["L"].size:
            I = n["w"] * deconv._cut_phi_omega(inp, np.asarray(theta, dtype=np.float64), f, n["L"], n["col"], n["logf"])
            up[f], down[f] = I[I > 0.0].sum(), -I[I < 0.0].sum()
    return up, down


def edge_gap(tw, th, seed, rid):
    """the twin's candidates and the smallest |L_obs - edge| among them (the precondition of identical keep flags)"""
    nodes, sigma, ld2n = tw.noise
    c = tw.candidates_cut(th, seed, rid)
    gap = np.inf
    o = 0
    for r in range(th.shape[0]):
        cd = [tw._cdfs(th[r]), tw._band._cdfs(th[r])]
        for f in range(tw.nf):
            for p, gen in enumerate((tw, tw._band)):
                n = int(c[6][r, f, p])
                if n:
                    k = gen._sources(th[r], rid[r], f, f | (p * mock.CUT_BAND), seed, np.arange(n, dtype=np.uint64), cd[p])[2]
                    gap = min(gap, float(np.min(np.abs(c[2][o:o + n] - tw.logL[0][k]))))
                    o += n
    return c, gap
