"""Runs the REFERENCE's own driver, in place, over this package's classes (tests/test_driver_contract.py starts it
under an interpreter that has astropy).  argv: <workdir> <reference dir> <nsources> <nwalkers> <nsteps> [--z] [--default-config]
[-fc] [-fsa].  --z: run_lumfuncmcmc_z.py over LumFuncMCMCz instead of run_lumfuncmcmc.py over LumFuncMCMC; --default-config:
configLF.output_dict as the reference ships it ('triangle plot': True), i.e. the driver with NO config edits.

sys.path order: dropin/ (lumfuncmcmc, lumfuncmcmc_z, VmaxLumFunc resolve to this package), the repo, oracle/ and
only then the reference checkout (run_lumfuncmcmc.py, configLF.py).  The GPU is not needed: `_Base._evaluate` is
pointed at the oracle (tests may use it) and the host sampler runs the chain; everything else - the constructor call
with the driver's keywords, fit_model, set_median_fit, the attributes the driver writes out, add_fitinfo_to_table - is
the product code.  Nothing of the reference is copied: it is imported where it lies.

--record FILE.npz: also keep, as data, what the driver did with the class - the constructor's arguments, and every
attribute the driver's own code read or set and every method it called, in order, with the shapes it got back - for
tests/test_driver_replay.py, which replays that transcript over the classes without the reference or astropy."""
import json
import os
import sys

import numpy as np

work, ref, nsrc, nwalk, nsteps = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
flags = sys.argv[6:]
RECORD = None
if "--record" in flags:
    i = flags.index("--record")
    RECORD = os.path.abspath(flags[i + 1])
    del flags[i:i + 2]
ZDRIVER = "--z" in flags
DEFAULT_CONFIG = "--default-config" in flags
flags = [f for f in flags if f not in ("--z", "--default-config")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dropin"), ROOT, os.path.join(ROOT, "oracle"), ref]

if not hasattr(np, "asscalar"):                       # astropy 4.3 predates its numpy
    for name, f in (("asscalar", lambda a: a.item()), ("alen", len), ("rank", np.ndim)):
        setattr(np, name, f)

import lf_oracle as O                                  # noqa: E402
from lumfuncmcmc_amd import model, synth               # noqa: E402

# ---- a synthetic catalogue in the driver's input format (flux columns, 5 field names sorting into
# Flim order, ID), and the hard-coded second table read_input_file insists on (run_lumfuncmcmc.py:241)
os.chdir(work)
cat = synth.catalogue(nsrc, seed=7)
fi = cat["field_ind"]
DL = np.asarray(model._cosmo.luminosity_distance(cat["z"]))
flux = 10.0 ** cat["lum"] / (4.0 * np.pi * (3.086e24 * DL) ** 2) / 1.0e-17
fields = np.concatenate([["F%d" % f] * int(fi[f + 1] - fi[f]) for f in range(5)])
ids = np.arange(nsrc)
with open("cat.dat", "w") as fh:
    fh.write("Field ID z OIII_flux OIII_flux_e\n")
    for i in range(nsrc):
        fh.write("%s %d %.10f %.10e %.10e\n" % (fields[i], ids[i], cat["z"][i], flux[i], 0.05 * flux[i]))
with open("combined_all_Swift_NoDust_Donley_removed.dat", "w") as fh:
    fh.write("Field ID E(B-V) E(B-V)err SFR100 SFR100err\n")
    for i in range(nsrc):
        fh.write("%s %d 0.1 0.01 1.0 0.1\n" % (fields[i], ids[i]))

# ---- the reference's driver, imported where it lies
import configLF                                        # noqa: E402
if ZDRIVER:
    import run_lumfuncmcmc_z as drv                    # noqa: E402
    assert drv.LumFuncMCMCz is model.LumFuncMCMCz, "the driver did not pick up the drop-in class"
    cls, outdir = model.LumFuncMCMCz, "LFMCMCzOut"
    # run_lumfuncmcmc_z.py:274-279 writes the (zlen, Llen) medianLF matrix as ONE table column next to two 1-d columns:
    # astropy (4.3.1 here) refuses that in the REFERENCE's own code, whatever class produced the arrays - the one output the
    # z driver cannot write in this container
    configLF.output_dict["bestfitLF"] = False
else:
    import run_lumfuncmcmc as drv                      # noqa: E402
    assert drv.LumFuncMCMC is model.LumFuncMCMC, "the driver did not pick up the drop-in class"
    cls, outdir = model.LumFuncMCMC, "LFMCMCOut"
assert os.path.dirname(os.path.abspath(drv.__file__)) == os.path.abspath(ref)
if not DEFAULT_CONFIG:
    configLF.output_dict["triangle plot"] = False      # (the other branch of the driver: set_median_fit)

cls.device_sampler = False                             # host sampler: no GPU in this test


def evaluate(self, theta):                             # the oracle in place of liblfmcmc.so (tests only)
    inp = self.kernel_inputs()
    inp["lims"] = {k: list(v) for k, v in inp["lims"].items()}
    th = np.asarray(theta, dtype=np.float64)
    out = O.lnprob_batch(inp, np.atleast_2d(th))
    return float(out[0]) if th.ndim == 1 else out


model._Base._evaluate = evaluate
SEED = 12345

if RECORD:
    REFDIR = os.path.abspath(ref) + os.sep
    arrays, events = {}, []

    def from_driver():                                 # the caller of the hook is the reference driver's own code
        return sys._getframe(2).f_code.co_filename.startswith(REFDIR)

    def enc(v, key):                                   # arguments as data: arrays into the npz, the rest as JSON
        if isinstance(v, np.ndarray):
            arrays[key] = np.array(v)                  # (astropy columns as plain arrays)
            return {"npz": key}
        if isinstance(v, (list, tuple)):
            return {"list": [enc(x, "%s_%d" % (key, i)) for i, x in enumerate(v)]}
        if isinstance(v, np.generic):
            return {"v": v.item()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return {"v": v}
        raise TypeError("cannot record %s of type %s" % (key, type(v).__name__))

    def desc(v):
        if isinstance(v, np.ndarray):
            return {"type": "ndarray", "shape": list(v.shape), "dtype": v.dtype.kind}
        if isinstance(v, (list, tuple)):
            return {"type": "list", "len": len(v)}
        if v is None or isinstance(v, (np.generic, bool, int, float, str)):
            return {"type": "scalar"}
        return {"type": type(v).__name__}

    def last_row(obj):
        return [x.decode() if isinstance(x, bytes) else x.item() if isinstance(x, np.generic) else x for x in obj.table[-1]]

    class Recorded(cls):
        def __init__(self, *a, **kw):
            if from_driver():
                events.append({"op": "init", "args": [enc(x, "arg%d" % i) for i, x in enumerate(a)],
                               "kwargs": {k: enc(x, "kw_" + k) for k, x in kw.items()}})
            super().__init__(*a, **kw)

        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if not from_driver():
                return v
            if callable(v) and getattr(v, "__self__", None) is self:
                def call(*a, **kw):
                    n = len(events)
                    ev = {"op": "call", "name": name, "args": [enc(x, "call%d_%d" % (n, i)) for i, x in enumerate(a)],
                          "kwargs": {k: enc(x, "call%d_%s" % (n, k)) for k, x in kw.items()}}
                    if name == "add_fitinfo_to_table":
                        ev["row_before"] = last_row(self)
                    r = v(*a, **kw)
                    if name == "add_fitinfo_to_table":
                        ev["row_after"] = last_row(self)
                    ev["result"] = desc(r)
                    events.append(ev)
                    return r
                return call
            events.append({"op": "get", "name": name, "desc": desc(v)})
            return v

        def __setattr__(self, name, v):
            if from_driver():
                events.append({"op": "set", "name": name, "desc": desc(v)})
            object.__setattr__(self, name, v)

    setattr(drv, cls.__name__, Recorded)

np.random.seed(SEED)
drv.main(["-f", "cat.dat", "-o", "contract.dat", "-nw", str(nwalk), "-ns", str(nsteps), "-nbins", "10", "-nboot", "20"] + flags)

out = sorted(os.listdir(outdir))
from astropy.table import Table                        # noqa: E402
post = [f for f in out if f.startswith("fitposterior")][0]
t = Table.read(os.path.join(outdir, post), format="ascii.fixed_width_two_line")
if RECORD:
    tr = {"class": cls.__name__, "seed": SEED, "nsources": nsrc, "nwalkers": nwalk, "nsteps": nsteps, "driver_flags": flags,
          "z_driver": ZDRIVER, "default_config": DEFAULT_CONFIG, "outdir": outdir, "files": out, "events": events}
    np.savez_compressed(RECORD, transcript=np.array(json.dumps(tr)), **arrays)
print(json.dumps({"files": out, "posterior_columns": len(t.colnames), "posterior_rows": len(t),
                  "finite_lnprob": int(np.isfinite(np.asarray(t[t.colnames[-1]], dtype=float)).sum())}))
