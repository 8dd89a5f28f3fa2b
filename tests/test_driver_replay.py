"""The drop-in contract without the reference checkout: tests/test_driver_contract.py runs the reference's own CLI drivers
over LumFuncMCMC / LumFuncMCMCz where a reference checkout and an interpreter with astropy are at hand, and there the same
runs were recorded as data (tests/driver_contract_runner.py --record, oracle/gen_golden.py --only driver): the
constructor's arguments, then every method the driver called, in order, and every attribute it read or set, with the
shapes it got back.  This replays each transcript over the classes - same arguments, same calls, same seed, the oracle in
place of liblfmcmc.so, the host sampler - and asks for what the driver's output files are made of: the same attributes
with the same shapes, samples of ndim + 1 columns after a burn-in of at most nsteps // 2 with finite lnprob, and the fit's
percentiles written into the same cells of the table's last row."""
import json
import os

import numpy as np
import pytest

import lf_oracle as O
from lumfuncmcmc_amd import model

CASES = ["driver_plain", "driver_fc", "driver_fsa", "driver_default", "driver_default_fc", "driver_z", "driver_z_fsa",
         "driver_z_default"]


def evaluate(self, theta):                             # the oracle in place of liblfmcmc.so, as in driver_contract_runner.py
    inp = self.kernel_inputs()
    inp["lims"] = {k: list(v) for k, v in inp["lims"].items()}
    th = np.asarray(theta, dtype=np.float64)
    out = O.lnprob_batch(inp, np.atleast_2d(th))
    return float(out[0]) if th.ndim == 1 else out


def decode(spec, arrays):
    if "npz" in spec:
        return arrays[spec["npz"]]
    if "list" in spec:
        return [decode(x, arrays) for x in spec["list"]]
    return spec["v"]


def check(name, v, want, tr):
    kind = want["type"]
    if kind == "ndarray":
        assert isinstance(v, np.ndarray), (name, type(v))
        assert v.dtype.kind == want["dtype"], (name, v.dtype)
        if name == "samples":
            # walkers x the steps after the burn-in, whose length comes from the chain's autocorrelation time
            assert list(v.shape[1:]) == want["shape"][1:], (name, v.shape, want)
            assert v.shape[0] % tr["nwalkers"] == 0 and v.shape[0] >= tr["nwalkers"] * (tr["nsteps"] - tr["nsteps"] // 2)
        else:
            assert list(v.shape) == want["shape"], (name, v.shape, want)
    elif kind == "list":
        assert isinstance(v, (list, tuple)) and len(v) == want["len"], (name, v, want)
    elif kind == "scalar":
        assert v is None or np.isscalar(v), (name, type(v))
    else:
        pytest.fail("%s: the driver got a %s" % (name, kind))


@pytest.mark.parametrize("case", CASES)
def test_dropin_classes_replay_the_reference_driver(case, golden_dir, tmp_path, monkeypatch):
    rec = np.load(os.path.join(golden_dir, case + ".npz"), allow_pickle=False)
    tr = json.loads(str(rec["transcript"]))
    cls = getattr(model, tr["class"])
    monkeypatch.setattr(model._Base, "_evaluate", evaluate)
    monkeypatch.setattr(cls, "device_sampler", False, raising=False)     # host sampler: no GPU in this test
    monkeypatch.chdir(tmp_path)
    os.makedirs(tr["outdir"])
    init, events = tr["events"][0], tr["events"][1:]
    assert init["op"] == "init" and events
    np.random.seed(tr["seed"])
    obj = cls(*decode({"list": init["args"]}, rec), **{k: decode(v, rec) for k, v in init["kwargs"].items()})
    set_by_driver, names, filled = set(), None, False
    for ev in events:
        op, name = ev["op"], ev["name"]
        if op == "set":
            # the driver's own table: a list of rows stands in for the astropy Table (add_fitinfo_to_table fills cells of
            # its last row, the row the driver added before the call)
            assert name == "table", ev
            obj.table = []
            set_by_driver.add(name)
        elif op == "get":
            if name not in set_by_driver:
                check(name, getattr(obj, name), ev["desc"], tr)
        else:
            args = decode({"list": ev["args"]}, rec)
            kwargs = {k: decode(v, rec) for k, v in ev["kwargs"].items()}
            if name == "add_fitinfo_to_table":
                obj.table.append(list(ev["row_before"]))
            r = getattr(obj, name)(*args, **kwargs)
            check(name + "()", r, ev["result"], tr)
            if name == "get_param_names":
                names = list(r)
            if name == "add_fitinfo_to_table":
                before, after, row = ev["row_before"], ev["row_after"], obj.table[-1]
                written = [i for i, (a, b) in enumerate(zip(before, after)) if a != b]
                assert len(row) == len(before) and written
                assert [i for i, (a, b) in enumerate(zip(before, row)) if a != b] == written
                assert all(np.isfinite(row[i]) for i in written)
                filled = True
    # what the driver writes as fitposterior: the parameters and lnprob, one row per kept step of every walker
    assert names is not None and filled
    assert obj.samples.shape[1] == len(names) + 1
    assert np.isfinite(obj.samples[:, -1]).all()
