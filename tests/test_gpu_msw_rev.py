"""The second pass of mate rescue two alignments per quad (msw_rev2_kernel behind the class sort, msw_kernel.hip) on the requests of
tests/msw_rev_cases.py, through the stage entry: every field of every record equals ksw_align2's (the library's host form and, where it
is built, the compiled reference's); the same records, byte for byte, from a process with MPIBWA_MSW_REV2=0 (one alignment per quad,
msw_tail_kernel); and the work items the device ran are those msw_rev_cases.plan() predicts from the expected records — equal, not
at least."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msw_cases as mc
import msw_rev_cases as rv
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()   # the device index is a process-wide singleton: (re)upload this module's genome
    return api.Engine(genome["prefix"], device=0)


@pytest.fixture(scope="module")
def switched_off(genome, tmp_path_factory):
    """the worker's records with MPIBWA_MSW_REV2=0 (read once per process: a child of its own)"""
    out = str(tmp_path_factory.mktemp("msw_rev") / "off.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "msw_rev_worker.py"), genome["prefix"], out], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, MPIBWA_MSW_REV2="0"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["rev2_env"] == "0" and res["sets"] == len(rv.all_cases()), res
    return np.load(out)


_GOT = {}


def records(engine, family, name):
    """Engine.matesw on a family and what its second pass ran, once per session"""
    if (family, name) not in _GOT:
        cs = rv.cases(family, name)
        got = engine.matesw(mc.set_opt(engine.opt(), name), *cs.matesw_args())[0]
        _GOT[family, name] = got, engine.matesw_counts()
    return _GOT[family, name]


@pytest.mark.parametrize("family,name", rv.all_cases())
def test_two_per_quad_equals_ksw_align2_and_runs_the_predicted_items(engine, family, name):
    assert os.environ.get("MPIBWA_MSW_REV2", "1") != "0"
    cs = rv.cases(family, name)
    got, counts = records(engine, family, name)
    if name in mc.GATED:
        assert (got[:, 7] == 1).all() and counts == [0, 0, 0, 0], (name, counts, "the device must hand every request back under o_ins = 0")
        return
    wants = [mc.want_from_host(engine.lib, cs)]
    if po.ref_available():
        wants.append(mc.Want(cs, mc.reference_results(po.ref_lib(), cs), mc.host_results(engine.lib, cs, full_width=True)))
    for want in wants:
        st = mc.compare(got, want)
        pl = rv.plan(want)
        for m in pl["members"].values():   # what the second pass completes: all eight fields, flags = 0
            for i in m:
                assert (got[i][:7] == want.res[i]).all() and got[i][7] == 0, (family, name, i, list(got[i]), list(want.res[i]))
        assert int(got[:, 7].sum()) == st["sat"], (family, name, st)
        assert counts == pl["counts"], (family, name, counts, pl["counts"])
    print("msw rev %s/%s: requests %d hits %d flagged %d; second pass: pairs %d alone %d (register items %d, general items %d)" %
          (family, name, st["n"], st["hit"], st["sat"], *counts))


@pytest.mark.parametrize("family,name", rv.all_cases())
def test_one_per_quad_gives_the_same_bytes(engine, switched_off, family, name):
    got, counts = records(engine, family, name)
    off, off_counts = switched_off["%s/%s" % (family, name)], switched_off["counts/%s/%s" % (family, name)].tolist()
    assert got.dtype == off.dtype and got.shape == off.shape and got.tobytes() == off.tobytes(), (family, name, np.nonzero((got != off).any(axis=1))[0][:10])
    # the same members, every one on a quad of its own
    assert off_counts == [0, counts[0] * 2 + counts[1], 0, counts[0] * 2 + counts[1]], (family, name, counts, off_counts)
