"""The three mate-rescue kernels (msw2_kernel, msw_tail_kernel, msw_kernel) under every scoring option they read, on the requests of
tests/msw_cases.py: exact equality with the library's host ksw_align2 and, where it is built, the compiled reference's.  Under the
option sets of msw_cases.GATED (o_ins = 0) mate rescue is the host's: the stage entry hands every request back and the pipeline does not
use the kernels, which the two end-to-end tests at the bottom hold against the reference's SAM."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import msw_cases as mc
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()   # the device index is a process-wide singleton: (re)upload this module's genome
    return api.Engine(genome["prefix"], device=0)


def check(engine, name, got):
    """got against the host restatement and the reference -> (coverage, work-list census)"""
    cs = mc.cases(name)
    want = mc.want_from_host(engine.lib, cs)
    st = mc.compare(got, want)
    if po.ref_available():
        mc.compare(got, mc.Want(cs, mc.reference_results(po.ref_lib(), cs), mc.host_results(engine.lib, cs, full_width=True)))
    wc = mc.check_coverage(name, cs, st)
    # a request is handed back only at the byte flavour's ceiling, which takes a score of 255 - b: a * qlen < 250 leaves that to
    # the sets with b >= 6
    assert int(got[:, 7].sum()) == st["sat"] and (st["sat"] == 0 or cs.o["b"] >= 6), (name, st)
    return st, wc


@pytest.mark.parametrize("name", list(mc.OPTION_SETS))
def test_msw_kernels_under_option_set(engine, name):
    cs = mc.cases(name)
    got, _ = engine.matesw(mc.set_opt(engine.opt(), name), *cs.matesw_args())
    if name in mc.GATED:
        assert (got[:, 7] == 1).all(), (name, "the device must hand every request back under o_ins = 0")
        return
    st, wc = check(engine, name, got)
    print("msw options %s: requests %d hits %d flagged %d uniform waves %d mixed waves %d %s" % (name, st["n"], st["hit"], int(got[:, 7].sum()),
                                                                                              wc["uniform"], wc["mixed"], st))


def test_msw_kernel_byte_flavour_forward_pass(genome):
    """MPIBWA_MSW_PAIRS=0 (read once per process: a child of its own): every request goes to msw_kernel, whose forward pass otherwise
    only sees the word flavour.  The default set, the same comparison."""
    env = dict(os.environ, MPIBWA_MSW_PAIRS="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "msw_worker.py"), genome["prefix"], "default"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["pairs_env"] == "0" and res["n"] == len(mc.cases("default")) and res["hit"] >= 0.4 * res["n"] and res["flagged"] == 0, res


# sha256 of the reference's SAM for the session's 600 simulated pairs (tests/conftest.py: genome, reads_pe) under the two gated sets
GOLDEN = os.path.join(HERE, "golden", "msw_gated_sam.json")


@pytest.mark.parametrize("case", ["O0", "Oins0"])
def test_pipeline_without_insertion_open_penalty(engine, genome, reads_pe, case):
    """-O 0 and -O 6,0 end to end: the SAM of the session's 600 pairs equals the reference's (its recorded digest; the compiled
    reference itself where it is built), with mate rescue computed by the host."""
    kw = dict(flag=abi.MEM_F_PE, **{k: v for k, v in mc.options(case).items() if k in ("o_del", "o_ins")})
    ra = simulate.reads_to_ascii(reads_pe)
    got = engine.process(engine.opt(**kw), ra)
    assert engine.stats()["n_msw"] == 0
    with open(GOLDEN) as f:
        gold = json.load(f)[case]
    assert len(got) == gold["records"]
    if po.ref_available():
        ref = po.RefIndex(genome["prefix"])
        want = ref.process(ref.opt(**kw), ra)
        assert hashlib.sha256(b"".join(want)).hexdigest() == gold["sha256"]
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (i, a[:300], b[:300])
    assert hashlib.sha256(b"".join(got)).hexdigest() == gold["sha256"]
    # the kernels are back under the defaults, in the same process
    engine.process(engine.opt(flag=abi.MEM_F_PE), ra[:200])
    assert engine.stats()["n_msw"] > 0
