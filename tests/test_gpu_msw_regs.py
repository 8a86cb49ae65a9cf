"""The register form of msw2_kernel (one instantiation per segment length, launch_msw sorts the work items by it) on the requests of
tests/msw_regs_cases.py: exact equality with the library's host ksw_align2 and, where it is built, the compiled reference's; the same
records, byte for byte, from a process with MPIBWA_MSW_REGS=0 (everything in the general form); and one chunk of reads of two lengths
end to end against the reference's SAM."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msw_cases as mc
import msw_regs_cases as rc
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# sha256 and record count of the reference's SAM for two_length_reads() on the session's genome
GOLDEN = os.path.join(HERE, "golden", "msw_regs_sam.json")


def two_length_reads(genome):
    """300 pairs of 2 x 150 bp and 300 of 2 x 100 bp, pair by pair in turn: segment lengths 10 and 7 in one chunk"""
    a = simulate.reads_to_ascii(simulate.simulate_reads(genome["seqs"], 300, 150, paired=True, seed=31))
    b = simulate.reads_to_ascii(simulate.simulate_reads(genome["seqs"], 300, 100, paired=True, seed=32))
    return [("%s_%d" % (r[0], len(r[1])), r[1], r[2]) for pair in zip(a, b) for r in pair]


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()   # the device index is a process-wide singleton: (re)upload this module's genome
    return api.Engine(genome["prefix"], device=0)


@pytest.fixture(scope="module")
def switched_off(genome, tmp_path_factory):
    """the worker's records and SAM with MPIBWA_MSW_REGS=0 (read once per process: a child of its own)"""
    d = tmp_path_factory.mktemp("msw_regs")
    reads = str(d / "reads.json")
    with open(reads, "w") as f:
        json.dump([(n, a.decode(), b.decode()) for n, a, b in two_length_reads(genome)], f)
    out = str(d / "off.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "msw_regs_worker.py"), genome["prefix"], out, reads], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, MPIBWA_MSW_REGS="0"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["regs_env"] == "0" and res["n_msw"] > 0, res
    return np.load(out)


_GOT = {}


def records(engine, family, name):
    """Engine.matesw on a family, once per session"""
    if (family, name) not in _GOT:
        cs = rc.cases(family, name)
        _GOT[family, name] = engine.matesw(mc.set_opt(engine.opt(), name), *cs.matesw_args())[0]
    return _GOT[family, name]


@pytest.mark.parametrize("family,name", rc.all_cases())
def test_register_form_equals_ksw_align2(engine, family, name):
    assert os.environ.get("MPIBWA_MSW_REGS", "1") != "0"
    cs = rc.cases(family, name)
    got = records(engine, family, name)
    want = mc.want_from_host(engine.lib, cs)
    st = mc.compare(got, want)
    if po.ref_available():
        mc.compare(got, mc.Want(cs, mc.reference_results(po.ref_lib(), cs), mc.host_results(engine.lib, cs, full_width=True)))
    assert int(got[:, 7].sum()) == st["sat"], (family, name, st)
    plan, order = rc.launch_plan(cs)
    print("msw regs %s/%s: requests %d hits %d flagged %d; work items per launch %s, register launches in order %s" %
          (family, name, st["n"], st["hit"], st["sat"], {str(s): len(v) for s, v in plan.items()}, order))


@pytest.mark.parametrize("family,name", rc.all_cases())
def test_general_form_gives_the_same_bytes(engine, switched_off, family, name):
    got, off = records(engine, family, name), switched_off["%s/%s" % (family, name)]
    assert got.dtype == off.dtype and got.shape == off.shape and got.tobytes() == off.tobytes(), (family, name, np.nonzero((got != off).any(axis=1))[0][:10])


def test_chunk_of_two_read_lengths(engine, genome, switched_off):
    reads = two_length_reads(genome)
    assert {len(r[1]) for r in reads} == {100, 150}
    got = engine.process(engine.opt(flag=abi.MEM_F_PE), reads)
    assert engine.stats()["n_msw"] > 0
    sam = b"".join(got)
    with open(GOLDEN) as f:
        gold = json.load(f)
    if po.ref_available():
        ref = po.RefIndex(genome["prefix"])
        want = ref.process(ref.opt(flag=abi.MEM_F_PE), reads)
        assert hashlib.sha256(b"".join(want)).hexdigest() == gold["sha256"]
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (i, a[:300], b[:300])
    assert len(got) == gold["records"] and hashlib.sha256(sam).hexdigest() == gold["sha256"]
    assert sam == switched_off["sam"].tobytes()
