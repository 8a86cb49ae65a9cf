"""Stage test of the redundancy pass on the device: dedup_small_kernel and dedup_wave_kernel through mi355x_dedup_batch (the pipeline's
own launch sequence) against the reference's OWN mem_sort_dedup_patch (oracle/_ref/libbwaref.so, called with the sequences, the way
tests/se_stage_cases.py calls it), on the cases of tests/dedup_cases.py — tests/test_dedup_cases.py shows on the CPU that every family
reaches its branch.

Per option set (default; mask_level_redun = 0.8, w = 40; max_chain_gap = 300), for every read of every family:
  * the invariant: a taken read's regs[keep[:m]] is the reference's result, in number and in all 11 fields (rb ... frac_rep) — so
    wherever the reference merged two regions, the read was declined;
  * the statuses the families same_span, far and patch are built for: taken up to mi355x_dedup_maxreg() regions, 3 above it, 4 where
    the reference merged;
  * keep entries past m, and the whole span of a declined read, still hold the caller's fill pattern;
  * on `random` the kernel takes at least half of the lists with two or more regions (the share is printed; no floor on `mixed`);
  * launches of 1, 7, 8, 9, 63, 64 and 65 reads, and launches whose reads are all of one class (lane-per-read only, wavefront-per-read
    only)."""
import numpy as np
import pytest

import dedup_cases as dc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

_SETS = {}


@pytest.fixture(scope="module")
def stage(genome):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api
    lib = api.load_library()
    assert hasattr(lib, "mi355x_dedup_batch") and int(lib.mi355x_dedup_maxreg()) == dc.CAP and int(lib.mi355x_pair_maxreg()) == dc.SMALL
    return {"eng": api.Engine(genome["prefix"], upload=False), "ref": po.RefIndex(genome["prefix"]), "prefix": genome["prefix"], "seqs": genome["seqs"]}


def the_set(stage, name):
    """cases and the reference's results of an option set, computed once and left unchanged"""
    if name not in _SETS:
        kw = dc.OPTION_SETS[name]
        ropt = stage["ref"].opt(**kw)
        ix = dc.Index(stage["prefix"], stage["ref"].bns)
        cases, want = dc.full_set(stage["ref"], ropt, ix, stage["seqs"])
        _SETS[name] = (stage["eng"].opt(**kw), cases, want)
    return _SETS[name]


def check(eng, cases, want, status, m, keep, tag):
    """the invariant and the fill pattern -> indices of the taken reads"""
    taken = []
    for i, cs in enumerate(cases):
        raw, k = cs["regs"], keep[i]
        st = int(status[i])
        assert len(k) == len(raw)
        if st != eng.DD_TAKEN:
            assert st in (eng.DD_HOST_MAXREG, eng.DD_HOST_PATCH) and int(m[i]) == -1, (tag, i, cs["family"], cs["tag"], st, int(m[i]))
            assert (k == eng.DD_FILL).all(), (tag, i, cs["family"], "the span of a declined read was written")
            continue
        taken.append(i)
        mi = int(m[i])
        assert 0 <= mi <= len(raw) and (k[mi:] == eng.DD_FILL).all(), (tag, i, cs["family"], cs["tag"], mi, len(raw), k)
        sel = k[:mi]
        assert ((sel >= 0) & (sel < max(1, len(raw)))).all() and len(set(sel.tolist())) == mi, (tag, i, cs["family"], sel)
        got = raw[sel]
        assert mi == len(want[i]), (tag, i, cs["family"], cs["tag"], mi, len(want[i]))
        for f in dc.FIELDS:
            assert (got[f] == want[i][f]).all(), (tag, i, cs["family"], cs["tag"], f, got[f], want[i][f])
        if len(raw) <= 1:
            assert mi == len(raw)
    return taken


def to_reg_dt(eng, a):
    """ALNREG_DT -> REG_DT, field by field"""
    out = np.zeros(len(a), dtype=eng.REG_DT)
    for f in dc.FIELDS:
        out[f] = a[f]
    return out


def run(stage, opt, cases):
    eng = stage["eng"]
    return eng.dedup(opt, [to_reg_dt(eng, cs["regs"]) for cs in cases])


@pytest.mark.parametrize("name", list(dc.OPTION_SETS))
def test_dedup_stage_matches_mem_sort_dedup_patch(stage, name):
    eng = stage["eng"]
    opt, cases, want = the_set(stage, name)
    status, m, keep = run(stage, opt, cases)
    taken = set(check(eng, cases, want, status, m, keep, name))
    codes = {int(c): int((status == c).sum()) for c in np.unique(status)}
    print(name, "reads", len(cases), "taken", len(taken), "status codes", codes, "kernels %.3f ms" % eng.last_dedup_ms)
    code = dict(taken=eng.DD_TAKEN, maxreg=eng.DD_HOST_MAXREG, patch=eng.DD_HOST_PATCH)
    n_exp = 0
    for i, cs in enumerate(cases):
        if cs["family"] in ("same_span", "far", "patch") and cs["expect"] is not None:
            n_exp += 1
            assert int(status[i]) == code[cs["expect"]], (name, i, cs["family"], cs["tag"], cs["expect"], int(status[i]))
        if cs["family"] == "patch" and cs.get("merged"):
            assert i not in taken
    assert n_exp >= 90 + 28 + 20
    # both kernels took reads, and lists where the order of equal keys shows
    assert any(len(cases[i]["regs"]) > dc.SMALL for i in taken) and any(2 <= len(cases[i]["regs"]) <= dc.SMALL for i in taken)
    # the floor on the random lists
    rnd = [i for i, cs in enumerate(cases) if cs["family"] == "random" and len(cs["regs"]) >= 2]
    got = sum(i in taken for i in rnd)
    mixed = [i for i, cs in enumerate(cases) if cs["family"] == "mixed"]
    print(name, "random lists with two or more regions", len(rnd), "taken", got, "share %.3f" % (got / max(1, len(rnd))),
          "| mixed", len(mixed), "taken", sum(i in taken for i in mixed))
    assert len(rnd) >= 1000 and got >= len(rnd) / 2, (name, got, len(rnd), codes)


def test_dedup_stage_launch_shapes(stage):
    eng = stage["eng"]
    opt, cases, want = the_set(stage, "default")
    synth = [i for i, cs in enumerate(cases) if cs["family"] != "random"]
    for n in (1, 7, 8, 9, 63, 64, 65):
        for start in (0, 11):
            idx = synth[start:start + n]
            sub, w = [cases[i] for i in idx], [want[i] for i in idx]
            status, m, keep = run(stage, opt, sub)
            check(eng, sub, w, status, m, keep, "%d reads from %d" % (n, start))
    small = [i for i, cs in enumerate(cases) if len(cs["regs"]) <= dc.SMALL][:200]
    wave = [i for i, cs in enumerate(cases) if dc.SMALL < len(cs["regs"]) <= dc.CAP]
    over = [i for i, cs in enumerate(cases) if len(cs["regs"]) > dc.CAP]
    assert len(small) == 200 and len(wave) >= 70 and over
    for tag, idx in (("lane per read only", small), ("wavefront per read only", wave), ("past the cap only", over)):
        sub, w = [cases[i] for i in idx], [want[i] for i in idx]
        status, m, keep = run(stage, opt, sub)
        tk = check(eng, sub, w, status, m, keep, tag)
        print(tag, "reads", len(sub), "taken", len(tk))
        if tag == "past the cap only":
            assert not tk and (status == eng.DD_HOST_MAXREG).all()
        else:
            assert tk


@pytest.mark.parametrize("name", list(dc.OPTION_SETS))
def test_dedup_wave_kernel_sorts_on_lists_that_reach_the_comb_sort(stage, name):
    """ks_introsort_at in dedup_wave_kernel where its depth budget runs out: the lists of dedup_cases.sorted_cases take the first (sorted_re) or the second
    sort (sorted_score) of dedup_wave_kernel into ks_introsort's comb sort with equal keys in the range — the regions the pass keeps,
    or the twin that stays, are the comb sort's order (tests/test_introsort_model.py).  Every list is taken and is the reference's
    result in the reference's order.  The launch holds these lists alone, so a wavefront goes from one comb-sorted read to the next
    over the same LDS arrays and frame stack; a second launch has them among the other families."""
    eng = stage["eng"]
    kw = dc.OPTION_SETS[name]
    ix = dc.Index(stage["prefix"], stage["ref"].bns)
    cases = dc.sorted_cases(ix)
    want = dc.reference_results(stage["ref"], stage["ref"].opt(**kw), cases, True)
    opt = eng.opt(**kw)
    assert all(dc.SMALL < len(cs["regs"]) <= dc.CAP for cs in cases) and {cs["family"] for cs in cases} == {"sorted_re", "sorted_score"}
    status, m, keep = run(stage, opt, cases)
    for i, cs in enumerate(cases):
        assert int(status[i]) == eng.DD_TAKEN, (name, cs["family"], cs["tag"], int(status[i]))
    assert len(check(eng, cases, want, status, m, keep, name + " sorted only")) == len(cases)
    _, others, want_o = the_set(stage, name)
    idx = [i for i, cs in enumerate(others) if cs["family"] in ("same_span", "mixed", "far")][:120]
    mixed, want_m = [], []
    for k, cs in enumerate(cases):
        mixed += [cs] + [others[i] for i in idx[3 * k % len(idx):][:2]]
        want_m += [want[k]] + [want_o[i] for i in idx[3 * k % len(idx):][:2]]
    status, m, keep = run(stage, opt, mixed)
    taken = set(check(eng, mixed, want_m, status, m, keep, name + " sorted among others"))
    assert all(i in taken for i, cs in enumerate(mixed) if cs["family"].startswith("sorted_"))
