"""tests/msw_model.py — the kernels' recurrence in plain Python — against the reference's ksw_align2: equal under every option set the
device accepts, and different on recorded requests under o_ins = 0, which is why mbw::msw_on_device sends those options to the host."""
import numpy as np
import pytest

import msw_cases as mc
import msw_model as mm
from oracle import pyoracle as po

MAX_CELLS = 30000        # query length x window length of a case the model is run on
PER_SET = 30

# (option set, query, window, the reference's ksw_align2, the model) — recorded from the cases of the two gated sets
RECORDED = [
    ("O0", "CGGACTCTGCGTAAAG",
     "GATCATGTAGGCCTGCCTCAACTCTTACTCCGCGTCTCACAGCTAATCATCGGTTCCGGCAGCATGGCATTGATTGTCGTAACGGACTGTAAAGGTCTGATGCTGGCTCAAAAGTTCCTGACTTTCAAAATGCGCGCCAACTGAATTACCTGCTATTATATTCAGGCGGCTGGATGTCTAAGAACCGACGAGAGTGTTCGAGGATTATACCGGCAACGGGGGTACATCAACTGATTATGCTGTGGACGGACAATCGCCTTTGGAAGGAAACAATCC",
     [7, 81, 13, -1, -1, -1, -1], [8, 93, 15, -1, -1, -1, -1]),
    ("O0", "ACCAAGATAGGCTCGACTCGCGTCCGTCGGGCGTGAAGCCTAGCTGCCTGTTGCTTGCGTATGGCGAACCGCATCAGTTTCGTCTCAAGATGAAGGGTGTCGGGAACGGCAGAACATACGAGTG",
     "TACCAAACCTGGAGGTCATACACCAAGATAGGCTCGACTCGCGTCCGTCGGGCGTGAAGCCTATGCCTGTTGCTTGCGTATGGCGAACCGCATCAGTTTCGTCTCAAGATGAAGGGTGTCGGGAACGGCAGAACATACGAGTGAACCAGTTGAAAGCGTCACCA",
     [120, 142, 123, -1, -1, -1, -1], [120, 142, 123, -1, -1, 21, 0]),
    ("Oins0", "TCGAGACATATGAGACCCGACCGCAGCTGAAGT",
     "TTCCGGTCCCGATCGCCACTCTCGTCGAGACATATGAGACCCGACCGCATGAAGTACTCGGGTAGAAACGTAATCGGTCCGTTGAATGGTTGCTTGTGGTCTGTTATTAC",
     [29, 54, 32, -1, -1, -1, -1], [29, 54, 32, -1, -1, 24, 0]),
    ("Oins0", "AGGGAAAAACTTCAGA",
     "CCGGATTTATATTCCTATGTAGAACCGAGTGTGCCGGTTACCGACAGGTCCCCTTATCGCATCCCTAGTCACCTGACACGGTACTGAAACAGGGAATTCAGAGAGATAACCTCGAGCACATGGCCCCGAACCTGCAAGGGT",
     [7, 101, 15, -1, -1, -1, -1], [8, 101, 15, -1, -1, -1, -1]),
]


def _model(cs, q, win):
    o = cs.o
    return mm.align2(q, win, cs.mat, o["a"], o["o_del"], o["e_del"], o["o_ins"], o["e_ins"], o["min_seed_len"])


def _short_cases(cs):
    """up to PER_SET requests of at most MAX_CELLS cells, taken kind by kind so that every kind of request is among them"""
    by_kind = {}
    for i in range(len(cs)):
        if len(cs.reads[cs.rd[i]]) * (cs.re[i] - cs.rb[i]) <= MAX_CELLS and cs.re[i] > cs.rb[i]:
            by_kind.setdefault(cs.kind[i].split(":")[0], []).append(i)
    out = []
    while len(out) < PER_SET and any(by_kind.values()):
        for k in sorted(by_kind):
            if by_kind[k] and len(out) < PER_SET:
                out.append(by_kind[k].pop(0))
    return out


@pytest.mark.parametrize("name", [n for n in mc.OPTION_SETS if n not in mc.GATED])
def test_model_equals_reference_where_the_device_runs(built, name):
    if not po.ref_available():
        pytest.skip("the reference library is not built")
    cs = mc.cases(name)
    ref = mc.reference_results(po.ref_lib(), cs)
    dref = cs.dref
    minsc = cs.o["min_seed_len"] * cs.o["a"]
    n = n_hit = 0
    for i in _short_cases(cs):
        m = _model(cs, cs.query(i), dref[cs.rb[i]:cs.re[i]])
        if m is None:          # the byte flavour's ceiling: the host's request
            continue
        w = [int(x) for x in ref[i]]
        if w[0] < minsc:
            assert m[0] == w[0] and m[5] == -1 and m[6] == -1, (name, i, cs.kind[i], m, w)
        else:
            assert m == w, (name, i, cs.kind[i], m, w)
            n_hit += 1
        n += 1
    assert n >= 20 and n_hit >= 8, (name, n, n_hit)


def test_model_departs_from_reference_without_insertion_open_penalty(built):
    """The reason for the gate, on record: under o_ins = 0 the closed form gives another forward score (first and last case) or finds a
    start where the reference's reverse pass falls short of the forward score (the other two).  The recorded reference results are
    checked against the compiled reference where it is there."""
    code = {c: i for i, c in enumerate("ACGTN")}
    for name, qs, ws, want, model in RECORDED:
        assert name in mc.GATED
        cs = mc.Cases(name)
        q = np.array([code[c] for c in qs], dtype=np.uint8)
        win = np.array([code[c] for c in ws], dtype=np.uint8)
        assert _model(cs, q, win) == model and model != want
        if po.ref_available():
            cs.reads, cs.rb, cs.re, cs.rd, cs.rev, cs.fwd = [q], [0], [len(win)], [0], [0], win
            assert [int(x) for x in mc.reference_results(po.ref_lib(), cs)[0]] == want
