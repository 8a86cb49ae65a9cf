"""The row loop of wave_extend (one-strip rows, rows of several strips, the switch between the two, empty rows) against the
oracle's ksw_extend2, through mi355x_extend_batch2: every row the reference computes (early = 0), and the loop c2a_kernel runs
(early = 1: it stops as soon as nothing mem_chain2aln reads can change, given the clipping penalty)."""
import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

QLENS = [1, 2, 17, 62, 63, 64, 65, 66, 126, 127, 128, 129, 131, 150]
BANDS = [3, 7, 40, 100]
N_JOBS = 2016          # every (kind, qlen) pair 16 times over, every (kind, qlen, w) four times
KINDS = ["same", "chance", "indel", "noisy", "short_target", "ambiguous", "low_h0", "indel_low_h0", "indel_far"]


def _job(rng, kind, qlen):
    """(query, target, h0) of one extension"""
    q = rng.integers(0, 4, size=qlen, dtype=np.uint8)
    tail = rng.integers(0, 4, size=int(rng.integers(0, 50)), dtype=np.uint8)
    h0 = int(rng.integers(30, 180))
    if kind == "same":                  # full-width rows: the live range only grows
        t, h0 = np.concatenate([q, tail]), int(rng.integers(100, 200))
    elif kind == "chance":              # a chance hit: the live range shrinks to nothing within a few rows
        t, h0 = rng.integers(0, 4, size=max(1, qlen + int(rng.integers(-5, 40))), dtype=np.uint8), int(rng.integers(19, 31))
    elif kind in ("indel", "indel_low_h0", "indel_far"):
        # one insertion or deletion of 1-40 bases: the live range moves across the border between one strip and two
        # (columns 63 / 64), growing and shrinking, from one row to the next
        g = int(rng.integers(1, 41))
        at = int(rng.integers(0, qlen + 1)) if kind == "indel_far" else int(np.clip(64 + rng.integers(-30, 31), 0, qlen))
        if rng.random() < 0.5:
            t = np.concatenate([q[:at], rng.integers(0, 4, size=g, dtype=np.uint8), q[at:], tail])
        else:
            t = np.concatenate([q[:at], q[at + g:], tail])
        if len(t) == 0:
            t = tail if len(tail) else np.zeros(1, np.uint8)
        h0 = int(rng.integers(20, 60)) if kind == "indel_low_h0" else int(rng.integers(60, 200))
    elif kind == "noisy":
        t = np.concatenate([q, tail])
        mut = rng.random(len(t)) < float(rng.choice([0.01, 0.05, 0.15, 0.4]))
        t[mut] = rng.integers(0, 4, size=int(mut.sum()))
        h0 = int(rng.integers(1, 180))
    elif kind == "short_target":        # tlen < qlen
        t = q[:max(1, int(rng.integers(1, qlen + 1)) - 1)].copy() if qlen > 1 else rng.integers(0, 4, size=1, dtype=np.uint8)
    elif kind == "ambiguous":
        t = np.concatenate([q, tail])
        if rng.random() < 0.5:
            q = q.copy()
            q[rng.integers(0, qlen)] = 4
        else:
            t[rng.integers(0, len(t))] = 4
    elif kind == "low_h0":              # the first row is partly zero
        t, h0 = np.concatenate([q, tail]), int(rng.choice([1, 5, 6, 7]))
    return q, np.ascontiguousarray(t, dtype=np.uint8), h0


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    return api.Engine(genome["prefix"], device=0)


@pytest.fixture(scope="module")
def jobs(engine):
    """the jobs and what the oracle says about each, computed once"""
    opt = engine.opt()
    o = opt.contents
    mat = np.array(list(o.mat), dtype=np.int8)
    rng = np.random.default_rng(77)
    qs, ts, ws, h0s, ebs, kinds = [], [], [], [], [], []
    for it in range(N_JOBS):
        kind, qlen = KINDS[it % len(KINDS)], QLENS[(it // len(KINDS)) % len(QLENS)]
        q, t, h0 = _job(rng, kind, qlen)
        qs.append(q); ts.append(t); h0s.append(h0); kinds.append(kind)
        ws.append(BANDS[(it // (len(KINDS) * len(QLENS))) % len(BANDS)])
        ebs.append(int(rng.choice([5, 0])))
    want = np.zeros((N_JOBS, 6), dtype=np.int64)
    cells = np.zeros(N_JOBS, dtype=np.int64)
    for i in range(N_JOBS):
        r, c = po.oracle_extend2(qs[i], ts[i], mat, o.o_del, o.e_del, o.o_ins, o.e_ins, ws[i], ebs[i], o.zdrop, h0s[i])
        want[i] = r
        cells[i] = c
    want.setflags(write=False)
    cells.setflags(write=False)
    return dict(opt=opt, qs=qs, ts=ts, ws=ws, h0s=h0s, ebs=ebs, kinds=kinds, want=want, cells=cells)


def test_jobs_cover_the_cases(jobs):
    qs, ts, ws, h0s, kinds = jobs["qs"], jobs["ts"], jobs["ws"], jobs["h0s"], jobs["kinds"]
    assert {len(q) for q in qs} == set(QLENS) and set(ws) == set(BANDS) and set(kinds) == set(KINDS)
    for ql in QLENS:
        assert {k for k, q in zip(kinds, qs) if len(q) == ql} == set(KINDS)
        assert {w for w, q in zip(ws, qs) if len(q) == ql} == set(BANDS)
    assert any(len(t) < len(q) for q, t in zip(qs, ts))
    assert any((q == 4).any() for q in qs) and any((t == 4).any() for t in ts)
    assert {1, 5, 6, 7} <= set(h0s) and any(19 <= h <= 30 for h, k in zip(h0s, kinds) if k == "chance")
    # the oracle's cell counts say that rows of every shape occur: extensions that die within a few rows, and ones whose rows
    # are wider than a strip (more cells than 64 per row of the target)
    cells = jobs["cells"]
    assert (cells[[k == "chance" for k in kinds]] < 64).any()
    assert any(c > 64 * len(t) for c, t in zip(cells, ts))


def test_every_row_matches_oracle(engine, jobs):
    got, ms, cells = engine.extend2(jobs["opt"], jobs["qs"], jobs["ts"], jobs["ws"], jobs["h0s"], jobs["ebs"], 0, 0)
    want = jobs["want"]
    for i in np.flatnonzero((got != want).any(axis=1))[:5]:
        print(i, jobs["kinds"][i], len(jobs["qs"][i]), len(jobs["ts"][i]), jobs["ws"][i], jobs["h0s"][i], got[i], want[i])
    assert (got == want).all()
    assert int(cells.sum()) == int(jobs["cells"].sum())


@pytest.mark.parametrize("clip", [5, 0])
def test_early_rows_match_oracle_in_what_the_caller_reads(engine, jobs, clip):
    got, ms, cells = engine.extend2(jobs["opt"], jobs["qs"], jobs["ts"], jobs["ws"], jobs["h0s"], jobs["ebs"], 1, clip)
    want = jobs["want"]
    SCORE, QLE, TLE, GTLE, GSCORE, MAX_OFF = range(6)

    def local(r):
        return (r[:, GSCORE] <= 0) | (r[:, GSCORE] <= r[:, SCORE] - clip)
    bad = (got[:, [SCORE, QLE, TLE, MAX_OFF]] != want[:, [SCORE, QLE, TLE, MAX_OFF]]).any(axis=1) | (local(got) != local(want))
    glob = ~local(want)
    bad |= glob & ((got[:, GSCORE] != want[:, GSCORE]) | (got[:, GTLE] != want[:, GTLE]))
    for i in np.flatnonzero(bad)[:5]:
        print(i, jobs["kinds"][i], len(jobs["qs"][i]), len(jobs["ts"][i]), jobs["ws"][i], jobs["h0s"][i], got[i], want[i])
    assert not bad.any()
    # both decisions occur (with clip = 0 every extension is "local": the score at the query end never beats the best cell)
    assert (~glob).any() and (glob.any() or clip == 0)
    assert int(cells.sum()) <= int(jobs["cells"].sum())
