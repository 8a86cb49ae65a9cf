"""Single-end leg next to bench.py: trimmed single-end reads (BASELINE config 3: lengths uniform 50-300) through mem_process_seqs with
the device path of the stage after the CIGAR kernel (se_simple_kernel, se_wave_kernel, single-end sam_emit_kernel), with
MPIBWA_HOST_SE_WAVE=1 (se_simple_kernel alone: reads with more than eight regions or an XA tag stay on the host) and with
MPIBWA_HOST_SE=1 (the host path: what the library did before it had either), alternately, on the same chunks.  --legs chooses among
them and "nosupp" (MPIBWA_HOST_SUPP=1: reads with supplementary lines stay on the host).

    python tools/bench_se.py [--reads N] [--chunks C] [--steps K] [--repeats R] [--genome-mbp M] [--chimeric-frac F] [--legs a,b] [--out FILE]

--chimeric-frac F makes that share of the reads chimeric: two or three segments of at least 40 bases, each cut from a read of the
generator that lies elsewhere in the genome, every second one reverse-complemented — reads whose record has supplementary lines.

The reads come from the generator and the index cache bench.py uses (bigindex.make_or_get / simulate_pairs with 300-base reads; read 1 of
every pair, cut to a seeded length in [50, 300]).  Every leg is a fresh child process under its own `timeout`; the run stops at the
first leg that fails.  One JSON line per leg: Mreads/s, emit_ms and plan_ms per chunk, host CPU-seconds per chunk, n_se_dev / n_reads,
n_sam_dev / n_reads, n_se_wave_dev, n_se_xa_dev, n_se_xa_sam_dev, n_se_supp_dev and n_se_supp_sam_dev per chunk, and a hash of the SAM of all chunks, which must be the
same in every leg.  A last child (one step, MPIBWA_CPUSEC=1) reports the status codes of the two deciding kernels."""
import argparse
import hashlib
import json
import os
import re
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def chimeric(reads, lens, frac, rng):
    """reads: [(name, ASCII read of 300 bases, None)], lens: the lengths they are cut to -> the cut reads, a share `frac` of them put
    together from 2 or 3 segments (each at least 40 bases) of other reads of the chunk: other places, every second one the other strand"""
    import numpy as np
    out = []
    n = len(reads)
    for (name, a, _), ln in zip(reads, lens):
        ln = int(ln)
        k = 3 if ln >= 150 and rng.random() < 0.5 else 2
        if frac <= 0 or rng.random() >= frac or ln < 40 * k:
            out.append((name, a[:ln], None))
            continue
        if k == 2:
            cuts = [int(rng.choice(np.arange(40, ln - 40 + 1, dtype=np.int64), size=1)[0])]
        else:
            c0 = int(rng.integers(40, ln - 80 + 1))
            cuts = [c0, int(rng.integers(c0 + 40, ln - 40 + 1))]
        edges = [0] + cuts + [ln]
        parts = []
        for j in range(k):
            src = reads[int(rng.integers(n))][1] if j else a
            seg = src[edges[j]:edges[j + 1]]
            parts.append(seg[::-1].translate(_RC) if j % 2 else seg)
        out.append((name, b"".join(parts), None))
    return out


def child(args):
    import numpy as np
    from mpibwa_amd import abi, api, bigindex
    os.makedirs(args.workdir, exist_ok=True)
    idx = bigindex.make_or_get(args.workdir, genome_mbp=args.genome_mbp, seed=38, log=log, repeat_frac=args.repeat_frac, model=args.genome_model)
    eng = idx.engine
    lib = api.load_library(build_if_missing=False)
    batches = []
    for c in range(args.chunks):
        rng = np.random.default_rng(args.seed + 100 + c)
        pairs = idx.simulate_pairs(args.reads, seed=args.seed + c, read_len=300, frag_mean=660.0)
        lens = rng.integers(50, 301, size=len(pairs))
        batches.append(abi.SeqBatch(api.libc, chimeric(pairs, lens, args.chimeric_frac, rng)))
    opt = eng.opt(flag=0, n_threads=int(lib.mi355x_host_cpus()))
    import ctypes as C
    C.c_int.in_dll(eng.lib, "bwa_verbose").value = 1
    # one pass over the chunks: the hash of their SAM, and the work buffers of the call context grow to their size
    h = hashlib.sha256()
    for c in range(args.chunks):
        eng.process_batch(opt, batches[c], n_processed=c * args.reads)
        h.update(eng.collect_sam(batches[c]))
    acc, wall, cpu = {}, 0.0, 0.0
    for s in range(args.steps):
        c = s % args.chunks
        ru0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
        eng.process_batch(opt, batches[c], n_processed=c * args.reads)
        t1, ru1 = time.perf_counter(), resource.getrusage(resource.RUSAGE_SELF)
        wall += t1 - t0
        cpu += (ru1.ru_utime + ru1.ru_stime) - (ru0.ru_utime + ru0.ru_stime)
        for k, v in eng.stats().items():
            acc[k] = acc.get(k, 0) + v
        eng.collect_sam(batches[c])   # (the caller's writer: outside the timed region)
    n = max(1, args.steps)
    print(json.dumps({
        "leg": args.leg, "rep": args.rep, "workload": "single-end, lengths uniform 50-300, %d chunks x %d reads vs %d Mbp (%s)" %
        (args.chunks, args.reads, int(args.genome_mbp), args.genome_model) + (", %g of the reads chimeric" % args.chimeric_frac if args.chimeric_frac > 0 else ""),
        "steps": args.steps,
        "mreads_s": round(acc.get("n_reads", 0) / wall / 1e6, 4), "ms_per_chunk": round(wall / n * 1e3, 2),
        "emit_ms": round(acc.get("emit_ms", 0) / n, 2), "plan_ms": round(acc.get("plan_ms", 0) / n, 2),
        "host_cpu_s_per_chunk": round(cpu / n, 3),
        "se_dev_frac": round(acc.get("n_se_dev", 0) / max(1, acc.get("n_reads", 1)), 4),
        "sam_dev_frac": round(acc.get("n_sam_dev", 0) / max(1, acc.get("n_reads", 1)), 4),
        "se_wave_dev_per_chunk": round(acc.get("n_se_wave_dev", 0) / n, 1), "se_xa_dev_per_chunk": round(acc.get("n_se_xa_dev", 0) / n, 1),
        "se_xa_sam_dev_per_chunk": round(acc.get("n_se_xa_sam_dev", 0) / n, 1),
        "se_supp_dev_per_chunk": round(acc.get("n_se_supp_dev", 0) / n, 1), "se_supp_sam_dev_per_chunk": round(acc.get("n_se_supp_sam_dev", 0) / n, 1),
        "sam_sha256": h.hexdigest()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=300000, help="reads per chunk")
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9, help="timed calls per leg (after one untimed pass over the chunks)")
    ap.add_argument("--repeats", type=int, default=2, help="alternations host / device")
    ap.add_argument("--seed", type=int, default=3000)
    ap.add_argument("--genome-mbp", type=float, default=float(os.environ.get("MPIBWA_BENCH_GENOME_MBP", "3100")))
    ap.add_argument("--repeat-frac", type=float, default=float(os.environ.get("MPIBWA_BENCH_REPEAT_FRAC", "0.05")))
    ap.add_argument("--genome-model", default=os.environ.get("MPIBWA_BENCH_GENOME_MODEL", "grch38like"))
    ap.add_argument("--workdir", default=os.environ.get("MPIBWA_BENCH_DIR", "/tmp/mpibwa_bench"))
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a leg may take (index load included)")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--chimeric-frac", type=float, default=0.0, help="share of the reads put together from 2 or 3 segments of different places and strands")
    ap.add_argument("--legs", default="host,nowave,dev", help="the legs of a round, of host, nowave, nosupp, dev")
    ap.add_argument("--leg", choices=["host", "nowave", "nosupp", "dev", "codes"], help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    lines = []
    passthrough = ["--reads", str(args.reads), "--chunks", str(args.chunks), "--seed", str(args.seed), "--genome-mbp", str(args.genome_mbp),
                   "--repeat-frac", str(args.repeat_frac), "--genome-model", args.genome_model, "--workdir", args.workdir, "--chimeric-frac", str(args.chimeric_frac)]
    names = [x for x in args.legs.split(",") if x]
    if not names or any(x not in ("host", "nowave", "nosupp", "dev") for x in names):
        ap.error("--legs: a comma-separated choice of host, nowave, nosupp, dev")
    legs = [(leg, rep) for rep in range(args.repeats) for leg in names] + [("codes", 0)]
    for leg, rep in legs:
        env = dict(os.environ)
        env.pop("MPIBWA_HOST_SE", None)
        env.pop("MPIBWA_HOST_SE_WAVE", None)
        env.pop("MPIBWA_CPUSEC", None)
        env.pop("MPIBWA_HOST_SUPP", None)
        if leg == "nosupp":
            env["MPIBWA_HOST_SUPP"] = "1"
        if leg == "host":
            env["MPIBWA_HOST_SE"] = "1"
        if leg == "nowave":
            env["MPIBWA_HOST_SE_WAVE"] = "1"
        if leg == "codes":
            env["MPIBWA_CPUSEC"] = "1"
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rep", str(rep),
               "--steps", "1" if leg == "codes" else str(args.steps)] + passthrough
        # (the timed legs report their progress — genome, index, reads — on this process's stderr; the last one's is read for its line)
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE if leg == "codes" else None, text=True)
        if p.returncode != 0:
            log((p.stderr or "")[-4000:])
            log("leg %s (repeat %d) ended with status %d: stopping here" % (leg, rep, p.returncode))
            return 1
        rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        if leg == "codes":
            m = [ln for ln in p.stderr.splitlines() if ln.startswith("[se_kernel]")]
            rec = {"leg": "status codes of se_simple_kernel and se_wave_kernel, last chunk", "line": m[-1] if m else None, "sam_sha256": rec["sam_sha256"]}
            if m:
                rec["counts"] = {k.strip(" ;:").replace("host: ", ""): int(v) for k, v in re.findall(r"([a-zA-Z>: ][a-zA-Z0-9>: ]*?) (\d+)(?=[,;]|$)", m[-1].split(":", 1)[1])}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    same = len({r["sam_sha256"] for r in lines}) == 1
    by = {leg: [r for r in lines if r["leg"] == leg] for leg in names}
    summary = {"leg": "summary", "sam_identical_across_legs": same}
    for leg in names:
        summary[leg + "_mreads_s"] = [r["mreads_s"] for r in by[leg]]
        summary[leg + "_cpu_s_per_chunk"] = [r["host_cpu_s_per_chunk"] for r in by[leg]]
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    return 0 if same else 2


if __name__ == "__main__":
    sys.exit(main())
