"""Worker of tests/test_gpu_msw_rev.py: a process of its own, so that what launch_msw reads from the environment once per process
(MPIBWA_MSW_REV2) can differ from the test session's.
usage: msw_rev_worker.py <index prefix> <out.npz>
Writes Engine.matesw's records of every family and option set of tests/msw_rev_cases.py (key "<family>/<option set>") and what the
second pass ran (key "counts/<family>/<option set>") to out.npz; prints RESULT <json>."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msw_cases as mc  # noqa: E402
import msw_rev_cases as rv  # noqa: E402
from mpibwa_amd import api  # noqa: E402

prefix, out = sys.argv[1], sys.argv[2]
eng = api.Engine(prefix, device=0)
res = {}
for family, name in rv.all_cases():
    cs = rv.cases(family, name)
    res["%s/%s" % (family, name)] = eng.matesw(mc.set_opt(eng.opt(), name), *cs.matesw_args())[0]
    res["counts/%s/%s" % (family, name)] = np.array(eng.matesw_counts(), dtype=np.int64)
np.savez(out, **res)
print("RESULT " + json.dumps(dict(rev2_env=os.environ.get("MPIBWA_MSW_REV2"), sets=len(res) // 2)), flush=True)
