"""Worker of tests/test_gpu_msw_options.py: one option set of tests/msw_cases.py through Engine.matesw in a process of its own, so that
what launch_msw reads from the environment once per process (MPIBWA_MSW_PAIRS) can differ from the test session's.
usage: msw_worker.py <index prefix> <option set>; prints RESULT <json>, exit status 0 when every request equals the host's answer (and the
reference's, where it is built) and the cases reach their floors."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msw_cases as mc  # noqa: E402
from mpibwa_amd import api  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

prefix, name = sys.argv[1], sys.argv[2]
eng = api.Engine(prefix, device=0)
cs = mc.cases(name)
got, _ = eng.matesw(mc.set_opt(eng.opt(), name), *cs.matesw_args())
st = mc.compare(got, mc.want_from_host(eng.lib, cs))
if po.ref_available():
    mc.compare(got, mc.Want(cs, mc.reference_results(po.ref_lib(), cs), mc.host_results(eng.lib, cs, full_width=True)))
mc.check_coverage(name, cs, st)
print("RESULT " + json.dumps(dict(pairs_env=os.environ.get("MPIBWA_MSW_PAIRS"), n=int(st["n"]), hit=int(st["hit"]), ref=bool(po.ref_available()), flagged=int(got[:, 7].sum()))), flush=True)
