"""Time of the init stage's tail (confidence ranking, co-visibility masks, ordered compaction) at two sizes, 3 x 512 x 288 and
12 x 512 x 288 pointmaps (tests/init_stage_util.py's seeded generator), two forms:
  (a) host:  the numpy restatement of the reference's loop over the views (init_stage_util.covis_numpy: projection in float64, the
      reference's arithmetic) and numpy's boolean indexing (compact_numpy), on host arrays;
  (b) fused: ONE init_stage.init_from_pointmaps call on device tensors without the file writing (source_path None): statistics,
      the read-back of the ranking, masks, compaction and the read of the count — six kernel dispatches.
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock; the medians and
every repetition are reported, and the two forms must agree (masks and counts equal).  Prints one JSON line.
  --fused-only   warm-up and ONE fused call per size (for `rocprofv3 --kernel-trace --stats`)
Measurement helper, not product code."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fused-only", action="store_true")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd.init_stage import confidence_ranking, init_from_pointmaps  # noqa: E402
from tests import init_stage_util as iu  # noqa: E402

dev = torch.device("cuda:0")
THR = 0.01
SETS = {"v3_512x288": iu.synthetic_views(3, 288, 512, 14), "v12_512x288": iu.synthetic_views(12, 288, 512, 15)}


def host(d):
    c = d["confidences"]
    order = confidence_ranking(c.astype(np.float64).sum(axis=(1, 2)), c.shape[1], c.shape[2]).tolist()
    masks = iu.covis_numpy(order, d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], THR)
    p, _, _ = iu.compact_numpy(d["pointmaps"], d["images"], d["confidences"], masks)
    return masks, p.shape[0]


def fused(t, d):
    r = init_from_pointmaps(None, t["depthmaps"].shape[0], t["images"], t["pointmaps"], t["depthmaps"], t["confidences"], t["intrinsics"],
                            t["w2c"], d["focals"], (2048, 1152), depth_threshold=THR, conf_aware_ranking=True)
    return r["keep_masks"], r["pts_num"]["co_mask_dsp"]


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


out = {"depth_threshold": THR, "reps": a.reps, "sets": {}}
for name, d in SETS.items():
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items() if k != "focals"}
    keep, M = fused(t, d)   # warm-up
    if a.fused_only:
        out["sets"][name] = {"points": int(d["depthmaps"].size), "kept": int(M), "ms_fused_single_run": timed(fused, t, d)[0]}
        continue
    masks, Mh = host(d)     # warm-up, and the two forms must agree
    assert Mh == M and np.array_equal(~keep.cpu().numpy(), masks), name
    ms = {"host": [], "fused": []}
    for _ in range(a.reps):
        ms["host"].append(timed(host, d)[0])
        ms["fused"].append(timed(fused, t, d)[0])
    mh, mf = statistics.median(ms["host"]), statistics.median(ms["fused"])
    out["sets"][name] = {"views": int(d["depthmaps"].shape[0]), "H": int(d["depthmaps"].shape[1]), "W": int(d["depthmaps"].shape[2]),
                         "points": int(d["depthmaps"].size), "kept": int(M), "masks_equal": True,
                         "ms_host": mh, "ms_host_runs": ms["host"], "ms_fused": mf, "ms_fused_runs": ms["fused"], "speedup": mh / mf}
print(json.dumps(out), flush=True)
