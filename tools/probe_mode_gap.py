#!/usr/bin/env python3
"""Where does a measure gap between QREC_MODE=exact and =throughput of a pairwise graph model come from?  The two modes differ in
(a) the batch stream (CPython replay vs device Philox) and (b) the reduction order of the batch gradients (ordered vs float atomics).
Runs the drop-in class on the FilmTrust golden rows over S sampling streams for each of the four combinations and prints the measures.

    python tools/probe_mode_gap.py NGCF 8 20      (model, streams, epochs)

With --paired the two modes run on the SAME stream instead (tests/device_stream.py: exact mode replays on the host the stream the
throughput mode draws on the device), QREC_REDUCTIONS=ordered in both, so that the gap is a per-seed difference and not a difference of
two noisy means.  Prints one JSON object (profiles/r07_paired_mode_gap.json): per model the bytes of the final tables and measure
strings that differ, summed over the seeds, and the paired Recall@10 gap, mean +- standard error over S seeds.

    python tools/probe_mode_gap.py --paired 8 20 LightGCN NGCF SimGCL      (seeds, epochs, models)
"""
import io
import json
import os
import random
import sys
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import conf_from_text, load_golden, rows_from_golden      # noqa: E402
from qrec_amd.QRec import resolve_model                                # noqa: E402

if sys.argv[1] == "--paired":
    import device_stream as DS
    S, epochs, names = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:]
    out = dict(what="QREC_MODE=throughput vs QREC_MODE=exact replaying the same device stream on the host, QREC_REDUCTIONS=ordered in both; "
                    "FilmTrust golden rows, d = 16, lr 0.002, top-10", epochs=epochs, batch_size=DS.PAIRED_BATCH, models={})
    for name in names:
        conf, train, test = DS.paired_conf(name, epochs)
        d, nbytes, rec = [], 0, []
        for k in range(S):
            a = DS.run_mode(name, conf, train, test, "throughput", 3 + k, "ordered")
            b = DS.run_mode(name, conf, train, test, "exact", 3 + k, "ordered")
            d.append(a["values"][1] - b["values"][1]); nbytes += DS.bytes_differing(a["arrays"], b["arrays"]); rec.append(a["values"][1])
        d = np.array(d)
        out["models"][name] = dict(bytes_differing=nbytes, paired_recall_gap_mean=float(d.mean()), paired_recall_gap_se=float(d.std(ddof=1) / np.sqrt(S)) if S > 1 else None,
                                   S=S, recall_at_10_mean=float(np.mean(rec)))
        print(name, out["models"][name], file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))
    sys.exit(0)

name, S, epochs = sys.argv[1], int(sys.argv[2]), sys.argv[3]
extra = dict(kv.split("=") for kv in sys.argv[4:])
meta, z = load_golden("pairwise_adj_filmtrust")
train, test = rows_from_golden(load_golden("bpr_filmtrust")[1])
conf = conf_from_text(meta["conf"]); conf["model.name"] = name; conf["num.max.epoch"] = epochs; conf["num.factors"] = "16"
conf["item.ranking"] = "on -topN 10"; conf["learnRate"] = "-init 0.002 -max 1"
if name == "SimGCL":
    conf["SimGCL"] = "-n_layer 2 -lambda 0.5 -eps 0.1"
os.environ["QREC_QUIET"] = "1"
os.environ.update(extra)
cls = resolve_model(name)
out = {}
for mode in ("exact", "throughput"):
    for red in ("ordered", "atomic"):
        rows = []
        for k in range(S):
            os.environ["QREC_MODE"] = mode; os.environ["QREC_REDUCTIONS"] = red; os.environ["QREC_SEED"] = str(3 + k)
            random.seed(3 + k); np.random.seed(3)
            with redirect_stdout(io.StringIO()):
                m = cls(conf, train, test)
                measure = m.execute()
            rows.append([float(x.split(":")[1]) for x in measure if ":" in x])
        a = np.array(rows)
        out[f"{mode}/{red}"] = dict(mean=a.mean(0).tolist(), sd=a.std(0, ddof=1).tolist(), recall=a[:, 1].tolist())
        print(f"{name} {mode:10s} {red:8s} P/R/F1/NDCG@10 mean {np.round(a.mean(0), 4)} sd {np.round(a.std(0, ddof=1), 4)}", flush=True)
print(json.dumps(out))
