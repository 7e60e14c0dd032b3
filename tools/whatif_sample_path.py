"""Per-scenario time of LinkFailureSweep (mode kChangedOnly, launch +
fetchUpdates) over the 64-scenario stratified sample of each G1 what-if set,
for the built tree given as argv[1] (the parent commit's or this one's), named
in the log's first line by argv[2] (default: the tree's path).
Two timed series per set, so that the run-to-run difference shows.

  python tools/whatif_sample_path.py TREE [LABEL]"""
import os
import random
import sys
import time
from statistics import median

ROOT = os.path.abspath(sys.argv[1])
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401
import openr_amd  # noqa: E402
import whatif as W  # noqa: E402
import whatif_metric as WM  # noqa: E402
from openr_amd.workloads import G1_OPTS  # noqa: E402

openr_amd.require_gpu()
M = openr_amd.decision
FORMS = {0: "kRegisterList", 1: "kEdgeBitset", 2: "kTopologyCopies", 3: "kGlobalState"}
me = "0"
w = WM.as_metric_world(W.generated_world(M, "wan", dict(G1_OPTS)))
als = M.AreaLinkStates()
ls = als.add(w.area, me)
for d in w.adjdbs.values():
    ls.updateAdjacencyDatabase(d, w.area)
ps = M.PrefixState()
for pdb in w.prefix_dbs:
    for e in pdb["prefixEntries"]:
        ps.updatePrefix(pdb["thisNodeName"], w.area, e)
names = sorted(n for n in w.adjdbs if n != me)
links = sorted({min((n, a["ifName"]), (a["otherNodeName"], a["otherIfName"]))
                for n, d in w.adjdbs.items() for a in d["adjacencies"]})


def both(n, ifn, metric):
    a = next(a for a in w.adjdbs[n]["adjacencies"] if a["ifName"] == ifn)
    weight = max(a["metric"], next(b["metric"] for b in w.adjdbs[a["otherNodeName"]]["adjacencies"]
                                   if b["ifName"] == a["otherIfName"]))
    m = metric(weight)
    return [(n, ifn, m), (a["otherNodeName"], a["otherIfName"], m)]


every = lambda xs, n: xs[::max(1, len(xs) // n)][:n]  # noqa: E731
sets = [
    ("h: every 10th node down", [{"nodesDown": [n]} for n in names[::10]]),
    ("i: every 10th node drained", [{"nodesDrained": [n]} for n in names[::10]]),
    ("j: single-link failures", [{"links": [l]} for l in every(links, 2000)]),
    ("k: every 20th link x8", [{"linkMetrics": both(n, i, lambda x: 8 * x)} for n, i in links[::20]]),
    ("l: every 20th link to 1", [{"linkMetrics": both(n, i, lambda x: 1)} for n, i in links[::20]]),
]
LABEL = sys.argv[2] if len(sys.argv) > 2 else f"tree {sys.argv[1]}"
print(f"sample path, {LABEL}: {len(w.adjdbs)} nodes, {w.directed_edges()} directed edges")
for label, scs in sets:
    idx = sorted({i * len(scs) // 64 for i in range(64)})
    sample = [scs[i] for i in idx]
    try:
        sw = M.LinkFailureSweep(me, ls, ps, sample, True, False)
        sw.setMode(2)
        series = []
        for run in range(2):
            ms = []
            for i in range(4):
                t0 = time.perf_counter()
                sw.launch()
                sw.fetchUpdates()
                ms.append((time.perf_counter() - t0) * 1e3)
            series.append(median(ms[1:]) / len(sample))
        n = sum(sum(sw.counts(v)) for v in range(len(sample)))
        print(f"  {label:28s} {len(sample)} scenarios  {FORMS[sw.form()]:15s} "
              f"{series[0]:8.3f} / {series[1]:8.3f} ms per scenario (two series)  changed routes {n}")
    except Exception as e:  # noqa: BLE001
        print(f"  {label:28s} {len(sample)} scenarios  THROWS {type(e).__name__}: {str(e)[:120]}")
