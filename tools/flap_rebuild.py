"""Flap rebuild on the G1 WAN (20,000 nodes, one prefix per node, source
G1_SOURCES[0]): what Decision::rebuildRoutes' full branch costs after a
one-link metric flap, two ways on twin solvers, interleaved per flap:
  (a) SpfSolver::rebuildRoutes (device delta of the previous and the next
      record block, only the changed records downloaded and materialised);
  (b) buildRouteDb + calculateUpdate + update, the full rebuild and host diff.
The two updates of every flap must be equal (flap_rebuild_bench throws
otherwise). Prints the medians, the change counts and (a)'s
decision.gpu.*_ms split (medians and per flap), then one JSON line.

  python tools/flap_rebuild.py [--flaps 20] [--seed 0xF1A9] [--nodes 20000]"""
import argparse
import json
import os
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flaps", type=int, default=20)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xF1A9)
    ap.add_argument("--nodes", type=int, default=0, help="override G1's node count (smoke runs)")
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime: torch's)
    import openr_amd
    from openr_amd.workloads import G1_OPTS, G1_SOURCES
    openr_amd.require_gpu()
    opts = dict(G1_OPTS)
    src = G1_SOURCES[0]
    if args.nodes:
        opts["nodes"] = args.nodes
    r = openr_amd.decision.flap_rebuild_bench("wan", opts, src, args.flaps, args.seed)
    a, b = [x / 1e3 for x in r["rebuild_us"]], [x / 1e3 for x in r["full_us"]]
    names = ("prepare_ms", "launch_ms", "delta_ms", "materialize_ms")
    split = {n: median(s[i] for s in r["splits_ms"]) for i, n in enumerate(names)}
    print(f"G1 flap rebuild, source {src}, {opts['nodes']} nodes, {r['routes']} routes, "
          f"{args.flaps} one-link metric flaps (seed {args.seed:#x})")
    print(f"  per-flap changes (updates + deletions): {r['changes']}")
    print(f"  (a) rebuildRoutes                          median {median(a):8.3f} ms  "
          f"min {min(a):8.3f}  max {max(a):8.3f}")
    print(f"  (b) buildRouteDb + calculateUpdate + update median {median(b):8.3f} ms  "
          f"min {min(b):8.3f}  max {max(b):8.3f}")
    print("  (a) split, medians: " + "  ".join(f"{n} {v:.3f}" for n, v in split.items()))
    print("  per flap: changes, (a) ms = prepare + launch + delta + materialize (+ rest), (b) ms")
    for c, x, y, sp in zip(r["changes"], a, b, r["splits_ms"]):
        print(f"    {c:6d}  {x:7.3f} = " + " + ".join(f"{v:.3f}" for v in sp) +
              f" (+ {x - sum(sp):.3f})  {y:7.3f}")
    print(f"  delta builds {r['delta_builds']}, fallbacks {r['delta_fallbacks']} "
          f"(the first call); target <= 3 ms: {'met' if median(a) <= 3.0 else 'MISSED'}")
    print(json.dumps(dict(workload="g1_flap_rebuild", flaps=args.flaps, seed=args.seed,
                          nodes=opts["nodes"], routes=r["routes"],
                          rebuild_ms_median=median(a), full_ms_median=median(b),
                          rebuild_ms=a, full_ms=b, changes=r["changes"], split_ms_median=split,
                          split_ms=r["splits_ms"],
                          delta_builds=r["delta_builds"],
                          delta_fallbacks=r["delta_fallbacks"])))


if __name__ == "__main__":
    main()
