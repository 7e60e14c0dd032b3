"""What-if sweep on the C4 WAN (2,000 nodes, one prefix per node) from source
"0", mode kChangedOnly: one LinkFailureSweep launch per scenario set,
  (a) every other node down (1,999 scenarios),
  (b) every other node drained,
  (c) 2,000 seeded link groups of 16 links,
  (d) the C4 link-failure variants (bench.py's 10,000, the same generator
      and seed) through the register form and, in the same process and
      interleaved, forced through the bitset form,
  (e) every link cost out to 8x its weight, one scenario per link,
  (f) every other node soft-drained by 1000,
  (g) every link set to weight 1 (a lowered metric: the repair recomputes the
      unit from the source inside the kernel), and the same set in mode kFull
      (the full frontier form) beside it.
Per set: launch + fetchUpdates ms (median of 5 after 2 warm-ups), the
materialisation of every DecisionRouteUpdate, the total changed routes and the
form taken. The CPU baseline is the oracle's own loop -- mutate its LinkState,
buildRouteDb, calculateUpdate, restore -- on one thread over a 64-scenario
stratified sample of each set, EXTRAPOLATED to the set's size; the sample's
updates, counts and updated RouteDbs must equal the sweep's.

With --g1 the world is the G1 WAN (20,000 nodes, one prefix per node: past the
LDS forms, so every set takes the global-state form, kGlobalState) and the
sets are 2,000 scenarios each,
  (h) every 10th node down,         (i) every 10th node drained,
  (j) single-link failures,         (k) every 20th link cost out to 8x,
  (l) every 20th link set to 1,
each row also giving the share of exit-only units (no node bit, no lowered
metric, no dead or raised edge tight in the base SPF: computed here on the
host from the base SPF, the rule the kernel applies).

With --restore the world carries a drained baseline -- every other node
hard-drained, every 20th link overloaded at one end, every other node (the
other half) soft-drained by 1000 -- and the sets put things back, one scenario
per restoration (--drain-every N: every Nth node instead of every other one;
with every other node hard-drained the source reaches few nodes, so most
restorations move few routes):
  (m) each drained node undrained,  (n) each overloaded link brought up,
  (o) each soft-drained node soft-undrained,
  (s) a sample of 64 from (m) and (o),
in mode kChangedOnly; (n) and (s) also in kFull beside it: link revivals run
there in the full frontier form, and cleared node bits are not built in that
form, so (s) runs as topology copies -- the kernels every sweep had before
restorations. With --g1 --restore the first three on the G1 WAN, 2,000
scenarios each, as (p), (q), (r) in the global-state form (restoring units take
no exit).

With --labels (also with --g1 and --restore) every node carries the node label
100000 + id and each row is timed twice, interleaved: the sweep as above and
the same sweep with enableNodeSegmentLabel. The oracle's solver then builds the
label routes too and the sample is compared with MPLS included
(tests/whatif_labels.py); the row adds launch + fetch with labels, the bytes of
SPF rows the launch wrote (4 (1 + W) S_n per scenario) and the changed-node
total.

With --sources N the question is network-wide: the first N nodes are sources
and every (source, scenario) pair of a set is computed, on the C4 WAN, sets
from a .. g (default "ea"). Per set, from one process:
  - NetworkWhatifSweep: construction, then launch + fetchUpdates (records) and
    launch(records=False) + fetchImpact, each the median of 3 after a warm-up;
  - the loop of one LinkFailureSweep per source over the same scenarios (mode
    kChangedOnly): construction + base run summed, and launch + fetchUpdates
    summed (each sweep's second launch, so its descendant rows are cached);
    every pair's counts must equal the batch's;
  - the oracle's own loop on a sample of 64 pairs (8 sources x 8 scenarios), ms
    per pair; the sample's updates, counts and updated RouteDbs must equal the
    batch's.

  python tools/whatif_sweep.py [--nodes 2000] [--sample 64] [--sets abcdefg] [--labels]
  python tools/whatif_sweep.py --sources 64 [--sets ea]
  python tools/whatif_sweep.py --g1 [--nodes 20000] [--sample 64] [--sets hijkl]
  python tools/whatif_sweep.py --restore [--g1] [--sets mnos | pqr]"""
import argparse
import hashlib
import json
import os
import random
import sys
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

FORMS = {0: "kRegisterList", 1: "kEdgeBitset", 2: "kTopologyCopies", 3: "kGlobalState"}


def fresh_world(base):
    """a World whose prefix load is linear: every database goes into a FRESH
    PrefixState, so no earlier advertisement has to be looked up and withdrawn
    (tests/lsdb.py's sync lists the whole state per database)"""
    class FreshWorld(base):
        def load(self, M, me):
            als = M.AreaLinkStates()
            ls = als.add(self.area, me)
            for d in self.adjdbs.values():
                ls.updateAdjacencyDatabase(d, self.area)
            ps = M.PrefixState()
            for pdb in self.prefix_dbs:
                for e in pdb["prefixEntries"]:
                    ps.updatePrefix(pdb["thisNodeName"], self.area, e)
            return als, ls, ps
    return FreshWorld


def network_rows(args, M, O, W, w, ls, ps, sets):
    """--sources N: the batched sweep beside the per-source loop and the oracle"""
    from test_gpu_network_whatif import Source
    sources = sorted(w.adjdbs, key=int)[:args.sources]
    out = []
    for label, scs, _, _ in sets:
        t0 = time.perf_counter()
        net = M.NetworkWhatifSweep(ls, ps, sources, scs, True, False)
        build_ms = (time.perf_counter() - t0) * 1e3
        rec, imp = [], []
        for i in range(4):
            t0 = time.perf_counter()
            net.launch()
            net.fetchUpdates()
            rec.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            net.launch(records=False)
            net.fetchImpact()
            imp.append((time.perf_counter() - t0) * 1e3)
        net.launch()
        net.fetchUpdates()
        S, K = len(sources), len(scs)
        live = [[k for k in range(K) if net.state(s, k) == M.kComputed] for s in range(S)]
        pairs = sum(len(l) for l in live)
        changed = sum(sum(net.counts(s, k)) for s in range(S) for k in live[s])
        affected = sum(len(net.affectedSources(k)) for k in range(K))
        # the per-source loop: the same pairs, one LinkFailureSweep a source
        loop_build, loop_run = 0.0, 0.0
        for s, me in enumerate(sources):
            t0 = time.perf_counter()
            sw = M.LinkFailureSweep(me, ls, ps, [scs[k] for k in live[s]], True, False)
            sw.setMode(2)
            sw.launch()  # the first launch runs the base and builds its descendant rows
            sw.fetchUpdates()
            loop_build += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            sw.launch()
            sw.fetchUpdates()
            loop_run += (time.perf_counter() - t0) * 1e3
            for v, k in enumerate(live[s]):
                assert tuple(sw.counts(v)) == tuple(net.counts(s, k)), (label, me, k)
            del sw
        # the oracle on 8 sources x 8 scenarios
        n = max(1, int(args.sample ** 0.5))
        cpu, checked = [], 0
        for s in sorted({i * S // n for i in range(n)}):
            oracle = W.Oracle(O, w, sources[s])
            ks = [k for k in sorted({i * K // n for i in range(n)}) if k in set(live[s])]
            t0 = time.perf_counter()
            for k in ks:
                oracle.answer(scs[k], canonical=False)
            cpu.append((time.perf_counter() - t0) * 1e3 / max(1, len(ks)))
            W.check_sweep(Source(net, s), [oracle.answer(scs[k]) for k in ks], (label, s), ks)
            checked += len(ks)
        row = dict(set=label, sources=S, scenarios=K, pairs=pairs, batched=net.batchedSources(),
                   chunks=net.numChunks(), impact_chunks=net.numChunks(False),
                   construct_ms=build_ms, batched_records_ms=median(rec[1:]),
                   batched_impact_ms=median(imp[1:]), loop_construct_base_ms=loop_build,
                   loop_launch_fetch_ms=loop_run, ratio_loop_over_batched=loop_run / median(rec[1:]),
                   changed_routes=changed, affected_pairs=affected,
                   cpu_ms_per_pair=median(cpu), sample=checked)
        out.append(row)
        print(f"  {label:22s} {S} sources x {K} scenarios = {pairs} pairs, "
              f"{row['batched']} batched, {row['chunks']} chunk(s)\n"
              f"    batched: construct {build_ms:9.1f} ms, launch+fetchUpdates "
              f"{row['batched_records_ms']:9.2f} ms, impact only {row['batched_impact_ms']:9.2f} ms\n"
              f"    per-source loop: construct+base {loop_build:9.1f} ms, launch+fetchUpdates "
              f"{loop_run:9.2f} ms summed over {S} sweeps (every pair's counts equal)\n"
              f"    loop / batched = {row['ratio_loop_over_batched']:.2f}x; changed routes {changed}, "
              f"affected (source, scenario) pairs {affected}\n"
              f"    oracle loop {row['cpu_ms_per_pair']:.3f} ms/pair x {pairs} = "
              f"{row['cpu_ms_per_pair'] * pairs / 1e3:.1f} s (extrapolated from {checked}; sample equal)")
    print(json.dumps(dict(workload="c4_whatif_network", nodes=len(w.adjdbs), rows=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="override C4's node count (smoke runs)")
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--sets", default=None, help="the sets to run, by letter")
    ap.add_argument("--g1", action="store_true", help="the G1 WAN and its sets (h .. l)")
    ap.add_argument("--restore", action="store_true",
                    help="the drained baseline and its restoring sets (m .. o and s, with --g1 p .. r)")
    ap.add_argument("--drain-every", type=int, default=2,
                    help="the baseline drains every Nth node hard and every Nth (the next one) "
                         "soft; 2 (default): every other node each")
    ap.add_argument("--labels", action="store_true",
                    help="node label 100000 + id on every node; each set also with "
                         "enableNodeSegmentLabel, the sample compared with MPLS included")
    ap.add_argument("--sources", type=int, default=0,
                    help="network-wide: the first N nodes as sources (NetworkWhatifSweep beside "
                         "the per-source loop and the oracle)")
    args = ap.parse_args()
    if args.sources and (args.g1 or args.restore or args.labels):
        ap.error("--sources runs on the plain C4 WAN")
    if args.sets is None and args.sources:
        args.sets = "ea"
    if args.sets is None:
        if args.restore:
            args.sets = "pqr" if args.g1 else "mnos"
        else:
            args.sets = "hijkl" if args.g1 else "abcdefg"
    if args.restore != all(c in "mnopqrs" for c in args.sets):
        ap.error("sets m .. s run on the drained baseline (--restore), the others without it")
    import torch  # noqa: F401  (one HIP runtime: torch's)
    import _refcpu as O
    import openr_amd
    import whatif as W
    import whatif_metric as WM
    import whatif_labels as WL
    import whatif_restore as WR
    from openr_amd.workloads import (C4_DUAL_PERMILLE, C4_OPTS, C4_SEED, C4_SOURCE,
                                     C4_VARIANTS)
    openr_amd.require_gpu()
    M = openr_amd.decision
    from openr_amd.workloads import G1_OPTS
    opts = dict(G1_OPTS if args.g1 else C4_OPTS)
    if args.nodes:
        opts["nodes"] = args.nodes
    me = C4_SOURCE
    w = WR.as_restore_world(W.generated_world(M, "wan", opts))
    if args.g1:
        w = fresh_world(WR.RestoreWorld)(list(w.adjdbs.values()), w.prefix_dbs, w.area)
    names = sorted(n for n in w.adjdbs if n != me)
    links = sorted({min((n, a["ifName"]), (a["otherNodeName"], a["otherIfName"]))
                    for n, d in w.adjdbs.items() for a in d["adjacencies"]})
    step = max(2, args.drain_every)
    hard, over, softs = names[::step], links[::20], names[1::step]
    if args.restore:  # the drained baseline
        for n in hard:
            w.adjdbs[n]["isOverloaded"] = True
        for n, i in over:
            next(a for a in w.adjdbs[n]["adjacencies"] if a["ifName"] == i)["isOverloaded"] = True
        for n in softs:
            w.adjdbs[n]["nodeMetricIncrementVal"] = 1000
            for a in w.adjdbs[n]["adjacencies"]:
                a["metric"] += 1000
    if args.labels:
        for n, d in w.adjdbs.items():
            d["nodeLabel"] = 100000 + int(n)
    rng = random.Random(0xC4F)

    def both(n, ifn, metric):  # the link behind (n, ifn): both directions sent with `metric`
        a = next(a for a in w.adjdbs[n]["adjacencies"] if a["ifName"] == ifn)
        weight = max(a["metric"], next(b["metric"] for b in w.adjdbs[a["otherNodeName"]]["adjacencies"]
                                       if b["ifName"] == a["otherIfName"]))
        m = metric(weight)
        return [(n, ifn, m), (a["otherNodeName"], a["otherIfName"], m)]

    # (label, scenarios, register / bitset A/B, modes: 2 kChangedOnly, 0 kFull)
    sets = [
        ("a: node down", [{"nodesDown": [n]} for n in names], False, (2,)),
        ("b: node drained", [{"nodesDrained": [n]} for n in names], False, (2,)),
        ("c: 16-link groups", [{"links": rng.sample(links, 16)} for _ in range(2000)], False,
         (2,)),
        ("d: C4 variants", [{"links": v} for v in M.link_failure_variants(
            "wan", opts, C4_VARIANTS, C4_SEED, C4_DUAL_PERMILLE)], True, (2,)),
        ("e: link cost-out x8", [{"linkMetrics": both(n, i, lambda x: 8 * x)} for n, i in links],
         False, (2,)),
        ("f: node soft-drained", [{"nodesSoftDrained": [(n, 1000)]} for n in names], False, (2,)),
        ("g: link set to 1", [{"linkMetrics": both(n, i, lambda x: 1)} for n, i in links], False,
         (2, 0)),
    ]
    every = lambda xs, n: xs[::max(1, len(xs) // n)][:n]  # noqa: E731
    sets += [
        ("h: every 10th node down", [{"nodesDown": [n]} for n in names[::10]], False, (2,)),
        ("i: every 10th node drained", [{"nodesDrained": [n]} for n in names[::10]], False, (2,)),
        ("j: single-link failures", [{"links": [l]} for l in every(links, 2000)], False, (2,)),
        ("k: every 20th link x8", [{"linkMetrics": both(n, i, lambda x: 8 * x)}
                                   for n, i in links[::20]], False, (2,)),
        ("l: every 20th link to 1", [{"linkMetrics": both(n, i, lambda x: 1)}
                                     for n, i in links[::20]], False, (2,)),
    ]
    sets += [
        ("m: node undrained", [{"nodesUndrained": [n]} for n in hard], False, (2,)),
        ("n: link brought up", [{"linksUndrained": [l]} for l in over], False, (2, 0)),
        ("o: node soft-undrained", [{"nodesSoftUndrained": [n]} for n in softs], False, (2,)),
        ("s: sample of m and o", [{"nodesUndrained": [n]} for n in every(hard, 32)] +
         [{"nodesSoftUndrained": [n]} for n in every(softs, 32)], False, (2, 0)),
        ("p: node undrained", [{"nodesUndrained": [n]} for n in every(hard, 2000)], False, (2,)),
        ("q: link brought up", [{"linksUndrained": [l]} for l in every(over, 2000)], False, (2,)),
        ("r: node soft-undrained", [{"nodesSoftUndrained": [n]} for n in every(softs, 2000)],
         False, (2,)),
    ]
    sets = [s for s in sets if s[0][0] in args.sets]
    print(f"what-if sweep, {'G1' if args.g1 else 'C4'} WAN: {len(w.adjdbs)} nodes, "
          f"{w.directed_edges()} directed edges, "
          f"source {me}, mode kChangedOnly unless a row says kFull")
    als, ls, ps = w.load(M, me)
    if args.sources:
        sets.sort(key=lambda s: args.sets.index(s[0][0]))
        return network_rows(args, M, O, W, w, ls, ps, sets)
    oracle = (WL.LabelOracle if args.labels else W.Oracle)(O, w, me)
    base, weight, far = {}, {}, {}  # the exit-only rule's inputs: the G1 rows alone
    if args.g1:
        base = {n: r[0] for n, r in oracle.ls.getSpfResult(me).items()}  # reached nodes' distances
        # (node, ifName) -> the link's SPF weight, its other end
        for n, d in w.adjdbs.items():
            for a in d["adjacencies"]:
                weight[(n, a["ifName"])] = both(n, a["ifName"], lambda x: x)[0][2]
                far[(n, a["ifName"])] = (a["otherNodeName"], a["otherIfName"])

    def exit_only(sc):
        """the kernel's rule for a unit that runs nothing, from the base SPF
        (the G1 sets' scenario kinds; the world has no link down)"""
        if sc.get("nodesDrained") or sc.get("nodesSoftDrained"):
            return False
        if any(sc.get(k) for k in WR.RESTORING):  # a restoring unit takes no exit
            return False

        def tight(n, ifn):  # either direction of the link behind (n, ifn)
            return any(a in base and (a == me or not w.adjdbs[a].get("isOverloaded")) and
                       base[a] + weight[(a, i)] == base.get(far[(a, i)][0])
                       for a, i in ((n, ifn), far[(n, ifn)]))
        dead = list(sc.get("links", ())) + [(n, a["ifName"]) for n in sc.get("nodesDown", ())
                                            for a in w.adjdbs[n]["adjacencies"]]
        if any(tight(n, i) for n, i in dead):
            return False
        return not any(m < weight[(n, i)] or (m > weight[(n, i)] and tight(n, i))
                       for n, i, m in sc.get("linkMetrics", ()))
    out = []
    for label, scs, ab, modes in sets:
        sweeps, names = [], []  # one sweep and its row label per (mode, list form)
        for force, mode in [(f, m) for m in modes for f in ((False, True) if ab else (False,))]:
            for on in ((False, True) if args.labels else (False,)):
                sw = M.LinkFailureSweep(me, ls, ps, scs, True, False, enableNodeSegmentLabel=on)
                sw.setMode(mode)
                sw.setListForm(force)
                sweeps.append(sw)
                names.append((label if mode == 2 else label + " (kFull)") +
                             (" +labels" if on else ""))
        # interleaved: one timed series per sweep, alternating
        ms = [[] for _ in sweeps]
        for i in range(7):
            for k, sw in enumerate(sweeps):
                t0 = time.perf_counter()
                sw.launch()
                sw.fetchUpdates()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        idx = sorted({i * len(scs) // args.sample for i in range(args.sample)})
        t0 = time.perf_counter()
        for i in idx:  # the timed loop: mutate, buildRouteDb, calculateUpdate, restore
            oracle.answer(scs[i], canonical=False)
        cpu_ms = (time.perf_counter() - t0) * 1e3 / len(idx)
        answers = [oracle.answer(scs[i]) for i in idx]
        digest = hashlib.sha1()
        for _, canon in answers:
            digest.update(canon)
        for k, sw in enumerate(sweeps):
            # raises on any difference; beside a labelled oracle the label-free
            # sweep is compared on its unicast counts alone (its RouteDbs carry
            # no MPLS routes, the oracle's do)
            if names[k].endswith("+labels"):
                WL.check_labels(sw, answers, label, idx)
            elif args.labels:
                for i, (want, _) in zip(idx, answers):
                    assert tuple(sw.counts(i)) == (len(want["unicastRoutesToUpdate"]),
                                                   len(want["unicastRoutesToDelete"])), (label, i)
            else:
                W.check_sweep(sw, answers, label, idx)
            n, mat_ms = sw.materializeAll(0)
            row = dict(set=names[k], scenarios=len(scs), form=FORMS[sw.form()],
                       sweep_ms=median(ms[k][2:]), materialize_ms=mat_ms, changed_routes=n,
                       cpu_ms_per_scenario=cpu_ms, cpu_ms_extrapolated=cpu_ms * len(scs),
                       sample=len(idx), sample_digest=digest.hexdigest()[:16])
            if args.g1:
                row["exit_only_share"] = sum(exit_only(sc) for sc in scs) / len(scs)
            if names[k].endswith("+labels"):
                row["row_bytes"] = 4 * (1 + sw.nhWords()) * len(w.adjdbs) * len(scs)
                row["changed_nodes"] = sw.totalChangedNodes()
            out.append(row)
            print(f"  {row['set']:26s} {len(scs):6d} scenarios  {row['form']:15s} "
                  f"launch+fetch {row['sweep_ms']:8.3f} ms  materialise {mat_ms:8.3f} ms  "
                  f"changed routes {n:9d}  | oracle loop {cpu_ms:7.3f} ms/scenario x "
                  f"{len(scs)} = {cpu_ms * len(scs) / 1e3:8.2f} s (extrapolated from "
                  f"{len(idx)}); sample equal, sha1 {row['sample_digest']}" +
                  (f"; exit-only units {100 * row['exit_only_share']:.1f} %" if args.g1 else "") +
                  (f"; SPF rows {row['row_bytes'] / 1e6:.1f} MB, changed nodes "
                   f"{row['changed_nodes']}" if "row_bytes" in row else ""))
    print(json.dumps(dict(workload="g1_whatif_sweep" if args.g1 else "c4_whatif_sweep", nodes=len(w.adjdbs), rows=out)))


if __name__ == "__main__":
    main()
