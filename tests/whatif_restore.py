"""The oracle's literal answer to the what-if sweep's restoring scenarios:
tests/whatif_metric.py's MetricWorld with the three kinds that put things back.

  "linksUndrained": [(node, ifName)]  the one adjacency of `node` re-sent with
      isOverloaded = false (LinkState.cpp:574, Link::setOverloadFromNode);
  "nodesUndrained": [node]  the node's database re-sent with
      isOverloaded = false (LinkState.cpp:480, 309-333);
  "nodesSoftUndrained": [node]  the node's database re-sent with
      nodeMetricIncrementVal = 0 and every adjacency metric lowered by the
      increment it carried (LinkMonitor.cpp:971-1001), after the scenario's own
      linkMetrics.

Oracle.answer's restore step re-sends the original databases, so it serves
these scenarios as it stands."""
import copy

import whatif_metric as WM

RESTORING = ("linksUndrained", "nodesUndrained", "nodesSoftUndrained")


class RestoreWorld(WM.MetricWorld):
    def mutated(self, sc):
        dbs, down = super().mutated({k: v for k, v in sc.items() if k not in RESTORING})

        def db(node):
            if node not in dbs:
                dbs[node] = copy.deepcopy(self.adjdbs[node])
            return dbs[node]

        for node, ifn in sc.get("linksUndrained", ()):
            assert node not in down
            for a in db(node)["adjacencies"]:
                if a["ifName"] == ifn:
                    a["isOverloaded"] = False
        for node in sc.get("nodesUndrained", ()):
            assert node not in down
            db(node)["isOverloaded"] = False
        for node in sc.get("nodesSoftUndrained", ()):
            assert node not in down
            d = db(node)
            inc = d.get("nodeMetricIncrementVal", 0)
            d["nodeMetricIncrementVal"] = 0
            for a in d["adjacencies"]:
                a["metric"] -= inc
        return dbs, down


def as_restore_world(world):
    """the same databases as a RestoreWorld"""
    return RestoreWorld(list(world.adjdbs.values()), world.prefix_dbs, world.area)


def drain_baseline(world, rng, me, node_share=0.05, adj_share=0.03, soft=30, increment=40,
                   spare=()):
    """Drains a share of a generated world in place: `node_share` of the nodes
    hard-drained, `adj_share` of the adjacencies overloaded at one end, `soft`
    nodes soft-drained by `increment` (their adjacency metrics raised by it);
    never `me` or a node of `spare`. Returns (drained nodes, overloaded (node,
    ifName), soft-drained nodes), each sorted."""
    names = sorted(n for n in world.adjdbs
                   if n != me and n not in spare and world.adjdbs[n]["adjacencies"])
    hard = sorted(rng.sample(names, max(1, int(len(names) * node_share))))
    for n in hard:
        world.adjdbs[n]["isOverloaded"] = True
    adjs = [(n, a) for n in names for a in world.adjdbs[n]["adjacencies"]]
    over = rng.sample(adjs, max(1, int(len(adjs) * adj_share)))
    for _, a in over:
        a["isOverloaded"] = True
    softs = sorted(rng.sample([n for n in names if n not in hard], soft))
    for n in softs:
        d = world.adjdbs[n]
        d["nodeMetricIncrementVal"] = increment
        for a in d["adjacencies"]:
            a["metric"] += increment
    return hard, sorted((n, a["ifName"]) for n, a in over), softs
