"""The oracle's literal answer to the what-if sweep's metric scenarios:
tests/whatif.py's World with the two scenario kinds that move metrics.

  "linkMetrics": [(node, ifName, metric)]  the one adjacency of `node` re-sent
      with `metric` (setLinkMetric / setAdjacencyMetric: one direction);
  "nodesSoftDrained": [(node, increment)]  the node's database re-sent with
      nodeMetricIncrementVal = increment and the increment added to every
      adjacency metric (LinkMonitor.cpp:971-1001), after the scenario's own
      linkMetrics. The worlds here carry no increment of their own.

Oracle.answer's restore step re-sends the original databases, so it serves
these scenarios as it stands."""
import copy

import whatif as W


class MetricWorld(W.World):
    def mutated(self, sc):
        dbs, down = super().mutated({k: v for k, v in sc.items()
                                     if k in ("links", "nodesDown", "nodesDrained")})

        def db(node):
            if node not in dbs:
                dbs[node] = copy.deepcopy(self.adjdbs[node])
            return dbs[node]

        for node, ifn, metric in sc.get("linkMetrics", ()):
            if node in down:
                continue
            for a in db(node)["adjacencies"]:
                if a["ifName"] == ifn:
                    a["metric"] = metric
        for node, inc in sc.get("nodesSoftDrained", ()):
            d = db(node)
            assert d.get("nodeMetricIncrementVal", 0) == 0
            d["nodeMetricIncrementVal"] = inc
            for a in d["adjacencies"]:
                a["metric"] += inc
        return dbs, down


def as_metric_world(world):
    """the same databases as a MetricWorld"""
    return MetricWorld(list(world.adjdbs.values()), world.prefix_dbs, world.area)
