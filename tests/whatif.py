"""What-if scenario helpers shared by the scenario tests and
tools/whatif_sweep.py: a world as plain dicts (tests/lsdb.py shapes), loaded
alike into the product's and the oracle's LinkState / PrefixState, and the
oracle's literal answer to a scenario -- mutate its LinkState the way the
reference would (adjacencies removed at both ends; deleteAdjacencyDatabase;
the database re-sent with the overload bit), buildRouteDb, calculateUpdate
against the base, restore.

A scenario is {"links": [(node, ifName), ...], "nodesDown": [...],
"nodesDrained": [...]}, every key optional."""
import copy

import lsdb as L


class World:
    def __init__(self, adjdbs, prefix_dbs, area=L.kTestingAreaName):
        self.area = area
        self.adjdbs = {d["thisNodeName"]: d for d in adjdbs}
        self.prefix_dbs = list(prefix_dbs)

    def load(self, M, me):
        als = M.AreaLinkStates()
        ls = als.add(self.area, me)
        for d in self.adjdbs.values():
            ls.updateAdjacencyDatabase(d, self.area)
        ps = M.PrefixState()
        for pdb in self.prefix_dbs:
            L.updatePrefixDatabase(ps, pdb, self.area)
        return als, ls, ps

    def directed_edges(self):
        return sum(len(d["adjacencies"]) for d in self.adjdbs.values())

    def mutated(self, sc):
        """(databases to re-send, nodes whose database is deleted)"""
        dbs = {}

        def db(node):
            if node not in dbs:
                dbs[node] = copy.deepcopy(self.adjdbs[node])
            return dbs[node]

        for node, ifn in sc.get("links", ()):
            adj = next(a for a in self.adjdbs[node]["adjacencies"] if a["ifName"] == ifn)
            other, oifn = adj["otherNodeName"], adj["otherIfName"]
            db(node)["adjacencies"] = [a for a in db(node)["adjacencies"] if a["ifName"] != ifn]
            db(other)["adjacencies"] = [a for a in db(other)["adjacencies"]
                                        if not (a["ifName"] == oifn and a["otherNodeName"] == node)]
        for node in sc.get("nodesDrained", ()):
            db(node)["isOverloaded"] = True
        down = list(sc.get("nodesDown", ()))
        for node in down:
            dbs.pop(node, None)
        return dbs, down


class Oracle:
    """The oracle's replica of a world and its base RouteDb from `me`."""

    def __init__(self, O, world, me, v4=True, brs=False):
        self.world, self.me = world, me
        self.als, self.ls, self.ps = world.load(O, me)
        self.solver = O.SpfSolver(me, v4, False, brs)
        self.base = self.solver.buildRouteDb(me, self.als, self.ps)

    def answer(self, sc, canonical=True):
        """(calculateUpdate dict, the scenario RouteDb's canonical text)"""
        w = self.world
        dbs, down = w.mutated(sc)
        for d in dbs.values():
            self.ls.updateAdjacencyDatabase(d, w.area)
        for node in down:
            self.ls.deleteAdjacencyDatabase(node)
        new = self.solver.buildRouteDb(self.me, self.als, self.ps)
        upd = self.base.calculateUpdate(new)
        for node in list(dbs) + down:
            self.ls.updateAdjacencyDatabase(w.adjdbs[node], w.area)
        return upd, (new.canonical() if canonical else None)


def kind_of(upd):
    """'empty', 'update', 'delete' or 'mixed'"""
    u, d = bool(upd["unicastRoutesToUpdate"]), bool(upd["unicastRoutesToDelete"])
    return {(False, False): "empty", (True, False): "update", (False, True): "delete",
            (True, True): "mixed"}[(u, d)]


def check_sweep(sw, answers, label="", index=None):
    """after launch + fetchUpdates: every scenario's update, the base with the
    update applied, the counts and the changed prefixes against the oracle
    (answers[k] is scenario index[k]'s; every scenario's without `index`)"""
    for k, (want, canon) in enumerate(answers):
        v = index[k] if index is not None else k
        got = sw.routeUpdate(v)
        # deletions as a set: the sweep lists them in prefix-table order, the
        # oracle in its RouteDb's
        gd, wd = set(got["unicastRoutesToDelete"]), set(want["unicastRoutesToDelete"])
        assert len(got["unicastRoutesToDelete"]) == len(gd)
        assert gd == wd, (label, v, "delete", sorted(gd ^ wd)[:8])
        gu, wu = got["unicastRoutesToUpdate"], want["unicastRoutesToUpdate"]
        assert gu == wu, (label, v, "update",
                          sorted(p for p in set(gu) | set(wu) if gu.get(p) != wu.get(p))[:8])
        assert sw.updatedCanonical(v) == canon, (label, v)
        nu, nd = len(want["unicastRoutesToUpdate"]), len(want["unicastRoutesToDelete"])
        assert tuple(sw.counts(v)) == (nu, nd), (label, v)
        assert sw.changedPrefixes(v) == sorted(
            list(want["unicastRoutesToUpdate"]) + list(want["unicastRoutesToDelete"])), (label, v)


def generated_world(M, kind, opts):
    """a generated LSDB (M.gen_publication) as a World"""
    area, keys, vals = M.gen_publication(kind, opts)
    adjdbs, by_node = [], {}
    for k, v in zip(keys, vals):
        if k.startswith("adj:"):
            adjdbs.append(M.decodeAdjDb(v))
        else:  # one key per (node, prefix): a node's entries into one database
            d = M.decodePrefixDb(v)
            by_node.setdefault(d["thisNodeName"], []).extend(d["prefixEntries"])
    return World(adjdbs, [L.createPrefixDb(n, es) for n, es in by_node.items()], area)
