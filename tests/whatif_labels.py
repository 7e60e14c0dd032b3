"""Node-label MPLS routes in the what-if sweep: the oracle with
enableNodeSegmentLabel on (the reference's default, SpfSolver.h:269) and the
comparison of a sweep's label answers with it. Shared by
tests/test_gpu_whatif_labels.py and tools/whatif_sweep.py --labels."""
import whatif as W


class LabelOracle(W.Oracle):
    """W.Oracle whose solver also builds the node-label routes
    (SpfSolver.cpp:352-445), so calculateUpdate carries mplsRoutesToUpdate /
    mplsRoutesToDelete."""

    def __init__(self, O, world, me, v4=True, brs=False):
        self.world, self.me = world, me
        self.als, self.ls, self.ps = world.load(O, me)
        self.solver = O.SpfSolver(me, v4, True, brs)
        self.base = self.solver.buildRouteDb(me, self.als, self.ps)


def mpls_kind(upd):
    """'empty', 'update', 'delete' or 'mixed' of the update's MPLS half"""
    return W.kind_of({"unicastRoutesToUpdate": upd["mplsRoutesToUpdate"],
                      "unicastRoutesToDelete": upd["mplsRoutesToDelete"]})


def check_labels(sw, answers, label="", index=None):
    """after launch + fetchUpdates: W.check_sweep (the unicast half, and the
    canonical RouteDb, which prints the MPLS routes), then per scenario
    mplsRoutesToUpdate as a dict, mplsRoutesToDelete as a set, mplsCounts and
    changedLabels against the oracle"""
    W.check_sweep(sw, answers, label, index)
    for k, (want, _) in enumerate(answers):
        v = index[k] if index is not None else k
        got = sw.routeUpdate(v)
        gu, wu = got["mplsRoutesToUpdate"], want["mplsRoutesToUpdate"]
        assert gu == wu, (label, v, "mpls update",
                          sorted(x for x in set(gu) | set(wu) if gu.get(x) != wu.get(x))[:8])
        gd, wd = got["mplsRoutesToDelete"], want["mplsRoutesToDelete"]
        assert len(gd) == len(set(gd)) and set(gd) == set(wd), (label, v, "mpls delete", gd, wd)
        assert tuple(sw.mplsCounts(v)) == (len(wu), len(wd)), (label, v)
        assert sw.changedLabels(v) == sorted(list(wu) + list(wd)), (label, v)
