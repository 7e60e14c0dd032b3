// restore_asan.cpp — LinkFailureSweep's restoring scenario kinds
// (linksUndrained, nodesUndrained, nodesSoftUndrained) under AddressSanitizer
// and UndefinedBehaviorSanitizer, over the host-only C-ABI stubs (no device):
// expandScenario on a 5x5 grid with a link overloaded at one end, one at both
// ends, two drained nodes and a node that carries an increment (the revived
// edges and their weights, the cleared bits, every no-op and every
// invalid_argument case) and the sweep's constructor merging them into its
// lists, with the form and the domain guards each set of scenarios selects.
// Exit status 0 = every check passed (the sanitizers abort on a finding).
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "decision.h"
#include "lsdb_gen.h"

using namespace openr_amd;
using Sweep = LinkFailureSweep;

namespace {

int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

template <typename Fn>
bool throwsInvalid(Fn fn) {
  try {
    fn();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

std::string ifn(int a, int b) { return "if_" + std::to_string(a) + "_" + std::to_string(b); }

void setOverload(topogen::Lsdb& g, int a, int b) {
  for (auto& adj : g.adjDbs[a].adjs) {
    if (adj.ifName == ifn(a, b)) adj.isOverloaded = true;
  }
}

bool sortedUnique(const std::vector<uint32_t>& v) {
  return std::adjacent_find(v.begin(), v.end(), std::greater_equal<uint32_t>()) == v.end();
}

bool nothing(const Sweep::Expanded& x) {
  return x.deadEdges.empty() && x.drainedNodes.empty() && x.metricEdges.empty() &&
      x.flagNodes.empty() && x.revivedEdges.empty() && x.clearedNodes.empty();
}

}  // namespace

int main() {
  topogen::GridOpts o;
  o.n = 5;
  o.prefixesPerNode = 3;
  auto g = topogen::grid(o);
  setOverload(g, 6, 11);                    // link 6 - 11: overloaded at 6's end
  setOverload(g, 13, 18);                   // link 13 - 18: at both ends
  setOverload(g, 18, 13);
  g.adjDbs[7].isOverloaded = true;          // nodes "7" and the source drained
  g.adjDbs[12].isOverloaded = true;
  g.adjDbs[23].nodeMetricIncrementVal = 4;  // node "23" carries an increment
  for (auto& adj : g.adjDbs[23].adjs) adj.metric += 4;
  LinkState ls(g.area, "test_node");
  PrefixState ps;
  loadLsdb(g, ls, ps);
  const std::string me = "12";

  auto scLinks = [](std::vector<Sweep::LinkDown> l) {
    Sweep::Scenario sc;
    sc.linksUndrained = std::move(l);
    return sc;
  };
  // one end overloaded: both directed edges, the link's weight
  {
    const auto x = Sweep::expandScenario(ls, me, scLinks({{"6", ifn(6, 11)}, {"6", ifn(6, 11)}}));
    EXPECT(x.revivedEdges.size() == 2 && sortedUnique(x.revivedEdges));
    EXPECT(x.revivedVals == std::vector<uint64_t>({1, 1}));
    EXPECT(x.metricEdges.empty() && x.clearedNodes.empty() && x.deadEdges.empty());
  }
  // named from the end that is not overloaded; an up link: no-ops
  EXPECT(nothing(Sweep::expandScenario(ls, me, scLinks({{"11", ifn(11, 6)}}))));
  EXPECT(nothing(Sweep::expandScenario(ls, me, scLinks({{"12", ifn(12, 13)}}))));
  // both ends overloaded: nothing from one end, both edges from both
  EXPECT(nothing(Sweep::expandScenario(ls, me, scLinks({{"13", ifn(13, 18)}}))));
  EXPECT(nothing(Sweep::expandScenario(ls, me, scLinks({{"18", ifn(18, 13)}}))));
  {
    const auto x = Sweep::expandScenario(
        ls, me, scLinks({{"13", ifn(13, 18)}, {"18", ifn(18, 13)}, {"6", ifn(6, 11)}}));
    EXPECT(x.revivedEdges.size() == 4 && sortedUnique(x.revivedEdges));
  }
  // a revived link that also gets a metric: the max of both directions; zero
  // and negative weights expand (the sweep then takes topology copies)
  {
    auto sc = scLinks({{"6", ifn(6, 11)}});
    sc.linkMetrics = {{"11", ifn(11, 6), 9}};
    auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.revivedVals == std::vector<uint64_t>({9, 9}) && x.metricEdges.empty());
    sc.linkMetrics = {{"11", ifn(11, 6), 0}, {"6", ifn(6, 11), 0}};
    x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.revivedVals == std::vector<uint64_t>({0, 0}));
    sc.linkMetrics = {{"11", ifn(11, 6), -3}, {"6", ifn(6, 11), -3}};
    x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.revivedVals.size() == 2 && x.revivedVals[0] > 0xFFFFFFFFull);
    // a link of a downed node stays withdrawn
    sc.linkMetrics.clear();
    sc.nodesDown = {"11"};
    EXPECT(Sweep::expandScenario(ls, me, sc).revivedEdges.empty());
  }
  // node undrain: the bit it carries, the source included; others are no-ops
  {
    Sweep::Scenario sc;
    sc.nodesUndrained = {"7", "12", "3", "7"};
    const auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.clearedNodes.size() == 2 && sortedUnique(x.clearedNodes));
    EXPECT(x.clearedBits == std::vector<uint8_t>({OGS_NODE_OVERLOADED, OGS_NODE_OVERLOADED}));
    EXPECT(x.flagNodes.empty() && x.drainedNodes.empty() && x.revivedEdges.empty());
    sc.nodesUndrained = {"3"};
    EXPECT(nothing(Sweep::expandScenario(ls, me, sc)));
  }
  // soft-undrain: published - the increment on every up link, both bits off
  {
    Sweep::Scenario sc;
    sc.nodesSoftUndrained = {"23", "23"};
    auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.metricEdges.size() == 6 && sortedUnique(x.metricEdges));
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 1u) == 6);
    EXPECT(x.clearedNodes.size() == 1 &&
           x.clearedBits[0] == (OGS_NODE_SOFTDRAIN | OGS_NODE_METRICINC));
    sc.linkMetrics = {{"23", ifn(23, 22), 20}};  // the override first, the increment off it
    x = Sweep::expandScenario(ls, me, sc);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 16u) == 2);
    sc = Sweep::Scenario{};
    sc.nodesSoftUndrained = {"3", "12"};  // increment 0
    EXPECT(nothing(Sweep::expandScenario(ls, me, sc)));
  }
  {
    Sweep::Scenario a, b, c, d, e, f2, h, i, j, k;
    a.linksUndrained = {{"99", "x"}};
    b.linksUndrained = {{"6", "nope"}};
    c.nodesUndrained = {"99"};
    d.nodesSoftUndrained = {"99"};
    e.linksUndrained = {{"6", ifn(6, 11)}};
    e.nodesDown = {"6"};
    f2.nodesUndrained = {"7"};
    f2.nodesDown = {"7"};
    h.nodesSoftUndrained = {"23"};
    h.nodesDown = {"23"};
    i.nodesUndrained = {"7"};
    i.nodesDrained = {"7"};
    j.nodesSoftUndrained = {"23"};
    j.nodesSoftDrained = {{"23", 9}};
    k.linksUndrained = {{"6", ifn(6, 11)}};
    k.linksDown = {{"11", ifn(11, 6)}};  // the same link by its other end
    for (const Sweep::Scenario* bad : {&a, &b, &c, &d, &e, &f2, &h, &i, &j, &k}) {
      EXPECT(throwsInvalid([&] { Sweep::expandScenario(ls, me, *bad); }));
    }
  }

  // the sweep's merged lists and the form each set selects
  std::vector<Sweep::Scenario> scs(4);
  scs[0].linksDown = {{"11", ifn(11, 10)}};
  scs[1] = scLinks({{"6", ifn(6, 11)}});
  scs[1].linkMetrics = {{"13", ifn(13, 14), 8}};  // an override beside the revival
  scs[2].nodesUndrained = {"7"};
  scs[2].nodesSoftDrained = {{"8", 5}};
  scs[3].nodesSoftUndrained = {"23"};
  {
    Sweep sw(me, ls, ps, scs, true);
    EXPECT(sw.numVariants() == 4 && sw.form() == Sweep::kEdgeBitset);
    sw.setMode(Sweep::kFull);
    EXPECT(sw.form() == Sweep::kEdgeBitset);  // copies only once the entry refuses the clears
    sw.setGlobalForm(true);
    EXPECT(sw.form() == Sweep::kGlobalState);
  }
  {
    std::vector<Sweep::Scenario> folded(2);  // restorations that fold away: the register form
    folded[0].linksDown = {{"11", ifn(11, 10)}};
    folded[1].linksUndrained = {{"11", ifn(11, 6)}};
    folded[1].nodesUndrained = {"3"};
    folded[1].nodesSoftUndrained = {"3"};
    Sweep sw(me, ls, ps, folded, true);
    EXPECT(sw.form() == Sweep::kRegisterList);
  }
  for (int64_t m : {int64_t(0), int64_t(-2), int64_t(1) << 30}) {  // the domain guards
    auto exact = scs;
    exact[1].linkMetrics = {{"6", ifn(6, 11), m}, {"11", ifn(11, 6), m}};
    Sweep sw(me, ls, ps, exact, true);
    EXPECT(sw.form() == Sweep::kTopologyCopies);
  }
  if (failures) {
    std::fprintf(stderr, "restore_asan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("restore_asan ok\n");
  return 0;
}
