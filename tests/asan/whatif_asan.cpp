// whatif_asan.cpp — LinkFailureSweep's metric-override and soft-drain
// expansion and list building under AddressSanitizer and
// UndefinedBehaviorSanitizer, over the host-only C-ABI stubs (no device):
// expandScenario on a 5x5 grid with asymmetric metrics, a link that is down
// and a node that already carries an increment (max of directions, no-op
// folding, dead wins, sorting, the soft-drain edge and flag lists, every
// invalid_argument case) and the sweep's constructor with the form and the
// domain guards each set of scenarios selects.
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

void setMetric(topogen::Lsdb& g, int a, int b, int32_t m) {
  for (auto& adj : g.adjDbs[a].adjs) {
    if (adj.ifName == ifn(a, b)) adj.metric = m;
  }
}

bool sortedUnique(const std::vector<uint32_t>& v) {
  return std::adjacent_find(v.begin(), v.end(), std::greater_equal<uint32_t>()) == v.end();
}

}  // namespace

int main() {
  topogen::GridOpts o;
  o.n = 5;
  o.prefixesPerNode = 3;
  auto g = topogen::grid(o);
  setMetric(g, 11, 12, 3);  // link 11 - 12: 3 one way, 7 the other: weight 7
  setMetric(g, 12, 11, 7);
  g.adjDbs[0].adjs[0].isOverloaded = true;  // link 0 - 1 is down already
  g.adjDbs[18].nodeMetricIncrementVal = 4;  // node "18" carries an increment
  for (auto& adj : g.adjDbs[18].adjs) adj.metric += 4;
  LinkState ls(g.area, "test_node");
  PrefixState ps;
  loadLsdb(g, ls, ps);
  const std::string me = "12";

  auto scMetric = [](std::vector<Sweep::LinkMetric> m) {
    Sweep::Scenario sc;
    sc.linkMetrics = std::move(m);
    return sc;
  };
  // the lower direction raised below the higher one: the weight stays, folded
  EXPECT(Sweep::expandScenario(ls, me, scMetric({{"11", ifn(11, 12), 5}})).metricEdges.empty());
  // the lower direction raised past it: both directed edges, the max
  {
    const auto x = Sweep::expandScenario(ls, me, scMetric({{"11", ifn(11, 12), 9}}));
    EXPECT(x.metricEdges.size() == 2 && sortedUnique(x.metricEdges));
    EXPECT(x.metricVals == std::vector<uint64_t>({9, 9}));
    EXPECT(x.deadEdges.empty() && x.flagNodes.empty());
  }
  // the higher direction lowered: the other direction holds the weight up
  {
    const auto x = Sweep::expandScenario(ls, me, scMetric({{"12", ifn(12, 11), 1}}));
    EXPECT(x.metricVals == std::vector<uint64_t>({3, 3}));
  }
  // both directions named: one override per directed edge, the last value of a side wins
  {
    const auto x = Sweep::expandScenario(
        ls, me, scMetric({{"12", ifn(12, 11), 1}, {"11", ifn(11, 12), 2}, {"11", ifn(11, 12), 1}}));
    EXPECT(x.metricEdges.size() == 2 && x.metricVals == std::vector<uint64_t>({1, 1}));
  }
  // the same metric again, a link that is down, a link the scenario takes down
  EXPECT(Sweep::expandScenario(ls, me, scMetric({{"12", ifn(12, 11), 7}})).metricEdges.empty());
  EXPECT(Sweep::expandScenario(ls, me, scMetric({{"1", ifn(1, 0), 50}})).metricEdges.empty());
  {
    auto sc = scMetric({{"11", ifn(11, 12), 50}, {"13", ifn(13, 12), 50}});
    sc.linksDown = {{"12", ifn(12, 11)}};
    const auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.deadEdges.size() == 2 && x.metricEdges.size() == 2);
    for (uint32_t e : x.metricEdges) {
      EXPECT(std::find(x.deadEdges.begin(), x.deadEdges.end(), e) == x.deadEdges.end());
    }
    sc.nodesDown = {"13"};
    EXPECT(Sweep::expandScenario(ls, me, sc).metricEdges.empty());
  }
  // zero and negative metrics expand (the sweep then takes topology copies)
  {
    const auto x = Sweep::expandScenario(
        ls, me, scMetric({{"13", ifn(13, 12), 0}, {"12", ifn(12, 13), 0}, {"7", ifn(7, 12), -3}}));
    EXPECT(x.metricEdges.size() == 4);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 0u) == 2);
    EXPECT(std::count_if(x.metricVals.begin(), x.metricVals.end(),
                         [](uint64_t v) { return v > 0xFFFFFFFFull; }) == 2);
  }
  // soft drain of the centre: its 4 links (8 directed edges) and the two bits;
  // the source itself may be soft-drained
  {
    Sweep::Scenario sc;
    sc.nodesSoftDrained = {{"12", 50}, {"12", 50}};
    const auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.metricEdges.size() == 8 && sortedUnique(x.metricEdges));
    // link 11 - 12: max(3, 7 + 50); the unit links: 51
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 57u) == 2);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 51u) == 6);
    EXPECT(x.flagNodes.size() == 1 && x.flagBits[0] == (OGS_NODE_SOFTDRAIN | OGS_NODE_METRICINC));
    EXPECT(x.drainedNodes.empty());
  }
  // a corner whose one link is down: one link moves
  {
    Sweep::Scenario sc;
    sc.nodesSoftDrained = {{"0", 10}};
    EXPECT(Sweep::expandScenario(ls, me, sc).metricEdges.size() == 2);
  }
  // a node that carries 4 already: the same value is a no-op, another moves by
  // the difference and adds no bit; with a hard drain the bits are ORed
  {
    Sweep::Scenario sc;
    sc.nodesSoftDrained = {{"18", 4}};
    auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.metricEdges.empty() && x.flagNodes.empty());
    sc.nodesSoftDrained = {{"18", 10}};
    sc.nodesDrained = {"18", "13"};
    x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.metricEdges.size() == 8);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 11u) == 8);
    EXPECT(x.flagNodes.size() == 2 && x.drainedNodes.size() == 2);
    EXPECT(x.flagBits == std::vector<uint8_t>({OGS_NODE_OVERLOADED, OGS_NODE_OVERLOADED}));
    // an override on a drained node's adjacency, then the increment on top
    sc.nodesDrained.clear();
    sc.nodesSoftDrained = {{"6", 5}};
    sc.linkMetrics = {{"6", ifn(6, 7), 20}};
    x = Sweep::expandScenario(ls, me, sc);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 25u) == 2);
    EXPECT(std::count(x.metricVals.begin(), x.metricVals.end(), 6u) == 6);
  }
  {
    Sweep::Scenario a, b, c, d, e, f2, h;
    a.linkMetrics = {{"99", "x", 1}};
    b.linkMetrics = {{"11", "nope", 1}};
    c.nodesSoftDrained = {{"99", 1}};
    d.nodesSoftDrained = {{"11", 0}};
    e.nodesSoftDrained = {{"11", 5}};
    e.nodesDown = {"11"};
    f2.nodesSoftDrained = {{"11", 5}, {"11", 6}};
    h.linkMetrics = {{"11", ifn(11, 12), int64_t(1) << 40}};
    for (const Sweep::Scenario* bad : {&a, &b, &c, &d, &e, &f2, &h}) {
      EXPECT(throwsInvalid([&] { Sweep::expandScenario(ls, me, *bad); }));
    }
  }

  // the sweep's lists and the form each set selects
  std::vector<Sweep::Scenario> scs(3);
  scs[0].linksDown = {{"11", ifn(11, 12)}};
  scs[1] = scMetric({{"13", ifn(13, 12), 8}});
  {
    Sweep sw(me, ls, ps, scs, true);
    EXPECT(sw.numVariants() == 3 && sw.form() == Sweep::kEdgeBitset);
    sw.setMode(Sweep::kFull);
    EXPECT(sw.form() == Sweep::kEdgeBitset);
  }
  {
    auto folded = scs;  // an override that folds away leaves the register form
    folded[1] = scMetric({{"11", ifn(11, 12), 5}});
    Sweep sw(me, ls, ps, folded, true);
    EXPECT(sw.form() == Sweep::kRegisterList);
  }
  {
    auto soft = scs;
    soft[2].nodesSoftDrained = {{"6", 1000}};
    Sweep sw(me, ls, ps, soft, true);
    EXPECT(sw.form() == Sweep::kEdgeBitset);
  }
  for (int64_t m : {int64_t(0), int64_t(-2), int64_t(1) << 30}) {  // the domain guards
    auto exact = scs;
    exact[2] = scMetric({{"13", ifn(13, 14), m}, {"14", ifn(14, 13), m}});
    Sweep sw(me, ls, ps, exact, true);
    EXPECT(sw.form() == Sweep::kTopologyCopies);
  }
  if (failures) {
    std::fprintf(stderr, "whatif_asan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("whatif_asan ok\n");
  return 0;
}
