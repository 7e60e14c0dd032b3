// scenario_asan.cpp — LinkFailureSweep's scenario expansion and list
// building under AddressSanitizer and UndefinedBehaviorSanitizer, over the
// host-only C-ABI stubs (no device): expandScenario on a 5x5 grid with a
// seeded share of overloaded adjacencies and nodes (links down named from
// either end, nodes down, drains, every invalid_argument case) and the
// sweep's constructor (CSR lists, register slots, uploads into the stub's
// host memory) with the form each set of scenarios selects.
// Exit status 0 = every check passed (the sanitizers abort on a finding).
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

}  // namespace

int main() {
  topogen::GridOpts o;
  o.n = 5;
  o.prefixesPerNode = 3;
  auto g = topogen::grid(o);
  g.adjDbs[7].isOverloaded = true;           // node "7" is drained already
  g.adjDbs[0].adjs[0].isOverloaded = true;   // link 0 - 1 is down already
  LinkState ls(g.area, "test_node");
  PrefixState ps;
  loadLsdb(g, ls, ps);
  const std::string me = "12";

  // a downed node of degree d: 2d directed edges; the centre's neighbour 11
  {
    Sweep::Scenario sc;
    sc.nodesDown = {"11"};
    const auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.deadEdges.size() == 8 && x.drainedNodes.empty());
  }
  // a corner whose one link is down already: 2 edges left
  {
    Sweep::Scenario sc;
    sc.nodesDown = {"0"};
    EXPECT(Sweep::expandScenario(ls, me, sc).deadEdges.size() == 2);
  }
  // the same link from both ends, and as a link of a downed node: folded
  {
    Sweep::Scenario sc;
    sc.linksDown = {{"11", ifn(11, 12)}, {"12", ifn(12, 11)}, {"11", ifn(11, 10)}};
    EXPECT(Sweep::expandScenario(ls, me, sc).deadEdges.size() == 4);
    sc.nodesDown = {"11"};
    EXPECT(Sweep::expandScenario(ls, me, sc).deadEdges.size() == 8);
  }
  // drains: an overloaded node is a no-op, duplicates fold, `me` may drain
  {
    Sweep::Scenario sc;
    sc.nodesDrained = {"7", "13", "13", "12"};
    const auto x = Sweep::expandScenario(ls, me, sc);
    EXPECT(x.deadEdges.empty() && x.drainedNodes.size() == 2);
  }
  // a link that is down already: no-op
  {
    Sweep::Scenario sc;
    sc.linksDown = {{"1", ifn(1, 0)}};
    EXPECT(Sweep::expandScenario(ls, me, sc).deadEdges.empty());
  }
  for (const Sweep::Scenario& bad : {
           Sweep::Scenario{{{"99", "x"}}, {}, {}}, Sweep::Scenario{{{"11", "nope"}}, {}, {}},
           Sweep::Scenario{{}, {"99"}, {}}, Sweep::Scenario{{}, {}, {"99"}},
           Sweep::Scenario{{}, {me}, {}}, Sweep::Scenario{{}, {"11"}, {"11"}}}) {
    EXPECT(throwsInvalid([&] { Sweep::expandScenario(ls, me, bad); }));
  }

  // the sweep's lists: register form while every list has <= 8 edges and
  // nothing drains, the bitset form past that, forced, or with a drain
  std::vector<Sweep::Scenario> small(3);
  small[0].linksDown = {{"11", ifn(11, 12)}};
  small[1].nodesDown = {"11"};  // exactly 8
  {
    Sweep sw(me, ls, ps, small, true);
    EXPECT(sw.numVariants() == 3 && sw.form() == Sweep::kRegisterList);
    sw.setListForm(true);
    EXPECT(sw.form() == Sweep::kEdgeBitset);
    sw.setListForm(false);
    EXPECT(sw.form() == Sweep::kRegisterList);
  }
  {
    auto big = small;
    big[2].nodesDown = {"11"};
    big[2].linksDown = {{"13", ifn(13, 14)}};  // 10 edges
    Sweep sw(me, ls, ps, big, true);
    EXPECT(sw.form() == Sweep::kEdgeBitset);
  }
  {
    auto drain = small;
    drain[2].nodesDrained = {"13"};
    Sweep sw(me, ls, ps, drain, true);
    EXPECT(sw.form() == Sweep::kEdgeBitset);
  }
  {
    Sweep sw(me, ls, ps, std::vector<Sweep::Scenario>{}, true);
    EXPECT(sw.numVariants() == 0);
  }
  // the two-link constructor delegates; more than two links are taken now
  {
    std::vector<std::vector<Sweep::LinkDown>> v{
        {{"11", ifn(11, 12)}, {"13", ifn(13, 12)}, {"7", ifn(7, 12)}}};
    Sweep sw(me, ls, ps, v, true);
    EXPECT(sw.numVariants() == 1 && sw.form() == Sweep::kRegisterList);
  }
  EXPECT(throwsInvalid([&] { Sweep sw("nobody", ls, ps, small, true); }));
  if (failures) {
    std::fprintf(stderr, "scenario_asan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("scenario_asan ok\n");
  return 0;
}
