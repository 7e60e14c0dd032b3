// network_asan.cpp — NetworkWhatifSweep's host side under AddressSanitizer
// and UndefinedBehaviorSanitizer, over the host-only C-ABI stubs (no device):
// plan building (pair order, the pairs whose source is down), chunk planning
// at several bounds, the batched / fallback split on a fabric whose FSWs keep
// two next-hop words and on an area with a zero metric, the validation
// errors, and the sweep's constructor with its accessors before any launch.
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

using Pairs = std::vector<std::pair<uint32_t, uint32_t>>;

}  // namespace

int main() {
  topogen::GridOpts o;
  o.n = 5;
  o.prefixesPerNode = 3;
  auto g = topogen::grid(o);
  LinkState ls(g.area, "test_node");
  PrefixState ps;
  loadLsdb(g, ls, ps);

  std::vector<Sweep::Scenario> scs(5);
  scs[0].linksDown = {{"11", ifn(11, 12)}};
  scs[1].nodesDown = {"7"};
  scs[2].nodesSoftDrained = {{"12", 40}};
  scs[3].nodesDown = {"3", "7"};
  scs[3].nodesDrained = {"12"};
  const std::vector<std::string> sources = {"12", "7", "0", "3"};
  {
    const NetworkWhatifPlan p = network_whatif_plan(ls, ps, sources, scs);
    EXPECT(p.batched == std::vector<uint32_t>({0, 1, 2, 3}) && p.fallback.empty());
    EXPECT(p.sourceDown == Pairs({{1, 1}, {1, 3}, {3, 3}}));
    Pairs want;
    for (uint32_t s = 0; s < 4; ++s) {
      for (uint32_t k = 0; k < 5; ++k) {
        if (std::find(p.sourceDown.begin(), p.sourceDown.end(), std::make_pair(s, k)) ==
            p.sourceDown.end()) {
          want.emplace_back(s, k);
        }
      }
    }
    EXPECT(p.pairs == want);
    EXPECT(p.chunks == std::vector<size_t>({0, want.size()}));
    EXPECT(p.unitBytes > p.impactUnitBytes && p.impactUnitBytes >= 12);
    // chunk planning: whole units, every unit once, also below one unit
    for (size_t units : {size_t(1), size_t(3), size_t(7), size_t(100)}) {
      for (size_t extra : {size_t(0), p.unitBytes - 1}) {
        const auto c = network_whatif_plan(ls, ps, sources, scs, units * p.unitBytes + extra);
        EXPECT(c.chunks.front() == 0 && c.chunks.back() == want.size());
        for (size_t i = 0; i + 1 < c.chunks.size(); ++i) {
          const size_t n = c.chunks[i + 1] - c.chunks[i];
          EXPECT(n >= 1 && n <= units && (n == units || i + 2 == c.chunks.size()));
        }
        EXPECT(c.impactChunks.front() == 0 && c.impactChunks.back() == want.size());
        EXPECT(c.impactChunks.size() <= c.chunks.size());
      }
    }
    EXPECT(network_whatif_plan(ls, ps, sources, scs, 0).chunks.size() == want.size() + 1);
    EXPECT(network_whatif_plan(ls, ps, {}, scs).chunks == std::vector<size_t>({0}));
    EXPECT(network_whatif_plan(ls, ps, sources, {}).pairs.empty());
  }
  // validation: as the sweep's, but for a source in nodesDown
  {
    Sweep::Scenario a, b, c;
    a.nodesDown = {"99"};
    b.linksDown = {{"11", "nope"}};
    c.nodesDown = {"7"};
    c.nodesDrained = {"7"};
    for (const Sweep::Scenario* bad : {&a, &b, &c}) {
      EXPECT(throwsInvalid([&] { network_whatif_plan(ls, ps, sources, {*bad}); }));
      EXPECT(throwsInvalid([&] { NetworkWhatifSweep(ls, ps, sources, {*bad}, true); }));
    }
    EXPECT(throwsInvalid([&] { network_whatif_plan(ls, ps, {"12", "99"}, scs); }));
  }
  // the sweep before any launch: states, and what needs a fetch throws
  {
    NetworkWhatifSweep net(ls, ps, sources, scs, true);
    EXPECT(net.numSources() == 4 && net.numScenarios() == 5 && net.batchedSources() == 4);
    EXPECT(net.state(1, 1) == NetworkWhatifSweep::kSourceDown);
    EXPECT(net.state(1, 0) == NetworkWhatifSweep::kComputed);
    EXPECT(throwsInvalid([&] { net.routeUpdate(3, 3); }));
    bool threw = false;
    try {
      net.counts(0, 0);
    } catch (const std::logic_error&) {
      threw = true;
    }
    EXPECT(threw);
    net.setChunkBytes(2 * net.plan().unitBytes);
    EXPECT(net.numChunks() == (net.plan().pairs.size() + 1) / 2);
    EXPECT(net.numChunks(false) < net.numChunks());
  }
  // an area with a zero metric: every source through its own sweep
  {
    auto z = topogen::grid(o);
    for (auto& d : z.adjDbs) {  // node "6"'s links, both directions
      for (auto& adj : d.adjs) {
        if (d.thisNodeName == "6" || adj.otherNodeName == "6") adj.metric = 0;
      }
    }
    LinkState zls(z.area, "test_node");
    PrefixState zps;
    loadLsdb(z, zls, zps);
    const NetworkWhatifPlan p = network_whatif_plan(zls, zps, sources, scs);
    EXPECT(p.batched.empty() && p.fallback.size() == 4 && p.pairs.empty());
    EXPECT(p.sourceDown.size() == 3);
    NetworkWhatifSweep net(zls, zps, sources, scs, true);
    EXPECT(net.batchedSources() == 0 && net.numChunks() == 0);
    EXPECT(net.state(3, 3) == NetworkWhatifSweep::kSourceDown);
  }
  // a weight of the exact domain in one scenario: the same
  {
    auto exact = scs;
    exact[4].linkMetrics = {{"13", ifn(13, 14), 0}, {"14", ifn(14, 13), 0}};
    EXPECT(network_whatif_plan(ls, ps, sources, exact).batched.empty());
  }
  // a fabric: FSWs of 40 links keep two next-hop words and fall back, SSWs
  // and RSWs are batched
  {
    topogen::FabricOpts fo;
    fo.pods = 2;
    fo.planes = 2;
    fo.sswPerPlane = 4;
    fo.rswPerPod = 36;
    auto fab = topogen::fabric(fo);
    LinkState fls(fab.area, "test_node");
    PrefixState fps;
    loadLsdb(fab, fls, fps);
    std::vector<std::string> wide, narrow;
    for (const auto& d : fab.adjDbs) (d.adjs.size() > 32 ? wide : narrow).push_back(d.thisNodeName);
    EXPECT(wide.size() == 4 && narrow.size() == 8 + 72);
    std::vector<Sweep::Scenario> fs(3);
    fs[0].nodesDown = {wide[0]};
    fs[1].nodesDrained = {wide[1]};
    fs[2].nodesDown = {narrow[0], wide[3]};
    const std::vector<std::string> src = {narrow[0], wide[0], narrow[20], wide[3], narrow[79]};
    const NetworkWhatifPlan p = network_whatif_plan(fls, fps, src, fs);
    EXPECT(p.batched == std::vector<uint32_t>({0, 2, 4}));
    EXPECT(p.fallback == std::vector<uint32_t>({1, 3}));
    EXPECT(p.sourceDown == Pairs({{0, 2}, {1, 0}, {3, 2}}));
    EXPECT(p.pairs == Pairs({{0, 0}, {0, 1}, {2, 0}, {2, 1}, {2, 2}, {4, 0}, {4, 1}, {4, 2}}));
    NetworkWhatifSweep net(fls, fps, src, fs, true);  // builds the two fallback sweeps
    EXPECT(net.batchedSources() == 3 && net.plan().fallback.size() == 2);
    EXPECT(net.state(1, 0) == NetworkWhatifSweep::kSourceDown);
    EXPECT(net.state(1, 1) == NetworkWhatifSweep::kComputed);
  }
  if (failures) {
    std::fprintf(stderr, "network_asan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("network_asan ok\n");
  return 0;
}
