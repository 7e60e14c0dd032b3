// network_asan.cpp — NetworkWhatifSweep's host side under AddressSanitizer
// and UndefinedBehaviorSanitizer, over the host-only C-ABI stubs (no device):
// plan building (pair order, the pairs whose source is down), chunk planning
// at several bounds, the batched / fallback split on a fabric whose FSWs keep
// two next-hop words and on an area with a zero metric, the validation
// errors, and the sweep's constructor with its accessors before any launch;
// and the pieces the two sweeps share: the counts scan, CompactChanges' chunk
// order rules, WhatifDeviceLists' upload and descriptor.
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
  // the counts scan both sweeps share: a refused unit adds nothing
  {
    const uint32_t R = OGS_WHATIF_REFUSED;
    const std::vector<uint32_t> counts = {3, 1, R, R, 0, 2};
    std::vector<uint32_t> offsets;
    EXPECT(scanChangeCounts<2>(counts.data(), 3, offsets) == 6);
    EXPECT(offsets == std::vector<uint32_t>({0, 4, 4, 6}));
    const std::vector<uint32_t> rows = {2, 0, 5};  // label rows: one count a unit
    EXPECT(scanChangeCounts<1>(rows.data(), 3, offsets) == 7);
    EXPECT(offsets == std::vector<uint32_t>({0, 2, 2, 7}));
    const std::vector<uint32_t> big = {0xFFFFFFFEu, 0, 2, 0};
    bool threw = false;
    try {
      scanChangeCounts<2>(big.data(), 2, offsets);
    } catch (const std::length_error&) {
      threw = true;
    }
    EXPECT(threw);
    EXPECT(scanChangeCounts<2>(big.data() + 2, 1, offsets, 0xFFFFFFFDu) == 2);  // 2^32 - 1: fits
  }
  // compact records: chunks append in unit order, and only at W = 1 (chunks
  // without changes reach no device call)
  {
    const std::vector<uint32_t> none(8, 0);
    const ogs_spf_out rec{};
    auto throwsLogic = [&](CompactChanges& c, size_t u0) {
      try {
        c.gather(u0, 2, none.data(), nullptr, rec, 1, nullptr);
      } catch (const std::logic_error&) {
        return true;
      }
      return false;
    };
    CompactChanges one, two;
    one.reset(4, 1);
    EXPECT(!throwsLogic(one, 0) && throwsLogic(one, 0) && !throwsLogic(one, 2));
    EXPECT(throwsLogic(one, 4));  // past the units
    const ChangeRecords v = one.view();
    EXPECT(v.variants == 4 && v.total == 0 && v.W == 1 && v.offsets[4] == 0);
    two.reset(4, 2);
    EXPECT(!throwsLogic(two, 0) && throwsLogic(two, 2));
  }
  // the device scenario lists: no flag list, a revived link among the metrics
  {
    Sweep::Scenario down, up, cost;
    down.linksDown = {{"11", ifn(11, 12)}};
    LinkState dls(g.area, "test_node");  // the link 12-13 overloaded at one end
    PrefixState dps;
    auto dg = topogen::grid(o);
    for (auto& d : dg.adjDbs) {
      for (auto& adj : d.adjs) {
        if (d.thisNodeName == "12" && adj.otherNodeName == "13") adj.isOverloaded = true;
      }
    }
    loadLsdb(dg, dls, dps);
    up.linksUndrained = {{"12", ifn(12, 13)}};
    cost.linkMetrics = {{"6", ifn(6, 7), 9}, {"7", ifn(7, 6), 9}};
    Sweep::Lists lists;
    for (const Sweep::Scenario* sc : {&down, &up, &cost}) {
      lists.append(Sweep::expandScenario(dls, "0", *sc));
    }
    EXPECT(lists.flagNode.empty() && lists.restores && lists.metricEdge.size() == 4);
    Sweep::WhatifDeviceLists dl;
    dl.upload(lists);
    dl.upload(lists);  // once
    const ogs_whatif_mods m0 = dl.mods(), m2 = dl.mods(2);
    EXPECT(!m0.node_off && !m0.node_ids && !m0.node_bits);
    EXPECT(!m2.node_off && !m2.node_ids && !m2.node_bits);
    EXPECT(m0.dead_off == dl.deadOff.as<uint32_t>() && m2.dead_off == m0.dead_off + 2);
    EXPECT(m0.metric_off && m2.metric_off == m0.metric_off + 2);
    EXPECT(m2.dead_edges == m0.dead_edges && m2.metric_edges == m0.metric_edges &&
           m2.metric_vals == m0.metric_vals);
    EXPECT(m0.max_metric_per_unit == lists.maxMetricList && m2.max_metric_per_unit == 2);
    // (the stub's device memory is host memory)
    for (size_t i = 0; i < lists.metricEdge.size(); ++i) {
      EXPECT(m0.metric_edges[i] == lists.metricEdge[i]);
      EXPECT((m0.metric_vals[i] & ~OGS_WHATIF_EDGE_UP) == uint32_t(lists.metricVal[i]));
      EXPECT(((m0.metric_vals[i] & OGS_WHATIF_EDGE_UP) != 0) == (lists.metricUp[i] != 0));
      EXPECT((lists.metricUp[i] != 0) == (i < 2));  // scenario 1 revives, scenario 2 overrides
    }
    // no metric list either: only the dead lists are passed
    Sweep::Lists deadOnly;
    deadOnly.append(Sweep::expandScenario(dls, "0", down));
    Sweep::WhatifDeviceLists dd;
    dd.uploadDead(deadOnly);
    dd.upload(deadOnly);
    const ogs_whatif_mods md = dd.mods();
    EXPECT(md.dead_off && md.dead_edges && !md.node_off && !md.metric_off && !md.metric_vals);
    EXPECT(md.dead_off[1] == 2 && md.dead_edges[0] == deadOnly.deadList[0]);
  }
  if (failures) {
    std::fprintf(stderr, "network_asan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("network_asan ok\n");
  return 0;
}
