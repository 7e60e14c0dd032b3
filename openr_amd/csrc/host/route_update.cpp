// route_update.cpp — LinkFailureSweep: batched what-if route updates
// (SURVEY.md §8(f) f1 over config C4).
//
// Reference: Decision::rebuildRoutes (Decision.cpp:912-951) rebuilds the
// RouteDb after a topology change and publishes
// DecisionRouteDb::calculateUpdate(old, new) (SpfSolver.cpp:21-56) to Fib.
// Here the "new" RouteDbs of many what-if variants (links down, nodes down,
// nodes drained) come out of one ogs_spf_routes_variants or
// ogs_spf_routes_scenarios launch with that diff fused in; the changed records
// are gathered on the device and only those are materialised into
// DecisionRouteUpdate (unicastRoutesToUpdate / unicastRoutesToDelete).
#include <algorithm>
#include <atomic>
#include <exception>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>

#include "decision.h"

namespace openr_amd {

// Best-entry equality classes for the route diffs (ogs_route_diff.adv_class,
// ogs_route_delta): per prefix, the list [entries as is, entries with the
// drain override] of materialised best entries (weight cleared,
// RibEntry.h:77), each numbered by the first equal one.
std::vector<uint32_t> advClasses(const PrefixHostTable& table) {
  std::vector<uint32_t> cls(std::max<size_t>(2 * table.advEntry.size(), 1), 0);
  for (size_t p = 0; p + 1 < table.advOff.size(); ++p) {
    const uint32_t a0 = table.advOff[p], k = table.advOff[p + 1] - a0;
    std::vector<PrefixEntry> eff;
    eff.reserve(2 * k);
    for (int drained = 0; drained < 2; ++drained) {
      for (uint32_t i = 0; i < k; ++i) {
        PrefixEntry e = *table.advEntry[a0 + i];
        e.weight = std::nullopt;
        if (drained) e.metrics.drain_metric = 1;
        eff.push_back(std::move(e));
      }
    }
    for (uint32_t j = 0; j < 2 * k; ++j) {
      uint32_t c = j;
      for (uint32_t i = 0; i < j; ++i) {
        if (eff[i] == eff[j]) {
          c = i;
          break;
        }
      }
      const uint32_t i = j % k, drained = j / k;
      cls[2 * (a0 + i) + drained] = c;
    }
  }
  return cls;
}

namespace {

std::vector<LinkFailureSweep::Scenario> linkScenarios(
    const std::vector<std::vector<LinkFailureSweep::LinkDown>>& variants) {
  std::vector<LinkFailureSweep::Scenario> out(variants.size());
  for (size_t v = 0; v < variants.size(); ++v) out[v].linksDown = variants[v];
  return out;
}

}  // namespace

LinkFailureSweep::LinkFailureSweep(
    const std::string& myNodeName, const LinkState& ls, const PrefixState& ps,
    const std::vector<std::vector<LinkDown>>& variants, bool enableV4,
    bool enableBestRouteSelection, bool v4OverV6Nexthop, bool enableNodeSegmentLabel)
    : LinkFailureSweep(myNodeName, ls, ps, linkScenarios(variants), enableV4,
                       enableBestRouteSelection, v4OverV6Nexthop, enableNodeSegmentLabel) {}

LinkFailureSweep::Expanded LinkFailureSweep::expandScenario(const LinkState& ls,
                                                            const std::string& me,
                                                            const Scenario& sc) {
  const FlatTopology& f = ls.flat();
  auto nodeId = [&](const std::string& node) {
    auto it = f.id.find(node);
    if (it == f.id.end()) throw std::invalid_argument("LinkFailureSweep: unknown node " + node);
    return it->second;
  };
  Expanded x;
  std::set<const Link*> killed;
  // edge of row u behind interface ifName
  auto edgeOf = [&](uint32_t u, const std::string& node, const std::string& ifName) {
    uint32_t e = f.rowPtr[u];
    while (e < f.rowPtr[u + 1] && f.edgeLink[e]->getIfaceFromNode(node) != ifName) ++e;
    if (e == f.rowPtr[u + 1]) {
      throw std::invalid_argument("LinkFailureSweep: no link " + node + "%" + ifName);
    }
    return e;
  };
  // both directed edges of the link behind edge e of row u, when it is up
  auto kill = [&](uint32_t u, uint32_t e) {
    const Link* link = f.edgeLink[e];
    if (!link->isUp()) return;  // already down: removing it changes nothing
    killed.insert(link);
    x.deadEdges.push_back(e);
    const uint32_t o = f.id.at(link->getOtherNodeName(f.names[u]));
    for (uint32_t r = f.rowPtr[o]; r < f.rowPtr[o + 1]; ++r) {
      if (f.edgeLink[r] == link) x.deadEdges.push_back(r);
    }
  };
  std::set<const Link*> namedDown;
  for (const auto& d : sc.linksDown) {
    const uint32_t u = nodeId(d.node);
    const uint32_t e = edgeOf(u, d.node, d.ifName);
    namedDown.insert(f.edgeLink[e]);
    kill(u, e);
  }
  std::vector<uint32_t> down;
  for (const auto& n : sc.nodesDown) {
    if (n == me) throw std::invalid_argument("LinkFailureSweep: " + me + " itself in nodesDown");
    const uint32_t u = nodeId(n);
    down.push_back(u);
    for (uint32_t e = f.rowPtr[u]; e < f.rowPtr[u + 1]; ++e) kill(u, e);
  }
  for (const auto& n : sc.nodesDrained) {
    const uint32_t u = nodeId(n);
    if (std::find(down.begin(), down.end(), u) != down.end()) {
      throw std::invalid_argument("LinkFailureSweep: " + n + " both down and drained");
    }
    if (!(f.nodeFlags[u] & OGS_NODE_OVERLOADED)) x.drainedNodes.push_back(u);
  }
  // ---- restorations: the overload bit off an adjacency or a node -----------
  auto notDown = [&](uint32_t u, const std::string& n, const char* what) {
    if (std::find(down.begin(), down.end(), u) != down.end()) {
      throw std::invalid_argument("LinkFailureSweep: " + n + " both down and " + what);
    }
  };
  std::map<const Link*, unsigned> undrained;  // sides re-sent with isOverloaded = false
  for (const auto& d : sc.linksUndrained) {
    const uint32_t u = nodeId(d.node);
    const Link* l = f.edgeLink[edgeOf(u, d.node, d.ifName)];
    notDown(u, d.node, "in linksUndrained");
    if (namedDown.count(l)) {
      throw std::invalid_argument("LinkFailureSweep: link " + d.node + "%" + d.ifName +
                                  " both down and undrained");
    }
    undrained[l] |= d.node == l->firstNodeName() ? 1u : 2u;
  }
  std::map<uint32_t, uint8_t> cleared;
  for (const auto& n : sc.nodesUndrained) {
    const uint32_t u = nodeId(n);
    notDown(u, n, "undrained");
    if (std::find(sc.nodesDrained.begin(), sc.nodesDrained.end(), n) != sc.nodesDrained.end()) {
      throw std::invalid_argument("LinkFailureSweep: " + n + " both drained and undrained");
    }
    if (f.nodeFlags[u] & OGS_NODE_OVERLOADED) cleared[u] |= uint8_t(OGS_NODE_OVERLOADED);
  }
  for (auto* l : {&x.deadEdges, &x.drainedNodes}) {  // the same link named twice folds
    std::sort(l->begin(), l->end());
    l->erase(std::unique(l->begin(), l->end()), l->end());
  }
  // ---- metrics: what every touched link's two directions would carry ------
  // (keyed by the edge of the link in its first node's row: a stable order)
  struct Moved {
    const Link* link;
    LinkStateMetric m[2];  // from firstNodeName(), from secondNodeName()
  };
  std::map<const Link*, Moved> moved;
  auto sideMetric = [&](const Link* l, const std::string& node) -> LinkStateMetric& {
    auto it = moved.find(l);
    if (it == moved.end()) {
      it = moved.emplace(l, Moved{l, {l->getMetricFromNode(l->firstNodeName()),
                                      l->getMetricFromNode(l->secondNodeName())}}).first;
    }
    return it->second.m[node == l->firstNodeName() ? 0 : 1];
  };
  auto i32 = [](int64_t v, const char* what) {
    if (v < INT32_MIN || v > INT32_MAX) {
      throw std::invalid_argument(std::string("LinkFailureSweep: ") + what + " outside i32");
    }
    return static_cast<LinkStateMetric>(static_cast<int64_t>(static_cast<int32_t>(v)));
  };
  for (const auto& d : sc.linkMetrics) {
    const uint32_t u = nodeId(d.node);
    const Link* l = f.edgeLink[edgeOf(u, d.node, d.ifName)];
    sideMetric(l, d.node) = i32(d.metric, "link metric");
  }
  std::map<uint32_t, uint8_t> bits;
  for (uint32_t u : x.drainedNodes) bits[u] |= uint8_t(OGS_NODE_OVERLOADED);
  std::map<uint32_t, int64_t> soft;
  for (const auto& d : sc.nodesSoftDrained) {
    const uint32_t u = nodeId(d.node);
    if (std::find(down.begin(), down.end(), u) != down.end()) {
      throw std::invalid_argument("LinkFailureSweep: " + d.node + " both down and soft-drained");
    }
    if (d.increment < 1) {
      throw std::invalid_argument("LinkFailureSweep: soft-drain increment of " + d.node + " < 1");
    }
    i32(d.increment, "soft-drain increment");
    auto [it, fresh] = soft.emplace(u, d.increment);
    if (!fresh && it->second != d.increment) {
      throw std::invalid_argument("LinkFailureSweep: " + d.node + " soft-drained twice");
    }
  }
  for (const auto& [u, inc] : soft) {
    const std::string& node = f.names[u];
    // LinkMonitor.cpp:1001: published - the increment it carries + the new one
    const LinkStateMetric delta =
        static_cast<LinkStateMetric>(inc) - ls.getNodeMetricIncrement(node);
    for (uint32_t e = f.rowPtr[u]; e < f.rowPtr[u + 1]; ++e) {
      sideMetric(f.edgeLink[e], node) += delta;
    }
    const uint8_t add = uint8_t((OGS_NODE_SOFTDRAIN | OGS_NODE_METRICINC) & ~f.nodeFlags[u]);
    if (add) bits[u] |= add;
  }
  std::set<uint32_t> softOff;
  for (const auto& n : sc.nodesSoftUndrained) {
    const uint32_t u = nodeId(n);
    notDown(u, n, "soft-undrained");
    if (soft.count(u)) {
      throw std::invalid_argument("LinkFailureSweep: " + n +
                                  " both soft-drained and soft-undrained");
    }
    if (!softOff.insert(u).second) continue;  // named twice: once
    const uint64_t inc = ls.getNodeMetricIncrement(n);
    if (inc == 0) continue;  // nothing to take off
    // LinkMonitor.cpp:1001: published - the increment it carries
    for (uint32_t e = f.rowPtr[u]; e < f.rowPtr[u + 1]; ++e) {
      sideMetric(f.edgeLink[e], n) -= static_cast<LinkStateMetric>(inc);
    }
    const uint8_t off = uint8_t((OGS_NODE_SOFTDRAIN | OGS_NODE_METRICINC) & f.nodeFlags[u]);
    if (off) cleared[u] |= off;
  }
  // both directed edges of link l with weight w
  auto bothEdges = [&](const Link* l, uint64_t w, std::vector<std::pair<uint32_t, uint64_t>>& to) {
    for (const std::string* n : {&l->firstNodeName(), &l->secondNodeName()}) {
      const uint32_t u = f.id.at(*n);
      for (uint32_t e = f.rowPtr[u]; e < f.rowPtr[u + 1]; ++e) {
        if (f.edgeLink[e] == l) to.emplace_back(e, w);
      }
    }
  };
  std::vector<std::pair<uint32_t, uint64_t>> over, revived;
  for (const auto& [l, mv] : moved) {
    if (!l->isUp() || killed.count(l)) continue;  // down stays down (or comes up, below)
    const LinkStateMetric w = std::max(mv.m[0], mv.m[1]);
    if (w == l->getMaxMetric()) continue;  // the link's weight stays: a no-op
    bothEdges(l, w, over);
  }
  // a link comes up when Link::isUp() holds with the named ends' bits off; one
  // that touches a downed node stays withdrawn
  for (const auto& [l, sides] : undrained) {
    if (l->isUp()) continue;  // up already: a no-op
    const bool ov0 = l->getOverloadFromNode(l->firstNodeName()) && !(sides & 1u);
    const bool ov1 = l->getOverloadFromNode(l->secondNodeName()) && !(sides & 2u);
    if (ov0 || ov1 || !l->getUsability()) continue;  // stays down: a no-op
    bool gone = false;
    for (const std::string* n : {&l->firstNodeName(), &l->secondNodeName()}) {
      gone |= std::find(down.begin(), down.end(), f.id.at(*n)) != down.end();
    }
    if (gone) continue;
    const auto it = moved.find(l);
    bothEdges(l, it == moved.end() ? l->getMaxMetric() : std::max(it->second.m[0], it->second.m[1]),
              revived);
  }
  for (auto* l : {&over, &revived}) {
    std::sort(l->begin(), l->end());
    l->erase(std::unique(l->begin(), l->end()), l->end());
  }
  for (const auto& [e, w] : over) {
    x.metricEdges.push_back(e);
    x.metricVals.push_back(w);
  }
  for (const auto& [e, w] : revived) {
    x.revivedEdges.push_back(e);
    x.revivedVals.push_back(w);
  }
  for (const auto& [u, b] : cleared) {
    x.clearedNodes.push_back(u);
    x.clearedBits.push_back(b);
  }
  for (const auto& [u, b] : bits) {
    x.flagNodes.push_back(u);
    x.flagBits.push_back(b);
  }
  return x;
}

// One scenario's lists appended as CSR slices: dead edges and drained nodes;
// the metric slice (overrides and revived edges, disjoint: an override is of
// an up link, merged ascending by edge id); the node list (one entry a node,
// set bits low, cleared bits high).
void LinkFailureSweep::Lists::append(const Expanded& x) {
  deadList.insert(deadList.end(), x.deadEdges.begin(), x.deadEdges.end());
  drainList.insert(drainList.end(), x.drainedNodes.begin(), x.drainedNodes.end());
  deadOff.push_back(uint32_t(deadList.size()));
  drainOff.push_back(uint32_t(drainList.size()));
  maxDead = std::max(maxDead, uint32_t(x.deadEdges.size()));
  for (size_t i = 0, j = 0; i < x.metricEdges.size() || j < x.revivedEdges.size();) {
    const bool rev = i == x.metricEdges.size() ||
        (j < x.revivedEdges.size() && x.revivedEdges[j] < x.metricEdges[i]);
    metricEdge.push_back(rev ? x.revivedEdges[j] : x.metricEdges[i]);
    metricVal.push_back(rev ? x.revivedVals[j] : x.metricVals[i]);
    metricUp.push_back(rev ? 1 : 0);
    ++(rev ? j : i);
  }
  std::map<uint32_t, uint8_t> nb;
  for (size_t i = 0; i < x.flagNodes.size(); ++i) nb[x.flagNodes[i]] |= x.flagBits[i];
  for (size_t i = 0; i < x.clearedNodes.size(); ++i) {
    nb[x.clearedNodes[i]] |= uint8_t(x.clearedBits[i] << OGS_NODE_CLEAR_SHIFT);
  }
  for (const auto& [u, b] : nb) {
    flagNode.push_back(u);
    flagBits.push_back(b);
    whatif = whatif || (b & ~uint8_t(OGS_NODE_OVERLOADED)) != 0;
  }
  restores = restores || !x.revivedEdges.empty() || !x.clearedNodes.empty();
  metricOff.push_back(uint32_t(metricEdge.size()));
  flagOff.push_back(uint32_t(flagNode.size()));
  maxMetricList = std::max(maxMetricList, uint32_t(x.metricEdges.size() + x.revivedEdges.size()));
  whatif = whatif || restores || !metricEdge.empty();
}

// Zero / negative link metrics (extraction-order replay) or path sums past
// 32 bits: the packed 32-bit {dist, nh} repair does not apply, every variant
// runs as a topology of its own (exactLaunch); so do next-hop sets of more
// than 4 words (source degree > 128: past the variants kernel, ogs_spf_routes
// takes up to 16). The overrides' own guards: a zero / negative weight replays
// the extraction order, a weight that pushes max_metric x (N - 1) past the
// 32-bit guard needs 64-bit distances -- either way topology copies.
LinkFailureSweep::AreaDomain LinkFailureSweep::areaDomain(
    const FlatTopology& f, const HostBatch& hb, int W, const std::vector<uint64_t>& metricVals) {
  AreaDomain d;
  d.exact = wideDistancesNeeded(f) || hb.hasZeroMetric || W > 4;
  d.exactOrder = f.hasZeroMetric || f.hasWideMetric;
  const uint64_t n = f.names.empty() ? 0 : f.names.size() - 1;
  for (const uint64_t w : metricVals) {
    if (w == 0 || w > 0xFFFFFFFFull) d.exact = d.exactOrder = true;
    if (n != 0 && w > 0x7FFFFFFEull / n) d.exact = true;
  }
  if (!d.exact) {
    ogs_graph shape{};  // the two fields the question reads
    shape.max_nodes = hb.maxNodes;
    shape.max_degree = hb.maxDegree;
    d.needsGlobal = ogs_whatif_needs_global(&shape, 0u, W) != 0;
  }
  return d;
}

LinkFailureSweep::Form LinkFailureSweep::selectForm() const {
  if (exact_) return kTopologyCopies;
  if (needsGlobal_ || forceGlobal_) return kGlobalState;
  if (lists_.maxDead <= kRegisterMax && lists_.drainList.empty() && !forceBitset_ &&
      !lists_.whatif) {
    return kRegisterList;
  }
  return kEdgeBitset;  // launch() falls back to copies when the entry refuses
}

// The lists as ogs_unit_mods slots: 4 a unit (two links, both directions) as
// every sweep before scenarios had them, up to 8 when a list is longer.
void LinkFailureSweep::uploadRegisterSlots() {
  deadPer_ = int(std::max<uint32_t>(4, lists_.maxDead));
  std::vector<uint32_t> slots(numVariants() * size_t(deadPer_), OGS_NODE_NONE);
  for (size_t v = 0; v < numVariants(); ++v) {
    std::copy(lists_.deadList.begin() + lists_.deadOff[v],
              lists_.deadList.begin() + lists_.deadOff[v + 1],
              slots.begin() + v * size_t(deadPer_));
  }
  dDead_.upload(slots.data(), slots.size());
}

void LinkFailureSweep::reselect() {
  form_ = selectForm();
  recordsRun_ = changedOnlyRun_ = false;
  compact_.offsets.clear();
  changed_.clear();
  counts_.clear();
  meta_.clear();
  xDb_.clear();
  xUpd_.clear();
  base_.reset();
  baseMeta_.clear();
  nodeOffsets_.clear();
  dist_.clear();
}

void LinkFailureSweep::setListForm(bool forceBitset) {
  forceBitset_ = forceBitset;
  reselect();
}

void LinkFailureSweep::setGlobalForm(bool forceGlobal) {
  forceGlobal_ = forceGlobal;
  reselect();
  if (form_ == kGlobalState && !exact_) dLists_.upload(lists_);
}

void LinkFailureSweep::setGlobalChunk(size_t n) {
  globalChunk_ = n;
  reselect();
}

void LinkFailureSweep::WhatifDeviceLists::uploadDead(const Lists& l) {
  if (dead_) return;
  dead_ = true;
  deadOff.upload(l.deadOff.data(), l.deadOff.size());
  deadList.upload(l.deadList.data(), l.deadList.size());
}

void LinkFailureSweep::WhatifDeviceLists::upload(const Lists& l) {
  uploadDead(l);
  if (all_) return;
  all_ = true;
  nodes_ = !l.flagNode.empty();
  metrics_ = !l.metricEdge.empty();
  maxMetricList_ = l.maxMetricList;
  if (nodes_) {
    flagOff.upload(l.flagOff.data(), l.flagOff.size());
    flagNode.upload(l.flagNode.data(), l.flagNode.size());
    flagBits.upload(l.flagBits.data(), l.flagBits.size());
  }
  if (metrics_) {
    std::vector<uint32_t> vals(l.metricVal.begin(), l.metricVal.end());
    for (size_t i = 0; i < vals.size(); ++i) {
      if (l.metricUp[i]) vals[i] |= OGS_WHATIF_EDGE_UP;
    }
    metricOff.upload(l.metricOff.data(), l.metricOff.size());
    metricEdge.upload(l.metricEdge.data(), l.metricEdge.size());
    metricVal.upload(vals.data(), vals.size());
  }
}

ogs_whatif_mods LinkFailureSweep::WhatifDeviceLists::mods(size_t firstScenario) const {
  return ogs_whatif_mods{deadOff.as<uint32_t>() + firstScenario,
                         deadList.as<uint32_t>(),
                         nodes_ ? flagOff.as<uint32_t>() + firstScenario : nullptr,
                         nodes_ ? flagNode.as<uint32_t>() : nullptr,
                         nodes_ ? flagBits.as<uint8_t>() : nullptr,
                         metrics_ ? metricOff.as<uint32_t>() + firstScenario : nullptr,
                         metrics_ ? metricEdge.as<uint32_t>() : nullptr,
                         metrics_ ? metricVal.as<uint32_t>() : nullptr,
                         maxMetricList_};
}

// Scenarios per ogs_spf_routes_whatif_global call: the most whose workspace
// (openr_gpu.h: the per-unit bytes, each of the call's six regions rounded up
// to 256) stays within 1 GiB. ownRows: the launch passes dist / next-hop
// rows of its own, so the workspace holds none.
size_t LinkFailureSweep::globalChunkUnits(bool ownRows) const {
  if (globalChunk_) return globalChunk_;
  const size_t Sn = size_t(std::max(hb_.maxNodes, 1));
  const size_t E = size_t(std::max(hb_.maxEdges, 0));
  const size_t rows = ownRows ? 0 : 4 * Sn + 4 * size_t(W_) * Sn;
  const size_t flagRow = lists_.flagNode.empty() ? 0 : ((Sn + 3) & ~size_t(3));
  const size_t perUnit = 12 * Sn + 8 * ((E + 31) / 32) + 4 + flagRow + rows;
  constexpr size_t kBudget = (size_t(1) << 30) - 6 * 255;  // the regions' padding
  return std::max<size_t>(1, kBudget / perUnit);
}

// ogs_spf_routes_whatif_global over chunks of scenarios: unit, record and
// diff rows advance per chunk; the lists' offsets are absolute, so each
// chunk's slice of an offset array serves as it is.
void LinkFailureSweep::globalLaunch(const ogs_graph& g, const ogs_prefix_table& pt,
                                    const ogs_route_diff& diff, uint32_t fl,
                                    const ogs_spf_out& out, void* stream) {
  dLists_.upload(lists_);
  const size_t U = numVariants(), Sn = size_t(std::max(hb_.maxNodes, 1));
  const size_t chunk = globalChunkUnits(out.dist && out.nh);
  for (size_t c0 = 0; c0 < U; c0 += chunk) {
    const size_t n = std::min(chunk, U - c0);
    const ogs_whatif_mods mods = dLists_.mods(c0);
    ogs_route_diff d = diff;
    d.changed += c0 * words_;
    d.counts += c0 * 2;
    d.base_desc = nullptr;
    ogs_spf_out o = out;
    auto adv = [&](auto*& p, size_t stride) {
      if (p) p += c0 * stride;
    };
    uint32_t* dist = static_cast<uint32_t*>(o.dist);
    uint32_t* metric = static_cast<uint32_t*>(o.metric);
    adv(dist, Sn);
    adv(metric, Sp_);
    o.dist = dist;
    o.metric = metric;
    adv(o.nh, size_t(W_) * Sn);
    adv(o.meta, Sp_);
    adv(o.sel, Sp_);
    adv(o.mask, size_t(W_) * Sp_);
    ogsCheck(ogs_spf_routes_whatif_global(&g, &pt, dUnits_.as<ogs_unit>() + c0, int32_t(n), &mods,
                                          &d, fl, W_, &o, stream),
             "ogs_spf_routes_whatif_global");
  }
}

LinkFailureSweep::LinkFailureSweep(
    const std::string& myNodeName, const LinkState& ls, const PrefixState& ps,
    const std::vector<Scenario>& scenarios, bool enableV4,
    bool enableBestRouteSelection, bool v4OverV6Nexthop, bool enableNodeSegmentLabel)
    : ls_(ls),
      ps_(ps),
      me_(myNodeName),
      area_(ls.getArea()),
      enableV4_(enableV4),
      brs_(enableBestRouteSelection),
      v4OverV6_(v4OverV6Nexthop),
      labels_(enableNodeSegmentLabel) {
  const FlatTopology& f = ls.flat();
  auto sIt = f.id.find(me_);
  if (sIt == f.id.end()) {
    throw std::invalid_argument("LinkFailureSweep: " + me_ + " is not in area " + area_);
  }
  table_.build(ps);
  hb_.append(f, ps, area_);
  const uint32_t s = sIt->second;
  W_ = std::max(1, ogs_nh_words_for_degree(int(f.rowPtr[s + 1] - f.rowPtr[s])));
  // every scenario's lists (Lists::append), then the area's domain
  for (const Scenario& sc : scenarios) lists_.append(expandScenario(ls, me_, sc));
  {
    const AreaDomain d = areaDomain(f, hb_, W_, lists_.metricVal);
    exact_ = d.exact;
    exactOrder_ = d.exactOrder;
    needsGlobal_ = d.needsGlobal;
  }
  form_ = selectForm();

  const size_t U = scenarios.size(), Sn = size_t(std::max(hb_.maxNodes, 1));
  Sp_ = size_t(std::max(hb_.maxPrefixes, 1));
  words_ = (Sp_ + 31) / 32;
  std::vector<ogs_unit> units(U, ogs_unit{0, s});
  const ogs_unit base{0, s};
  img_.uploadGraph(hb_);
  img_.uploadTable(hb_);
  dUnits_.upload(units.data(), units.size());
  dBaseUnit_.upload(&base, 1);
  if (form_ == kRegisterList) uploadRegisterSlots();
  dLists_.uploadDead(lists_);
  if (!lists_.drainList.empty()) {
    dDrainOff_.upload(lists_.drainOff.data(), lists_.drainOff.size());
    dDrainList_.upload(lists_.drainList.data(), lists_.drainList.size());
  }
  if ((lists_.whatif || form_ == kGlobalState) && !exact_) dLists_.upload(lists_);
  {
    const std::vector<uint32_t> cls = advClasses(table_);
    dAdvClass_.upload(cls.data(), cls.size());
  }
  bDist_.resize(Sn * 4);
  bNh_.resize(W_ * Sn * 4);
  for (auto* b : {&bMeta_, &bMetric_, &bSel_}) b->resize(Sp_ * 4);
  bMask_.resize(W_ * Sp_ * 4);
  const size_t Uc = std::max<size_t>(U, 1);
  dDist_.resize(Uc * Sn * 4);
  dNh_.resize(Uc * W_ * Sn * 4);
  for (auto* b : {&dMeta_, &dMetric_, &dSel_}) b->resize(Uc * Sp_ * 4);
  dMask_.resize(Uc * W_ * Sp_ * 4);
  dChanged_.resize(Uc * words_ * 4);
  dCounts_.resize(Uc * 2 * 4);
  if (labels_) {
    // the label owners: who is compared on the device, who competes per label
    nodeWords_ = (Sn + 31) / 32;
    nodeLabel_.assign(f.names.size(), 0);
    std::vector<uint32_t> interest(nodeWords_, 0u);
    for (const auto& [node, adjDb] : ls.getAdjacencyDatabases()) {  // node name ascending
      const auto it = f.id.find(node);
      if (it == f.id.end() || !validNodeLabel(adjDb.nodeLabel)) continue;
      nodeLabel_[it->second] = adjDb.nodeLabel;
      labelOwners_[adjDb.nodeLabel].push_back(it->second);
      interest[it->second >> 5] |= 1u << (it->second & 31u);
    }
    dInterest_.upload(interest.data(), interest.size());
    dNodeChanged_.resize(Uc * nodeWords_ * 4);
    dNodeCounts_.resize(Uc * 4);
  }
}

// Variants outside the repair kernel's domain: ogs_spf_routes launches over
// the base (topology 0) and every variant's own topology copy (the failed
// links' edges marked down, the same skip the variants kernel applies to its
// dead-edge list), kExactChunk topologies per launch so that device and host
// copies stay bounded, in the exact extraction order when the area has zero
// or negative metrics, with 64-bit distances. fetch materialises the records and
// the update is DecisionRouteDb::calculateUpdate (SpfSolver.cpp:21-56) of the
// base and variant RouteDbs, as Decision::rebuildRoutes computes it.
void LinkFailureSweep::exactLaunch(void* stream) {
  const size_t U = numVariants(), T = U + 1;
  const FlatTopology& f = ls_.flat();
  const uint32_t s = f.id.at(me_);
  const uint32_t fl = flags() | OGS_F_WIDE_METRIC | (exactOrder_ ? OGS_F_EXACT_ORDER : 0u);
  xMeta_.assign(T * Sp_, 0);
  xMetric_.assign(T * Sp_, 0);
  xMask_.assign(T * W_ * Sp_, 0);
  // label routes come from each copy's SPF rows: fetched with the records
  const size_t Sn = size_t(std::max(hb_.maxNodes, 1)), rw = (Sn + 31) / 32;
  if (labels_) {
    xDist_.assign(T * Sn, 0);
    xNh_.assign(T * W_ * Sn, 0);
    xReach_.assign(exactOrder_ ? T * rw : 0, 0);
  }
  HostBatchImage img;  // reused (grow-only) by every chunk
  DeviceBuffer units, meta, metric, mask, dist, nh, reach;
  for (size_t c0 = 0; c0 < T; c0 += kExactChunk) {
    const size_t c1 = std::min(T, c0 + kExactChunk), n = c1 - c0;
    HostBatch hb;  // topology t - c0 = the base (t = 0) or variant t - 1
    for (size_t t = c0; t < c1; ++t) {
      const uint32_t e0 = uint32_t(hb.edges.size()), n0 = uint32_t(hb.nodeFlags.size());
      hb.append(f, ps_, area_);
      if (t == 0) continue;
      for (uint32_t i = lists_.deadOff[t - 1]; i < lists_.deadOff[t]; ++i) {
        hb.edges[e0 + lists_.deadList[i]] |= OGS_EDGE_DOWN;
      }
      // OGS_EDGE_DST_OVERLOADED on (or off) every edge into node x: the
      // reverse of each edge of its row (links are two-way)
      auto markEdgesInto = [&](uint32_t x, bool overloaded) {
        for (uint32_t e = f.rowPtr[x]; e < f.rowPtr[x + 1]; ++e) {
          const uint32_t o = uint32_t(f.edges[e]) & OGS_EDGE_DST_MASK;
          for (uint32_t r = f.rowPtr[o]; r < f.rowPtr[o + 1]; ++r) {
            if (f.edgeLink[r] != f.edgeLink[e]) continue;
            uint64_t& w = hb.edges[e0 + r];
            w = overloaded ? w | OGS_EDGE_DST_OVERLOADED : w & ~uint64_t(OGS_EDGE_DST_OVERLOADED);
          }
        }
      };
      // a drain, as LinkState::patchFlat encodes it: the node's flag and
      // OGS_EDGE_DST_OVERLOADED on every edge into it
      for (uint32_t i = lists_.drainOff[t - 1]; i < lists_.drainOff[t]; ++i) {
        const uint32_t x = lists_.drainList[i];
        hb.nodeFlags[n0 + x] |= OGS_NODE_OVERLOADED;
        markEdgesInto(x, true);
      }
      // metric overrides, as LinkState::patchFlat re-encodes a moved metric,
      // and the soft-drain bits (link_state.cpp: the node's flags alone)
      for (uint32_t i = lists_.metricOff[t - 1]; i < lists_.metricOff[t]; ++i) {
        uint64_t& w = hb.edges[e0 + lists_.metricEdge[i]];
        w = (w & 0xFFFFFFFFull) | (uint64_t(uint32_t(lists_.metricVal[i])) << 32);
        // a revived link: up again with that weight (a dead edge stays dead)
        const bool dead = std::binary_search(lists_.deadList.begin() + lists_.deadOff[t - 1],
                                             lists_.deadList.begin() + lists_.deadOff[t],
                                             lists_.metricEdge[i]);
        if (lists_.metricUp[i] && !dead) w &= ~uint64_t(OGS_EDGE_DOWN);
        hb.maxMetric = std::max(hb.maxMetric, lists_.metricVal[i]);
        hb.hasZeroMetric |= lists_.metricVal[i] == 0;
      }
      // flag bits: cleared first, then set -- an undrain is the mirror image
      // of the drain above (the flag, and OGS_EDGE_DST_OVERLOADED off every
      // edge into the node)
      for (uint32_t i = lists_.flagOff[t - 1]; i < lists_.flagOff[t]; ++i) {
        const uint32_t x = lists_.flagNode[i];
        const uint8_t clr = uint8_t((lists_.flagBits[i] >> OGS_NODE_CLEAR_SHIFT) & 0x7u);
        uint8_t& nf = hb.nodeFlags[n0 + x];
        const bool was = (nf & OGS_NODE_OVERLOADED) != 0;
        nf = uint8_t((nf & ~clr) | (lists_.flagBits[i] & 0x0Fu));
        if (was && !(nf & OGS_NODE_OVERLOADED)) markEdgesInto(x, false);
      }
    }
    std::vector<ogs_unit> us(n);
    for (size_t i = 0; i < n; ++i) us[i] = ogs_unit{uint32_t(i), s};
    img.uploadGraph(hb, stream);
    img.uploadTable(hb, stream);
    units.upload(us.data(), us.size(), stream);
    meta.resize(n * Sp_ * 4);
    metric.resize(n * Sp_ * 8);
    mask.resize(n * W_ * Sp_ * 4);
    const ogs_graph g = img.graph(hb, int(n));
    const ogs_prefix_table pt = img.table(hb);
    ogs_spf_out out{nullptr, nullptr, meta.as<uint32_t>(), metric.get(), mask.as<uint32_t>(),
                    nullptr};
    if (labels_) {
      dist.resize(n * Sn * 8);
      nh.resize(n * W_ * Sn * 4);
      out.dist = dist.get();
      out.nh = nh.as<uint32_t>();
      if (exactOrder_) {
        reach.resize(n * rw * 4);
        out.reached = reach.as<uint32_t>();
      }
    }
    ogsCheck(ogs_spf_routes(&g, &pt, units.as<ogs_unit>(), int32_t(n), fl, W_, &out, stream),
             "ogs_spf_routes(variant topologies)");
    if (labels_) {
      dist.download(xDist_.data() + c0 * Sn, n * Sn, stream);
      nh.download(xNh_.data() + c0 * W_ * Sn, n * W_ * Sn, stream);
      if (exactOrder_) reach.download(xReach_.data() + c0 * rw, n * rw, stream);
    }
    meta.download(xMeta_.data() + c0 * Sp_, n * Sp_, stream);
    metric.download(xMetric_.data() + c0 * Sp_, n * Sp_, stream);
    // mask rows [(i * W + w) * Sp + p] of the chunk follow the previous ones
    mask.download(xMask_.data() + c0 * W_ * Sp_, n * W_ * Sp_, stream);
    ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");  // buffers reused
  }
  baseRun_ = recordsRun_ = true;
  changedOnlyRun_ = false;
}

void LinkFailureSweep::exactFetch(void* /*stream*/) {
  if (!recordsRun_) throw std::logic_error("LinkFailureSweep: launch() first");
  const size_t U = numVariants();
  const FlatTopology& f = ls_.flat();
  auto dbOf = [&](size_t t) {
    DecisionRouteDb db;
    addUnicastRoutes(db, f, me_, table_, &xMeta_[t * Sp_], &xMetric_[t * Sp_],
                     &xMask_[t * W_ * Sp_], Sp_, W_, v4OverV6_);
    if (labels_) {  // the copy's own rows through the solver's label pass
      const size_t Sn = size_t(std::max(hb_.maxNodes, 1)), rw = (Sn + 31) / 32;
      LabelRoutes labelToNode;
      addNodeLabelRoutes(ls_, f, area_, me_, &xDist_[t * Sn], &xNh_[t * W_ * Sn], Sn, W_,
                         labelToNode, exactOrder_ ? &xReach_[t * rw] : nullptr);
      for (auto& [label, ne] : labelToNode) db.mplsRoutes.emplace(label, std::move(ne.second));
    }
    return db;
  };
  base_ = dbOf(0);
  xDb_.clear();
  xUpd_.clear();
  counts_.assign(2 * U, 0);
  for (size_t v = 0; v < U; ++v) {
    xDb_.push_back(dbOf(v + 1));
    xUpd_.push_back(base_->calculateUpdate(xDb_.back()));
    counts_[2 * v] = uint32_t(xUpd_.back().unicastRoutesToUpdate.size());
    counts_[2 * v + 1] = uint32_t(xUpd_.back().unicastRoutesToDelete.size());
  }
  scanChangeCounts<2>(counts_.data(), U, compact_.offsets);
}

void LinkFailureSweep::runBase(void* stream) {
  if (copies()) return exactLaunch(stream);
  const ogs_graph g = img_.graph(hb_, 1);
  const ogs_prefix_table pt = img_.table(hb_);
  ogs_spf_out out{bDist_.get(), bNh_.as<uint32_t>(), bMeta_.as<uint32_t>(),
                  bMetric_.get(), bMask_.as<uint32_t>(), bSel_.as<uint32_t>()};
  ogsCheck(ogs_spf_routes(&g, &pt, dBaseUnit_.as<ogs_unit>(), 1, flags(), W_, &out, stream),
           "ogs_spf_routes(base)");
  baseRun_ = true;
  descValid_ = false;  // a new base SPF: its descendant rows are rebuilt
  base_.reset();
}

void LinkFailureSweep::launch(void* stream, bool records) {
  if (copies()) return exactLaunch(stream);  // records are always written
  if (!baseRun_) runBase(stream);
  compact_.offsets.clear();  // results of an earlier launch are stale now
  changed_.clear();
  meta_.clear();
  counts_.clear();
  nodeOffsets_.clear();
  dist_.clear();
  const ogs_graph g = img_.graph(hb_, 1);
  const ogs_prefix_table pt = img_.table(hb_);
  const bool changedOnly = mode_ == kChangedOnly && W_ == 1;
  ogs_spf_out out{};
  if (records) {
    out = ogs_spf_out{dDist_.get(), dNh_.as<uint32_t>(), dMeta_.as<uint32_t>(),
                      dMetric_.get(), dMask_.as<uint32_t>(), dSel_.as<uint32_t>()};
    if (changedOnly) out.dist = out.nh = nullptr;  // records of changed routes only
  }
  if (labels_) {  // the label routes are read off every scenario's SPF rows
    out.dist = dDist_.get();
    out.nh = dNh_.as<uint32_t>();
  }
  // the base's tight-DAG descendant rows: built by the first repair launch
  // after runBase, reused by the next ones (same topology, source, base SPF)
  const size_t Sn = size_t(std::max(hb_.maxNodes, 1));
  if (Sn <= kDescMaxNodes) bDesc_.resize(Sn * ((Sn + 31) / 32) * 4);
  ogs_route_diff diff{bMeta_.as<uint32_t>(), bMetric_.as<uint32_t>(), bMask_.as<uint32_t>(),
                      dChanged_.as<uint32_t>(), dCounts_.as<uint32_t>(),
                      bDist_.as<uint32_t>(), bNh_.as<uint32_t>(), dAdvClass_.as<uint32_t>(),
                      Sn <= kDescMaxNodes ? bDesc_.as<uint32_t>() : nullptr,
                      descValid_ ? 1 : 0};
  uint32_t fl = flags();
  if (mode_ != kFull) fl |= OGS_F_INCREMENTAL;
  if (changedOnly) fl |= OGS_F_CHANGED_ONLY;
  // (lists_.restores implies lists_.whatif: only the two what-if entries below see the flag)
  if (lists_.restores) fl |= OGS_F_RESTORE;
  if (form_ == kGlobalState) {
    globalLaunch(g, pt, diff, fl, out, stream);
  } else if (form_ == kRegisterList) {
    // the lists as ogs_unit_mods slots: 4 a unit (two links, both directions)
    // as every sweep before scenarios had them, up to 8 when a list is longer
    if (!deadPer_) uploadRegisterSlots();
    ogs_unit_mods mods{dDead_.as<uint32_t>(), deadPer_};
    ogsCheck(ogs_spf_routes_variants(&g, &pt, dUnits_.as<ogs_unit>(), int32_t(numVariants()),
                                     &mods, &diff, fl, W_, &out, stream),
             "ogs_spf_routes_variants");
  } else if (lists_.whatif) {
    const ogs_whatif_mods mods = dLists_.mods();
    const int rc = ogs_spf_routes_whatif(&g, &pt, dUnits_.as<ogs_unit>(),
                                         int32_t(numVariants()), &mods, &diff, fl, W_, &out,
                                         stream);
    if (rc == OGS_E_UNSUPPORTED) {
      // node bits the repair cannot take (kFull mode, W > 1, its LDS budget):
      // one topology per scenario (nothing was launched)
      form_ = kTopologyCopies;
      return exactLaunch(stream);
    }
    ogsCheck(rc, "ogs_spf_routes_whatif");
  } else {
    const bool drains = !lists_.drainList.empty();
    ogs_scenario_mods mods{dLists_.deadOff.as<uint32_t>(), dLists_.deadList.as<uint32_t>(),
                           drains ? dDrainOff_.as<uint32_t>() : nullptr,
                           drains ? dDrainList_.as<uint32_t>() : nullptr};
    const int rc = ogs_spf_routes_scenarios(&g, &pt, dUnits_.as<ogs_unit>(),
                                            int32_t(numVariants()), &mods, &diff, fl, W_, &out,
                                            stream);
    if (rc == OGS_E_UNSUPPORTED) {
      // drains the repair cannot take (kFull mode, W > 1, its LDS budget):
      // one topology per scenario (nothing was launched)
      form_ = kTopologyCopies;
      return exactLaunch(stream);
    }
    ogsCheck(rc, "ogs_spf_routes_scenarios");
  }
  descValid_ = diff.base_desc_valid != 0;  // set by the library when it wrote the rows
  if (labels_) runNodeDiff(g, stream);
  recordsRun_ = records;
  changedOnlyRun_ = records && changedOnly;
}

// The label owners whose SPF row left the base's, over every scenario's rows
// (whichever form wrote them; a refused unit wrote none and reports none).
void LinkFailureSweep::runNodeDiff(const ogs_graph& g, void* stream) {
  nodeOffsets_.clear();
  const ogs_spf_out rows{dDist_.get(), dNh_.as<uint32_t>()};
  const ogs_node_diff nd{bDist_.as<uint32_t>(),        bNh_.as<uint32_t>(),
                         dInterest_.as<uint32_t>(),    dCounts_.as<uint32_t>(),
                         dNodeChanged_.as<uint32_t>(), dNodeCounts_.as<uint32_t>()};
  ogsCheck(ogs_spf_node_diff(&g, dUnits_.as<ogs_unit>(), int32_t(numVariants()), &rows, &nd, 0u,
                             W_, stream),
           "ogs_spf_node_diff");
}

void CompactChanges::reset(size_t units, int W) {
  W_ = W;
  done_ = 0;
  offsets.assign(units + 1, 0);
  for (auto* h : {&prefix, &meta, &metric, &mask}) h->clear();
}

void CompactChanges::gather(size_t u0, size_t n, const uint32_t* counts, const uint32_t* dChanged,
                            const ogs_spf_out& rec, size_t Sp, void* stream) {
  if (u0 != done_ || u0 + n + 1 > offsets.size() || (W_ > 1 && done_ != 0)) {
    throw std::logic_error("CompactChanges: chunks append in unit order, and only at W = 1");
  }
  done_ += n;
  const size_t held = prefix.size();
  const size_t t = scanChangeCounts<2>(counts, n, local_, held);
  for (size_t i = 1; i <= n; ++i) offsets[u0 + i] = uint32_t(held + local_[i]);
  if (t == 0) return;
  dOffsets.upload(local_.data(), local_.size(), stream);
  for (auto* b : {&cPrefix, &cMeta, &cMetric}) b->resize(t * 4);
  cMask.resize(t * W_ * 4);
  const ogs_route_changes ch{dOffsets.as<uint32_t>(), t, cPrefix.as<uint32_t>(),
                             cMeta.as<uint32_t>(), cMetric.as<uint32_t>(), cMask.as<uint32_t>()};
  ogsCheck(ogs_route_changes_gather(dChanged, int32_t(n), int32_t(Sp), &rec, W_, &ch, stream),
           "ogs_route_changes_gather");
  for (auto* h : {&prefix, &meta, &metric}) h->resize(held + t);
  mask.resize((held + t) * W_);
  cPrefix.download(&prefix[held], t, stream);
  cMeta.download(&meta[held], t, stream);
  cMetric.download(&metric[held], t, stream);
  cMask.download(&mask[held * W_], t * W_, stream);
}

ChangeRecords CompactChanges::view() const {
  ChangeRecords c;
  c.offsets = offsets.data();
  c.variants = offsets.empty() ? 0 : offsets.size() - 1;
  c.prefix = prefix.data();
  c.meta = meta.data();
  c.metric = metric.data();
  c.mask = mask.data();
  c.total = prefix.size();
  c.W = W_;
  return c;
}

void LinkFailureSweep::fetchUpdates(void* stream) {
  if (copies()) return exactFetch(stream);
  if (!recordsRun_) {
    throw std::logic_error("LinkFailureSweep::fetchUpdates: launch(records=true) first");
  }
  const size_t U = numVariants();
  counts_.resize(U * 2);
  if (U) dCounts_.download(counts_.data(), U * 2, stream);
  if (labels_) {
    nodeCounts_.resize(U);
    if (U) dNodeCounts_.download(nodeCounts_.data(), U, stream);
  }
  ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
  // one chunk of all the units; the sync below ends it
  compact_.reset(U, W_);
  const ogs_spf_out rec{nullptr, nullptr, dMeta_.as<uint32_t>(), dMetric_.get(),
                        dMask_.as<uint32_t>(), nullptr};
  compact_.gather(0, U, counts_.data(), dChanged_.as<uint32_t>(), rec, Sp_, stream);
  if (labels_) {  // the same for the changed SPF rows
    const size_t Sn = size_t(std::max(hb_.maxNodes, 1));
    const uint64_t nodes = scanChangeCounts<1>(nodeCounts_.data(), U, nodeOffsets_);
    const size_t Tn = std::max<size_t>(nodes, 1);
    dNodeOffsets_.upload(nodeOffsets_.data(), nodeOffsets_.size(), stream);
    cNode_.resize(Tn * 4);
    cNodeDist_.resize(Tn * 4);
    cNodeNh_.resize(Tn * W_ * 4);
    const ogs_spf_out rows{dDist_.get(), dNh_.as<uint32_t>()};
    const ogs_node_changes nc{dNodeOffsets_.as<uint32_t>(), size_t(nodes), cNode_.as<uint32_t>(),
                              cNodeDist_.as<uint32_t>(), cNodeNh_.as<uint32_t>()};
    ogsCheck(ogs_spf_node_changes_gather(dNodeChanged_.as<uint32_t>(), int32_t(U), int32_t(Sn),
                                         &rows, W_, &nc, stream),
             "ogs_spf_node_changes_gather");
    cNodeH_.resize(nodes);
    cNodeDistH_.resize(nodes);
    cNodeNhH_.resize(nodes * W_);
    if (nodes) {
      cNode_.download(cNodeH_.data(), nodes, stream);
      cNodeDist_.download(cNodeDistH_.data(), nodes, stream);
      cNodeNh_.download(cNodeNhH_.data(), nodes * W_, stream);
    }
    baseDist_.resize(Sn);
    baseNh_.resize(W_ * Sn);
    bDist_.download(baseDist_.data(), Sn, stream);
    bNh_.download(baseNh_.data(), W_ * Sn, stream);
    dist_.clear();
  }
  baseMeta_.resize(Sp_);
  baseMetric_.resize(Sp_);
  baseMask_.resize(W_ * Sp_);
  bMeta_.download(baseMeta_.data(), Sp_, stream);
  bMetric_.download(baseMetric_.data(), Sp_, stream);
  bMask_.download(baseMask_.data(), W_ * Sp_, stream);
  ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
  base_.reset();
}

void LinkFailureSweep::fetchRecords(void* stream) {
  if (copies()) return exactFetch(stream);
  // the diff (bitmap + counts) always; the records when the launch wrote them
  const size_t U = numVariants();
  const size_t R = (recordsRun_ && !changedOnlyRun_) ? U : 0;
  counts_.resize(U * 2);
  changed_.resize(U * words_);
  meta_.resize(R * Sp_);
  metric_.resize(R * Sp_);
  mask_.resize(R * W_ * Sp_);
  if (U) {
    dCounts_.download(counts_.data(), U * 2, stream);
    dChanged_.download(changed_.data(), U * words_, stream);
  }
  if (R) {
    dMeta_.download(meta_.data(), U * Sp_, stream);
    dMetric_.download(metric_.data(), U * Sp_, stream);
    dMask_.download(mask_.data(), U * W_ * Sp_, stream);
  }
  if (labels_) {  // every scenario's SPF rows: the launch always writes them
    const size_t Sn = size_t(std::max(hb_.maxNodes, 1));
    dist_.resize(U * Sn);
    nh_.resize(U * W_ * Sn);
    if (U) {
      dDist_.download(dist_.data(), U * Sn, stream);
      dNh_.download(nh_.data(), U * W_ * Sn, stream);
    }
    baseDist_.resize(Sn);
    baseNh_.resize(W_ * Sn);
    bDist_.download(baseDist_.data(), Sn, stream);
    bNh_.download(baseNh_.data(), W_ * Sn, stream);
  }
  baseMeta_.resize(Sp_);
  baseMetric_.resize(Sp_);
  baseMask_.resize(W_ * Sp_);
  bMeta_.download(baseMeta_.data(), Sp_, stream);
  bMetric_.download(baseMetric_.data(), Sp_, stream);
  bMask_.download(baseMask_.data(), W_ * Sp_, stream);
  ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
  base_.reset();
}

const DecisionRouteDb& LinkFailureSweep::baseRouteDb() const {
  if (copies()) {
    if (!base_) throw std::logic_error("LinkFailureSweep: nothing fetched yet");
    return *base_;
  }
  if (baseMeta_.empty()) throw std::logic_error("LinkFailureSweep: nothing fetched yet");
  if (!base_) {
    DecisionRouteDb db;
    addUnicastRoutes(db, ls_.flat(), me_, table_, baseMeta_.data(), baseMetric_.data(),
                     baseMask_.data(), Sp_, W_, v4OverV6_);
    if (labels_) addBaseLabelRoutes(db);
    base_ = std::move(db);
  }
  return *base_;
}

namespace {

// 32-bit SPF rows as addNodeLabelRoutes reads them (all-ones = unreachable)
std::vector<uint64_t> widenDist(const uint32_t* d, size_t n) {
  std::vector<uint64_t> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = d[i] == 0xFFFFFFFFu ? ~0ull : d[i];
  return out;
}

void addLabelRoutes(const LinkState& ls, const std::string& area, const std::string& me,
                    const uint32_t* dist, const uint32_t* nh, size_t Sn, int W,
                    DecisionRouteDb& db) {
  const std::vector<uint64_t> wide = widenDist(dist, Sn);
  LabelRoutes labelToNode;
  addNodeLabelRoutes(ls, ls.flat(), area, me, wide.data(), nh, Sn, W, labelToNode);
  for (auto& [label, ne] : labelToNode) db.mplsRoutes.emplace(label, std::move(ne.second));
}

}  // namespace

void LinkFailureSweep::addBaseLabelRoutes(DecisionRouteDb& db) const {
  addLabelRoutes(ls_, area_, me_, baseDist_.data(), baseNh_.data(), baseDist_.size(), W_, db);
}

// SpfSolver.cpp:352-445 + 41-54 for the labels variant v can have moved: those
// owned by its changed nodes. Each is resolved again over ALL its owners (the
// smallest node name with a route wins, SpfSolver.cpp:370-375), an owner's row
// taken from its changed record when it has one, else from the base, and
// compared with the base's entry.
void LinkFailureSweep::addMplsUpdate(size_t v, DecisionRouteUpdate& u) const {
  const uint32_t r0 = nodeOffsets_[v], r1 = nodeOffsets_[v + 1];
  if (r0 == r1) return;
  const FlatTopology& f = ls_.flat();
  const uint32_t rb = f.rowPtr[f.id.at(me_)];
  const size_t Sn = baseDist_.size(), total = cNodeH_.size();
  const auto& baseMpls = baseRouteDb().mplsRoutes;
  const uint32_t* first = cNodeH_.data() + r0;  // node ids ascending
  const uint32_t* last = cNodeH_.data() + r1;
  std::set<int32_t> touched;
  for (const uint32_t* n = first; n != last; ++n) touched.insert(nodeLabel_[*n]);
  for (const int32_t label : touched) {
    std::optional<RibMplsEntry> now;
    for (const uint32_t o : labelOwners_.at(label)) {
      const uint32_t* rec = std::lower_bound(first, last, o);
      if (rec != last && *rec == o) {
        const size_t i = size_t(rec - cNodeH_.data());
        now = nodeLabelEntry(f, area_, me_, rb, f.names[o], label,
                             cNodeDistH_[i] != 0xFFFFFFFFu, cNodeDistH_[i], &cNodeNhH_[i], total,
                             W_);
      } else {
        now = nodeLabelEntry(f, area_, me_, rb, f.names[o], label, baseDist_[o] != 0xFFFFFFFFu,
                             baseDist_[o], &baseNh_[o], Sn, W_);
      }
      if (now) break;
    }
    const auto was = baseMpls.find(label);
    if (now) {
      if (was == baseMpls.end() || was->second != *now) {
        u.mplsRoutesToUpdate.emplace(label, std::move(*now));
      }
    } else if (was != baseMpls.end()) {
      u.mplsRoutesToDelete.push_back(label);
    }
  }
}

DecisionRouteUpdate LinkFailureSweep::mplsUpdate(size_t v) const {
  if (v >= numVariants()) throw std::out_of_range("LinkFailureSweep: variant");
  DecisionRouteUpdate u;
  if (!labels_) return u;
  if (copies()) {
    if (v >= xUpd_.size()) throw std::logic_error("LinkFailureSweep: nothing fetched yet");
    u.mplsRoutesToUpdate = xUpd_[v].mplsRoutesToUpdate;
    u.mplsRoutesToDelete = xUpd_[v].mplsRoutesToDelete;
  } else if (nodeOffsets_.size() == numVariants() + 1) {
    addMplsUpdate(v, u);
  } else if (dist_.size() == numVariants() * baseDist_.size() && !dist_.empty()) {
    // fetchRecords: the variant's whole label table against the base's
    DecisionRouteDb db;
    if (counts_[2 * v] == OGS_WHATIF_REFUSED) return u;  // wrote no rows
    const size_t Sn = baseDist_.size();
    addLabelRoutes(ls_, area_, me_, &dist_[v * Sn], &nh_[v * W_ * Sn], Sn, W_, db);
    DecisionRouteDb baseLabels;
    baseLabels.mplsRoutes = baseRouteDb().mplsRoutes;
    u = baseLabels.calculateUpdate(db);
  } else {
    throw std::logic_error("LinkFailureSweep: nothing fetched yet");
  }
  return u;
}

std::pair<uint32_t, uint32_t> LinkFailureSweep::mplsCounts(size_t v) const {
  const DecisionRouteUpdate u = mplsUpdate(v);
  return {uint32_t(u.mplsRoutesToUpdate.size()), uint32_t(u.mplsRoutesToDelete.size())};
}

std::vector<int32_t> LinkFailureSweep::changedLabels(size_t v) const {
  const DecisionRouteUpdate u = mplsUpdate(v);
  std::vector<int32_t> out = u.mplsRoutesToDelete;
  for (const auto& [label, _] : u.mplsRoutesToUpdate) out.push_back(label);
  std::sort(out.begin(), out.end());
  return out;
}

namespace {

// SpfSolver.cpp:21-56 for one variant, prefixes in table order
DecisionRouteUpdate updateOf(const FlatTopology& f, uint32_t rb, const std::string& me,
                             const PrefixHostTable& pt, const ChangeRecords& c, size_t v,
                             bool v4OverV6) {
  DecisionRouteUpdate u;
  for (uint32_t i = c.offsets[v]; i < c.offsets[v + 1]; ++i) {
    const uint32_t p = c.prefix[i];
    auto e = materializeRouteAt(f, rb, me, pt, p, c.meta[i], c.metric[i], &c.mask[i], c.total,
                                c.W, v4OverV6, nullptr, OGS_POLICY_NONE, OGS_POLICY_NONE);
    if (e) {
      u.unicastRoutesToUpdate.emplace_hint(u.unicastRoutesToUpdate.end(), e->prefix,
                                           std::move(*e));
    } else {
      u.unicastRoutesToDelete.push_back(pt.prefixes.at(p));
    }
  }
  return u;
}

}  // namespace

DecisionRouteUpdate materializeUpdate(const FlatTopology& f, const std::string& me,
                                      const PrefixHostTable& pt, const ChangeRecords& c,
                                      size_t v, bool v4OverV6) {
  return updateOf(f, f.rowPtr[f.id.at(me)], me, pt, c, v, v4OverV6);
}

std::vector<DecisionRouteUpdate> materializeUpdates(const FlatTopology& f, const std::string& me,
                                                    const PrefixHostTable& pt,
                                                    const ChangeRecords& c, bool v4OverV6,
                                                    int threads) {
  const size_t V = c.variants;
  const uint32_t rb = f.rowPtr[f.id.at(me)];
  std::vector<DecisionRouteUpdate> out(V);
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  constexpr size_t kBlockV = 16;  // variants per work item
  const size_t T = std::min<size_t>(threads > 0 ? size_t(threads) : std::min(16u, hw),
                                    (V + kBlockV - 1) / kBlockV);
  std::atomic<size_t> next{0};
  std::exception_ptr err;
  std::mutex errMu;
  auto work = [&] {
    try {
      for (size_t b; (b = next.fetch_add(kBlockV)) < V;) {
        for (size_t v = b; v < std::min(V, b + kBlockV); ++v) {
          out[v] = updateOf(f, rb, me, pt, c, v, v4OverV6);
        }
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(errMu);
      if (!err) err = std::current_exception();
    }
  };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < T; ++t) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  if (err) std::rethrow_exception(err);
  return out;
}

DecisionRouteUpdate LinkFailureSweep::routeUpdate(size_t v) const {
  if (v >= numVariants() || compact_.offsets.size() != numVariants() + 1) {
    throw std::out_of_range("LinkFailureSweep::routeUpdate: variant / fetchUpdates");
  }
  if (copies()) return xUpd_.at(v);
  if (counts_[2 * v] == OGS_WHATIF_REFUSED) {
    throw std::logic_error("LinkFailureSweep: the device refused the scenario");
  }
  const FlatTopology& f = ls_.flat();
  DecisionRouteUpdate u =
      updateOf(f, f.rowPtr[f.id.at(me_)], me_, table_, changeRecords(), v, v4OverV6_);
  if (labels_) addMplsUpdate(v, u);
  return u;
}

std::vector<DecisionRouteUpdate> LinkFailureSweep::routeUpdates(int threads) const {
  const size_t V = numVariants();
  if (compact_.offsets.size() != V + 1) {
    throw std::out_of_range("LinkFailureSweep::routeUpdates: fetchUpdates first");
  }
  if (copies()) return xUpd_;
  std::vector<DecisionRouteUpdate> out =
      materializeUpdates(ls_.flat(), me_, table_, changeRecords(), v4OverV6_, threads);
  // label routes: a few records a variant, on the caller's thread
  for (size_t v = 0; labels_ && v < V; ++v) addMplsUpdate(v, out[v]);
  return out;
}

DecisionRouteDb LinkFailureSweep::routeDb(size_t v) const {
  if (copies()) {
    if (v >= xDb_.size()) throw std::out_of_range("LinkFailureSweep::routeDb: variant / fetch");
    return xDb_[v];
  }
  if (v >= numVariants() || meta_.size() != numVariants() * Sp_) {
    throw std::out_of_range("LinkFailureSweep::routeDb: variant / fetchRecords");
  }
  DecisionRouteDb db;
  addUnicastRoutes(db, ls_.flat(), me_, table_, &meta_[v * Sp_], &metric_[v * Sp_],
                   &mask_[v * W_ * Sp_], Sp_, W_, v4OverV6_);
  if (labels_) {
    const size_t Sn = baseDist_.size();
    if (counts_[2 * v] == OGS_WHATIF_REFUSED) {  // wrote no rows: no MPLS change
      db.mplsRoutes = baseRouteDb().mplsRoutes;
    } else {
      addLabelRoutes(ls_, area_, me_, &dist_[v * Sn], &nh_[v * W_ * Sn], Sn, W_, db);
    }
  }
  return db;
}

std::vector<std::string> LinkFailureSweep::changedPrefixes(size_t v) const {
  if (v >= numVariants()) throw std::out_of_range("LinkFailureSweep: variant");
  std::vector<std::string> out;
  if (copies()) {
    if (v >= xUpd_.size()) throw std::logic_error("LinkFailureSweep: nothing fetched yet");
    for (const auto& [p, _] : xUpd_[v].unicastRoutesToUpdate) out.push_back(p);
    out.insert(out.end(), xUpd_[v].unicastRoutesToDelete.begin(),
               xUpd_[v].unicastRoutesToDelete.end());
  } else if (compact_.offsets.size() == numVariants() + 1) {
    for (uint32_t i = compact_.offsets[v]; i < compact_.offsets[v + 1]; ++i) {
      out.push_back(table_.prefixes.at(compact_.prefix[i]));
    }
  } else if (changed_.size() == numVariants() * words_) {
    for (size_t p = 0; p < table_.prefixes.size(); ++p) {
      if (changed_[v * words_ + p / 32] >> (p % 32) & 1u) out.push_back(table_.prefixes[p]);
    }
  } else {
    throw std::logic_error("LinkFailureSweep: nothing fetched yet");
  }
  std::sort(out.begin(), out.end());
  return out;
}

std::pair<uint32_t, uint32_t> LinkFailureSweep::counts(size_t v) const {
  if (v >= numVariants() || counts_.size() != 2 * numVariants()) {
    throw std::out_of_range("LinkFailureSweep::counts: variant / fetch");
  }
  return {counts_[2 * v], counts_[2 * v + 1]};
}

}  // namespace openr_amd
