// network_whatif.cpp — NetworkWhatifSweep: every source's what-if route
// updates in one batch.
//
// Reference: every Open/R node runs its own Decision, so "which nodes' FIBs
// change under this scenario" is one buildRouteDb(node) (Decision.cpp:341-360)
// and one DecisionRouteDb::calculateUpdate (SpfSolver.cpp:21-56) per node per
// scenario. Here a (source, scenario) pair is one unit of
// ogs_spf_routes_whatif_pairs: the sources' base records come out of ONE
// ogs_spf_routes launch, the scenario lists (which do not depend on the
// source) are expanded and uploaded once, and the units are launched in chunks
// whose dense outputs are reused, the changed records gathered per chunk
// (ogs_route_changes_gather). Sources the batch cannot take run through their
// own LinkFailureSweep behind the same accessors.
#include <algorithm>
#include <stdexcept>

#include "decision.h"

namespace openr_amd {

namespace {

// a name no node of the topology carries: the scenario lists are expanded
// once, for no source in particular ("the source is in nodesDown" is a pair's
// state here, not an error)
std::string noNode(const FlatTopology& f) {
  std::string n = "\x01";
  while (f.id.count(n)) n += "\x01";
  return n;
}

bool sourceIsDown(const LinkFailureSweep::Scenario& sc, const std::string& node) {
  return std::find(sc.nodesDown.begin(), sc.nodesDown.end(), node) != sc.nodesDown.end();
}

std::vector<size_t> chunkBounds(size_t units, size_t unitBytes, size_t chunkBytes) {
  std::vector<size_t> b{0};
  const size_t per = std::max<size_t>(1, chunkBytes / std::max<size_t>(unitBytes, 1));
  for (size_t c0 = 0; c0 < units; c0 += per) b.push_back(std::min(units, c0 + per));
  return b;
}

// the plan and, for the sweep, what it was made from
NetworkWhatifPlan makePlan(const LinkState& ls, const PrefixState& ps,
                           const std::vector<std::string>& sources,
                           const std::vector<LinkFailureSweep::Scenario>& scenarios,
                           size_t chunkBytes, LinkFailureSweep::Lists* listsOut,
                           HostBatch* hbOut) {
  const FlatTopology& f = ls.flat();
  for (const std::string& s : sources) {
    if (!f.id.count(s)) {
      throw std::invalid_argument("NetworkWhatifSweep: " + s + " is not in area " + ls.getArea());
    }
  }
  LinkFailureSweep::Lists lists;
  const std::string nobody = noNode(f);
  for (const auto& sc : scenarios) {
    lists.append(LinkFailureSweep::expandScenario(ls, nobody, sc));
  }
  HostBatch hb;
  hb.append(f, ps, ls.getArea());
  // the area's part of LinkFailureSweep's form choice, at one next-hop word
  const LinkFailureSweep::AreaDomain d = LinkFailureSweep::areaDomain(f, hb, 1, lists.metricVal);
  const bool areaOk = !d.exact && !d.needsGlobal;

  NetworkWhatifPlan plan;
  for (uint32_t s = 0; s < sources.size(); ++s) {
    const uint32_t v = f.id.at(sources[s]);
    const int W = ogs_nh_words_for_degree(int(f.rowPtr[v + 1] - f.rowPtr[v]));
    const bool batched = areaOk && W <= 1;
    (batched ? plan.batched : plan.fallback).push_back(s);
    for (uint32_t k = 0; k < scenarios.size(); ++k) {
      if (sourceIsDown(scenarios[k], sources[s])) {
        plan.sourceDown.emplace_back(s, k);
      } else if (batched) {
        plan.pairs.emplace_back(s, k);
      }
    }
  }
  const size_t Sp = size_t(std::max(hb.maxPrefixes, 1)), words = (Sp + 31) / 32;
  plan.impactUnitBytes = words * 4 + 8;
  plan.unitBytes = 3 * Sp * 4 + plan.impactUnitBytes;
  plan.chunks = chunkBounds(plan.pairs.size(), plan.unitBytes, chunkBytes);
  plan.impactChunks = chunkBounds(plan.pairs.size(), plan.impactUnitBytes, chunkBytes);
  if (listsOut) *listsOut = std::move(lists);
  if (hbOut) *hbOut = std::move(hb);
  return plan;
}

}  // namespace

NetworkWhatifPlan network_whatif_plan(const LinkState& ls, const PrefixState& ps,
                                      const std::vector<std::string>& sources,
                                      const std::vector<LinkFailureSweep::Scenario>& scenarios,
                                      size_t chunkBytes) {
  return makePlan(ls, ps, sources, scenarios, chunkBytes, nullptr, nullptr);
}

NetworkWhatifSweep::NetworkWhatifSweep(const LinkState& ls, const PrefixState& ps,
                                       const std::vector<std::string>& sources,
                                       const std::vector<LinkFailureSweep::Scenario>& scenarios,
                                       bool enableV4, bool enableBestRouteSelection,
                                       bool v4OverV6Nexthop)
    : ls_(ls),
      ps_(ps),
      sources_(sources),
      scenarios_(scenarios),
      enableV4_(enableV4),
      brs_(enableBestRouteSelection),
      v4OverV6_(v4OverV6Nexthop),
      K_(scenarios.size()) {
  plan_ = makePlan(ls, ps, sources, scenarios, chunkBytes_, &lists_, &hb_);
  table_.build(ps);
  Sn_ = size_t(std::max(hb_.maxNodes, 1));
  Sp_ = size_t(std::max(hb_.maxPrefixes, 1));
  words_ = (Sp_ + 31) / 32;
  down_.assign(sources.size() * K_, 0);
  for (const auto& [s, k] : plan_.sourceDown) down_[s * K_ + k] = 1;
  replan();
  for (const uint32_t s : plan_.fallback) addFallback(s);
}

// row_ / unit_ from the plan's batched sources and pairs
void NetworkWhatifSweep::replan() {
  row_.assign(sources_.size(), -1);
  for (size_t r = 0; r < plan_.batched.size(); ++r) row_[plan_.batched[r]] = int32_t(r);
  unit_.assign(plan_.batched.size() * K_, kNoUnit);
  for (size_t u = 0; u < plan_.pairs.size(); ++u) {
    unit_[size_t(row_[plan_.pairs[u].first]) * K_ + plan_.pairs[u].second] = uint32_t(u);
  }
}

// source s through its own LinkFailureSweep, over the scenarios it runs in
void NetworkWhatifSweep::addFallback(size_t s) {
  Fallback fb;
  fb.local.assign(K_, -1);
  std::vector<LinkFailureSweep::Scenario> scs;
  for (size_t k = 0; k < K_; ++k) {
    if (down_[s * K_ + k]) continue;
    fb.local[k] = int32_t(scs.size());
    scs.push_back(scenarios_[k]);
  }
  fb.sweep = std::make_unique<LinkFailureSweep>(sources_[s], ls_, ps_, scs, enableV4_, brs_,
                                                v4OverV6_);
  fb_[s] = std::move(fb);
}

void NetworkWhatifSweep::setChunkBytes(size_t bytes) {
  chunkBytes_ = std::max<size_t>(bytes, 1);
  plan_.chunks = chunkBounds(plan_.pairs.size(), plan_.unitBytes, chunkBytes_);
  plan_.impactChunks = chunkBounds(plan_.pairs.size(), plan_.impactUnitBytes, chunkBytes_);
  launched_ = impactFetched_ = updatesFetched_ = false;
  counts_.clear();
  compact_.reset(0, 1);
}

// graph, table, units, pair indices and the scenario lists: once
void NetworkWhatifSweep::upload() {
  if (uploaded_) return;
  uploaded_ = true;
  const FlatTopology& f = ls_.flat();
  img_.uploadGraph(hb_);
  img_.uploadTable(hb_);
  std::vector<ogs_unit> baseUnits;
  for (const uint32_t s : plan_.batched) baseUnits.push_back(ogs_unit{0, f.id.at(sources_[s])});
  std::vector<ogs_unit> units;
  std::vector<uint32_t> base, scen;
  for (const auto& [s, k] : plan_.pairs) {
    units.push_back(baseUnits[size_t(row_[s])]);
    base.push_back(uint32_t(row_[s]));
    scen.push_back(k);
  }
  dBaseUnits_.upload(baseUnits.data(), baseUnits.size());
  dUnits_.upload(units.data(), units.size());
  dBase_.upload(base.data(), base.size());
  dScen_.upload(scen.data(), scen.size());
  dLists_.upload(lists_);
  const std::vector<uint32_t> cls = advClasses(table_);
  dAdvClass_.upload(cls.data(), cls.size());
  const size_t B = std::max<size_t>(plan_.batched.size(), 1);
  bDist_.resize(B * Sn_ * 4);
  bNh_.resize(B * Sn_ * 4);
  for (auto* b : {&bMeta_, &bMetric_, &bMask_, &bSel_}) b->resize(B * Sp_ * 4);
  dCounts_.resize(std::max<size_t>(plan_.pairs.size(), 1) * 8);
}

// every batched source's base SPF and records: one launch, unit-major rows
void NetworkWhatifSweep::runBase(void* stream) {
  const ogs_graph g = img_.graph(hb_, 1);
  const ogs_prefix_table pt = img_.table(hb_);
  ogs_spf_out out{bDist_.get(),   bNh_.as<uint32_t>(),   bMeta_.as<uint32_t>(),
                  bMetric_.get(), bMask_.as<uint32_t>(), bSel_.as<uint32_t>()};
  ogsCheck(ogs_spf_routes(&g, &pt, dBaseUnits_.as<ogs_unit>(), int32_t(plan_.batched.size()),
                          routeFlags(enableV4_, brs_), 1, &out, stream),
           "ogs_spf_routes(bases)");
  baseRun_ = true;
  base_.clear();
}

bool NetworkWhatifSweep::launchChunks(void* stream, bool records) {
  const size_t U = plan_.pairs.size();
  const std::vector<size_t>& chunks = records ? plan_.chunks : plan_.impactChunks;
  size_t most = 1;
  for (size_t c = 0; c + 1 < chunks.size(); ++c) most = std::max(most, chunks[c + 1] - chunks[c]);
  dChanged_.resize(most * words_ * 4);
  if (records) {
    for (auto* b : {&dMeta_, &dMetric_, &dMask_}) b->resize(most * Sp_ * 4);
  }
  const ogs_graph g = img_.graph(hb_, 1);
  const ogs_prefix_table pt = img_.table(hb_);
  // the pairs index the scenarios themselves: every chunk passes the same mods
  const ogs_whatif_mods mods = dLists_.mods();
  uint32_t fl = routeFlags(enableV4_, brs_) | OGS_F_INCREMENTAL | OGS_F_CHANGED_ONLY;
  if (lists_.restores) fl |= OGS_F_RESTORE;
  ogs_spf_out out{};
  if (records) {
    out.meta = dMeta_.as<uint32_t>();
    out.metric = dMetric_.get();
    out.mask = dMask_.as<uint32_t>();
    counts_.assign(U * 2, 0);
    compact_.reset(U, 1);
  }
  for (size_t c = 0; c + 1 < chunks.size(); ++c) {
    const size_t c0 = chunks[c], n = chunks[c + 1] - c0;
    const ogs_whatif_pairs pairs{dBase_.as<uint32_t>() + c0, dScen_.as<uint32_t>() + c0,
                                 int32_t(plan_.batched.size()), int32_t(K_)};
    ogs_route_diff diff{bMeta_.as<uint32_t>(), bMetric_.as<uint32_t>(), bMask_.as<uint32_t>(),
                        dChanged_.as<uint32_t>(), dCounts_.as<uint32_t>() + c0 * 2,
                        bDist_.as<uint32_t>(), bNh_.as<uint32_t>(), dAdvClass_.as<uint32_t>(),
                        nullptr, 0};
    const int rc = ogs_spf_routes_whatif_pairs(&g, &pt, dUnits_.as<ogs_unit>() + c0, int32_t(n),
                                               &pairs, &mods, &diff, fl, 1, &out, stream);
    if (rc == OGS_E_UNSUPPORTED && c == 0) return false;  // nothing was launched
    ogsCheck(rc, "ogs_spf_routes_whatif_pairs");
    if (!records) continue;
    // counts -> the chunk's offsets -> gather -> its compact records
    ogsCheck(ogs_memcpy_d2h(&counts_[c0 * 2], dCounts_.as<uint32_t>() + c0 * 2, n * 8, stream),
             "ogs_memcpy_d2h");
    ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
    compact_.gather(c0, n, &counts_[c0 * 2], dChanged_.as<uint32_t>(), out, Sp_, stream);
    // the host vectors grow and the offsets are rewritten by the next chunk
    ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
  }
  return true;
}

void NetworkWhatifSweep::launch(void* stream, bool records) {
  launched_ = impactFetched_ = updatesFetched_ = false;
  if (!plan_.batched.empty()) {
    upload();
    if (!baseRun_) runBase(stream);
    if (!launchChunks(stream, records)) {
      // past the repair's LDS budget: every source through its own sweep
      for (const uint32_t s : plan_.batched) addFallback(s);
      plan_.fallback.insert(plan_.fallback.end(), plan_.batched.begin(), plan_.batched.end());
      std::sort(plan_.fallback.begin(), plan_.fallback.end());
      plan_.batched.clear();
      plan_.pairs.clear();
      plan_.chunks = plan_.impactChunks = {0};
      replan();
    }
  }
  for (auto& [s, fb] : fb_) fb.sweep->launch(stream, records);
  launched_ = true;
  records_ = records;
}

void NetworkWhatifSweep::fetchImpact(void* stream) {
  if (!launched_) throw std::logic_error("NetworkWhatifSweep::fetchImpact: launch() first");
  const size_t U = plan_.pairs.size();
  if (!records_) {  // (a launch with records fetched the counts chunk by chunk)
    counts_.assign(U * 2, 0);
    if (U) dCounts_.download(counts_.data(), U * 2, stream);
    ogsCheck(ogs_stream_sync(stream), "ogs_stream_sync");
  }
  for (auto& [s, fb] : fb_) {
    if (records_) {
      fb.sweep->fetchUpdates(stream);
    } else {
      fb.sweep->fetchRecords(stream);
    }
  }
  impactFetched_ = true;
  updatesFetched_ = records_;
}

void NetworkWhatifSweep::fetchUpdates(void* stream) {
  if (!launched_ || !records_) {
    throw std::logic_error("NetworkWhatifSweep::fetchUpdates: launch(records=true) first");
  }
  fetchImpact(stream);
}

void NetworkWhatifSweep::check(size_t s, size_t k) const {
  if (s >= sources_.size() || k >= K_) throw std::out_of_range("NetworkWhatifSweep: pair");
}

NetworkWhatifSweep::PairState NetworkWhatifSweep::state(size_t s, size_t k) const {
  check(s, k);
  return down_[s * K_ + k] ? kSourceDown : kComputed;
}

std::pair<uint32_t, uint32_t> NetworkWhatifSweep::counts(size_t s, size_t k) const {
  check(s, k);
  if (!impactFetched_) throw std::logic_error("NetworkWhatifSweep: nothing fetched yet");
  if (down_[s * K_ + k]) return {0u, 0u};
  if (row_[s] < 0) {
    const Fallback& fb = fb_.at(s);
    return fb.sweep->counts(size_t(fb.local[k]));
  }
  const size_t u = unit_[size_t(row_[s]) * K_ + k];
  return {counts_[2 * u], counts_[2 * u + 1]};
}

std::vector<uint32_t> NetworkWhatifSweep::affectedSources(size_t k) const {
  std::vector<uint32_t> out;
  for (size_t s = 0; s < sources_.size(); ++s) {
    if (counts(s, k) != std::pair<uint32_t, uint32_t>{0u, 0u}) out.push_back(uint32_t(s));
  }
  return out;
}

std::vector<std::string> NetworkWhatifSweep::changedPrefixes(size_t s, size_t k) const {
  check(s, k);
  if (!updatesFetched_) throw std::logic_error("NetworkWhatifSweep: fetchUpdates() first");
  if (down_[s * K_ + k]) return {};
  if (row_[s] < 0) {
    const Fallback& fb = fb_.at(s);
    return fb.sweep->changedPrefixes(size_t(fb.local[k]));
  }
  const size_t u = unit_[size_t(row_[s]) * K_ + k];
  std::vector<std::string> out;
  for (uint32_t i = compact_.offsets[u]; i < compact_.offsets[u + 1]; ++i) {
    out.push_back(table_.prefixes.at(compact_.prefix[i]));
  }
  std::sort(out.begin(), out.end());
  return out;
}

DecisionRouteUpdate NetworkWhatifSweep::routeUpdate(size_t s, size_t k) const {
  check(s, k);
  if (down_[s * K_ + k]) {
    throw std::invalid_argument("NetworkWhatifSweep: " + sources_[s] +
                                " is down in that scenario and runs no Decision");
  }
  if (!updatesFetched_) throw std::logic_error("NetworkWhatifSweep: fetchUpdates() first");
  if (row_[s] < 0) {
    const Fallback& fb = fb_.at(s);
    return fb.sweep->routeUpdate(size_t(fb.local[k]));
  }
  const size_t u = unit_[size_t(row_[s]) * K_ + k];
  if (counts_[2 * u] == OGS_WHATIF_REFUSED) {
    throw std::logic_error("NetworkWhatifSweep: the device refused the pair");
  }
  return materializeUpdate(ls_.flat(), sources_[s], table_, compact_.view(), u, v4OverV6_);
}

// the source's base RouteDb from its row of the base launch's records
const DecisionRouteDb& NetworkWhatifSweep::baseRouteDb(size_t s) const {
  if (s >= sources_.size()) throw std::out_of_range("NetworkWhatifSweep: source");
  if (!impactFetched_) throw std::logic_error("NetworkWhatifSweep: nothing fetched yet");
  if (row_[s] < 0) return fb_.at(s).sweep->baseRouteDb();
  auto it = base_.find(s);
  if (it != base_.end()) return it->second;
  const size_t r = size_t(row_[s]);
  std::vector<uint32_t> meta(Sp_), metric(Sp_), mask(Sp_);
  ogsCheck(ogs_memcpy_d2h(meta.data(), bMeta_.as<uint32_t>() + r * Sp_, Sp_ * 4, nullptr), "d2h");
  ogsCheck(ogs_memcpy_d2h(metric.data(), bMetric_.as<uint32_t>() + r * Sp_, Sp_ * 4, nullptr),
           "d2h");
  ogsCheck(ogs_memcpy_d2h(mask.data(), bMask_.as<uint32_t>() + r * Sp_, Sp_ * 4, nullptr), "d2h");
  ogsCheck(ogs_stream_sync(nullptr), "ogs_stream_sync");
  DecisionRouteDb db;
  addUnicastRoutes(db, ls_.flat(), sources_[s], table_, meta.data(), metric.data(), mask.data(),
                   Sp_, 1, v4OverV6_);
  return base_.emplace(s, std::move(db)).first->second;
}

}  // namespace openr_amd
