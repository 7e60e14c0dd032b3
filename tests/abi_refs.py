"""Plain numpy / Python restatements of three device entries of
include/openr_gpu.h, written from the header's text and the reference lines
it cites, for the tests that call the entries directly:

  rib_policy_ref        ogs_rib_policy_apply   (RibPolicy.cpp:74-161, 221-249)
  route_changes_ref     ogs_route_changes_gather (SpfSolver.cpp:21-56 hands Fib
                        the changed records; the header fixes their order)
  routes_multiarea_ref  ogs_routes_multiarea   (SpfSolver.cpp:160-311, 455-688,
                        LsdbUtil.cpp:374-389, 700-823)

Each takes the flat arrays the entry takes and returns the arrays the entry
writes. Arrays the entry updates in place (or leaves partly untouched) start
from the caller's copy, so poison in columns the entry must not write stays
where it was. tests/test_abi_refs.py pins every rule on hand-worked cases."""
import numpy as np

NONE = 0xFFFFFFFF            # OGS_NODE_NONE
POLICY_NONE = 0xFFFF         # OGS_POLICY_NONE
NODE_OVERLOADED, NODE_SOFTDRAIN, NODE_METRICINC = 0x1, 0x2, 0x4
PFX_V4, PFX_HAS_MIN_NH = 0x1, 0x2
ROUTE_VALID, ROUTE_DRAINED, ROUTE_LOCAL, ROUTE_SELECTED = 0x1, 0x2, 0x4, 0x8
REASON_SHIFT, BEST_SHIFT = 4, 8
REASON_V4_DISABLED, REASON_UNREACHABLE, REASON_SELF = 1, 2, 3
REASON_NO_NEXTHOP, REASON_MIN_NEXTHOP = 4, 5
F_ENABLE_V4, F_V4_OVER_V6, F_BEST_ROUTE_SELECTION, F_WIDE_METRIC = 0x1, 0x2, 0x4, 0x10
MIN_NH_UNSET = -2**63        # adv_min_nh: INT64_MIN when unset


def reason_of(meta):
    return (np.asarray(meta) >> REASON_SHIFT) & 0xF


# ---------------------------------------------------------------- RibPolicy
def rib_policy_ref(pfx_base, adv_off, max_prefixes, policy, num_areas, n_units, nh_words,
                   meta, mask, applied=None, counter=None):
    """policy: dict(num_statements, active, pfx_match, adv_tag_match,
    slot_nonzero, statement_base); a whole policy of more than 32 statements
    goes in one pass with `active` a Python int and the two match tables as
    [rows, K] bool arrays. meta [U*S_p]; mask [((u*A+a)*W+w)*S_p+p];
    applied / counter [U*S_p] uint16 or None (then every column starts at
    OGS_POLICY_NONE). Returns (mask, applied, counter), new arrays.

    RibPolicy::applyAction (221-229) walks the statements in order and stops at
    the first whose applyAction returns true. A statement's applyAction
    (109-161): no match -> false; else the route takes the statement's
    counterID; next hops of weight 0 are dropped; none left -> the route keeps
    its next hops and the call returns false (the walk goes on); else the route
    takes the kept ones and the call returns true. match (74-107): no matcher
    -> never; else tag matcher (on the route's BEST entry) and prefix matcher.
    A chunk with statement_base > 0 continues an earlier chunk's walk: routes
    with applied != OGS_POLICY_NONE are finished, the others keep the counter
    they have unless a statement of this chunk matches."""
    K, base = int(policy["num_statements"]), int(policy["statement_base"])
    A, W, U, Sp = num_areas, nh_words, n_units, max_prefixes
    p0 = int(pfx_base[0])
    P = int(pfx_base[1]) - p0
    meta = np.asarray(meta, dtype=np.uint32).reshape(U, Sp)
    mask = np.array(mask, dtype=np.uint32).reshape(U, A, W, Sp)
    app = (np.full((U, Sp), POLICY_NONE, np.uint16) if applied is None
           else np.array(applied, dtype=np.uint16).reshape(U, Sp))
    cnt = (np.full((U, Sp), POLICY_NONE, np.uint16) if counter is None
           else np.array(counter, dtype=np.uint16).reshape(U, Sp))
    nz = np.asarray(policy["slot_nonzero"], dtype=np.uint32).reshape(U, K, A, W)

    def column(table, k):  # bit k of every row: uint32 words, or a [rows, K] bool table
        table = np.asarray(table)
        return table[:, k].astype(bool) if table.ndim == 2 else ((table >> k) & 1).astype(bool)
    adv_off = np.asarray(adv_off, dtype=np.int64)
    if base == 0:  # a first chunk decides every column of the table's prefixes
        app[:, :P] = POLICY_NONE
        cnt[:, :P] = POLICY_NONE
    gp = p0 + np.arange(P)
    m = meta[:, :P]
    walking = ((m & ROUTE_VALID) != 0) & (app[:, :P] == POLICY_NONE)
    best = adv_off[gp][None, :] + (m >> BEST_SHIFT)          # [U, P] global entry
    best = np.where(walking, best, 0)
    for k in range(K):
        if not (int(policy["active"]) >> k) & 1:
            continue  # neither a tag nor a prefix matcher: never matches
        hit = (walking & column(policy["pfx_match"], k)[gp][None, :] &
               column(policy["adv_tag_match"], k)[best])
        cnt[:, :P][hit] = base + k
        kept = mask[:, :, :, :P] & nz[:, k][:, :, :, None]   # weight-0 next hops dropped
        took = hit & kept.any(axis=(1, 2))
        mask[:, :, :, :P] = np.where(took[:, None, None, :], kept, mask[:, :, :, :P])
        app[:, :P][took] = base + k
        walking = walking & ~took
    return mask.reshape(-1), app.reshape(-1), cnt.reshape(-1)


# ------------------------------------------------------------------- gather
def changed_bits(changed, n_units, max_prefixes):
    """[U, S_p] bool of the bitmap rows ([U * ceil(S_p/32)] words, bit p % 32
    of word p / 32); bits at or past max_prefixes are ignored"""
    words = (max_prefixes + 31) // 32
    rows = np.ascontiguousarray(changed, dtype=np.uint32).reshape(n_units, words)
    bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :max_prefixes].astype(bool)


def route_changes_counts(changed, n_units, max_prefixes):
    return changed_bits(changed, n_units, max_prefixes).sum(1).astype(np.uint32)


def route_changes_ref(changed, n_units, max_prefixes, meta, metric, mask, nh_words, offsets,
                      total, out=None):
    """Records of the marked prefixes, unit-major, prefix ascending within a
    unit, unit u's from offsets[u]; a record is carried whatever its meta holds
    (one without OGS_ROUTE_VALID is a deletion). A unit writes nothing at or
    past offsets[u + 1]. out: dict(prefix, meta, metric [total], mask
    [W * total]) the records start from (default zeros). Returns such a dict."""
    U, Sp, W = n_units, max_prefixes, nh_words
    bits = changed_bits(changed, U, Sp)
    meta = np.asarray(meta, dtype=np.uint32).reshape(U, Sp)
    metric = np.asarray(metric, dtype=np.uint32).reshape(U, Sp)
    mask = np.asarray(mask, dtype=np.uint32).reshape(U, W, Sp)
    res = {k: (np.zeros(n, np.uint32) if out is None else np.array(out[k], dtype=np.uint32))
           for k, n in (("prefix", total), ("meta", total), ("metric", total),
                        ("mask", W * total))}
    rmask = res["mask"].reshape(W, total)
    for u in range(U):
        ps = np.flatnonzero(bits[u])
        lo, hi = int(offsets[u]), int(offsets[u + 1])
        ps = ps[:max(hi - lo, 0)]
        sl = slice(lo, lo + len(ps))
        res["prefix"][sl] = ps
        res["meta"][sl] = meta[u, ps]
        res["metric"][sl] = metric[u, ps]
        rmask[:, sl] = mask[u][:, ps]
    return res


# --------------------------------------------------------------- multi-area
def routes_multiarea_ref(graph, prefixes, areas, units, n_units, spf_row, spf_dist, spf_nh,
                         flags, nh_words, out=None):
    """graph: dict(max_nodes, node_base, node_flags); prefixes: dict(max_prefixes,
    pfx_base, adv_off, adv_node, adv_metrics [A_total*4], adv_min_nh, pfx_flags);
    areas: dict(num_areas, name_local [G*A], adv_area, adv_name, reached or
    None). spf_dist [rows*S_n] (uint64 under OGS_F_WIDE_METRIC), spf_nh
    [(row*W+w)*S_n+v]. out: dict(meta, metric, sel [U*S_p], mask [U*A*W*S_p])
    the records start from (default zeros); returns such a dict.

    One createRouteForPrefix (SpfSolver.cpp:160-311) per (unit, prefix), in the
    reference's own order of steps; the sets of (node, area) keys are lists of
    entry indexes of the prefix's segment, which the header says is in key
    order. What a record without OGS_ROUTE_VALID holds is the state at the
    reference's return: LOCAL once the entries were scanned (193-214);
    SELECTED, the best index, DRAINED and sel once bestRoutesCache_ was set
    (247); the metric and masks handed to addBestPaths (303-310) for the two
    reasons it returns, all-ones and zero masks before."""
    Sn, Sp = int(graph["max_nodes"]), int(prefixes["max_prefixes"])
    A, W, U = int(areas["num_areas"]), nh_words, n_units
    wide = bool(flags & F_WIDE_METRIC)
    dt = np.uint64 if wide else np.uint32
    inf = int(np.iinfo(dt).max)
    node_base, node_flags = graph["node_base"], graph["node_flags"]
    p0 = int(prefixes["pfx_base"][0])
    P = int(prefixes["pfx_base"][1]) - p0
    adv_off, adv_node = prefixes["adv_off"], prefixes["adv_node"]
    metrics = np.asarray(prefixes["adv_metrics"], dtype=np.int32).reshape(-1, 4)
    min_nh, pfx_flags = prefixes["adv_min_nh"], prefixes["pfx_flags"]
    name_local = np.asarray(areas["name_local"], dtype=np.uint32).reshape(-1, A)
    adv_area, adv_name, reached = areas["adv_area"], areas["adv_name"], areas.get("reached")
    dist = np.asarray(spf_dist, dtype=dt).reshape(-1, Sn)
    nh = np.asarray(spf_nh, dtype=np.uint32).reshape(-1, W, Sn)
    rw = (Sn + 31) // 32
    enable_v4, v4_over_v6 = bool(flags & F_ENABLE_V4), bool(flags & F_V4_OVER_V6)
    brs = bool(flags & F_BEST_ROUTE_SELECTION)

    res = {}
    for k, n, t in (("meta", U * Sp, np.uint32), ("metric", U * Sp, dt), ("sel", U * Sp, np.uint32),
                    ("mask", U * A * W * Sp, np.uint32)):
        res[k] = np.zeros(n, t) if out is None or out.get(k) is None else np.array(out[k], dtype=t)
    o_meta, o_metric = res["meta"].reshape(U, Sp), res["metric"].reshape(U, Sp)
    o_sel, o_mask = res["sel"].reshape(U, Sp), res["mask"].reshape(U, A, W, Sp)

    for u in range(U):
        me = int(units[u])
        rows = [int(r) for r in spf_row[u * A:(u + 1) * A]]

        def spf_entry(b, name):
            """(metric, next-hop words) of `name` in getSpfResult(me) of area b,
            or None when it is not in the result. The source is always in it, at
            0 and with no next hop (LinkState.cpp:730-734)."""
            if name == me:
                return 0, np.zeros(W, np.uint32)
            r, v = rows[b], int(name_local[name, b])
            if r == NONE or v == NONE:
                return None
            if reached is not None:
                if not (int(reached[r * rw + v // 32]) >> (v % 32)) & 1:
                    return None
            elif int(dist[r, v]) == inf:
                return None
            return int(dist[r, v]), nh[r, :, v]

        def nflags(a):  # of the entry's node in the entry's own area
            v = int(adv_node[a])
            return 0 if v == NONE else int(node_flags[int(node_base[int(adv_area[a])]) + v])

        for p in range(P):
            gp = p0 + p

            def record(meta, metric=inf, sel=0, masks=None):
                o_meta[u, p], o_metric[u, p], o_sel[u, p] = meta, metric, sel
                o_mask[u, :, :, p] = 0 if masks is None else masks

            # 169-176
            if (int(pfx_flags[gp]) & PFX_V4) and not enable_v4 and not v4_over_v6:
                record(REASON_V4_DISABLED << REASON_SHIFT)
                continue
            seg0 = int(adv_off[gp])
            entries = list(range(seg0, int(adv_off[gp + 1])))
            # 193-214: reachable in the entry's OWN area only
            local = any(int(adv_name[a]) == me for a in entries)
            kept = [a for a in entries
                    if spf_entry(int(adv_area[a]), int(adv_name[a])) is not None]
            meta = ROUTE_LOCAL if local else 0
            if not kept:  # 217-223
                record(meta | (REASON_UNREACHABLE << REASON_SHIFT))
                continue
            # selectBestRoutes 455-494; filterHardDrainedNodes 526-541
            up = [a for a in kept if not nflags(a) & NODE_OVERLOADED]
            filtered = up if up else kept
            if brs:  # selectRoutes, LsdbUtil.cpp:760-823, SHORTEST_DISTANCE
                def key(a):
                    drained = metrics[a, 0] != 0 or bool(nflags(a) & NODE_SOFTDRAIN)
                    return (-int(drained), int(metrics[a, 1]), int(metrics[a, 2]))
                top = max(key(a) for a in filtered)
                tied = [a for a in filtered if key(a) == top]
                near = min(int(metrics[a, 3]) for a in tied)
                chosen = [a for a in tied if int(metrics[a, 3]) == near]
                mine = [a for a in chosen if int(adv_name[a]) == me]
                best = mine[0] if mine else chosen[0]  # selectBestNodeArea 700-711
            else:
                chosen = filtered
                best = chosen[0]  # *allNodeAreas.begin()
            meta |= ROUTE_SELECTED | ((best - seg0) << BEST_SHIFT)
            if nflags(best) & (NODE_OVERLOADED | NODE_METRICINC):  # isNodeDrained 543-551
                meta |= ROUTE_DRAINED
            sel = 0
            for a in chosen:
                if a - seg0 < 32:
                    sel |= 1 << (a - seg0)
            if any(int(adv_name[a]) == me for a in chosen):  # 253-258
                record(meta | (REASON_SELF << REASON_SHIFT), inf, sel)
                continue
            # 262-301
            names = [int(adv_name[a]) for a in chosen]
            total = np.zeros((A, W), np.uint32)
            shortest = inf
            for b in sorted({int(adv_area[a]) for a in chosen}):  # hasBestRoutesInArea
                # getNextHopsWithMetric 648-688: EVERY selected name, in b's SPF
                area_metric, closest = inf, []
                for name in names:
                    e = spf_entry(b, name)
                    if e is None:
                        continue
                    if area_metric >= e[0]:
                        if area_metric > e[0]:
                            area_metric, closest = e[0], []
                        closest.append(e[1])
                hops = np.zeros(W, np.uint32)
                for words in closest:
                    hops = hops | words
                if shortest >= area_metric:
                    if shortest > area_metric:
                        shortest = area_metric
                        total[:] = 0
                    total[b] = hops
            # addBestPaths 595-639
            count = sum(bin(int(x)).count("1") for x in total.reshape(-1))
            need = [int(min_nh[a]) for a in chosen if int(min_nh[a]) != MIN_NH_UNSET]
            if count == 0:
                meta |= REASON_NO_NEXTHOP << REASON_SHIFT
            elif need and (max(need) % 2**64) > count:  # int64 against size_t (612)
                meta |= REASON_MIN_NEXTHOP << REASON_SHIFT
            else:
                meta |= ROUTE_VALID
            record(meta, shortest, sel, total)
    return res
