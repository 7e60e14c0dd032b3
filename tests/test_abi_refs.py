"""The numpy restatements of tests/abi_refs.py on hand-worked cases: every
expected output below is written out literally, next to the rule of the
reference (openr/decision/RibPolicy.cpp, SpfSolver.cpp, openr/common/
LsdbUtil.cpp) or of include/openr_gpu.h it shows. No GPU: these pin the
references the device tests compare the kernels against."""
import numpy as np

import abi_refs as R

NONE, PN = R.NONE, R.POLICY_NONE
INF32, INF64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def u32(*a):
    return np.array(a, dtype=np.uint32)


# ---------------------------------------------------------------- RibPolicy
# four prefixes; prefix 0 has two advertisements, the others one each
PFX_BASE, ADV_OFF = u32(0, 4), u32(0, 2, 3, 4, 5)
VALID = R.ROUTE_VALID
UNREACHABLE = R.REASON_UNREACHABLE << R.REASON_SHIFT


def test_rib_policy_statement_walk():
    policy = dict(
        num_statements=3, statement_base=0,
        active=0b011,                       # statement 2 has no matcher
        pfx_match=u32(0b111, 0b111, 0b110, 0b111),
        adv_tag_match=u32(0b100, 0b111, 0b111, 0b111, 0b111),
        slot_nonzero=u32(0b0011, 0b0100, 0b1111))
    meta = u32(VALID | (1 << R.BEST_SHIFT), VALID, VALID, UNREACHABLE)
    mask = u32(0b0110, 0b0100, 0b1000, 0b0110)
    got = R.rib_policy_ref(PFX_BASE, ADV_OFF, 4, policy, 1, 1, 1, meta, mask)
    # p0: the tag match is read at the BEST entry, adv_off[0] + 1 (entry 0 meets
    #     no statement's tags): statement 0 matches and keeps slot 1 (74-107)
    # p1: statement 0 matches but its weights drop every next hop: counterID
    #     taken, route unchanged, the walk goes on (116, 149-155); statement 1
    #     then transforms it, so the first TRANSFORMING statement wins (221-229)
    # p2: not in statement 0's prefix set; statement 1 matches and drops all;
    #     statement 2 would keep everything but has no matcher (76-78)
    # p3: no route (OGS_ROUTE_VALID clear): untouched
    assert got[0].tolist() == [0b0010, 0b0100, 0b1000, 0b0110]
    assert got[1].tolist() == [0, 1, PN, PN]
    assert got[2].tolist() == [0, 1, 1, PN]
    # the poison of a first chunk's applied / counter columns does not survive
    again = R.rib_policy_ref(PFX_BASE, ADV_OFF, 4, policy, 1, 1, 1, meta, mask,
                             np.full(4, 0xAAAA, np.uint16), np.full(4, 0xAAAA, np.uint16))
    assert [a.tolist() for a in again] == [a.tolist() for a in got]


def test_rib_policy_continuation_chunk():
    policy = dict(num_statements=2, statement_base=32, active=0b11,
                  pfx_match=u32(0b11, 0b11, 0b00, 0b11), adv_tag_match=u32(3, 3, 3, 3, 3),
                  slot_nonzero=u32(0b0010, 0b0001))
    meta = u32(VALID, VALID, VALID, UNREACHABLE)
    mask = u32(0b0110, 0b0110, 0b1000, 0b0110)
    applied = np.array([5, PN, PN, PN], np.uint16)
    counter = np.array([5, 7, 7, PN], np.uint16)
    got = R.rib_policy_ref(PFX_BASE, ADV_OFF, 4, policy, 1, 1, 1, meta, mask, applied, counter)
    # p0: statement 5 of an earlier chunk transformed it: skipped (statement 32
    #     would have cut it to 0b0010)
    # p1: statement 32 transforms it: ids are statement_base + k
    # p2: matches nothing here: applied stays none, counter 7 is carried on
    # p3: no route: carried as it came
    assert got[0].tolist() == [0b0110, 0b0010, 0b1000, 0b0110]
    assert got[1].tolist() == [5, 32, PN, PN]
    assert got[2].tolist() == [5, 32, 7, PN]


def test_rib_policy_units_areas_words_and_slack():
    """mask[((u*A+a)*W+w)*S_p+p], slot_nonzero[u][k][a][w]: a route is cut when
    ANY area's word keeps a next hop; table of one prefix at global index 7 in
    rows of S_p = 2 (column 1 is slack)."""
    pfx_base, adv_off = u32(7, 8), np.arange(9, dtype=np.uint32) * 2  # prefix 7: entries 14, 15
    pfx_match, tag = np.zeros(8, np.uint32), np.zeros(16, np.uint32)
    pfx_match[7], tag[15] = 1, 1
    policy = dict(num_statements=1, statement_base=0, active=1, pfx_match=pfx_match,
                  adv_tag_match=tag,
                  slot_nonzero=u32(0, 2, 0, 0,    # unit 0: area 0 word 1 only
                                   1, 0, 4, 0,    # unit 1: word 0 of both areas
                                   0, 0, 0, 16))  # unit 2: nothing the route has
    meta = np.tile(u32(VALID | (1 << R.BEST_SHIFT), 0xDEAD), 3)
    mask = np.tile(np.stack([u32(1, 2, 4, 8), u32(99, 99, 99, 99)], 1).reshape(-1), 3)
    applied, counter = np.full(6, 0xAAAA, np.uint16), np.full(6, 0xAAAA, np.uint16)
    got = R.rib_policy_ref(pfx_base, adv_off, 2, policy, 2, 3, 2, meta, mask, applied, counter)
    assert got[0].reshape(3, 4, 2)[:, :, 0].tolist() == [[0, 2, 0, 0], [1, 0, 4, 0], [1, 2, 4, 8]]
    assert (got[0].reshape(3, 4, 2)[:, :, 1] == 99).all()
    assert got[1].tolist() == [0, 0xAAAA, 0, 0xAAAA, PN, 0xAAAA]
    assert got[2].tolist() == [0, 0xAAAA, 0, 0xAAAA, 0, 0xAAAA]


# ------------------------------------------------------------------- gather
def gather_inputs():
    # 2 units, S_p = 40 (2 bitmap words), W = 2
    changed = u32((1 << 1) | (1 << 31), (1 << 3) | (1 << 9),  # unit 0: 1, 31, 35; bit 41 >= S_p
                  1 << 0, 0)                                 # unit 1: 0
    meta = 1001 + 2 * np.arange(80, dtype=np.uint32)         # odd: OGS_ROUTE_VALID set
    meta[31] = UNREACHABLE                                   # a deletion record
    metric = 2000 + np.arange(80, dtype=np.uint32)
    mask = 3000 + np.arange(160, dtype=np.uint32)            # [(u*2+w)*40 + p]
    return changed, meta, metric, mask


def test_gather_order_and_deletion_record():
    changed, meta, metric, mask = gather_inputs()
    assert R.route_changes_counts(changed, 2, 40).tolist() == [3, 1]
    got = R.route_changes_ref(changed, 2, 40, meta, metric, mask, 2, u32(0, 3, 4), 4)
    # unit-major, prefix ascending; the record at prefix 31 has no
    # OGS_ROUTE_VALID and is carried like the others (unicastRoutesToDelete)
    assert got["prefix"].tolist() == [1, 31, 35, 0]
    assert got["meta"].tolist() == [1003, UNREACHABLE, 1071, 1081]
    assert got["metric"].tolist() == [2001, 2031, 2035, 2040]
    # word w of record i at mask[w * total + i]
    assert got["mask"].tolist() == [3001, 3031, 3035, 3080, 3041, 3071, 3075, 3120]


def test_gather_short_slice_keeps_the_first_records():
    changed, meta, metric, mask = gather_inputs()
    out = {k: np.full(n, 9, np.uint32) for k, n in
           (("prefix", 4), ("meta", 4), ("metric", 4), ("mask", 8))}
    got = R.route_changes_ref(changed, 2, 40, meta, metric, mask, 2, u32(0, 2, 3), 4, out)
    assert got["prefix"].tolist() == [1, 31, 0, 9]
    assert got["metric"].tolist() == [2001, 2031, 2040, 9]
    assert got["mask"].tolist() == [3001, 3031, 3080, 9, 3041, 3071, 3120, 9]


# --------------------------------------------------------------- multi-area
def domain(name_local, node_flags, prefixes, rows, W=1, wide=False, reached=None):
    """name_local [G][A]; node_flags [A][nodes of a]; prefixes: [(v4, [(name,
    area, (drain, path_pref, source_pref, distance), min_nh or None), ...])];
    rows: [(dist [S_n], nh [W][S_n])]"""
    name_local = np.array(name_local, dtype=np.uint32)
    A = name_local.shape[1]
    node_base = np.concatenate([[0], np.cumsum([len(f) for f in node_flags])]).astype(np.uint32)
    adv = [e for _, seg in prefixes for e in seg]
    graph = dict(max_nodes=len(rows[0][0]), node_base=node_base,
                 node_flags=np.concatenate([np.array(f, np.uint8) for f in node_flags]))
    table = dict(
        max_prefixes=len(prefixes), pfx_base=u32(0, len(prefixes)),
        adv_off=np.concatenate([[0], np.cumsum([len(s) for _, s in prefixes])]).astype(np.uint32),
        adv_node=np.array([name_local[n, a] for n, a, _, _ in adv], np.uint32),
        adv_metrics=np.array([m for _, _, m, _ in adv], np.int32).reshape(-1),
        adv_min_nh=np.array([R.MIN_NH_UNSET if t is None else t for *_, t in adv], np.int64),
        pfx_flags=np.array([(R.PFX_V4 if v4 else 0) |
                            (R.PFX_HAS_MIN_NH if any(t is not None for *_, t in s) else 0)
                            for v4, s in prefixes], np.uint8))
    areas = dict(num_areas=A, name_local=name_local.reshape(-1),
                 adv_area=np.array([a for _, a, _, _ in adv], np.uint32),
                 adv_name=np.array([n for n, _, _, _ in adv], np.uint32), reached=reached)
    dist = np.array([d for d, _ in rows], dtype=np.uint64 if wide else np.uint32).reshape(-1)
    nh = np.array([n for _, n in rows], dtype=np.uint32).reshape(-1)
    return graph, table, areas, dist, nh


def run(dom, units, spf_row, flags, W=1):
    graph, table, areas, dist, nh = dom
    out = R.routes_multiarea_ref(graph, table, areas, u32(*units), len(units), u32(*spf_row),
                                 dist, nh, flags, W)
    U, Sp, A = len(units), table["max_prefixes"], areas["num_areas"]
    mask = out["mask"].reshape(U, A, W, Sp)
    return [[(int(out["meta"][u * Sp + p]), int(out["metric"][u * Sp + p]),
              int(out["sel"][u * Sp + p]), mask[u, :, :, p].reshape(-1).tolist())
             for p in range(Sp)] for u in range(U)]


# names in key order: 0 x, 1 me, 2 o, 3 y, 4 z, 5 w, 6 v
X, ME, O, Y, Z, Wn, V = range(7)
NAME_LOCAL = [[0, NONE], [1, 0], [2, NONE], [3, 1], [NONE, 2], [NONE, 3], [4, NONE]]
# area 0: x me o y v; o is hard-drained, v soft-drained.  area 1: me y z w
NODE_FLAGS = [[0, 0, R.NODE_OVERLOADED, 0, R.NODE_SOFTDRAIN | R.NODE_METRICINC], [0, 0, 0, 0]]
ROWS = [([5, 0, 3, 20, 7], [[0b00001, 0, 0b10000, 0b00010, 0]]),     # (me, area 0)
        ([0, 5, 5, INF32, 777], [[0, 0b00100, 0b01000, 0xFF, 0xFF]])]  # (me, area 1); w unreached
D = (0, 100, 100, 1)
LOCAL, SELECTED, DRAINED = R.ROUTE_LOCAL, R.ROUTE_SELECTED, R.ROUTE_DRAINED


def reason(r):
    return r << R.REASON_SHIFT


def best(i):
    return i << R.BEST_SHIFT


PLAIN = [
    (False, [(Z, 1, D, None)]),
    (False, [(O, 0, D, None), (Y, 0, D, None)]),
    (False, [(O, 0, D, None)]),
    (False, [(Y, 0, D, None), (Z, 1, D, None)]),
    (False, [(X, 0, D, None), (Z, 1, D, None)]),
    (False, [(ME, 0, D, None), (O, 0, D, None)]),
    (False, [(Wn, 1, D, None)]),
    (True, [(X, 0, D, None)]),
    (False, [(V, 0, D, None)]),
    (False, [(Y, 0, D, 1), (Z, 1, D, 4)]),
    (False, [(X, 0, D, 2), (Z, 1, D, None)]),
    (False, [(X, 0, D, None), (ME, 0, D, None)]),
    (False, [(Y, 1, D, None)]),
    (False, [(X, 0, D, -1), (Z, 1, D, None)]),
]
PLAIN_WANT = [
    # reachable only in area 1, where the source also runs an SPF (194-214)
    (VALID | SELECTED, 5, 0b1, [0, 0b01000]),
    # o is overloaded in its own area and y is not: o is filtered (526-541);
    # without best-route selection the best entry is the first one left (482)
    (VALID | SELECTED | best(1), 20, 0b10, [0b00010, 0]),
    # every reachable advertiser overloaded: kept (540); isNodeDrained (543-551)
    (VALID | SELECTED | DRAINED, 3, 0b1, [0b10000, 0]),
    # A.4 (664-665): y advertises in area 0 only, yet in area 1 -- which holds
    # z's entry -- y is looked up by NAME, ties z at 5 and adds its next hop;
    # area 0 (y at 20) is longer, so its next hops are dropped (293-297)
    (VALID | SELECTED, 5, 0b11, [0, 0b01100]),
    # both areas reach a selected node at 5: the union is kept (293-300)
    (VALID | SELECTED, 5, 0b11, [0b00001, 0b01000]),
    # o filtered, the source's own entry is all that is selected (253-258)
    (LOCAL | SELECTED | reason(R.REASON_SELF), INF32, 0b1, [0, 0]),
    # w is in no SPF result: all-ones distance, garbage next hops unread (217-223)
    (reason(R.REASON_UNREACHABLE), INF32, 0, [0, 0]),
    # v4 prefix, neither enableV4 nor v4OverV6Nexthop (169-176)
    (reason(R.REASON_V4_DISABLED), INF32, 0, [0, 0]),
    # v reached at 7 over no link slot (605-607); its metric increment != 0
    (SELECTED | DRAINED | reason(R.REASON_NO_NEXTHOP), 7, 0b1, [0, 0]),
    # thresholds 1 and 4 among the selected entries: 4 > 2 next hops (496-509, 612)
    (SELECTED | reason(R.REASON_MIN_NEXTHOP), 5, 0b11, [0, 0b01100]),
    # threshold 2 is met by ONE next hop in EACH of two areas
    (VALID | SELECTED, 5, 0b11, [0b00001, 0b01000]),
    # x and the source selected; the best entry stays the first (no
    # selectBestNodeArea without best-route selection, 476-483)
    (LOCAL | SELECTED | reason(R.REASON_SELF), INF32, 0b11, [0, 0]),
    # y's area-1 entry: reachability and next hops from area 1's row
    (VALID | SELECTED, 5, 0b1, [0, 0b00100]),
    # a negative threshold is compared as size_t (612): never met
    (SELECTED | reason(R.REASON_MIN_NEXTHOP), 5, 0b11, [0b00001, 0b01000]),
]


def test_multiarea_plain_selection():
    dom = domain(NAME_LOCAL, NODE_FLAGS, PLAIN, ROWS)
    assert run(dom, [ME], [0, 1], 0) == [PLAIN_WANT]


def test_multiarea_v4_flags():
    dom = domain(NAME_LOCAL, NODE_FLAGS, PLAIN, ROWS)
    routed = (VALID | SELECTED, 5, 0b1, [0b00001, 0])
    for flags in (R.F_ENABLE_V4, R.F_V4_OVER_V6, R.F_ENABLE_V4 | R.F_V4_OVER_V6):
        want = list(PLAIN_WANT)
        want[7] = routed
        assert run(dom, [ME], [0, 1], flags) == [want]


def test_multiarea_source_without_adjacency_db_in_an_area():
    """spf_row == OGS_NODE_NONE: the source's SPF there is the source alone
    (LinkState.cpp:730-734); unit 1 of two, so the unit stride shows"""
    dom = domain(NAME_LOCAL, NODE_FLAGS, [
        (False, [(X, 0, D, None), (Z, 1, D, None)]),
        (False, [(ME, 0, D, None)]),
        (False, [(X, 0, D, None)])], ROWS)
    assert run(dom, [ME, ME], [0, 1, NONE, 1], 0) == [
        [(VALID | SELECTED, 5, 0b11, [0b00001, 0b01000]),
         (LOCAL | SELECTED | reason(R.REASON_SELF), INF32, 0b1, [0, 0]),
         (VALID | SELECTED, 5, 0b1, [0b00001, 0])],
        [(VALID | SELECTED | best(1), 5, 0b10, [0, 0b01000]),   # x dropped, z is entry 1
         (LOCAL | SELECTED | reason(R.REASON_SELF), INF32, 0b1, [0, 0]),
         (reason(R.REASON_UNREACHABLE), INF32, 0, [0, 0])]]


def test_multiarea_best_route_selection_key_order():
    dom = domain(NAME_LOCAL, NODE_FLAGS, [
        (False, [(X, 0, (1, 900, 100, 1), None), (Y, 0, (0, 100, 100, 9), None)]),
        (False, [(X, 0, (0, 100, 900, 1), None), (Y, 0, (0, 200, 100, 9), None)]),
        (False, [(X, 0, (0, 100, 100, 1), None), (Y, 0, (0, 100, 200, 9), None)]),
        (False, [(X, 0, (0, 100, 100, 4), None), (Y, 0, (0, 100, 100, 3), None)]),
        (False, [(X, 0, D, None), (Y, 0, D, None)]),
        (False, [(Y, 0, (0, 100, 100, 9), None), (V, 0, (0, 900, 900, 1), None)]),
        (False, [(X, 0, D, None), (ME, 0, D, None)]),
        (False, [(X, 0, (0, 200, 100, 1), None), (ME, 0, D, None)]),
        (False, [(O, 0, (0, 900, 900, 0), None), (Y, 0, D, None)]),
    ], ROWS)
    y_wins = (VALID | SELECTED | best(1), 20, 0b10, [0b00010, 0])
    assert run(dom, [ME], [0, 1], R.F_BEST_ROUTE_SELECTION) == [[
        y_wins,  # drain_metric set beats a higher path preference (786-790)
        y_wins,  # path preference beats source preference
        y_wins,  # source preference beats distance
        y_wins,  # then the shorter distance (716-736)
        # a full tie selects both; next hops toward the closer one only (670-676)
        (VALID | SELECTED, 5, 0b11, [0b00001, 0]),
        # v's metric increment > 0 in its area counts as drained (511-524)
        (VALID | SELECTED, 20, 0b1, [0b00010, 0]),
        # the source's entry is the best one when selected (700-711), not the first
        (LOCAL | SELECTED | best(1) | reason(R.REASON_SELF), INF32, 0b11, [0, 0]),
        # the source advertises but loses: a route, localPrefixConsidered set
        (VALID | LOCAL | SELECTED, 5, 0b1, [0b00001, 0]),
        # the hard-drain filter runs before the selection (466-474)
        y_wins]]


def test_multiarea_segment_past_32_entries():
    """36 advertisers: sel covers entries 0..31; the best index and the masks
    cover all of them. One area, two next-hop words: node i's next hop is
    link slot i."""
    G = 40
    name_local = [[i] for i in range(G)]
    nh = [[(1 << i) if i < 32 else 0 for i in range(G)],
          [(1 << (i - 32)) if i >= 32 else 0 for i in range(G)]]
    rows = [([0] + [5] * (G - 1), nh)]
    every = [(i, 0, D, None) for i in range(1, 37)]
    late = [(i, 0, (0, 200, 100, 1) if i in (34, 35) else D, None) for i in range(1, 37)]
    dom = domain(name_local, [[0] * G], [(False, every), (False, late)], rows, W=2)
    assert run(dom, [0], [0], 0, W=2) == [[
        (VALID | SELECTED, 5, 0xFFFFFFFF, [0xFFFFFFFE, 0x1F]),
        (VALID | SELECTED, 5, 0xFFFFFFFF, [0xFFFFFFFE, 0x1F])]]
    assert run(dom, [0], [0], R.F_BEST_ROUTE_SELECTION, W=2) == [[
        (VALID | SELECTED, 5, 0xFFFFFFFF, [0xFFFFFFFE, 0x1F]),
        # entries 33 and 34 (names 34, 35) selected: no bit of sel, best 33
        (VALID | SELECTED | best(33), 5, 0, [0, 0b1100])]]


def test_multiarea_reached_bitset_and_all_ones_distance():
    """a wrapped u64 distance of a settled node may be all ones: with
    areas->reached the bitset decides (node 1 settled, node 2 not), and the
    all-ones metric still ties the initial shortestMetric (670: >=)"""
    name_local = [[0], [1], [2]]
    rows = [([0, INF64, INF64], [[0, 0b01, 0b10]])]
    pfx = [(False, [(1, 0, D, None)]), (False, [(2, 0, D, None)])]
    dom = domain(name_local, [[0, 0, 0]], pfx, rows, wide=True, reached=u32(0b011))
    assert run(dom, [0], [0], R.F_WIDE_METRIC) == [[
        (VALID | SELECTED, INF64, 0b1, [0b01]),
        (reason(R.REASON_UNREACHABLE), INF64, 0, [0])]]
    dom = domain(name_local, [[0, 0, 0]], pfx, rows, wide=True)
    assert run(dom, [0], [0], R.F_WIDE_METRIC) == [[
        (reason(R.REASON_UNREACHABLE), INF64, 0, [0]),
        (reason(R.REASON_UNREACHABLE), INF64, 0, [0])]]


# ------------------------------------------------- the device tests' inputs
def test_device_cases_are_not_vacuous():
    """the seeded cases of the three device test files, on the references'
    side: every outcome the device tests rely on occurs in every case"""
    import test_gpu_rib_policy_abi as rib
    import test_gpu_routes_multiarea_abi as ma
    for i, shape in enumerate(rib.CASES):
        c = rib.make_case(rib.case_seed(i), *shape)
        rib.check_not_vacuous(c, rib.reference(c))
    c = rib.make_case(0xAB1E70, 3, 2, 2, 257, 5, 7, 70)
    rib.check_not_vacuous(c, rib.reference(c))
    for i, (U, A, W, flags, P, slack, p0, reached) in enumerate(ma.CASES):
        c = ma.make_case(ma.case_seed(i), U, A, W, flags, P, slack, p0, reached)
        ma.check_not_vacuous(c, ma.reference(c))


def test_device_cases_tell_stride_and_base_mistakes_apart():
    """the answers a kernel would give with a unit stride dropped or the
    prefix table read from global prefix 0 differ from the reference's on the
    seeded inputs, so the device comparison cannot pass by accident"""
    import test_gpu_rib_policy_abi as rib
    import test_gpu_routes_multiarea_abi as ma
    i = rib.CASES.index((3, 2, 2, 257, 5, 7, 32))
    c = rib.make_case(rib.case_seed(i), *rib.CASES[i])
    want = rib.reference(c)
    P, U = c["P"], c["U"]
    wrong = [dict(c, nz=np.repeat(c["nz"][:1], U, 0)),          # slot_nonzero of unit 0
             dict(c, pfx_base=np.array([0, P], np.uint32))]     # pfx_base[0] ignored
    for w in wrong:
        got = rib.reference(w)
        assert all((g != x).any() for g, x in zip(got, want))
    i = ma.CASES.index((4, 3, 2, ma.BRS, 257, 5, 7, False))
    U, A, W, flags, P, slack, p0, reached = ma.CASES[i]
    c = ma.make_case(ma.case_seed(i), U, A, W, flags, P, slack, p0, reached)
    want = ma.reference(c)
    wrong = [dict(c, spf_row=np.tile(c["spf_row"][:A], U)),     # SPF rows of unit 0
             dict(c, units=np.repeat(c["units"][:1], U)),       # source of unit 0
             dict(c, table=dict(c["table"], pfx_base=np.array([0, P], np.uint32)))]
    for w in wrong:
        got = ma.reference(w)
        assert all((got[k] != want[k]).any() for k in ("meta", "metric", "sel", "mask"))
