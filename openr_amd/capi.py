"""ctypes view of the C-ABI (include/openr_gpu.h) — what a Python consumer of
the boundary binds. bench.py drives the kernel through it with torch-owned
device memory and torch's current HIP stream."""
import contextlib
import ctypes

from . import LIB_PATH

OGS_OK = 0
OGS_ABI_VERSION = 8  # include/openr_gpu.h
OGS_F_ENABLE_V4 = 0x01
OGS_F_V4_OVER_V6 = 0x02
OGS_F_BEST_ROUTE_SELECTION = 0x04
OGS_F_HOP_METRIC = 0x08
OGS_F_WIDE_METRIC = 0x10
OGS_E_INVALID = -1
OGS_E_UNSUPPORTED = -4
OGS_DELTA_ROUTE = 0x1
OGS_DELTA_SELECTION = 0x2
OGS_ROUTE_DELTA_TILE = 2048

# every extern "C" entry point declared in include/openr_gpu.h
EXPORTS = [
    "ogs_version", "ogs_last_error", "ogs_device_count", "ogs_set_device",
    "ogs_malloc", "ogs_free", "ogs_memcpy_h2d", "ogs_memcpy_d2h", "ogs_memset",
    "ogs_stream_sync", "ogs_nh_words_for_degree", "ogs_spf_routes",
    "ogs_ksp_paths", "ogs_ksp2_paths", "ogs_set_option", "ogs_routes_multiarea",
    "ogs_spf_routes_variants", "ogs_rib_policy_apply", "ogs_route_changes_gather",
    "ogs_csr_patch", "ogs_host_alloc", "ogs_host_free", "ogs_routes_from_spf",
    "ogs_abi_version", "ogs_spf_routes_groups",
    "ogs_ctx_create", "ogs_ctx_destroy", "ogs_ctx_set_option", "ogs_ctx_spf_routes",
    "ogs_ctx_spf_routes_groups", "ogs_ctx_routes_from_spf", "ogs_ctx_spf_routes_variants",
    "ogs_ctx_ksp_paths", "ogs_ctx_ksp2_paths", "ogs_ctx_routes_multiarea",
    "ogs_ctx_rib_policy_apply",
    "ogs_get_option", "ogs_ctx_get_option", "ogs_option_name",
    "ogs_route_delta",
    "ogs_spf_routes_scenarios", "ogs_ctx_spf_routes_scenarios",
    "ogs_spf_routes_whatif", "ogs_ctx_spf_routes_whatif",
    "ogs_spf_routes_whatif_global", "ogs_whatif_needs_global",
    "ogs_spf_node_diff", "ogs_spf_node_changes_gather",
    "ogs_spf_routes_whatif_pairs", "ogs_ctx_spf_routes_whatif_pairs",
]

OGS_WHATIF_REFUSED = 0xFFFFFFFF
# the what-if entries' restorations (read under OGS_F_RESTORE only)
OGS_F_RESTORE = 0x100
OGS_WHATIF_EDGE_UP = 0x80000000
OGS_NODE_CLEAR_SHIFT = 4


class WhatifMods(ctypes.Structure):
    """ogs_whatif_mods: per unit, dead edges, node flag bits and metric
    overrides (device pointers; NULL node / metric triples: none)."""
    _fields_ = [("dead_off", ctypes.c_void_p), ("dead_edges", ctypes.c_void_p),
                ("node_off", ctypes.c_void_p), ("node_ids", ctypes.c_void_p),
                ("node_bits", ctypes.c_void_p),
                ("metric_off", ctypes.c_void_p), ("metric_edges", ctypes.c_void_p),
                ("metric_vals", ctypes.c_void_p), ("max_metric_per_unit", ctypes.c_uint32)]


class WhatifPairs(ctypes.Structure):
    """ogs_whatif_pairs: per unit, its row in the diff's base arrays and its
    row in the mods' offset arrays (device pointers)."""
    _fields_ = [("base", ctypes.c_void_p), ("scenario", ctypes.c_void_p),
                ("n_bases", ctypes.c_int32), ("n_scenarios", ctypes.c_int32)]


class Graph(ctypes.Structure):
    _fields_ = [("num_topos", ctypes.c_int32), ("max_nodes", ctypes.c_int32),
                ("max_edges", ctypes.c_int32), ("max_degree", ctypes.c_int32),
                ("node_base", ctypes.c_void_p),
                ("row_ptr", ctypes.c_void_p), ("edges", ctypes.c_void_p),
                ("node_flags", ctypes.c_void_p), ("topo_desc", ctypes.c_void_p),
                ("slot_node", ctypes.c_void_p), ("slot_stride", ctypes.c_int32),
                ("slot_edges", ctypes.c_void_p), ("slot_degree", ctypes.c_int32),
                ("edge_src", ctypes.c_void_p), ("rslot_ext", ctypes.c_void_p)]


class PrefixTable(ctypes.Structure):
    _fields_ = [("max_prefixes", ctypes.c_int32), ("max_advertisements", ctypes.c_int32),
                ("pfx_base", ctypes.c_void_p),
                ("adv_off", ctypes.c_void_p), ("adv_node", ctypes.c_void_p),
                ("adv_metrics", ctypes.c_void_p), ("adv_min_nh", ctypes.c_void_p),
                ("pfx_flags", ctypes.c_void_p)]


class SpfOut(ctypes.Structure):
    _fields_ = [("dist", ctypes.c_void_p), ("nh", ctypes.c_void_p),
                ("meta", ctypes.c_void_p), ("metric", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("sel", ctypes.c_void_p),
                ("reached", ctypes.c_void_p)]


class RouteGroup(ctypes.Structure):
    _fields_ = [("units", ctypes.c_void_p), ("n_units", ctypes.c_int32),
                ("nh_words", ctypes.c_int32), ("out", SpfOut)]


class RouteDeltaPolicy(ctypes.Structure):
    _fields_ = [("prev_applied", ctypes.c_void_p), ("prev_counter", ctypes.c_void_p),
                ("next_applied", ctypes.c_void_p), ("next_counter", ctypes.c_void_p)]


class RouteDeltaOut(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_uint32), ("prefix", ctypes.c_void_p),
                ("kind", ctypes.c_void_p), ("meta", ctypes.c_void_p),
                ("metric", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("sel", ctypes.c_void_p), ("applied", ctypes.c_void_p),
                ("counter", ctypes.c_void_p), ("header", ctypes.c_void_p)]


class ScenarioMods(ctypes.Structure):
    _fields_ = [("dead_off", ctypes.c_void_p), ("dead_edges", ctypes.c_void_p),
                ("drain_off", ctypes.c_void_p), ("drain_nodes", ctypes.c_void_p)]


class RouteDiff(ctypes.Structure):
    _fields_ = [("base_meta", ctypes.c_void_p), ("base_metric", ctypes.c_void_p),
                ("base_mask", ctypes.c_void_p), ("changed", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("base_dist", ctypes.c_void_p),
                ("base_nh", ctypes.c_void_p), ("adv_class", ctypes.c_void_p),
                ("base_desc", ctypes.c_void_p), ("base_desc_valid", ctypes.c_int32)]


class NodeDiff(ctypes.Structure):
    """ogs_node_diff: the base unit's SPF rows, optional interest mask and
    unit counts, and the changed bitmap / counts the call writes."""
    _fields_ = [("base_dist", ctypes.c_void_p), ("base_nh", ctypes.c_void_p),
                ("interest", ctypes.c_void_p), ("unit_counts", ctypes.c_void_p),
                ("changed", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


class NodeChanges(ctypes.Structure):
    """ogs_node_changes: offsets, total and the compact record arrays."""
    _fields_ = [("offsets", ctypes.c_void_p), ("total", ctypes.c_size_t),
                ("node", ctypes.c_void_p), ("dist", ctypes.c_void_p),
                ("nh", ctypes.c_void_p)]


class RibPolicy(ctypes.Structure):
    """ogs_rib_policy: one chunk of <= 32 statements compiled against a
    prefix table (device pointers)."""
    _fields_ = [("num_statements", ctypes.c_int32), ("active", ctypes.c_uint32),
                ("pfx_match", ctypes.c_void_p), ("adv_tag_match", ctypes.c_void_p),
                ("slot_nonzero", ctypes.c_void_p), ("statement_base", ctypes.c_int32)]


class AreaTable(ctypes.Structure):
    """ogs_area_table: the name-id tables of a multi-area domain and the
    optional settled bitsets of its SPF rows."""
    _fields_ = [("num_areas", ctypes.c_int32), ("num_names", ctypes.c_int32),
                ("name_local", ctypes.c_void_p), ("adv_area", ctypes.c_void_p),
                ("adv_name", ctypes.c_void_p), ("reached", ctypes.c_void_p)]


class RouteChanges(ctypes.Structure):
    """ogs_route_changes: offsets, total and the compact record arrays."""
    _fields_ = [("offsets", ctypes.c_void_p), ("total", ctypes.c_size_t),
                ("prefix", ctypes.c_void_p), ("meta", ctypes.c_void_p),
                ("metric", ctypes.c_void_p), ("mask", ctypes.c_void_p)]


def route_delta_workspace_bytes(num_prefixes):
    """OGS_ROUTE_DELTA_WORKSPACE_BYTES of include/openr_gpu.h."""
    return (num_prefixes + OGS_ROUTE_DELTA_TILE - 1) // OGS_ROUTE_DELTA_TILE * 528


def load(path=None):
    lib = ctypes.CDLL(path or LIB_PATH)
    lib.ogs_version.restype = ctypes.c_char_p
    if lib.ogs_abi_version() != OGS_ABI_VERSION:
        raise RuntimeError(f"libopenr_gpu ABI {lib.ogs_abi_version()}, "
                           f"this binding expects {OGS_ABI_VERSION}")
    lib.ogs_last_error.restype = ctypes.c_char_p
    lib.ogs_spf_routes.argtypes = [
        ctypes.POINTER(Graph), ctypes.POINTER(PrefixTable), ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(SpfOut),
        ctypes.c_void_p]
    lib.ogs_spf_routes.restype = ctypes.c_int
    lib.ogs_spf_routes_groups.argtypes = [
        ctypes.POINTER(Graph), ctypes.POINTER(PrefixTable), ctypes.POINTER(RouteGroup),
        ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p]
    lib.ogs_spf_routes_groups.restype = ctypes.c_int
    lib.ogs_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    lib.ogs_set_option.restype = ctypes.c_int
    lib.ogs_get_option.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    lib.ogs_get_option.restype = ctypes.c_int
    lib.ogs_option_name.argtypes = [ctypes.c_int32]
    lib.ogs_option_name.restype = ctypes.c_char_p
    lib.ogs_route_delta.argtypes = [
        ctypes.POINTER(SpfOut), ctypes.POINTER(SpfOut), ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.POINTER(RouteDeltaPolicy), ctypes.c_uint32, ctypes.c_int32,
        ctypes.POINTER(RouteDeltaOut), ctypes.c_void_p, ctypes.c_void_p]
    lib.ogs_route_delta.restype = ctypes.c_int
    # execution contexts (ABI 6): opaque handles
    lib.ogs_ctx_create.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.ogs_ctx_create.restype = ctypes.c_int
    lib.ogs_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.ogs_ctx_destroy.restype = ctypes.c_int
    lib.ogs_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    lib.ogs_ctx_set_option.restype = ctypes.c_int
    lib.ogs_ctx_get_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_int64)]
    lib.ogs_ctx_get_option.restype = ctypes.c_int
    lib.ogs_ctx_spf_routes.argtypes = [ctypes.c_void_p] + lib.ogs_spf_routes.argtypes
    lib.ogs_ctx_spf_routes.restype = ctypes.c_int
    lib.ogs_ctx_spf_routes_groups.argtypes = ([ctypes.c_void_p] +
                                             lib.ogs_spf_routes_groups.argtypes)
    lib.ogs_ctx_spf_routes_groups.restype = ctypes.c_int
    # the remaining compute entry points: structs this module does not model
    # (ogs_path_unit, ogs_unit_mods, ogs_area_table, ogs_rib_policy, ...)
    # pass as c_void_p, so 64-bit handles and device pointers never go
    # through ctypes' default int conversion
    P, I32, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    plain = {
        "ogs_routes_from_spf": [P, P, P, I32, P, P, P, U32, I32, P, P],
        "ogs_spf_routes_variants": [P, P, P, I32, P, P, U32, I32, P, P],
        "ogs_spf_routes_scenarios": [P, P, P, I32, P, P, U32, I32, P, P],
        "ogs_spf_routes_whatif": [P, P, P, I32, P, P, U32, I32, P, P],
        "ogs_spf_routes_whatif_pairs": [P, P, P, I32, P, P, P, U32, I32, P, P],
        "ogs_ksp_paths": [P, P, I32, P, U32, U32, P, P],
        "ogs_ksp2_paths": [P, P, I32, P, I32, U32, P, P, P],
        "ogs_routes_multiarea": [P, P, P, P, I32, P, P, P, U32, I32, P, P],
        "ogs_rib_policy_apply": [P, P, I32, I32, I32, P, P, P, P, P],
    }
    for name, args in plain.items():
        for fn, a in ((name, args), ("ogs_ctx_" + name[4:], [P] + args)):
            f = getattr(lib, fn)
            f.argtypes = a
            f.restype = ctypes.c_int
    # the global-state what-if form (no ogs_ctx_ twin)
    lib.ogs_spf_routes_whatif_global.argtypes = plain["ogs_spf_routes_whatif"]
    lib.ogs_spf_routes_whatif_global.restype = ctypes.c_int
    lib.ogs_whatif_needs_global.argtypes = [ctypes.POINTER(Graph), U32, I32]
    lib.ogs_whatif_needs_global.restype = ctypes.c_int
    # SPF-row diff and gather of the node-label sweep (no ogs_ctx_ twins)
    lib.ogs_spf_node_diff.argtypes = [
        ctypes.POINTER(Graph), P, I32, ctypes.POINTER(SpfOut), ctypes.POINTER(NodeDiff), U32,
        I32, P]
    lib.ogs_spf_node_diff.restype = ctypes.c_int
    lib.ogs_spf_node_changes_gather.argtypes = [
        P, I32, I32, ctypes.POINTER(SpfOut), I32, ctypes.POINTER(NodeChanges), P]
    lib.ogs_spf_node_changes_gather.restype = ctypes.c_int
    # changed-route gather of the variant / scenario / what-if sweeps
    lib.ogs_route_changes_gather.argtypes = [
        P, I32, I32, ctypes.POINTER(SpfOut), I32, ctypes.POINTER(RouteChanges), P]
    lib.ogs_route_changes_gather.restype = ctypes.c_int
    return lib


def check(lib, rc, what):
    if rc != OGS_OK:
        raise RuntimeError(f"{what} failed ({rc}): {lib.ogs_last_error().decode()}")


def get_option(lib, name):
    """Current value of one default-context knob."""
    value = ctypes.c_int64()
    check(lib, lib.ogs_get_option(name.encode(), ctypes.byref(value)), name)
    return value.value


@contextlib.contextmanager
def scoped_options(lib=None, **options):
    """Set default-context knobs for one `with` block: each knob's current
    value is read and the new one set (a rejected value raises through
    check()); on exit, exceptions and a rejected later knob included, the
    saved values go back in reverse order. Scopes nest."""
    lib = lib or load()
    saved = []
    try:
        for name, value in options.items():
            old = get_option(lib, name)
            check(lib, lib.ogs_set_option(name.encode(), value), name)
            saved.append((name, old))
        yield lib
    finally:
        for name, old in reversed(saved):
            lib.ogs_set_option(name.encode(), old)
